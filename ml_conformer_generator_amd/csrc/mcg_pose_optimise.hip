// Optimised pose ("Optimised pose"; the definition is the docstring of `interactions.optimise_pose`):
// every posed molecule is moved as a rigid body downhill on W, the weighted sum of the five terms of the receptor
// interaction score, by the accept / reject walk of mcg_rigid_step.h (`rotate_about`, `step_along`, `within_shift`,
// `StepLengths`) with the pair arithmetic of mcg_interaction_pair.h.
// THE PACKAGE'S OWN procedure: not a docking run, not AutoDock Vina's local optimisation; rigid
// body only - no torsions, no intramolecular term, no hydrogens, no global search.
//   k_receptor_optimise: one 256-lane workgroup per molecule, laid out as `k_receptor_interactions`: lane l holds ligand
//                       atom a = l & 63 in registers, wave w = l >> 6 walks the receptor atoms j = w, w + 4, ... of each
//                       kept 256-atom tile out of LDS, tiles and atoms in ascending order.  A counted pair adds its five
//                       terms (`mcg_interaction::pair_terms`, the text the scoring kernel runs) and its force
//                       F_i += g dx, g dy, g dz with g = -(dW/dd) / r (0 at r = 0) to the lane's eight accumulators.  The
//                       four waves' partials of an atom are combined as (w0 + w1) + (w2 + w3) through LDS; wave 0 forms the
//                       atom's torque u_i x F_i about p (u_i = (x_i - c) @ G, the atom seen from p) and the molecule's
//                       eleven sums by one butterfly over the 64 atom slots.  Every lane reads them back, so every lane
//                       holds the same state and takes the same branch.  No atomics.
//                       Pose x' = (x - c) @ G + p from G = I, p = c (c the atom centroid summed in atom order); the first
//                       evaluation reads the input rows as they came.  A trial rotates by s_r about the torque and moves p
//                       by s_t along the net force (from 0.05 rad, 0.25 A; a zero or non-finite vector skips its part, both
//                       skipped ends the walk); a trial with |p' - c| > max_shift is rejected unevaluated; an evaluated one
//                       is kept iff W' < W, strictly (NaN never is).  Kept: both lengths x 1.2; rejected: x 0.5.  The walk
//                       ends after `steps` trials or once s_t < 2^-8.  G is re-orthonormalised as each trial is formed, and
//                       each lane keeps the coordinates it evaluated, so the pose returned is the pose that was scored.
//   Tile list:          built once (`mcg_tiles::build_tile_list`, mcg_receptor_tiles.h) with the reach (rho + 8) +
//                       max_shift, the scoring kernel's with max_shift added: rotation is about
//                       p, so the ligand's radius about its centroid does not change, and p stays within max_shift of c.
//                       Every pair of a tile left out has r2 >= 64 in every pose the walk can evaluate and adds nothing.
// A molecule's outputs depend on its own atoms and the receptor arrays only: bit-identical whatever the batch, row or width.
// `k_receptor_optimise_flex` (mcg_pose_flex.hip) repeats this walk's text with torsions added and promises this kernel's
// bits to a molecule without a torsion: a change here is made there too ("Shared device text").  The
// step constants and the entry's argument check are mcg_receptor_walk.h's, shared with that kernel.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"
#include "mcg_rigid_step.h"
#include "mcg_receptor_tiles.h"
#include "mcg_interaction_pair.h"
#include "mcg_receptor_walk.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;
using namespace mcg_rigid;           // the trial, the step lengths, the returned transform: one text for every walk
using namespace mcg_tiles;           // the centroid and the tile list, shared by every kernel that reaches a receptor
using namespace mcg_interaction;     // the pair arithmetic, shared with k_receptor_interactions
using namespace mcg_receptor_walk;   // the step constants and the argument check, shared with k_receptor_optimise_flex

constexpr int PO_SUMS = 11;                   // g1, g2, rep, hyd, hb, F[3], torque[3]
constexpr int PO_TRACE = 24;                  // F[3], torque[3], s_r, s_t, G'[9], p'[3], W', evaluated, kept, W_cur

struct OptimiseShared {
    float4 tile[IX_THREADS];                  // the staged receptor tile: x, y, z, R_j
    unsigned char type[IX_THREADS];
    float part[IX_WAVES][MAX_ATOMS][8];       // per wave and atom: g1, g2, rep, hyd, hb, F
    float red[PO_SUMS];
    float c[3];
    float reach[IX_WAVES][1];                 // per wave: max |x_i - c|^2
    TileList<MAX_RECEPTOR_TILES> tiles;
};

// The five term sums, the net force and the torque about p of the pose whose atom a this lane holds at (x, y, z), seen
// from p at (ux, uy, uz), into v[11]; identical in every lane.
__device__ void evaluate(OptimiseShared& s, const float4* __restrict__ rec, const unsigned char* __restrict__ rec_t, int R,
                         bool real, float x, float y, float z, float ux, float uy, float uz, float ri, unsigned ti,
                         float* v) {
    const int tid = threadIdx.x, a = tid & 63, w = tid >> 6;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int nhb = 0;
    const int nt = s.tiles.n_tiles;
    for (int k = 0; k < nt; ++k) {
        const int j0 = (int)s.tiles.list[k] * IX_THREADS;
        const int cnt = min(IX_THREADS, R - j0);                   // the last tile's tail
        if (tid < cnt) {
            s.tile[tid] = rec[j0 + tid];
            s.type[tid] = rec_t[j0 + tid];
        }
        __syncthreads();
        for (int jj = w; jj < cnt; jj += IX_WAVES) {
            const float4 q = s.tile[jj];
            float dx, dy, dz;
            const float r2 = pair_r2(x, y, z, q, dx, dy, dz);
            const bool counts = real && r2 < IX_CUTOFF2;
            if (__ballot(counts) == 0ull) continue;                // nobody in this wave: nothing is added
            if (counts) {
                const unsigned tj = s.type[jj];
                const PairValues pv = pair_terms(r2, ri, q.w, ti, tj, acc, nhb);
                const float g = pv.r > 0.f ? -pair_slope(pv, ti, tj) / pv.r : 0.f;
                acc[5] += g * dx; acc[6] += g * dy; acc[7] += g * dz;
            }
        }
        __syncthreads();                      // the tile is free again
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s.part[w][a][k] = acc[k];
    __syncthreads();
    if (w == 0) {
        float t[PO_SUMS];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = (s.part[0][a][k] + s.part[1][a][k]) + (s.part[2][a][k] + s.part[3][a][k]);
        t[8] = uy * t[7] - uz * t[6];         // a padded slot: u = 0, F = 0
        t[9] = uz * t[5] - ux * t[7];
        t[10] = ux * t[6] - uy * t[5];
#pragma unroll
        for (int k = 0; k < PO_SUMS; ++k)
            for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_xor(t[k], o, 64);
        if (a == 0) {
#pragma unroll
            for (int k = 0; k < PO_SUMS; ++k) s.red[k] = t[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PO_SUMS; ++k) v[k] = s.red[k];
}

__global__ __launch_bounds__(IX_THREADS) void k_receptor_optimise(
    const float* __restrict__ lig, const float* __restrict__ lig_r, const unsigned char* __restrict__ lig_t,
    const int* __restrict__ n_nodes, int N, const float4* __restrict__ rec, const unsigned char* __restrict__ rec_t, int R,
    const float4* __restrict__ tile_sphere, int steps, float max_shift, float* __restrict__ coords_out,
    float* __restrict__ xform_out, float* __restrict__ stats_out, float* __restrict__ gradient_out,
    float* __restrict__ trace_out) {
    __shared__ OptimiseShared s;
    const int b = blockIdx.x, tid = threadIdx.x, a = tid & 63, w = tid >> 6;
    const int na = atom_count(n_nodes[b], N);
    const float* xin = lig + (size_t)b * N * 3;
    float* xout = coords_out + (size_t)b * N * 3;
    float* xf = xform_out + (size_t)b * 12;
    float* stats = stats_out + (size_t)b * 8;
    float* trace = trace_out != nullptr ? trace_out + (size_t)b * steps * PO_TRACE : nullptr;
    const bool real = a < na;
    float x0 = 0.f, y0 = 0.f, z0 = 0.f, ri = 0.f;
    unsigned ti = 0u;
    if (real) {
        x0 = xin[a * 3]; y0 = xin[a * 3 + 1]; z0 = xin[a * 3 + 2];
        ri = lig_r[(size_t)b * N + a];
        ti = lig_t[(size_t)b * N + a];
    }
    const bool bad = real && !(isfinite(x0) && isfinite(y0) && isfinite(z0));
    if (__syncthreads_or(bad) != 0 || na == 0) {                   // left exactly as it came, NaN transform and stats
        if (w == 0 && a < N) {
            xout[a * 3] = x0; xout[a * 3 + 1] = y0; xout[a * 3 + 2] = z0;       // a padded slot holds 0
        }
        if (tid < 12) xf[tid] = __builtin_nanf("");
        if (tid < 8) stats[tid] = __builtin_nanf("");
        if (gradient_out != nullptr && tid < 6) gradient_out[(size_t)b * 6 + tid] = __builtin_nanf("");
        if (trace != nullptr)
            for (int q = tid; q < steps * PO_TRACE; q += IX_THREADS) trace[q] = 0.f;
        return;
    }
    if (w == 0) s.part[0][a][0] = x0, s.part[0][a][1] = y0, s.part[0][a][2] = z0;   // borrowed for the centroid
    __syncthreads();
    if (tid < 3) {                            // atom centroid, summed in atom order (inline: DESIGN.md section 6)
        float acc = 0.f;
        for (int i = 0; i < na; ++i) acc += s.part[0][i][tid];
        s.c[tid] = acc / (float)na;
    }
    __syncthreads();
    const float c[3] = {s.c[0], s.c[1], s.c[2]};
    float rx = 0.f, ry = 0.f, rz = 0.f, rho2 = 0.f;
    if (real) {
        rx = x0 - c[0]; ry = y0 - c[1]; rz = z0 - c[2];
        rho2 = (rx * rx + ry * ry) + rz * rz;
    }
    block_max4<1>(s.reach, &rho2, a, w);
    // the tiles within reach of any pose of the walk
    build_tile_list(s.tiles, tile_sphere, (R + IX_THREADS - 1) / IX_THREADS, c[0], c[1], c[2],
                    (sqrtf(rho2) + IX_CUTOFF) + max_shift);

    float G[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, p[3] = {c[0], c[1], c[2]};
    float cur[PO_SUMS];
    float cx = x0, cy = y0, cz = z0;          // this lane's atom in the pose that holds
    evaluate(s, rec, rec_t, R, real, x0, y0, z0, rx, ry, rz, ri, ti, cur);     // the input rows as they came
    float w_cur = weighted(cur);
    const float w_start = w_cur;
    if (gradient_out != nullptr && tid == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) gradient_out[(size_t)b * 6 + k] = cur[5 + k];
    }
    StepLengths len = {RW_STEP_ROT, RW_STEP_TRANS};
    int trials = 0, kept = 0;
    for (; trials < steps && !(len.trans < RW_MIN_TRANS); ++trials) {
        float Gn[9], pn[3];
        const float fn = norm3(cur + 5), tn = norm3(cur + 8);
        const bool moves = fn > 0.f && isfinite(fn), turns = tn > 0.f && isfinite(tn);
        if (!moves && !turns) break;          // nothing to follow: the walk ends, the trial is not counted
        if (turns) {
            rotate_about<true>(G, cur[8] / tn, cur[9] / tn, cur[10] / tn, len.rot, Gn);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) Gn[k] = G[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) pn[k] = step_along(p[k], cur[5 + k], fn, moves, len.trans);
        const bool evaluated = within_shift(pn, c[0], c[1], c[2], max_shift);
        bool take = false;
        float nxt[PO_SUMS], w_nxt = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
        if (evaluated) {                      // the same in every lane
            float u[3] = {0.f, 0.f, 0.f};
            if (real) {
                rotate_row(rx, ry, rz, Gn, u);
                tx = u[0] + pn[0]; ty = u[1] + pn[1]; tz = u[2] + pn[2];
            }
            evaluate(s, rec, rec_t, R, real, tx, ty, tz, u[0], u[1], u[2], ri, ti, nxt);
            w_nxt = weighted(nxt);
            take = w_nxt < w_cur;
        }
        if (trace != nullptr && tid == 0) {   // one lane, constant indices: the state stays in registers
            float* row = trace + (size_t)trials * PO_TRACE;
#pragma unroll
            for (int k = 0; k < 6; ++k) row[k] = cur[5 + k];
            row[6] = len.rot; row[7] = len.trans;
#pragma unroll
            for (int k = 0; k < 9; ++k) row[8 + k] = Gn[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) row[17 + k] = pn[k];
            row[20] = w_nxt; row[21] = evaluated ? 1.f : 0.f; row[22] = take ? 1.f : 0.f; row[23] = w_cur;
        }
        if (take) {
            keep_trial<PO_SUMS>(G, p, cur, Gn, pn, nxt);
            w_cur = w_nxt;
            cx = tx; cy = ty; cz = tz;
            len.grow();
            ++kept;
        } else {
            len.shrink();
        }
    }
    if (trace != nullptr)                     // rows beyond the last trial are zero
        for (int q = trials * PO_TRACE + tid; q < steps * PO_TRACE; q += IX_THREADS) trace[q] = 0.f;
    if (kept == 0) {                          // nothing moved: the input's bits, the identity
        if (w == 0 && a < N) {
            xout[a * 3] = x0; xout[a * 3 + 1] = y0; xout[a * 3 + 2] = z0;
        }
        if (tid < 12) xf[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.f : 0.f;
        if (tid == 0) {
            stats[0] = w_start; stats[1] = w_start; stats[2] = (float)trials; stats[3] = 0.f;
            stats[4] = 0.f; stats[5] = len.trans; stats[6] = 0.f; stats[7] = 0.f;
        }
        return;
    }
    if (w == 0) {                             // the kept pose, as it was evaluated
        float d2 = 0.f;
        if (real) {
            const float ex = cx - x0, ey = cy - y0, ez = cz - z0;
            d2 = (ex * ex + ey * ey) + ez * ez;
        }
        if (a < N) {
            xout[a * 3] = cx; xout[a * 3 + 1] = cy; xout[a * 3 + 2] = cz;       // a padded slot holds 0
        }
        s.part[0][a][0] = d2;                 // every evaluation is over: nobody else reads it
    }
    __syncthreads();
    if (tid == 0) {
        write_transform(G, p, c[0], c[1], c[2], xf);
        float sum = 0.f;
        for (int i = 0; i < na; ++i) sum += s.part[0][i][0];       // in atom order
        stats[0] = w_start; stats[1] = w_cur; stats[2] = (float)trials; stats[3] = (float)kept;
        stats[4] = sqrtf(sum / (float)na); stats[5] = len.trans; stats[6] = 0.f; stats[7] = 0.f;
    }
}

}  // namespace

extern "C" int mcg_receptor_optimise(const float* lig_xyz, const float* lig_radius, const uint8_t* lig_type,
                                     const int32_t* n_nodes_dev, int B, int N, const float* rec_xyzr,
                                     const uint8_t* rec_type, int R, const float* tile_sphere, int steps, float max_shift,
                                     float* coords_out, float* xform_out, float* stats_out, float* gradient_out,
                                     float* trace_out, void* stream) {
    const bool buffers = lig_xyz && lig_radius && lig_type && n_nodes_dev && rec_xyzr && rec_type && coords_out &&
                         xform_out && stats_out;
    if (!walk_args_ok("mcg_receptor_optimise", buffers, B, N, R, steps, max_shift)) return MCG_ERR_ARG;
    hipLaunchKernelGGL(k_receptor_optimise, dim3(B), dim3(IX_THREADS), 0, (hipStream_t)stream, lig_xyz, lig_radius,
                       lig_type, n_nodes_dev, N, (const float4*)rec_xyzr, rec_type, R, (const float4*)tile_sphere, steps,
                       max_shift, coords_out, xform_out, stats_out, gradient_out, trace_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
