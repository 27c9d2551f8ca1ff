// Clash relief ("Clash relief"; the definition is the module docstring of receptor.py): every posed
// molecule is moved as a rigid body out of its steric contacts with the receptor, by the accept / reject walk of
// mcg_rigid_step.h (`rotate_about`, `step_along`, `within_shift`, `StepLengths`, `block_sums`) turned downhill.
//   k_receptor_relieve: one 256-lane workgroup per molecule.  The input rows, the ligand minus its atom centroid c and the
//                       pose being evaluated x' = (x - c) @ G + p sit in LDS.  Contact depth of ligand atom i and receptor
//                       atom j: h = max(0, ((r_i + r_j) - margin) - |x'_i - y_j|); penalty P = sum h^2, force on atom i
//                       F_i = sum_j 2 h (x'_i - y_j) / |x'_i - y_j|, torque about p: sum (x'_i - p) x F_i.  Lane l owns the
//                       receptor atoms j = 256 t + l; it walks the tiles t of its workgroup's list in ascending order and,
//                       inside a tile, the ligand atoms in ascending i (read from LDS by broadcast).  A pair without
//                       contact adds nothing.  The seven sums are reduced by a fixed butterfly per wave and the tree
//                       (w0 + w1) + (w2 + w3), read by every lane, so every lane holds the same state and takes the same
//                       branch.  No atomics.
//                       A trial rotates by s_r about the torque and moves by s_t along the force; it is kept only if P
//                       strictly decreases (then both lengths x 1.2; else both x 0.5); a trial whose centroid would lie
//                       more than max_shift from c is rejected unevaluated, the same way.  The walk ends after `steps`
//                       trials or as soon as P == 0.  G is re-orthonormalised as each trial is formed (Gram-Schmidt,
//                       `rotate_about<true>`), so the pose that was evaluated is the pose returned.
//   Tile list:          with `tile_sphere` the workgroup keeps only the tiles whose bounding sphere comes within reach of
//                       the ligand (`mcg_tiles::build_tile_list`, mcg_receptor_tiles.h), with the reach
//                       (rho + max_shift) + max r_i, rho the ligand's radius about c.  Every pair of a tile left out
//                       has h = 0 in every pose the walk can evaluate, and pairs with h = 0 are not summed, so the list
//                       changes no bit of the result.
// A molecule's result depends on its own atoms and the receptor array only: bit-identical whatever the batch, row or width.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"
#include "mcg_rigid_step.h"
#include "mcg_receptor_tiles.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;
using namespace mcg_rigid;     // the trial, the step lengths, the returned transform, the sums: one text for every walk
using namespace mcg_tiles;     // the centroid and the tile list, shared by every kernel that reaches a receptor

constexpr int RL_THREADS = TILE_ATOMS;        // lanes per workgroup = receptor atoms per tile
constexpr int RL_WAVES = RL_THREADS / 64;
constexpr float RL_STEP_ROT = 0.05f;          // initial rotation step, rad
constexpr float RL_STEP_TRANS = 0.25f;        // initial translation step, Angstrom

struct ReliefShared {
    float x[MAX_ATOMS][3];        // the input rows
    float r[MAX_ATOMS][3];        // x minus the atom centroid
    float4 rr[MAX_ATOMS];         // r @ G of the pose being evaluated: the atom seen from p
    float4 xp[MAX_ATOMS];         // that pose itself, r @ G + p; .w = r_i - margin
    float red[RL_WAVES][7];
    float c[3];
    float reach[RL_WAVES][2];     // per wave: max |r_i|^2, max r_i
    TileList<MAX_RECEPTOR_TILES> tiles;
};

// P / force / torque of the pose (G, p) into v[7]; identical in every lane.
__device__ void evaluate(ReliefShared& s, const float4* __restrict__ rec, int R, int na, const float* G, const float* p,
                         float* v) {
    const int tid = threadIdx.x;
    if (tid < na) {
        float o[3];
        rotate_row(s.r[tid][0], s.r[tid][1], s.r[tid][2], G, o);
        s.rr[tid] = make_float4(o[0], o[1], o[2], 0.f);
        s.xp[tid].x = o[0] + p[0]; s.xp[tid].y = o[1] + p[1]; s.xp[tid].z = o[2] + p[2];
    }
    __syncthreads();
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nt = s.tiles.n_tiles;
    for (int k = 0; k < nt; ++k) {
        const int j = (int)s.tiles.list[k] * RL_THREADS + tid;
        if (j >= R) continue;                                      // the last tile's tail
        const float4 y = rec[j];
        for (int i = 0; i < na; ++i) {
            const float4 x = s.xp[i];
            const float dx = x.x - y.x, dy = x.y - y.y, dz = x.z - y.z;
            const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
            const float h = (x.w + y.w) - d;
            if (h > 0.f) {
                const float4 a = s.rr[i];
                const float g = d > 0.f ? (h + h) / d : 0.f;
                const float fx = g * dx, fy = g * dy, fz = g * dz;
                acc[0] = __builtin_fmaf(h, h, acc[0]);
                acc[1] += fx; acc[2] += fy; acc[3] += fz;
                acc[4] += a.y * fz - a.z * fy;
                acc[5] += a.z * fx - a.x * fz;
                acc[6] += a.x * fy - a.y * fx;
            }
        }
    }
    block_sums<7>(acc, s.red, v);
}

__global__ __launch_bounds__(RL_THREADS) void k_receptor_relieve(
    const float* __restrict__ lig, const float* __restrict__ lig_r, const int* __restrict__ n_nodes, int N,
    const float4* __restrict__ rec, int R, const float4* __restrict__ tile_sphere, int steps, float margin,
    float max_shift, float* __restrict__ coords_out, float* __restrict__ xform_out, float* __restrict__ stats_out,
    float* __restrict__ gradient_out) {
    __shared__ ReliefShared s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int na = atom_count(n_nodes[b], N);
    const float* xin = lig + (size_t)b * N * 3;
    float* xout = coords_out + (size_t)b * N * 3;
    bool bad = false;
    float ri = 0.f;
    if (tid < na) {
        for (int k = 0; k < 3; ++k) s.x[tid][k] = xin[tid * 3 + k];
        ri = lig_r[(size_t)b * N + tid];
        s.xp[tid].w = ri - margin;
        bad = !(isfinite(s.x[tid][0]) && isfinite(s.x[tid][1]) && isfinite(s.x[tid][2]));
    }
    if (__syncthreads_or(bad) != 0 || na == 0) {                   // left exactly as it came, NaN transform and stats
        for (int q = tid; q < N * 3; q += RL_THREADS) xout[q] = q < na * 3 ? s.x[q / 3][q % 3] : 0.f;
        if (tid < 12) xform_out[(size_t)b * 12 + tid] = __builtin_nanf("");
        if (tid < 4) stats_out[(size_t)b * 4 + tid] = __builtin_nanf("");
        if (gradient_out != nullptr && tid < 6) gradient_out[(size_t)b * 6 + tid] = __builtin_nanf("");
        return;
    }
    atom_centroid(&s.x[0][0], 3, na, na, s.c);
    const float c[3] = {s.c[0], s.c[1], s.c[2]};
    float reach[2] = {0.f, ri};               // |r_i|^2 and r_i: the ligand's radius about c, its largest atom radius
    if (tid < na) {
        for (int k = 0; k < 3; ++k) s.r[tid][k] = s.x[tid][k] - c[k];
        reach[0] = (s.r[tid][0] * s.r[tid][0] + s.r[tid][1] * s.r[tid][1]) + s.r[tid][2] * s.r[tid][2];
    }
    block_max4<2>(s.reach, reach, tid & 63, tid >> 6);
    build_tile_list(s.tiles, tile_sphere, (R + RL_THREADS - 1) / RL_THREADS, c[0], c[1], c[2],
                    (sqrtf(reach[0]) + max_shift) + reach[1]);

    float G[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, p[3] = {c[0], c[1], c[2]};
    float cur[7];
    evaluate(s, rec, R, na, G, p, cur);
    const float p_start = cur[0];
    if (gradient_out != nullptr && tid < 6) gradient_out[(size_t)b * 6 + tid] = cur[1 + tid];
    StepLengths len = {RL_STEP_ROT, RL_STEP_TRANS};
    int accepted = 0;
    for (int it = 0; it < steps && cur[0] > 0.f; ++it) {
        float Gn[9], pn[3];
        const float fn = norm3(cur + 1), tn = norm3(cur + 4);
        if (tn > 0.f) {
            rotate_about<true>(G, cur[4] / tn, cur[5] / tn, cur[6] / tn, len.rot, Gn);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) Gn[k] = G[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) pn[k] = step_along(p[k], cur[1 + k], fn, fn > 0.f, len.trans);
        bool take = within_shift(pn, c[0], c[1], c[2], max_shift);
        float nxt[7];
        if (take) {                           // the same in every lane
            evaluate(s, rec, R, na, Gn, pn, nxt);
            take = nxt[0] < cur[0];
        }
        if (take) {
            keep_trial<7>(G, p, cur, Gn, pn, nxt);
            len.grow();
            ++accepted;
        } else {
            len.shrink();
        }
    }
    float* xf = xform_out + (size_t)b * 12;
    float* stats = stats_out + (size_t)b * 4;
    if (accepted == 0) {                      // nothing moved: the input's bits, the identity
        for (int q = tid; q < N * 3; q += RL_THREADS) xout[q] = q < na * 3 ? s.x[q / 3][q % 3] : 0.f;
        if (tid < 12) xf[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.f : 0.f;
        if (tid == 0) { stats[0] = p_start; stats[1] = p_start; stats[2] = 0.f; stats[3] = 0.f; }
        return;
    }
    __syncthreads();                          // the last trial's pose is read by every lane
    if (tid < na) {                           // the accepted pose, as it was evaluated: (x - c) @ G + p
        float o[3];
        rotate_row(s.r[tid][0], s.r[tid][1], s.r[tid][2], G, o);
        float d2 = 0.f;
        for (int k = 0; k < 3; ++k) {
            o[k] = o[k] + p[k];               // the bits `evaluate` saw
            const float d = o[k] - s.x[tid][k];
            d2 += d * d;
            xout[tid * 3 + k] = o[k];
        }
        s.r[tid][0] = d2;                     // this atom's own row: nobody else reads it
    }
    for (int q = na * 3 + tid; q < N * 3; q += RL_THREADS) xout[q] = 0.f;
    __syncthreads();
    if (tid == 0) {
        write_transform(G, p, c[0], c[1], c[2], xf);
        float sum = 0.f;
        for (int i = 0; i < na; ++i) sum += s.r[i][0];             // in atom order
        stats[0] = p_start; stats[1] = cur[0]; stats[2] = (float)accepted; stats[3] = sqrtf(sum / (float)na);
    }
}

}  // namespace

extern "C" int mcg_receptor_relieve(const float* lig_xyz, const float* lig_radius, const int32_t* n_nodes_dev, int B,
                                    int N, const float* rec_xyzr, int R, const float* tile_sphere, int steps,
                                    float margin, float max_shift, float* coords_out, float* xform_out, float* stats_out,
                                    float* gradient_out, void* stream) {
    static_assert(WALK_MAX_STEPS == 1024 && MAX_ATOMS == 64, "the bounds the message below states");
    if (!lig_xyz || !lig_radius || !n_nodes_dev || !rec_xyzr || !coords_out || !xform_out || !stats_out || B < 1 ||
        B > MCG_RECEPTOR_MAX_B || N < 1 || N > MAX_ATOMS || R < 1 || R > MCG_RECEPTOR_MAX_ATOMS || steps < 0 ||
        steps > WALK_MAX_STEPS || !(margin >= 0.f) || !isfinite(margin) || !(max_shift >= 0.f) || !isfinite(max_shift)) {
        mcg_set_error("mcg_receptor_relieve: bad arguments (non-null buffers, 1 <= B <= %d, 1 <= N <= 64, 1 <= R <= %d, "
                      "0 <= steps <= 1024, margin and max_shift finite and >= 0)", MCG_RECEPTOR_MAX_B,
                      MCG_RECEPTOR_MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    hipLaunchKernelGGL(k_receptor_relieve, dim3(B), dim3(RL_THREADS), 0, (hipStream_t)stream, lig_xyz, lig_radius,
                       n_nodes_dev, N, (const float4*)rec_xyzr, R, (const float4*)tile_sphere, steps, margin, max_shift,
                       coords_out, xform_out, stats_out, gradient_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
