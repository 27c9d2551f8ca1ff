// Flexible pose ("Flexible pose"; the definition is the docstring of
// `interactions.optimise_pose_flexible`, the C contract include/mlconfgen_hip_flex.h): the walk of mcg_pose_optimise.hip
// with the molecule's rotatable bonds turned beside the rigid move, and an intramolecular guard.
// THE PACKAGE'S OWN procedure: not a docking run, not AutoDock Vina's optimiser, no hydrogens, no global search.
//   k_torsion_tree:          one 64-lane wave per molecule, lane = atom.  The neighbour masks go to LDS; a lane finds its ring
//                            bonds by its own floods (mcg_ring_bonds.h), proposes the bonds (a, j > a) that are torsions, takes
//                            its slots behind the lanes in front of it (ascending (min, max) order) and floods the two sides
//                            of each bond it owns.  Integer work only.
//   k_receptor_optimise_flex: one 256-lane workgroup per molecule, laid out as `k_receptor_optimise`: lane l holds atom
//                            a = l & 63, so EVERY wave holds all 64 atoms and the ends of a torsion axis travel by `__shfl`
//                            inside a wave; wave w = l >> 6 walks the receptor atoms j = w, w + 4, ... of each kept tile and
//                            the atoms j = w, w + 4, ... of the 64 x 64 clash loop out of LDS.  The four waves' partials of an
//                            atom are combined as (w0 + w1) + (w2 + w3); wave 0 forms the torque, CLASH and one masked
//                            butterfly per torsion.  Every lane reads the sums back, holds the same state and takes the same
//                            branch.  No atomics.  The receptor loop, the pair arithmetic, the tile list and the rigid trial
//                            are the shared headers' text, in the order `k_receptor_optimise` uses them, so a molecule
//                            without a torsion gets that kernel's bits.  That part of this file is kept in step with
//                            mcg_pose_optimise.hip BY HAND ("Shared device text", says why it is not
//                            one body); the step constants and the entry's argument check are mcg_receptor_walk.h's.
//   Tile list:               built once with the reach (rho0 + 2 + 8) + max_shift: a trial with an atom further than
//                            rho0 + 2 from p in the molecule frame is rejected unevaluated.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"
#include "mcg_rigid_step.h"
#include "mcg_receptor_tiles.h"
#include "mcg_interaction_pair.h"
#include "mcg_receptor_walk.h"
#include "mcg_graph_rules.h"
#include "mcg_ring_bonds.h"
#include "../../include/mlconfgen_hip_flex.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;
using namespace mcg_rigid;
using namespace mcg_tiles;
using namespace mcg_interaction;
using namespace mcg_receptor_walk;   // the step constants and the argument check, shared with k_receptor_optimise

constexpr int FX_MAXW = MCG_FLEX_MAX_ATOMS;
constexpr int FX_T = MCG_FLEX_MAX_TORSIONS;
static_assert(FX_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");
static_assert(MAX_ATOMS == 64, "the pose walk holds the same 64 atoms");

// ---------------------------------------------------------------------------------------------------- the torsion tree
struct TreeShared {
    __attribute__((aligned(16))) uint8_t code[FX_MAXW * MCG_CODE_STRIDE];
    unsigned long long nbr[FX_MAXW];
    unsigned long long t_side[FX_T];
    int z[FX_MAXW], deg[FX_MAXW], carbonyl[FX_MAXW], cnt[FX_MAXW];
    int t_atoms[FX_T][2];
};

__global__ __launch_bounds__(FX_MAXW) void k_torsion_tree(
        const int32_t* __restrict__ z, const int8_t* __restrict__ bonds, const int32_t* __restrict__ n_nodes, int W,
        int32_t* __restrict__ torsion_atoms, unsigned long long* __restrict__ side_mask,
        unsigned long long* __restrict__ near_mask, int32_t* __restrict__ counts) {
    __shared__ TreeShared s;
    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), W);
    const bool real = a < n;

    mcg_stage_codes(s.code, bonds + (size_t)b * W * W, W, n, a, FX_MAXW);
    if (a < FX_T) {
        s.t_atoms[a][0] = -1; s.t_atoms[a][1] = -1;
        s.t_side[a] = 0ull;
    }
    __syncthreads();

    const McgBondTally tally = mcg_bond_tally(s.code + a * MCG_CODE_STRIDE, real ? n : 0);
    const unsigned long long mine = tally.mask, m1 = tally.m1, m2 = tally.m2;
    const int za = real ? z[(size_t)b * W + a] : 0;
    s.nbr[a] = mine;
    s.deg[a] = tally.deg;
    s.z[a] = za;
    __syncthreads();

    bool polar2 = false;                               // a code-2 bond to N, O or S
    for (unsigned long long g = m2; g != 0ull; g &= g - 1ull) {
        const int zj = s.z[low_bit(g)];
        polar2 = polar2 || zj == 7 || zj == 8 || zj == 16;
    }
    s.carbonyl[a] = (za == 6 && polar2) ? 1 : 0;
    const McgRingBonds rb = mcg_ring_bonds_of(s.nbr, a, mine, n);
    unsigned long long near = 0ull;
    if (real) {
        near = (1ull << a) | mine;
        for (unsigned long long g = mine; g != 0ull; g &= g - 1ull) near |= s.nbr[low_bit(g)];
    }
    if (a < W) near_mask[(size_t)b * W + a] = near;
    __syncthreads();

    unsigned long long cand = 0ull;                    // the torsions (a, j), j > a
    if (real && s.deg[a] >= 2) {
        for (unsigned long long g = m1 & ~rb.mask & ~low_bits(a + 1); g != 0ull; g &= g - 1ull) {
            const int j = low_bit(g);
            const bool amide = (s.carbonyl[a] != 0 && s.z[j] == 7) || (s.carbonyl[j] != 0 && za == 7);
            if (s.deg[j] >= 2 && !amide) cand |= 1ull << j;
        }
    }
    s.cnt[a] = __popcll(cand);
    __syncthreads();
    int k = 0;
    for (int i = 0; i < a; ++i) k += s.cnt[i];
    for (unsigned long long g = cand; g != 0ull; g &= g - 1ull, ++k) {
        if (k >= FX_T) break;
        const int j = low_bit(g);
        const unsigned long long side_j = mcg_flood(s.nbr, 1ull << j, 1ull << a, n),
                                 side_a = mcg_flood(s.nbr, 1ull << a, 1ull << j, n);
        const bool j_moves = __popcll(side_j) <= __popcll(side_a);            // a tie: the higher-indexed end's part
        s.t_atoms[k][0] = j_moves ? a : j;
        s.t_atoms[k][1] = j_moves ? j : a;
        s.t_side[k] = j_moves ? side_j : side_a;
    }
    __syncthreads();
    if (a < FX_T) {
        torsion_atoms[((size_t)b * FX_T + a) * 2] = s.t_atoms[a][0];
        torsion_atoms[((size_t)b * FX_T + a) * 2 + 1] = s.t_atoms[a][1];
        side_mask[(size_t)b * FX_T + a] = s.t_side[a];
    }
    if (a == 0) {
        int found = 0;
        for (int i = 0; i < FX_MAXW; ++i) found += s.cnt[i];
        counts[(size_t)b * 2] = found;
        counts[(size_t)b * 2 + 1] = min(found, FX_T);
    }
}

// ---------------------------------------------------------------------------------------------------- the walk
constexpr int FX_SUMS = 11;                   // g1, g2, rep, hyd, hb, F[3], torque[3]
constexpr int FX_RED = FX_SUMS + 1 + FX_T;    // ... CLASH, tau[16]
constexpr int FX_PART = 12;                   // per wave and atom: the rigid kernel's eight, the clash energy and force
constexpr int FX_TRACE = MCG_FLEX_TRACE;
constexpr int FX_STATS = MCG_FLEX_STATS;
constexpr int FX_GRAD = MCG_FLEX_GRADIENT;
static_assert(FX_TRACE == 24 + 1 + FX_T + 2 && FX_GRAD == 6 + FX_T, "the header's widths");

struct FlexShared {
    float4 tile[IX_THREADS];                  // the staged receptor tile: x, y, z, R_j
    unsigned char type[IX_THREADS];
    float part[IX_WAVES][MAX_ATOMS][FX_PART];
    float4 q[MAX_ATOMS];                      // the molecule-frame atoms of the state being evaluated, and c_i
    float red[FX_RED];
    float c[3];
    float reach[IX_WAVES][1];
    int ta[FX_T], tb[FX_T];
    unsigned long long side[FX_T];
    TileList<MAX_RECEPTOR_TILES> tiles;
};

// What one lane holds of its atom: the molecule-frame position, the world position and the lever seen from p.
struct FlexAtom {
    float qx, qy, qz, x, y, z, ux, uy, uz;
};

// One evaluation of the state whose atom a this lane holds: v[0..10] the rigid kernel's eleven sums in its order, v[11]
// CLASH, v[12 + k] tau_k (0 for k >= nt); identical in every lane.
__device__ void evaluate_flex(FlexShared& s, const float4* __restrict__ rec, const unsigned char* __restrict__ rec_t, int R,
                              bool real, int na, const FlexAtom& at, float ri, unsigned ti, float cr,
                              unsigned long long near, const float* G, int nt, float* v) {
    const int tid = threadIdx.x, a = tid & 63, w = tid >> 6;
    if (w == 0) s.q[a] = make_float4(at.qx, at.qy, at.qz, cr);
    __syncthreads();
    // the clash loop: this wave's j of the 64 x 64 pairs, energy on i < j, force on both
    float cl[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = w; j < na; j += IX_WAVES) {
        const float4 o = s.q[j];
        const float dx = at.qx - o.x, dy = at.qy - o.y, dz = at.qz - o.z;
        const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float e = (cr + o.w) - r;
        if (real && ((near >> j) & 1ull) == 0ull && e > 0.f) {
            if (j > a) cl[0] += e * e;
            const float g = r > 0.f ? (e + e) / r : 0.f;
            cl[1] += g * dx; cl[2] += g * dy; cl[3] += g * dz;
        }
    }
    // the receptor loop: `k_receptor_optimise`'s
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int nhb = 0;
    const int ntile = s.tiles.n_tiles;
    for (int k = 0; k < ntile; ++k) {
        const int j0 = (int)s.tiles.list[k] * IX_THREADS;
        const int cnt = min(IX_THREADS, R - j0);
        if (tid < cnt) {
            s.tile[tid] = rec[j0 + tid];
            s.type[tid] = rec_t[j0 + tid];
        }
        __syncthreads();
        for (int jj = w; jj < cnt; jj += IX_WAVES) {
            const float4 o = s.tile[jj];
            float dx, dy, dz;
            const float r2 = pair_r2(at.x, at.y, at.z, o, dx, dy, dz);
            const bool counts = real && r2 < IX_CUTOFF2;
            if (__ballot(counts) == 0ull) continue;
            if (counts) {
                const unsigned tj = s.type[jj];
                const PairValues pv = pair_terms(r2, ri, o.w, ti, tj, acc, nhb);
                const float g = pv.r > 0.f ? -pair_slope(pv, ti, tj) / pv.r : 0.f;
                acc[5] += g * dx; acc[6] += g * dy; acc[7] += g * dz;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s.part[w][a][k] = acc[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) s.part[w][a][8 + k] = cl[k];
    __syncthreads();
    if (w == 0) {
        float t[FX_SUMS], c4[4];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = (s.part[0][a][k] + s.part[1][a][k]) + (s.part[2][a][k] + s.part[3][a][k]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            c4[k] = (s.part[0][a][8 + k] + s.part[1][a][8 + k]) + (s.part[2][a][8 + k] + s.part[3][a][8 + k]);
        t[8] = at.uy * t[7] - at.uz * t[6];
        t[9] = at.uz * t[5] - at.ux * t[7];
        t[10] = at.ux * t[6] - at.uy * t[5];
        // this atom's whole force in the world frame: the receptor's and 0.840 x the clash force, rotated as the atom is
        float fw[3];
        rotate_row(c4[1], c4[2], c4[3], G, fw);
        const float fx = t[5] + W_REP * fw[0], fy = t[6] + W_REP * fw[1], fz = t[7] + W_REP * fw[2];
#pragma unroll
        for (int k = 0; k < FX_SUMS; ++k)
            for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_xor(t[k], o, 64);
        float ce = c4[0];
        for (int o = 32; o > 0; o >>= 1) ce += __shfl_xor(ce, o, 64);
        float tau[FX_T];
#pragma unroll
        for (int k = 0; k < FX_T; ++k) {
            tau[k] = 0.f;
            if (k < nt) {                     // the same in every lane
                const int ia = s.ta[k], ib = s.tb[k];
                const float ax = __shfl(at.x, ia, 64), ay = __shfl(at.y, ia, 64), az = __shfl(at.z, ia, 64);
                const float bx = __shfl(at.x, ib, 64), by = __shfl(at.y, ib, 64), bz = __shfl(at.z, ib, 64);
                float n[3] = {bx - ax, by - ay, bz - az};
                const float len = norm3(n);
                const float rx = at.x - bx, ry = at.y - by, rz = at.z - bz;
                const float mx = ry * fz - rz * fy, my = rz * fx - rx * fz, mz = rx * fy - ry * fx;
                const bool in = real && ((s.side[k] >> a) & 1ull) != 0ull;
                float m = in ? ((n[0] / len) * mx + (n[1] / len) * my) + (n[2] / len) * mz : 0.f;
                for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
                tau[k] = m;
            }
        }
        if (a == 0) {
#pragma unroll
            for (int k = 0; k < FX_SUMS; ++k) s.red[k] = t[k];
            s.red[FX_SUMS] = ce;
#pragma unroll
            for (int k = 0; k < FX_T; ++k) s.red[FX_SUMS + 1 + k] = tau[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FX_RED; ++k) v[k] = s.red[k];
}

__global__ __launch_bounds__(IX_THREADS) void k_receptor_optimise_flex(
    const float* __restrict__ lig, const float* __restrict__ lig_r, const unsigned char* __restrict__ lig_t,
    const int* __restrict__ n_nodes, int N, const float4* __restrict__ rec, const unsigned char* __restrict__ rec_t, int R,
    const float4* __restrict__ tile_sphere, int steps, float max_shift, const float* __restrict__ clash_radius,
    const int32_t* __restrict__ torsion_atoms, const unsigned long long* __restrict__ side_mask,
    const unsigned long long* __restrict__ near_mask, const int32_t* __restrict__ n_torsions,
    float* __restrict__ coords_out, float* __restrict__ xform_out, float* __restrict__ stats_out,
    float* __restrict__ angles_out, float* __restrict__ gradient_out, float* __restrict__ trace_out) {
    __shared__ FlexShared s;
    const int b = blockIdx.x, tid = threadIdx.x, a = tid & 63, w = tid >> 6;
    const int na = atom_count(n_nodes[b], N);
    const float* xin = lig + (size_t)b * N * 3;
    float* xout = coords_out + (size_t)b * N * 3;
    float* xf = xform_out + (size_t)b * 12;
    float* stats = stats_out + (size_t)b * FX_STATS;
    float* angles = angles_out + (size_t)b * FX_T;
    float* trace = trace_out != nullptr ? trace_out + (size_t)b * steps * FX_TRACE : nullptr;
    const bool real = a < na;
    float x0 = 0.f, y0 = 0.f, z0 = 0.f, ri = 0.f, cr = 0.f;
    unsigned ti = 0u;
    unsigned long long near = 0ull;
    if (real) {
        x0 = xin[a * 3]; y0 = xin[a * 3 + 1]; z0 = xin[a * 3 + 2];
        ri = lig_r[(size_t)b * N + a];
        ti = lig_t[(size_t)b * N + a];
        cr = clash_radius[(size_t)b * N + a];
        near = near_mask[(size_t)b * N + a];
    }
    const bool bad = real && !(isfinite(x0) && isfinite(y0) && isfinite(z0));
    if (__syncthreads_or(bad) != 0 || na == 0) {                   // left exactly as it came, NaN everywhere else
        if (w == 0 && a < N) {
            xout[a * 3] = x0; xout[a * 3 + 1] = y0; xout[a * 3 + 2] = z0;       // a padded slot holds 0
        }
        if (tid < 12) xf[tid] = __builtin_nanf("");
        if (tid < FX_STATS) stats[tid] = __builtin_nanf("");
        if (tid < FX_T) angles[tid] = __builtin_nanf("");
        if (gradient_out != nullptr && tid < FX_GRAD) gradient_out[(size_t)b * FX_GRAD + tid] = __builtin_nanf("");
        if (trace != nullptr)
            for (int q = tid; q < steps * FX_TRACE; q += IX_THREADS) trace[q] = 0.f;
        return;
    }
    if (w == 0) s.part[0][a][0] = x0, s.part[0][a][1] = y0, s.part[0][a][2] = z0;   // borrowed for the centroid
    if (tid < FX_T) {
        s.ta[tid] = torsion_atoms[((size_t)b * FX_T + tid) * 2];
        s.tb[tid] = torsion_atoms[((size_t)b * FX_T + tid) * 2 + 1];
        s.side[tid] = side_mask[(size_t)b * FX_T + tid];
    }
    __syncthreads();
    if (tid < 3) {                            // atom centroid, summed in atom order
        float acc = 0.f;
        for (int i = 0; i < na; ++i) acc += s.part[0][i][tid];
        s.c[tid] = acc / (float)na;
    }
    int nt = min(max(n_torsions[b], 0), FX_T);
    for (int k = 0; k < nt; ++k) {            // cut at the first slot that does not name two atoms of this row
        const int ia = s.ta[k], ib = s.tb[k];
        if (ia < 0 || ia >= na || ib < 0 || ib >= na || ia == ib) nt = k;
    }
    __syncthreads();
    const float c[3] = {s.c[0], s.c[1], s.c[2]};
    float rx = 0.f, ry = 0.f, rz = 0.f, rho2 = 0.f;
    if (real) {
        rx = x0 - c[0]; ry = y0 - c[1]; rz = z0 - c[2];
        rho2 = (rx * rx + ry * ry) + rz * rz;
    }
    block_max4<1>(s.reach, &rho2, a, w);
    const float qlim = sqrtf(rho2) + FX_MARGIN;
    build_tile_list(s.tiles, tile_sphere, (R + IX_THREADS - 1) / IX_THREADS, c[0], c[1], c[2],
                    (qlim + IX_CUTOFF) + max_shift);

    float G[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, p[3] = {c[0], c[1], c[2]};
    float cur[FX_RED];
    FlexAtom at = {rx, ry, rz, x0, y0, z0, rx, ry, rz};            // the input rows as they came, seen from c
    float cx = x0, cy = y0, cz = z0;          // this lane's atom in the state that holds
    float qx = rx, qy = ry, qz = rz;
    evaluate_flex(s, rec, rec_t, R, real, na, at, ri, ti, cr, near, G, nt, cur);
    float w_cur = weighted(cur);
    const float w_start = w_cur, c_start = cur[FX_SUMS];
    if (gradient_out != nullptr && tid == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) gradient_out[(size_t)b * FX_GRAD + k] = cur[5 + k];
#pragma unroll
        for (int k = 0; k < FX_T; ++k) gradient_out[(size_t)b * FX_GRAD + 6 + k] = cur[FX_SUMS + 1 + k];
    }
    StepLengths len = {RW_STEP_ROT, RW_STEP_TRANS};
    float s_tau = FX_STEP_TAU;
    float turned[FX_T];
#pragma unroll
    for (int k = 0; k < FX_T; ++k) turned[k] = 0.f;
    int trials = 0, kept = 0;
    for (; trials < steps && !(len.trans < RW_MIN_TRANS); ++trials) {
        float Gn[9], pn[3];
        const float fn = norm3(cur + 5), tn = norm3(cur + 8);
        const bool moves = fn > 0.f && isfinite(fn), turns = tn > 0.f && isfinite(tn);
        float mt = 0.f;
        bool tau_ok = true;
#pragma unroll
        for (int k = 0; k < FX_T; ++k) {
            const float m = fabsf(cur[FX_SUMS + 1 + k]);
            tau_ok = tau_ok && isfinite(m);
            mt = fmaxf(mt, m);
        }
        const bool twists = nt > 0 && tau_ok && mt > 0.f;
        if (!moves && !turns && !twists) break;                    // nothing to follow: the walk ends, the trial is not counted
        // the torsions, in ascending order, on a copy of q
        float tqx = qx, tqy = qy, tqz = qz, delta[FX_T];
#pragma unroll
        for (int k = 0; k < FX_T; ++k) {
            delta[k] = 0.f;
            if (twists && k < nt) {           // the same in every lane
                const float d = s_tau * (cur[FX_SUMS + 1 + k] / mt);
                delta[k] = d;
                if (d != 0.f) {               // a zero angle leaves the bits
                    const int ia = s.ta[k], ib = s.tb[k];
                    const float ax = __shfl(tqx, ia, 64), ay = __shfl(tqy, ia, 64), az = __shfl(tqz, ia, 64);
                    const float bx = __shfl(tqx, ib, 64), by = __shfl(tqy, ib, 64), bz = __shfl(tqz, ib, 64);
                    float n[3] = {bx - ax, by - ay, bz - az}, o[3];
                    const float ln = norm3(n);
                    turn_about_line(tqx, tqy, tqz, bx, by, bz, n[0] / ln, n[1] / ln, n[2] / ln, d, o);
                    if (real && ((s.side[k] >> a) & 1ull) != 0ull) {
                        tqx = o[0]; tqy = o[1]; tqz = o[2];
                    }
                }
            }
        }
        if (turns) {
            rotate_about<true>(G, cur[8] / tn, cur[9] / tn, cur[10] / tn, len.rot, Gn);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) Gn[k] = G[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) pn[k] = step_along(p[k], cur[5 + k], fn, moves, len.trans);
        const bool outside = real && ((tqx * tqx + tqy * tqy) + tqz * tqz) > qlim * qlim;
        const bool evaluated = within_shift(pn, c[0], c[1], c[2], max_shift) && __ballot(outside) == 0ull;
        bool take = false;
        float nxt[FX_RED], w_nxt = 0.f, c_nxt = 0.f;
        FlexAtom tr = {tqx, tqy, tqz, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (evaluated) {                      // the same in every lane
            float u[3] = {0.f, 0.f, 0.f};
            if (real) {
                rotate_row(tqx, tqy, tqz, Gn, u);
                tr.x = u[0] + pn[0]; tr.y = u[1] + pn[1]; tr.z = u[2] + pn[2];
            }
            tr.ux = u[0]; tr.uy = u[1]; tr.uz = u[2];
            evaluate_flex(s, rec, rec_t, R, real, na, tr, ri, ti, cr, near, Gn, nt, nxt);
            w_nxt = weighted(nxt);
            c_nxt = nxt[FX_SUMS];
            take = ((w_nxt - w_cur) + W_REP * (c_nxt - cur[FX_SUMS])) < 0.f;
        }
        if (trace != nullptr && tid == 0) {
            float* row = trace + (size_t)trials * FX_TRACE;
#pragma unroll
            for (int k = 0; k < 6; ++k) row[k] = cur[5 + k];
            row[6] = len.rot; row[7] = len.trans;
#pragma unroll
            for (int k = 0; k < 9; ++k) row[8 + k] = Gn[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) row[17 + k] = pn[k];
            row[20] = w_nxt; row[21] = evaluated ? 1.f : 0.f; row[22] = take ? 1.f : 0.f; row[23] = w_cur;
            row[24] = s_tau;
#pragma unroll
            for (int k = 0; k < FX_T; ++k) row[25 + k] = cur[FX_SUMS + 1 + k];
            row[41] = cur[FX_SUMS]; row[42] = c_nxt;
        }
        if (take) {
            keep_trial<FX_RED>(G, p, cur, Gn, pn, nxt);
            w_cur = w_nxt;
            cx = tr.x; cy = tr.y; cz = tr.z;
            qx = tqx; qy = tqy; qz = tqz;
#pragma unroll
            for (int k = 0; k < FX_T; ++k) turned[k] += delta[k];
            len.grow();
            s_tau *= WALK_GROW;
            ++kept;
        } else {
            len.shrink();
            s_tau *= WALK_SHRINK;
        }
    }
    if (trace != nullptr)                     // rows beyond the last trial are zero
        for (int q = trials * FX_TRACE + tid; q < steps * FX_TRACE; q += IX_THREADS) trace[q] = 0.f;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < FX_T; ++k) angles[k] = turned[k];
    }
    if (kept == 0) {                          // nothing moved: the input's bits, the identity
        if (w == 0 && a < N) {
            xout[a * 3] = x0; xout[a * 3 + 1] = y0; xout[a * 3 + 2] = z0;
        }
        if (tid < 12) xf[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.f : 0.f;
        if (tid == 0) {
            stats[0] = w_start; stats[1] = w_start; stats[2] = (float)trials; stats[3] = 0.f;
            stats[4] = 0.f; stats[5] = len.trans; stats[6] = c_start; stats[7] = c_start;
            stats[8] = (float)nt; stats[9] = 0.f; stats[10] = 0.f; stats[11] = 0.f;
        }
        return;
    }
    if (w == 0) {                             // the kept state, as it was evaluated
        float d2 = 0.f, e2 = 0.f;
        if (real) {
            const float ex = cx - x0, ey = cy - y0, ez = cz - z0;
            d2 = (ex * ex + ey * ey) + ez * ez;
            const float hx = qx - rx, hy = qy - ry, hz = qz - rz;
            e2 = (hx * hx + hy * hy) + hz * hz;
        }
        if (a < N) {
            xout[a * 3] = cx; xout[a * 3 + 1] = cy; xout[a * 3 + 2] = cz;       // a padded slot holds 0
        }
        s.part[0][a][0] = d2;                 // every evaluation is over: nobody else reads it
        s.part[0][a][1] = e2;
    }
    __syncthreads();
    if (tid == 0) {
        write_transform(G, p, c[0], c[1], c[2], xf);
        float sum = 0.f, sumq = 0.f;
        for (int i = 0; i < na; ++i) sum += s.part[0][i][0];       // in atom order
        for (int i = 0; i < na; ++i) sumq += s.part[0][i][1];
        stats[0] = w_start; stats[1] = w_cur; stats[2] = (float)trials; stats[3] = (float)kept;
        stats[4] = sqrtf(sum / (float)na); stats[5] = len.trans; stats[6] = c_start; stats[7] = cur[FX_SUMS];
        stats[8] = (float)nt; stats[9] = sqrtf(sumq / (float)na); stats[10] = 0.f; stats[11] = 0.f;
    }
}

}  // namespace

extern "C" int mcg_torsion_tree(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                                int32_t* torsion_atoms, uint64_t* side_mask, uint64_t* near_mask, int32_t* counts,
                                void* stream) {
    if (!z || !bonds || !n_nodes_dev || !torsion_atoms || !side_mask || !near_mask || !counts || B < 0 ||
        B > MCG_FLEX_MAX_B || W < 1 || W > FX_MAXW) {
        mcg_set_error("mcg_torsion_tree: bad arguments (non-null z, bonds, n_nodes, torsion_atoms, side_mask, near_mask and "
                      "counts, 0 <= B <= %d, 1 <= W <= %d)", MCG_FLEX_MAX_B, FX_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_torsion_tree, dim3((unsigned)B), dim3(FX_MAXW), 0, (hipStream_t)stream, z, bonds, n_nodes_dev, W,
                       torsion_atoms, reinterpret_cast<unsigned long long*>(side_mask),
                       reinterpret_cast<unsigned long long*>(near_mask), counts);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_receptor_optimise_flex(const float* lig_xyz, const float* lig_radius, const uint8_t* lig_type,
                                          const int32_t* n_nodes_dev, int B, int N, const float* rec_xyzr,
                                          const uint8_t* rec_type, int R, const float* tile_sphere, int steps,
                                          float max_shift, const float* clash_radius, const int32_t* torsion_atoms,
                                          const uint64_t* side_mask, const uint64_t* near_mask, const int32_t* n_torsions,
                                          float* coords_out, float* xform_out, float* stats_out, float* angles_out,
                                          float* gradient_out, float* trace_out, void* stream) {
    const bool buffers = lig_xyz && lig_radius && lig_type && n_nodes_dev && rec_xyzr && rec_type && clash_radius &&
                         torsion_atoms && side_mask && near_mask && n_torsions && coords_out && xform_out && stats_out &&
                         angles_out;
    if (!walk_args_ok("mcg_receptor_optimise_flex", buffers, B, N, R, steps, max_shift)) return MCG_ERR_ARG;
    hipLaunchKernelGGL(k_receptor_optimise_flex, dim3(B), dim3(IX_THREADS), 0, (hipStream_t)stream, lig_xyz, lig_radius,
                       lig_type, n_nodes_dev, N, (const float4*)rec_xyzr, rec_type, R, (const float4*)tile_sphere, steps,
                       max_shift, clash_radius, torsion_atoms, reinterpret_cast<const unsigned long long*>(side_mask),
                       reinterpret_cast<const unsigned long long*>(near_mask), n_torsions, coords_out, xform_out, stats_out,
                       angles_out, gradient_out, trace_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
