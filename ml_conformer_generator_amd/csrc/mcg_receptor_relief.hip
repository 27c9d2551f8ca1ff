// Clash relief ("Clash relief"; the definition is the module docstring of receptor.py): every posed
// molecule is moved as a rigid body out of its steric contacts with the receptor, by the accept / reject walk of
// `k_overlay_refine` turned downhill.
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
//                       trials or as soon as P == 0.  G is re-orthonormalised as each trial is formed (Gram-Schmidt, as
//                       `k_overlay_refine` does once at its end), so the pose that was evaluated is the pose returned.
//   Tile list:          with `tile_sphere` the workgroup keeps only the tiles whose bounding sphere comes within reach of
//                       the ligand: |q_t - c| <= rho + max_shift + max r_i + radius_t + slack, rho the ligand's radius
//                       about c.  Every pair of a tile left out has h = 0 in every pose the walk can evaluate, and pairs
//                       with h = 0 are not summed, so the list changes no bit of the result.
// A molecule's result depends on its own atoms and the receptor array only: bit-identical whatever the batch, row or width.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"
#include "mcg_rigid_step.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;
using namespace mcg_rigid;     // mat3_mul, rodrigues_row, orthonormalise: one text for every rigid-body walk

constexpr int RL_THREADS = 256;               // lanes per workgroup = receptor atoms per tile
constexpr int RL_WAVES = RL_THREADS / 64;
constexpr int RL_MAX_STEPS = 1024;
constexpr int RL_MAX_TILES = MCG_RECEPTOR_MAX_ATOMS / RL_THREADS;
constexpr float RL_STEP_ROT = 0.05f;          // initial rotation step, rad
constexpr float RL_STEP_TRANS = 0.25f;        // initial translation step, Angstrom
constexpr float RL_GROW = 1.2f, RL_SHRINK = 0.5f;
// What the reach of the tile test adds to the exact bound: G drifts from a rotation by a few ulp per accepted step and the
// shift test is itself rounded, both far below 1e-3 of the lengths involved.
constexpr float RL_SLACK_ABS = 0.05f, RL_SLACK_REL = 1e-3f;

static_assert(MCG_RECEPTOR_MAX_ATOMS % RL_THREADS == 0, "the tile list holds every tile of the largest receptor");

struct ReliefShared {
    float x[MAX_ATOMS][3];        // the input rows
    float r[MAX_ATOMS][3];        // x minus the atom centroid
    float4 rr[MAX_ATOMS];         // r @ G of the pose being evaluated: the atom seen from p
    float4 xp[MAX_ATOMS];         // that pose itself, r @ G + p; .w = r_i - margin
    float red[RL_WAVES][7];
    float c[3];
    float reach[RL_WAVES][2];     // per wave: max |r_i|^2, max r_i
    int wave_tiles[RL_WAVES];
    int n_tiles;
    unsigned short tile[RL_MAX_TILES];
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
    const int nt = s.n_tiles;
    for (int k = 0; k < nt; ++k) {
        const int j = (int)s.tile[k] * RL_THREADS + tid;
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
#pragma unroll
    for (int k = 0; k < 7; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) s.red[tid >> 6][k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = (s.red[0][k] + s.red[1][k]) + (s.red[2][k] + s.red[3][k]);
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
    if (tid < 3) {                            // atom centroid, summed in atom order
        float acc = 0.f;
        for (int i = 0; i < na; ++i) acc += s.x[i][tid];
        s.c[tid] = acc / (float)na;
    }
    __syncthreads();
    const float c[3] = {s.c[0], s.c[1], s.c[2]};
    float rho2 = 0.f;
    if (tid < na) {
        for (int k = 0; k < 3; ++k) s.r[tid][k] = s.x[tid][k] - c[k];
        rho2 = (s.r[tid][0] * s.r[tid][0] + s.r[tid][1] * s.r[tid][1]) + s.r[tid][2] * s.r[tid][2];
    }
    // the ligand's radius about c and its largest atom radius: maxima, exact in any order
    for (int o = 32; o > 0; o >>= 1) {
        rho2 = fmaxf(rho2, __shfl_xor(rho2, o, 64));
        ri = fmaxf(ri, __shfl_xor(ri, o, 64));
    }
    if ((tid & 63) == 0) { s.reach[tid >> 6][0] = rho2; s.reach[tid >> 6][1] = ri; }
    __syncthreads();
    const int T = (R + RL_THREADS - 1) / RL_THREADS;
    {
        // the tiles within reach, in ascending order: a ballot per wave over 256 tiles a round, the waves' counts
        // prefix-summed through LDS
        const float rho = sqrtf(fmaxf(fmaxf(s.reach[0][0], s.reach[1][0]), fmaxf(s.reach[2][0], s.reach[3][0])));
        const float rmax = fmaxf(fmaxf(s.reach[0][1], s.reach[1][1]), fmaxf(s.reach[2][1], s.reach[3][1]));
        const float reach0 = (rho + max_shift) + rmax;
        int base = 0;
        for (int t0 = 0; t0 < T; t0 += RL_THREADS) {
            const int t = t0 + tid;
            bool keep = t < T;
            if (keep && tile_sphere != nullptr) {
                const float4 q = tile_sphere[t];
                const float dx = q.x - c[0], dy = q.y - c[1], dz = q.z - c[2];
                const float reach = reach0 + q.w;
                const float lim = reach + (RL_SLACK_ABS + RL_SLACK_REL * reach);
                keep = !(((dx * dx + dy * dy) + dz * dz) > lim * lim);          // a NaN sphere keeps its tile
            }
            const unsigned long long m = __ballot(keep);
            if ((tid & 63) == 0) s.wave_tiles[tid >> 6] = __popcll(m);
            __syncthreads();
            int before = base;
            for (int w = 0; w < (tid >> 6); ++w) before += s.wave_tiles[w];
            if (keep) s.tile[before + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = (unsigned short)t;
            base += (s.wave_tiles[0] + s.wave_tiles[1]) + (s.wave_tiles[2] + s.wave_tiles[3]);
            __syncthreads();
        }
        if (tid == 0) s.n_tiles = base;
    }
    __syncthreads();

    float G[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, p[3] = {c[0], c[1], c[2]};
    float cur[7];
    evaluate(s, rec, R, na, G, p, cur);
    const float p_start = cur[0];
    if (gradient_out != nullptr && tid < 6) gradient_out[(size_t)b * 6 + tid] = cur[1 + tid];
    float sr = RL_STEP_ROT, st = RL_STEP_TRANS;
    int accepted = 0;
    for (int it = 0; it < steps && cur[0] > 0.f; ++it) {
        float Gn[9], pn[3];
        const float fn = sqrtf((cur[1] * cur[1] + cur[2] * cur[2]) + cur[3] * cur[3]);
        const float tn = sqrtf((cur[4] * cur[4] + cur[5] * cur[5]) + cur[6] * cur[6]);
        if (tn > 0.f) {
            float D[9];
            rodrigues_row(cur[4] / tn, cur[5] / tn, cur[6] / tn, sr, D);
            mat3_mul(G, D, Gn);
            orthonormalise(Gn);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) Gn[k] = G[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) pn[k] = fn > 0.f ? p[k] + st * (cur[1 + k] / fn) : p[k];
        const float sx = pn[0] - c[0], sy = pn[1] - c[1], sz = pn[2] - c[2];
        bool take = !(((sx * sx + sy * sy) + sz * sz) > max_shift * max_shift);
        float nxt[7];
        if (take) {                           // the same in every lane
            evaluate(s, rec, R, na, Gn, pn, nxt);
            take = nxt[0] < cur[0];
        }
        if (take) {
#pragma unroll
            for (int k = 0; k < 9; ++k) G[k] = Gn[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = pn[k];
#pragma unroll
            for (int k = 0; k < 7; ++k) cur[k] = nxt[k];
            sr *= RL_GROW; st *= RL_GROW;
            ++accepted;
        } else {
            sr *= RL_SHRINK; st *= RL_SHRINK;
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
    if (tid == 0) {                           // x' = (x - c) @ G + p = x @ G + (p - c @ G)
        float cg[3];
        rotate_row(c[0], c[1], c[2], G, cg);
        for (int k = 0; k < 9; ++k) xf[k] = G[k];
        for (int k = 0; k < 3; ++k) xf[9 + k] = p[k] - cg[k];
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
    static_assert(RL_MAX_STEPS == 1024 && MAX_ATOMS == 64, "the bounds the message below states");
    if (!lig_xyz || !lig_radius || !n_nodes_dev || !rec_xyzr || !coords_out || !xform_out || !stats_out || B < 1 ||
        B > MCG_RECEPTOR_MAX_B || N < 1 || N > MAX_ATOMS || R < 1 || R > MCG_RECEPTOR_MAX_ATOMS || steps < 0 ||
        steps > RL_MAX_STEPS || !(margin >= 0.f) || !isfinite(margin) || !(max_shift >= 0.f) || !isfinite(max_shift)) {
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
