// Pose search ("Pose search"; the definition is the docstring of `interactions.search_pose`, the C
// contract include/mlconfgen_hip_search.h): S keyed starts per posed molecule for the flexible walk, and the exact choice
// among the walked starts.  The walk between the two kernels is `mcg_receptor_optimise_flex` itself, on the B * S rows.
// THE PACKAGE'S OWN procedure: a bounded multi-start of its own downhill walk - not a docking run, not AutoDock Vina's Monte
// Carlo search.
//   k_pose_starts:        one 64-lane wave per (molecule, start), lane = atom.  Six Philox blocks keyed as the sampler noise
//                         is; every lane draws the same words, so the axis, the shift and the angles are uniform in the wave
//                         and the ends of a torsion axis travel by `__shfl`.  The torsions are turned by the walk's own
//                         `turn_about_line`, the rigid part is the walk's own `rotate_about<true>` of the identity, the
//                         transform its `write_transform`.  The centroid is summed in atom order out of LDS, as the walk
//                         sums it.  No atomics; nothing depends on the row, the batch or the padded width.
//   k_pose_search_select: one 64-lane wave per molecule.  Lane s forms J_s; lane 0 scans them in ascending s; then lane =
//                         atom gathers the winner's row and the two RMSDs are summed in atom order out of LDS.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"
#include "mcg_rigid_step.h"
#include "mcg_interaction_pair.h"
#include "mcg_philox.h"
#include "../../include/mlconfgen_hip_search.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;
using namespace mcg_rigid;

constexpr int PS_LANES = MCG_FLEX_MAX_ATOMS;
constexpr int PS_T = MCG_FLEX_MAX_TORSIONS;
constexpr int PS_STATS = MCG_FLEX_STATS;
constexpr int PS_PARAMS = MCG_SEARCH_PARAMS;
constexpr int PS_DRAWS = 6;
constexpr uint32_t PS_COUNTER_WORD = 0xfffffffeu;      // c3: the sampler's (run << 8) | block has block 0..2, the size draw 0xffffffff
constexpr float PS_TWO_PI = 6.28318530717958647692f, PS_PI = 3.14159265358979323846f;
static_assert(PS_LANES == 64 && MAX_ATOMS == 64 && PS_PARAMS == 4 * PS_DRAWS && PS_T == 4 * (PS_DRAWS - 2),
              "one lane per atom, four uniforms per draw, four draws of angles");

// u = (w >> 8) 2^-24 in [0, 1): exact, 24 bits
__device__ __forceinline__ float uniform24(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

// the unit vector of (u0, u1): z = 2 u0 - 1, phi = 2 pi u1, (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z)
__device__ __forceinline__ void sphere_point(float u0, float u1, float* v) {
    const float z = 2.f * u0 - 1.f, phi = PS_TWO_PI * u1;
    const float r = sqrtf(fmaxf(1.f - z * z, 0.f));
    v[0] = r * cosf(phi); v[1] = r * sinf(phi); v[2] = z;
}

__global__ __launch_bounds__(PS_LANES) void k_pose_starts(
        const float* __restrict__ lig, const int32_t* __restrict__ n_nodes, int N, const int32_t* __restrict__ torsion_atoms,
        const unsigned long long* __restrict__ side_mask, const int32_t* __restrict__ n_torsions,
        const int64_t* __restrict__ sample_ids, uint32_t k0, uint32_t k1, int S, float spread, float max_turn,
        float* __restrict__ start_xyz, float* __restrict__ start_xform, float* __restrict__ start_angles,
        float* __restrict__ start_params) {
    __shared__ float sx[PS_LANES][3];
    __shared__ float sc[3];
    __shared__ int sta[PS_T], stb[PS_T];
    __shared__ unsigned long long sside[PS_T];
    const int s = blockIdx.x, b = blockIdx.y, a = threadIdx.x;
    const int na = atom_count(n_nodes[b], N);
    const bool real = a < na;
    const float* xin = lig + (size_t)b * N * 3;
    const size_t row = (size_t)b * S + s;
    float* xout = start_xyz + row * N * 3;
    float* xf = start_xform + row * 12;
    float* angles = start_angles + row * PS_T;
    float x0 = 0.f, y0 = 0.f, z0 = 0.f;
    if (real) {
        x0 = xin[a * 3]; y0 = xin[a * 3 + 1]; z0 = xin[a * 3 + 2];
    }
    // the uniforms: a function of (seed, sample id, s) alone, the same in every lane
    float u[PS_PARAMS];
#pragma unroll
    for (int j = 0; j < PS_DRAWS; ++j) {
        const uint4 w = mcg_philox::philox4x32_10(make_uint4((uint32_t)sample_ids[b], (uint32_t)s, (uint32_t)j,
                                                             PS_COUNTER_WORD), k0, k1);
        u[4 * j] = s > 0 ? uniform24(w.x) : 0.f; u[4 * j + 1] = s > 0 ? uniform24(w.y) : 0.f;
        u[4 * j + 2] = s > 0 ? uniform24(w.z) : 0.f; u[4 * j + 3] = s > 0 ? uniform24(w.w) : 0.f;
    }
    if (start_params != nullptr && a < PS_PARAMS) {
        float mine = 0.f;
#pragma unroll
        for (int k = 0; k < PS_PARAMS; ++k) mine = a == k ? u[k] : mine;
        start_params[row * PS_PARAMS + a] = mine;
    }
    const bool bad = real && !(isfinite(x0) && isfinite(y0) && isfinite(z0));
    if (__syncthreads_or(bad) != 0 || na == 0) {                   // left exactly as it came, NaN in xform and angles
        if (a < N) {
            xout[a * 3] = x0; xout[a * 3 + 1] = y0; xout[a * 3 + 2] = z0;       // a padded slot holds 0
        }
        if (a < 12) xf[a] = __builtin_nanf("");
        if (a < PS_T) angles[a] = __builtin_nanf("");
        return;
    }
    if (s == 0) {                                                  // the input's bits, the identity, zero angles
        if (a < N) {
            xout[a * 3] = x0; xout[a * 3 + 1] = y0; xout[a * 3 + 2] = z0;
        }
        if (a < 12) xf[a] = (a == 0 || a == 4 || a == 8) ? 1.f : 0.f;
        if (a < PS_T) angles[a] = 0.f;
        return;
    }
    sx[a][0] = x0; sx[a][1] = y0; sx[a][2] = z0;
    if (a < PS_T) {
        sta[a] = torsion_atoms[((size_t)b * PS_T + a) * 2];
        stb[a] = torsion_atoms[((size_t)b * PS_T + a) * 2 + 1];
        sside[a] = side_mask[(size_t)b * PS_T + a];
    }
    __syncthreads();
    if (a < 3) {                              // atom centroid, summed in atom order
        float acc = 0.f;
        for (int i = 0; i < na; ++i) acc += sx[i][a];
        sc[a] = acc / (float)na;
    }
    int nt = min(max(n_torsions[b], 0), PS_T);
    for (int k = 0; k < nt; ++k) {            // cut at the first slot that does not name two atoms of this row
        const int ia = sta[k], ib = stb[k];
        if (ia < 0 || ia >= na || ib < 0 || ib >= na || ia == ib) nt = k;
    }
    __syncthreads();
    const float c[3] = {sc[0], sc[1], sc[2]};
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (real) {
        qx = x0 - c[0]; qy = y0 - c[1]; qz = z0 - c[2];
    }
    // the torsions, in ascending order, each about its current axis through q_b
    float theta[PS_T];
#pragma unroll
    for (int k = 0; k < PS_T; ++k) {
        theta[k] = 0.f;
        if (k < nt) {                         // the same in every lane
            const float d = PS_TWO_PI * u[8 + k] - PS_PI;
            theta[k] = d;
            if (d != 0.f) {                   // a zero angle leaves the bits
                const int ia = sta[k], ib = stb[k];
                const float ax = __shfl(qx, ia, 64), ay = __shfl(qy, ia, 64), az = __shfl(qz, ia, 64);
                const float bx = __shfl(qx, ib, 64), by = __shfl(qy, ib, 64), bz = __shfl(qz, ib, 64);
                float n[3] = {bx - ax, by - ay, bz - az}, o[3];
                const float ln = norm3(n);
                turn_about_line(qx, qy, qz, bx, by, bz, n[0] / ln, n[1] / ln, n[2] / ln, d, o);
                if (real && ((sside[k] >> a) & 1ull) != 0ull) {
                    qx = o[0]; qy = o[1]; qz = o[2];
                }
            }
        }
    }
    // the rigid part: the walk's trial rotation of the identity, and p = c + d
    const float eye[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    float axis[3], dir[3], R[9], p[3];
    sphere_point(u[0], u[1], axis);
    rotate_about<true>(eye, axis[0], axis[1], axis[2], max_turn * u[2], R);
    sphere_point(u[4], u[5], dir);
    const float len = spread * cbrtf(u[6]);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = c[k] + len * dir[k];
    float o[3] = {0.f, 0.f, 0.f};
    if (real) {
        rotate_row(qx, qy, qz, R, o);
        o[0] = o[0] + p[0]; o[1] = o[1] + p[1]; o[2] = o[2] + p[2];
    }
    if (a < N) {
        xout[a * 3] = o[0]; xout[a * 3 + 1] = o[1]; xout[a * 3 + 2] = o[2];     // a padded slot holds 0
    }
    if (a == 0) {
        write_transform(R, p, c[0], c[1], c[2], xf);
#pragma unroll
        for (int k = 0; k < PS_T; ++k) angles[k] = theta[k];
    }
}

__global__ __launch_bounds__(PS_LANES) void k_pose_search_select(
        const float* __restrict__ walk_coords, const float* __restrict__ walk_xform, const float* __restrict__ walk_stats,
        const float* __restrict__ walk_angles, const float* __restrict__ start_xform, const float* __restrict__ start_angles,
        const float* __restrict__ lig, const int32_t* __restrict__ n_nodes, int N, int S, float* __restrict__ coords_out,
        float* __restrict__ xform_out, float* __restrict__ stats_out, float* __restrict__ angles_out,
        int32_t* __restrict__ best_start, float* __restrict__ start_scores) {
    __shared__ float sj[MCG_SEARCH_MAX_STARTS];
    __shared__ float sd[PS_LANES][2];
    __shared__ float sxf[12];
    __shared__ int sbest;
    const int b = blockIdx.x, a = threadIdx.x;
    const int na = atom_count(n_nodes[b], N);
    const size_t row0 = (size_t)b * S;
    if (a < S) {
        const float* st = walk_stats + (row0 + a) * PS_STATS;
        // one rounded product, one rounded sum: plain operators under this file's `fp contract(off)` (the runtime's
        // __fmul_rn / __fadd_rn are inline `*` and `+` compiled where contraction is allowed, and fuse once inlined)
        const float prod = mcg_interaction::W_REP * st[7];
        const float j = st[1] + prod;
        sj[a] = j;
        start_scores[row0 + a] = j;
    }
    __syncthreads();
    if (a == 0) {
        int best = -1;
        float jb = 0.f;
        for (int s = 0; s < S; ++s) {         // the smallest finite J; a tie stays with the lower s
            const float j = sj[s];
            if (isfinite(j) && (best < 0 || j < jb)) {
                best = s; jb = j;
            }
        }
        sbest = best;
        best_start[b] = best;
    }
    __syncthreads();
    const int best = sbest, w = max(best, 0);
    const size_t row = row0 + w;
    const float* xw = walk_coords + row * N * 3;
    float* xout = coords_out + (size_t)b * N * 3;
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (a < N) {
        ox = xw[a * 3]; oy = xw[a * 3 + 1]; oz = xw[a * 3 + 2];
        xout[a * 3] = ox; xout[a * 3 + 1] = oy; xout[a * 3 + 2] = oz;
    }
    float* xf = xform_out + (size_t)b * 12;
    float* stats = stats_out + (size_t)b * PS_STATS;
    float* angles = angles_out + (size_t)b * PS_T;
    if (best <= 0) {                          // start 0's walk row, bit for bit
        if (a < 12) xf[a] = walk_xform[row * 12 + a];
        if (a < PS_STATS) stats[a] = walk_stats[row * PS_STATS + a];
        if (a < PS_T) angles[a] = walk_angles[row * PS_T + a];
        return;
    }
    if (a < PS_T) angles[a] = start_angles[row * PS_T + a] + walk_angles[row * PS_T + a];
    if (a < 12) {                             // the start's map, then the walk's: R = R_s @ G_w, t = t_s @ G_w + t_w
        const float* ms = start_xform + row * 12;
        const float* mw = walk_xform + row * 12;
        const int i = a / 3, j = a - 3 * i;   // i = 3: the translation row
        float v = (ms[i * 3] * mw[j] + ms[i * 3 + 1] * mw[3 + j]) + ms[i * 3 + 2] * mw[6 + j];   // in index order, unfused
        if (i == 3) v = v + mw[9 + j];
        sxf[a] = v;
        xf[a] = v;
    }
    __syncthreads();
    float d2 = 0.f, e2 = 0.f;
    if (a < na) {
        const float* xin = lig + (size_t)b * N * 3;
        const float x0 = xin[a * 3], y0 = xin[a * 3 + 1], z0 = xin[a * 3 + 2];
        const float ex = ox - x0, ey = oy - y0, ez = oz - z0;
        d2 = (ex * ex + ey * ey) + ez * ez;
        // the output taken back through the rigid part: (x_out - t) @ R^T against the input
        const float yx = ox - sxf[9], yy = oy - sxf[10], yz = oz - sxf[11];
        const float hx = ((yx * sxf[0] + yy * sxf[1]) + yz * sxf[2]) - x0;
        const float hy = ((yx * sxf[3] + yy * sxf[4]) + yz * sxf[5]) - y0;
        const float hz = ((yx * sxf[6] + yy * sxf[7]) + yz * sxf[8]) - z0;
        e2 = (hx * hx + hy * hy) + hz * hz;
    }
    sd[a][0] = d2; sd[a][1] = e2;
    __syncthreads();
    if (a == 0) {
        float sum = 0.f, sumq = 0.f;
        for (int i = 0; i < na; ++i) sum += sd[i][0];              // in atom order
        for (int i = 0; i < na; ++i) sumq += sd[i][1];
        const float* s0 = walk_stats + row0 * PS_STATS;
        const float* sw = walk_stats + row * PS_STATS;
        stats[0] = s0[0]; stats[1] = sw[1]; stats[2] = sw[2]; stats[3] = sw[3];
        stats[4] = sqrtf(sum / (float)na); stats[5] = sw[5]; stats[6] = s0[6]; stats[7] = sw[7];
        stats[8] = sw[8]; stats[9] = sqrtf(sumq / (float)na); stats[10] = 0.f; stats[11] = 0.f;
    }
}

}  // namespace

extern "C" int mcg_pose_starts(const float* lig_xyz, const int32_t* n_nodes_dev, int B, int N, const int32_t* torsion_atoms,
                               const uint64_t* side_mask, const int32_t* n_torsions, const int64_t* sample_ids_dev,
                               uint64_t seed, int S, float spread, float max_turn, float* start_xyz, float* start_xform,
                               float* start_angles, float* start_params, void* stream) {
    if (!lig_xyz || !n_nodes_dev || !torsion_atoms || !side_mask || !n_torsions || !sample_ids_dev || !start_xyz ||
        !start_xform || !start_angles || B < 1 || B > MCG_RECEPTOR_MAX_B || N < 1 || N > PS_LANES || S < 1 ||
        S > MCG_SEARCH_MAX_STARTS || !(spread >= 0.f) || !isfinite(spread) || !(max_turn >= 0.f) || !(max_turn <= PS_PI)) {
        mcg_set_error("mcg_pose_starts: bad arguments (non-null buffers, 1 <= B <= %d, 1 <= N <= 64, 1 <= S <= %d, spread "
                      "finite and >= 0, 0 <= max_turn <= pi)", MCG_RECEPTOR_MAX_B, MCG_SEARCH_MAX_STARTS);
        return MCG_ERR_ARG;
    }
    hipLaunchKernelGGL(k_pose_starts, dim3((unsigned)S, (unsigned)B), dim3(PS_LANES), 0, (hipStream_t)stream, lig_xyz,
                       n_nodes_dev, N, torsion_atoms, reinterpret_cast<const unsigned long long*>(side_mask), n_torsions,
                       sample_ids_dev, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), S, spread, max_turn,
                       start_xyz, start_xform, start_angles, start_params);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_pose_search_select(const float* walk_coords, const float* walk_xform, const float* walk_stats,
                                      const float* walk_angles, const float* start_xform, const float* start_angles,
                                      const float* lig_xyz, const int32_t* n_nodes_dev, int B, int N, int S,
                                      float* coords_out, float* xform_out, float* stats_out, float* angles_out,
                                      int32_t* best_start, float* start_scores, void* stream) {
    if (!walk_coords || !walk_xform || !walk_stats || !walk_angles || !start_xform || !start_angles || !lig_xyz ||
        !n_nodes_dev || !coords_out || !xform_out || !stats_out || !angles_out || !best_start || !start_scores || B < 1 ||
        B > MCG_RECEPTOR_MAX_B || N < 1 || N > PS_LANES || S < 1 || S > MCG_SEARCH_MAX_STARTS) {
        mcg_set_error("mcg_pose_search_select: bad arguments (non-null buffers, 1 <= B <= %d, 1 <= N <= 64, 1 <= S <= %d)",
                      MCG_RECEPTOR_MAX_B, MCG_SEARCH_MAX_STARTS);
        return MCG_ERR_ARG;
    }
    hipLaunchKernelGGL(k_pose_search_select, dim3((unsigned)B), dim3(PS_LANES), 0, (hipStream_t)stream, walk_coords,
                       walk_xform, walk_stats, walk_angles, start_xform, start_angles, lig_xyz, n_nodes_dev, N, S, coords_out,
                       xform_out, stats_out, angles_out, best_start, start_scores);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
