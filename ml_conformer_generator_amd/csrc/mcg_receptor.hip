// Steric contacts of posed molecules with a receptor ("Receptor clashes"): for every ligand heavy atom
// i its largest overlap max_j (r_i + r_j) - sqrt(dx*dx + dy*dy + dz*dz), d = x_i - y_j, over all R receptor heavy atoms,
// by brute force (no cell list, no cropping).
//   k_receptor_overlap: one lane per ligand atom (flat index over B*N, 256 per workgroup); blockIdx.y = receptor split s of
//                       S, which walks tiles [s*T/S, (s+1)*T/S) of RC_TILE receptor atoms (T = ceil(R / RC_TILE)).  Each
//                       tile is staged in LDS as float4 (x, y, z, r) and read by broadcast.  The split's maximum goes to
//                       part[s][B*N], or straight to the output when S = 1.
//   k_receptor_max:     out = the maximum over the S partial rows.
// A maximum is exact and order-free, so every S gives the same bits.  No atomics.  Padded atoms (i >= n_nodes[b]) get
// -inf; a ligand atom with a non-finite coordinate gets NaN; the other atoms are unaffected.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"

namespace {

using mcg_shape::MAX_ATOMS;
using mcg_shape::atom_count;

constexpr int RC_TILE = 256;                 // receptor atoms per LDS tile = lanes per workgroup (one load each)

// r_i + r_j - |x_i - y_j| in fp32, in exactly the order of the definition: no contraction, correctly rounded sqrtf.
__device__ __forceinline__ float pair_overlap(float x0, float x1, float x2, float ri, float4 q) {
#pragma clang fp contract(off)
    const float dx = x0 - q.x, dy = x1 - q.y, dz = x2 - q.z;
    return (ri + q.w) - sqrtf(dx * dx + dy * dy + dz * dz);
}

__global__ __launch_bounds__(RC_TILE) void k_receptor_overlap(const float* __restrict__ lig, const float* __restrict__ lig_r,
                                                              const int* __restrict__ n_nodes, int B, int N,
                                                              const float* __restrict__ rec,
                                                              const float* __restrict__ rec_r, int R, int S,
                                                              float* __restrict__ out) {
    __shared__ float4 tile[RC_TILE];
    const int tid = threadIdx.x;
    const long BN = (long)B * N;
    const long a = (long)blockIdx.x * RC_TILE + tid;
    bool live = false, bad = false;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f, ri = 0.f;
    if (a < BN) {
        const int b = (int)(a / N), i = (int)(a % N);
        if (i < atom_count(n_nodes[b], N)) {
            const float* x = lig + a * 3;
            x0 = x[0], x1 = x[1], x2 = x[2], ri = lig_r[a];
            bad = !(isfinite(x0) && isfinite(x1) && isfinite(x2));
            live = !bad;
        }
    }
    float* dst = out + (size_t)blockIdx.y * BN;
    const float fill = bad ? __builtin_nanf("") : -INFINITY;
    if (__syncthreads_or(live) == 0) {                           // a workgroup of padded / non-finite atoms only
        if (a < BN) dst[a] = fill;
        return;
    }
    const int T = (R + RC_TILE - 1) / RC_TILE;
    const int t0 = (int)((long)blockIdx.y * T / S), t1 = (int)((long)(blockIdx.y + 1) * T / S);
    float best = -INFINITY;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * RC_TILE, nj = min(RC_TILE, R - j0);
        __syncthreads();                                         // the previous tile is read by every lane
        if (tid < nj) {
            const float* y = rec + (size_t)(j0 + tid) * 3;
            tile[tid] = make_float4(y[0], y[1], y[2], rec_r[j0 + tid]);
        }
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int j = 0; j < nj; ++j) best = fmaxf(best, pair_overlap(x0, x1, x2, ri, tile[j]));
        }
    }
    if (a < BN) dst[a] = live ? best : fill;
}

// out[a] = max over s of part[s][a]; every partial of a padded (-inf) or non-finite (NaN) atom is that same value.
__global__ __launch_bounds__(256) void k_receptor_max(const float* __restrict__ part, long BN, int S,
                                                      float* __restrict__ out) {
    for (long a = (long)blockIdx.x * 256 + threadIdx.x; a < BN; a += (long)gridDim.x * 256) {
        float v = part[a];
        for (int s = 1; s < S; ++s) v = fmaxf(v, part[(size_t)s * BN + a]);
        out[a] = v;
    }
}

}  // namespace

extern "C" int mcg_receptor_overlap(const float* lig_xyz, const float* lig_radius, const int32_t* n_nodes_dev, int B,
                                    int N, const float* rec_xyz, const float* rec_radius, int R, int splits,
                                    float* partial_ws, float* overlap_out, void* stream) {
    if (!lig_xyz || !lig_radius || !n_nodes_dev || !rec_xyz || !rec_radius || !overlap_out || B < 1 ||
        B > MCG_RECEPTOR_MAX_B || N < 1 || N > MAX_ATOMS || R < 1 || R > MCG_RECEPTOR_MAX_ATOMS || splits < 1 ||
        splits > MCG_RECEPTOR_MAX_SPLITS || (splits > 1 && !partial_ws)) {
        mcg_set_error("mcg_receptor_overlap: bad arguments (non-null buffers, 1 <= B <= %d, 1 <= N <= %d, "
                      "1 <= R <= %d, 1 <= splits <= %d, partial_ws when splits > 1)", MCG_RECEPTOR_MAX_B, MAX_ATOMS,
                      MCG_RECEPTOR_MAX_ATOMS, MCG_RECEPTOR_MAX_SPLITS);
        return MCG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const long BN = (long)B * N;
    const int T = (R + RC_TILE - 1) / RC_TILE;
    const int S = splits < T ? splits : T;                       // no split without a tile of its own
    const unsigned xb = (unsigned)((BN + RC_TILE - 1) / RC_TILE);
    hipLaunchKernelGGL(k_receptor_overlap, dim3(xb, S), dim3(RC_TILE), 0, s, lig_xyz, lig_radius, n_nodes_dev, B, N,
                       rec_xyz, rec_radius, R, S, S == 1 ? overlap_out : partial_ws);
    if (S > 1) {
        const long blocks = (BN + 255) / 256;
        hipLaunchKernelGGL(k_receptor_max, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, partial_ws,
                           BN, S, overlap_out);
    }
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
