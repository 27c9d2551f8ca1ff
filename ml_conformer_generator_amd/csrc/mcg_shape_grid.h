// Device pieces shared by the shape kernels: the row-vector rotation, the Gaussian density at one grid point, the grid
// walk that turns candidate atom sets into Tanimoto scores, the handedness-fixed frame start and the posed-row write.
// Every multiply-add is written out (fmaf where one is fused) and contraction is off inside the bodies, so the compiler has
// no choice left and every kernel that calls them produces the same bits for the same inputs, however it schedules or packs
// them.  The expressions are the ones the compiler chose for the original unannotated code, so no output changed when
// they moved here.
#pragma once

#include <hip/hip_runtime.h>

namespace mcg_shape {

constexpr int MAX_ATOMS = 64;
constexpr int GRID_THREADS = 256;         // lanes of a grid-walking workgroup: four waves, the four leaves of its tree

// Atoms of a row: n_nodes[b] clamped to 0 .. min(N, MAX_ATOMS), so a row never reads past its N or the LDS atom list.
__device__ __forceinline__ int atom_count(int n_nodes_b, int N) { return min(max(n_nodes_b, 0), min(N, MAX_ATOMS)); }

// Grid point idx of the meshgrid(indexing="ij") flatten order over the three axes axes[3][n].
__device__ __forceinline__ float3 grid_point(const float* axes, int n, int idx) {
    const int ix = idx / (n * n), iy = (idx / n) % n, iz = idx % n;
    return make_float3(axes[ix], axes[n + iy], axes[2 * n + iz]);
}

// out = x @ m  (row vector times row-major 3x3: rotate_coord, shape_similarity.py:448-463)
__device__ __forceinline__ void rotate_row(float x0, float x1, float x2, const float* m, float* out) {
#pragma clang fp contract(off)
    out[0] = __builtin_fmaf(x2, m[6], __builtin_fmaf(x0, m[0], x1 * m[3]));
    out[1] = __builtin_fmaf(x2, m[7], __builtin_fmaf(x0, m[1], x1 * m[4]));
    out[2] = __builtin_fmaf(x2, m[8], __builtin_fmaf(x0, m[2], x1 * m[5]));
}

// z = x diag(1, 1, -1) @ R where flip, else x @ R: frame row x made to match the reference's handedness, in orientation R.
__device__ __forceinline__ void frame_start(float x0, float x1, float x2, bool flip, const float* R, float* z) {
    rotate_row(x0, x1, flip ? -x2 : x2, R, z);
}

// out = z @ M^T + t, m = M row-major [9], then t [3]: a row of the reference's frame back in its own coordinates.  Two
// roundings, each kept where it has always been: the fused one of `k_shape_overlay`, the unfused one of the refine pick.
__device__ __forceinline__ void posed_row_overlay(const float* z, const float* m, float* out) {
#pragma clang fp contract(off)
    out[0] = __builtin_fmaf(z[2], m[2], __builtin_fmaf(z[1], m[1], z[0] * m[0])) + m[9];
    out[1] = __builtin_fmaf(z[2], m[5], __builtin_fmaf(z[0], m[3], z[1] * m[4])) + m[10];
    out[2] = __builtin_fmaf(z[2], m[8], __builtin_fmaf(z[0], m[6], z[1] * m[7])) + m[11];
}

__device__ __forceinline__ void posed_row_pick(const float* z, const float* m, float* out) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; ++k) out[k] = ((z[0] * m[k * 3] + z[1] * m[k * 3 + 1]) + z[2] * m[k * 3 + 2]) + m[9 + k];
}

// 1 - prod_atoms (1 - A exp(-alpha |p - c|^2))
__device__ __forceinline__ float density_at(float px, float py, float pz, const float (*c)[3], int n, float alpha,
                                            float amp) {
#pragma clang fp contract(off)
    float prod = 1.f;
    for (int a = 0; a < n; ++a) {
        const float dx = px - c[a][0], dy = py - c[a][1], dz = pz - c[a][2];
        const float d2 = __builtin_fmaf(dy, dy, dx * dx) + dz * dz;
        prod *= __builtin_fmaf(-amp, __expf(-d2 * alpha), 1.f);
    }
    return 1.f - prod;
}

// Shape Tanimoto <f,g_w> / (<f,f> + <g_w,g_w> - <f,g_w>) of W candidate atom sets c[w] (LDS, na atoms each) against the
// reference density f on the grid, by a workgroup of GRID_THREADS lanes.  Lane l walks idx = l + 256 k and accumulates
// with fmaf; <f,f> is summed once for all W.  Each sum goes through an xor butterfly per wave, then the tree
// (w0 + w1) + (w2 + w3) through red[2W + 1][4] in LDS.  Lane w < W returns score w, the other lanes 0.  Every lane must
// call it.  A candidate scores the same bits whatever W and whichever slot it sits in.
template <int W>
__device__ __forceinline__ float overlap_scores(const float* __restrict__ f, const float* __restrict__ axes, int n,
                                                const float (*c)[MAX_ATOMS][3], int na, float alpha, float amp,
                                                float (*red)[4]) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, total = n * n * n;
    float v[2 * W + 1];                   // fg[W], gg[W], ff
#pragma unroll
    for (int k = 0; k < 2 * W + 1; ++k) v[k] = 0.f;
    for (int idx = tid; idx < total; idx += GRID_THREADS) {
        const float3 p = grid_point(axes, n, idx);
        // one candidate reads f after its density (two VGPRs fewer); more read it first, to hide the load behind them
        const float g0 = W == 1 ? density_at(p.x, p.y, p.z, c[0], na, alpha, amp) : 0.f;
        const float fv = f[idx];
        v[2 * W] = __builtin_fmaf(fv, fv, v[2 * W]);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const float g = W == 1 ? g0 : density_at(p.x, p.y, p.z, c[w], na, alpha, amp);
            v[w] = __builtin_fmaf(fv, g, v[w]);
            v[W + w] = __builtin_fmaf(g, g, v[W + w]);
        }
    }
#pragma unroll
    for (int k = 0; k < 2 * W + 1; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 2 * W + 1; ++k) red[k][tid >> 6] = v[k];
    }
    __syncthreads();
    if (tid >= W) return 0.f;
    const float sfg = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    const float sgg = (red[W + tid][0] + red[W + tid][1]) + (red[W + tid][2] + red[W + tid][3]);
    const float sff = (red[2 * W][0] + red[2 * W][1]) + (red[2 * W][2] + red[2 * W][3]);
    return sfg / (sff + sgg - sfg);
}

// Index of the first maximum of sc[0..3] (the reference's strict >); its score goes to *best.
__device__ __forceinline__ int first_max4(const float* sc, float* best) {
    int wb = 0;
    float sb = sc[0];
    for (int w = 1; w < 4; ++w)
        if (sc[w] > sb) { sb = sc[w]; wb = w; }
    *best = sb;
    return wb;
}

}  // namespace mcg_shape
