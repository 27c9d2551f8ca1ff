// Gaussian-volume shape Tanimoto on a regular grid (the grid half of
// `evaluate_samples`): reference cheminformatics/shape_similarity.py:405-492 `tanimoto_score`.
//   density(p) = 1 - prod_atoms (1 - A exp(-alpha |p - c|^2)),  score = <f,g> / (<f,f> + <g,g> - <f,g>)
// One workgroup per (candidate, orientation); the reference's density f is evaluated once.
// Transcendental-bound (n^3 x atoms exponentials), no reuse worth staging beyond the atom list in LDS.
// `k_shape_overlay` ("pose on the reference"): one workgroup per candidate runs all four orientations
// of its handedness-fixed frame in one walk over the grid, picks the best and writes the rigid pose that puts the
// candidate onto the reference's own coordinates.  Per orientation it evaluates the same density, in the same per-lane
// index order and with the same reduction tree as `k_shape_overlap` (mcg_shape_grid.h), so its four scores are
// bit-identical to `mcg_shape_tanimoto` on the handedness-fixed frames.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"

namespace {

using mcg_shape::MAX_ATOMS;
using mcg_shape::density_at;
using mcg_shape::rotate_row;

__global__ __launch_bounds__(256) void k_shape_density(const float* __restrict__ ref, int n_ref,
                                                        const float* __restrict__ axes, int n, float alpha, float amp,
                                                        float* __restrict__ f) {
    __shared__ float c[MAX_ATOMS][3];
    for (int i = threadIdx.x; i < n_ref * 3; i += 256) c[i / 3][i % 3] = ref[i];
    __syncthreads();
    const int total = n * n * n;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int ix = idx / (n * n), iy = (idx / n) % n, iz = idx % n;       // meshgrid(indexing="ij") flatten order
        f[idx] = density_at(axes[ix], axes[n + iy], axes[2 * n + iz], c, n_ref, alpha, amp);
    }
}

__global__ __launch_bounds__(256) void k_shape_overlap(const float* __restrict__ f, const float* __restrict__ cand,
                                                        const int* __restrict__ n_nodes, int N,
                                                        const float* __restrict__ rot /*[R][9]*/, int R,
                                                        const float* __restrict__ axes, int n, float alpha, float amp,
                                                        float* __restrict__ score) {
    __shared__ float c[MAX_ATOMS][3];
    __shared__ float red[3][4];
    const int b = blockIdx.x / R, r = blockIdx.x % R;
    const int na = min(n_nodes[b], MAX_ATOMS);
    const float* m = rot + r * 9;
    for (int i = threadIdx.x; i < na; i += 256) {
        const float* x = cand + ((size_t)b * N + i) * 3;
        rotate_row(x[0], x[1], x[2], m, c[i]);       // coord @ M
    }
    __syncthreads();
    const int total = n * n * n;
    float fg = 0.f, ff = 0.f, gg = 0.f;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int ix = idx / (n * n), iy = (idx / n) % n, iz = idx % n;
        const float g = density_at(axes[ix], axes[n + iy], axes[2 * n + iz], c, na, alpha, amp);
        const float fv = f[idx];
        fg = fmaf(fv, g, fg); ff = fmaf(fv, fv, ff); gg = fmaf(g, g, gg);
    }
    for (int o = 32; o > 0; o >>= 1) {
        fg += __shfl_xor(fg, o, 64); ff += __shfl_xor(ff, o, 64); gg += __shfl_xor(gg, o, 64);
    }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wid] = fg; red[1][wid] = ff; red[2][wid] = gg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float sfg = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const float sff = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const float sgg = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
        score[blockIdx.x] = sfg / (sff + sgg - sfg);
    }
}

__device__ __forceinline__ float det3(const float* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// xform = M row-major [9], then t [3]: frames = (coords - t) @ M on the real rows (mcg_shape_frames_tf).
__global__ __launch_bounds__(256) void k_shape_overlay(const float* __restrict__ f, const float* __restrict__ ref_xform,
                                                        const float* __restrict__ frames, const float* __restrict__ xform,
                                                        const int* __restrict__ n_nodes, int N,
                                                        const float* __restrict__ rot /*[4][9]*/,
                                                        const float* __restrict__ axes, int n, float alpha, float amp,
                                                        float* __restrict__ score, float* __restrict__ best,
                                                        int* __restrict__ which, int* __restrict__ flipped,
                                                        float* __restrict__ pose, float* __restrict__ posed) {
    __shared__ float c[4][MAX_ATOMS][3];      // the handedness-fixed frame under the four orientations
    __shared__ float red[9][4];               // per wave: fg[4], gg[4], ff
    __shared__ float sc[4];
    __shared__ float zr[12];                  // M_r row-major, then t_r
    __shared__ int s_flip, s_best;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int na = min(max(n_nodes[b], 0), min(N, MAX_ATOMS));
    const float* xs = xform + (size_t)b * 12;
    if (tid == 0) s_flip = det3(xs) * det3(ref_xform) < 0.f;      // M_s' = M_s diag(1, 1, -1): a proper Q
    if (tid < 12) zr[tid] = ref_xform[tid];
    __syncthreads();
    const bool flip = s_flip != 0;
    bool bad = false;
    for (int i = tid; i < na; i += 256) {
        const float* x = frames + ((size_t)b * N + i) * 3;
        const float x0 = x[0], x1 = x[1], x2 = flip ? -x[2] : x[2];
        bad |= !(isfinite(x0) && isfinite(x1) && isfinite(x2));
#pragma unroll
        for (int w = 0; w < 4; ++w) rotate_row(x0, x1, x2, rot + w * 9, c[w][i]);
    }
    const bool frame_bad = __syncthreads_or(bad) != 0;
    const int total = n * n * n;
    float fg[4] = {0.f, 0.f, 0.f, 0.f}, gg[4] = {0.f, 0.f, 0.f, 0.f}, ff = 0.f;
    for (int idx = tid; idx < total; idx += 256) {
        const int ix = idx / (n * n), iy = (idx / n) % n, iz = idx % n;
        const float px = axes[ix], py = axes[n + iy], pz = axes[2 * n + iz];
        const float fv = f[idx];
        ff = fmaf(fv, fv, ff);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float g = density_at(px, py, pz, c[w], na, alpha, amp);
            fg[w] = fmaf(fv, g, fg[w]); gg[w] = fmaf(g, g, gg[w]);
        }
    }
    float v[9] = {fg[0], fg[1], fg[2], fg[3], gg[0], gg[1], gg[2], gg[3], ff};
#pragma unroll
    for (int k = 0; k < 9; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    const int wid = tid >> 6;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) red[k][wid] = v[k];
    }
    __syncthreads();
    if (tid < 4) {                            // k_shape_overlap's tree, one orientation per lane
        const float sfg = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        const float sff = (red[8][0] + red[8][1]) + (red[8][2] + red[8][3]);
        const float sgg = (red[4 + tid][0] + red[4 + tid][1]) + (red[4 + tid][2] + red[4 + tid][3]);
        sc[tid] = sfg / (sff + sgg - sfg);
        if (score != nullptr) score[b * 4 + tid] = sc[tid];
    }
    __syncthreads();
    if (tid == 0) {
        bool ok = !frame_bad;
        for (int k = 0; k < 12; ++k) ok = ok && isfinite(xs[k]) && isfinite(zr[k]);
        int wb = 0;
        float sb = sc[0];
        for (int w = 1; w < 4; ++w)
            if (sc[w] > sb) { sb = sc[w]; wb = w; }                 // the first maximum (the reference's strict >)
        for (int w = 0; w < 4; ++w) ok = ok && !isnan(sc[w]);
        float Q[9], d[3];
        {                                     // Q = M_s' @ R_best @ M_r^T,  d = t_r - t_s @ Q
            float A[9];
            const float* R = rot + wb * 9;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    float acc = 0.f;
                    for (int k = 0; k < 3; ++k) acc += (k == 2 && flip ? -xs[i * 3 + k] : xs[i * 3 + k]) * R[k * 3 + j];
                    A[i * 3 + j] = acc;
                }
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    float acc = 0.f;
                    for (int k = 0; k < 3; ++k) acc += A[i * 3 + k] * zr[j * 3 + k];
                    Q[i * 3 + j] = acc;
                }
            for (int j = 0; j < 3; ++j) {
                float acc = 0.f;
                for (int k = 0; k < 3; ++k) acc += xs[9 + k] * Q[k * 3 + j];
                d[j] = zr[9 + j] - acc;
            }
        }
        best[b] = ok ? sb : __builtin_nanf("");
        which[b] = ok ? wb : -1;
        flipped[b] = flip ? 1 : 0;
        for (int k = 0; k < 9; ++k) pose[(size_t)b * 12 + k] = ok ? Q[k] : __builtin_nanf("");
        for (int k = 0; k < 3; ++k) pose[(size_t)b * 12 + 9 + k] = ok ? d[k] : __builtin_nanf("");
        s_best = ok ? wb : -1;
    }
    __syncthreads();
    const int wb = s_best;
    for (int i = tid; i < N; i += 256) {      // x_out = z_best @ M_r^T + t_r  (the reference's own coordinates)
        float* out = posed + ((size_t)b * N + i) * 3;
        if (i >= na) {
            out[0] = out[1] = out[2] = 0.f;
        } else if (wb < 0) {
            out[0] = out[1] = out[2] = __builtin_nanf("");
        } else {
            const float* z = c[wb][i];
            for (int k = 0; k < 3; ++k) out[k] = ((z[0] * zr[k * 3] + z[1] * zr[k * 3 + 1]) + z[2] * zr[k * 3 + 2]) + zr[9 + k];
        }
    }
}

}  // namespace

extern "C" int mcg_shape_tanimoto(const float* ref, int n_ref, const float* cand, const int32_t* n_nodes_dev, int B, int N,
                                  const float* rot, int R, const float* axes, int n, float alpha, float amplitude,
                                  float* f_scratch, float* score, void* stream) {
    if (!ref || !cand || !n_nodes_dev || !rot || !axes || !f_scratch || !score || n_ref < 1 || n_ref > MAX_ATOMS ||
        B < 1 || N < 1 || R < 1 || n < 2) {
        mcg_set_error("mcg_shape_tanimoto: bad arguments (1 <= n_ref <= %d)", MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int total = n * n * n;
    hipLaunchKernelGGL(k_shape_density, dim3((total + 255) / 256), dim3(256), 0, s, ref, n_ref, axes, n, alpha, amplitude,
                       f_scratch);
    hipLaunchKernelGGL(k_shape_overlap, dim3(B * R), dim3(256), 0, s, f_scratch, cand, n_nodes_dev, N, rot, R, axes, n, alpha,
                       amplitude, score);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_shape_overlay(const float* ref_frame, int n_ref, const float* ref_xform, const float* frames,
                                 const float* xform, const int32_t* n_nodes_dev, int B, int N, const float* rot,
                                 const float* axes, int n, float alpha, float amplitude, float* f_scratch, float* score,
                                 float* best, int32_t* which, int32_t* flipped, float* pose, float* posed, void* stream) {
    if (!ref_frame || !ref_xform || !frames || !xform || !n_nodes_dev || !rot || !axes || !f_scratch || !best || !which ||
        !flipped || !pose || !posed || B < 1 || N < 1 || N > MAX_ATOMS || n_ref < 3 || n_ref > MAX_ATOMS || n < 2) {
        mcg_set_error("mcg_shape_overlay: bad arguments (non-null buffers, B >= 1, 1 <= N <= %d, 3 <= n_ref <= %d, n >= 2)",
                      MAX_ATOMS, MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int total = n * n * n;
    hipLaunchKernelGGL(k_shape_density, dim3((total + 255) / 256), dim3(256), 0, s, ref_frame, n_ref, axes, n, alpha,
                       amplitude, f_scratch);
    hipLaunchKernelGGL(k_shape_overlay, dim3(B), dim3(256), 0, s, f_scratch, ref_xform, frames, xform, n_nodes_dev, N, rot,
                       axes, n, alpha, amplitude, score, best, which, flipped, pose, posed);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
