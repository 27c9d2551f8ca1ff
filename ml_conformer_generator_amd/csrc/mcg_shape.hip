// Gaussian-volume shape Tanimoto on a regular grid (the grid half of
// `evaluate_samples`): reference cheminformatics/shape_similarity.py:405-492 `tanimoto_score`.
//   density(p) = 1 - prod_atoms (1 - A exp(-alpha |p - c|^2)),  score = <f,g> / (<f,f> + <g,g> - <f,g>)
// One workgroup per (candidate, orientation); the reference's density f is evaluated once.
// Transcendental-bound (n^3 x atoms exponentials), no reuse worth staging beyond the atom list in LDS.
// `k_shape_overlay` ("pose on the reference"): one workgroup per candidate runs all four orientations
// of its handedness-fixed frame in one walk over the grid, picks the best and writes the rigid pose that puts the
// candidate onto the reference's own coordinates.  Both kernels score through `mcg_shape::overlap_scores`
// (mcg_shape_grid.h), so its four scores are bit-identical to `mcg_shape_tanimoto` on the handedness-fixed frames.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;

__global__ __launch_bounds__(256) void k_shape_density(const float* __restrict__ ref, int n_ref,
                                                        const float* __restrict__ axes, int n, float alpha, float amp,
                                                        float* __restrict__ f) {
    __shared__ float c[MAX_ATOMS][3];
    for (int i = threadIdx.x; i < n_ref * 3; i += 256) c[i / 3][i % 3] = ref[i];
    __syncthreads();
    const int total = n * n * n;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const float3 p = grid_point(axes, n, idx);
        f[idx] = density_at(p.x, p.y, p.z, c, n_ref, alpha, amp);
    }
}

__global__ __launch_bounds__(256) void k_shape_overlap(const float* __restrict__ f, const float* __restrict__ cand,
                                                        const int* __restrict__ n_nodes, int N,
                                                        const float* __restrict__ rot /*[R][9]*/, int R,
                                                        const float* __restrict__ axes, int n, float alpha, float amp,
                                                        float* __restrict__ score) {
    __shared__ float c[1][MAX_ATOMS][3];
    __shared__ float red[3][4];
    const int b = blockIdx.x / R, r = blockIdx.x % R;
    const int na = atom_count(n_nodes[b], N);
    for (int i = threadIdx.x; i < na; i += 256) {
        const float* x = cand + ((size_t)b * N + i) * 3;
        rotate_row(x[0], x[1], x[2], rot + r * 9, c[0][i]);       // coord @ M
    }
    __syncthreads();
    const float s = overlap_scores<1>(f, axes, n, c, na, alpha, amp, red);
    if (threadIdx.x == 0) score[blockIdx.x] = s;
}

// det3, dot3_chain and the pose below: the fused forms the compiler chose while contraction was left to it, written out so
// the bits stay.
__device__ __forceinline__ float det3(const float* m) {
    const float c0 = __builtin_fmaf(m[4], m[8], -(m[5] * m[7]));
    const float c1 = __builtin_fmaf(m[3], m[8], -(m[5] * m[6]));
    const float c2 = __builtin_fmaf(m[3], m[7], -(m[4] * m[6]));
    return __builtin_fmaf(m[2], c2, __builtin_fmaf(m[0], c0, -(m[1] * c1)));
}

// a0 b0 + a1 b1 + a2 b2 as the chain of fmaf from 0 that `acc = 0; acc += a_k * b_k` contracted to.
__device__ __forceinline__ float dot3_chain(float a0, float b0, float a1, float b1, float a2, float b2) {
    return __builtin_fmaf(a2, b2, __builtin_fmaf(a1, b1, __builtin_fmaf(a0, b0, 0.f)));
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
    const int na = atom_count(n_nodes[b], N);
    const float* xs = xform + (size_t)b * 12;
    if (tid == 0) s_flip = det3(xs) * det3(ref_xform) < 0.f;      // M_s' = M_s diag(1, 1, -1): a proper Q
    if (tid < 12) zr[tid] = ref_xform[tid];
    __syncthreads();
    const bool flip = s_flip != 0;
    bool bad = false;
    for (int i = tid; i < na; i += 256) {
        const float* x = frames + ((size_t)b * N + i) * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
        bad |= !(isfinite(x0) && isfinite(x1) && isfinite(x2));
#pragma unroll
        for (int w = 0; w < 4; ++w) frame_start(x0, x1, x2, flip, rot + w * 9, c[w][i]);
    }
    const bool frame_bad = __syncthreads_or(bad) != 0;
    const float s = overlap_scores<4>(f, axes, n, c, na, alpha, amp, red);
    if (tid < 4) {
        sc[tid] = s;
        if (score != nullptr) score[b * 4 + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        bool ok = !frame_bad;
        for (int k = 0; k < 12; ++k) ok = ok && isfinite(xs[k]) && isfinite(zr[k]);
        float sb;
        const int wb = first_max4(sc, &sb);
        for (int w = 0; w < 4; ++w) ok = ok && !isnan(sc[w]);
        float Q[9], d[3];
        {   // Q = M_s' @ R_best @ M_r^T,  d = t_r - t_s @ Q; row 2 of M_s' R_best kept only its first product fused
            float S[9], A[9];
            const float* R = rot + wb * 9;
            for (int k = 0; k < 9; ++k) S[k] = k % 3 == 2 && flip ? -xs[k] : xs[k];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    const float* a = S + i * 3;
                    A[i * 3 + j] = i < 2 ? dot3_chain(a[0], R[j], a[1], R[3 + j], a[2], R[6 + j])
                                         : (__builtin_fmaf(a[0], R[j], 0.f) + a[1] * R[3 + j]) + a[2] * R[6 + j];
                }
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    Q[i * 3 + j] = dot3_chain(A[i * 3], zr[j * 3], A[i * 3 + 1], zr[j * 3 + 1], A[i * 3 + 2], zr[j * 3 + 2]);
            for (int j = 0; j < 3; ++j) d[j] = zr[9 + j] - dot3_chain(xs[9], Q[j], xs[10], Q[3 + j], xs[11], Q[6 + j]);
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
            posed_row_overlay(c[wb][i], zr, out);
        }
    }
}

// The reference's density f[n^3] on its grid.
void launch_density(const float* ref, int n_ref, const float* axes, int n, float alpha, float amplitude, float* f,
                    hipStream_t s) {
    const int total = n * n * n;
    hipLaunchKernelGGL(k_shape_density, dim3((total + 255) / 256), dim3(256), 0, s, ref, n_ref, axes, n, alpha, amplitude,
                       f);
}

}  // namespace

extern "C" int mcg_shape_tanimoto(const float* ref, int n_ref, const float* cand, const int32_t* n_nodes_dev, int B, int N,
                                  const float* rot, int R, const float* axes, int n, float alpha, float amplitude,
                                  float* f_scratch, float* score, void* stream) {
    if (!ref || !cand || !n_nodes_dev || !rot || !axes || !f_scratch || !score || n_ref < 1 || n_ref > MAX_ATOMS ||
        B < 1 || N < 1 || N > MAX_ATOMS || R < 1 || n < 2) {
        mcg_set_error("mcg_shape_tanimoto: bad arguments (non-null buffers, 1 <= n_ref <= %d, B >= 1, 1 <= N <= %d, R >= 1, "
                      "n >= 2)", MAX_ATOMS, MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    launch_density(ref, n_ref, axes, n, alpha, amplitude, f_scratch, s);
    hipLaunchKernelGGL(k_shape_overlap, dim3(B * R), dim3(256), 0, s, f_scratch, cand, n_nodes_dev, N, rot, R, axes, n, alpha,
                       amplitude, score);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

int mcg_shape_overlay_launch(const char* who, bool more_ok, const char* more, const float* ref_frame, int n_ref,
                             const float* ref_xform, const float* frames, const float* xform, const int32_t* n_nodes_dev,
                             int B, int N, const float* rot, const float* axes, int n, float alpha, float amplitude,
                             float* f_scratch, float* score, float* best, int32_t* which, int32_t* flipped, float* pose,
                             float* posed, void* stream) {
    if (!more_ok || !ref_frame || !ref_xform || !frames || !xform || !n_nodes_dev || !rot || !axes || !f_scratch || !best ||
        !which || !flipped || !pose || !posed || B < 1 || N < 1 || N > MAX_ATOMS || n_ref < 3 || n_ref > MAX_ATOMS ||
        n < 2) {
        mcg_set_error("%s: bad arguments (non-null buffers, B >= 1, 1 <= N <= %d, 3 <= n_ref <= %d, n >= 2%s)", who,
                      MAX_ATOMS, MAX_ATOMS, more);
        return MCG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    launch_density(ref_frame, n_ref, axes, n, alpha, amplitude, f_scratch, s);
    hipLaunchKernelGGL(k_shape_overlay, dim3(B), dim3(256), 0, s, f_scratch, ref_xform, frames, xform, n_nodes_dev, N, rot,
                       axes, n, alpha, amplitude, score, best, which, flipped, pose, posed);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_shape_overlay(const float* ref_frame, int n_ref, const float* ref_xform, const float* frames,
                                 const float* xform, const int32_t* n_nodes_dev, int B, int N, const float* rot,
                                 const float* axes, int n, float alpha, float amplitude, float* f_scratch, float* score,
                                 float* best, int32_t* which, int32_t* flipped, float* pose, float* posed, void* stream) {
    return mcg_shape_overlay_launch("mcg_shape_overlay", true, "", ref_frame, n_ref, ref_xform, frames, xform, n_nodes_dev,
                                    B, N, rot, axes, n, alpha, amplitude, f_scratch, score, best, which, flipped, pose,
                                    posed, stream);
}

// The two entries above with the density launch skipped: f[n^3] is the caller's (the occupancy of a solid, mcg_mesh.hip, or
// anything else on the grid of `axes`).  The same kernels: with f = what k_shape_density would have written, the same bits.
extern "C" int mcg_shape_tanimoto_field(const float* f, const float* cand, const int32_t* n_nodes_dev, int B, int N,
                                        const float* rot, int R, const float* axes, int n, float alpha, float amplitude,
                                        float* score, void* stream) {
    if (!f || !cand || !n_nodes_dev || !rot || !axes || !score || B < 1 || N < 1 || N > MAX_ATOMS || R < 1 || n < 2) {
        mcg_set_error("mcg_shape_tanimoto_field: bad arguments (non-null buffers, B >= 1, 1 <= N <= %d, R >= 1, n >= 2)",
                      MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    hipLaunchKernelGGL(k_shape_overlap, dim3(B * R), dim3(256), 0, (hipStream_t)stream, f, cand, n_nodes_dev, N, rot, R, axes,
                       n, alpha, amplitude, score);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_shape_overlay_field(const float* f, const float* ref_xform, const float* frames, const float* xform,
                                       const int32_t* n_nodes_dev, int B, int N, const float* rot, const float* axes, int n,
                                       float alpha, float amplitude, float* score, float* best, int32_t* which,
                                       int32_t* flipped, float* pose, float* posed, void* stream) {
    if (!f || !ref_xform || !frames || !xform || !n_nodes_dev || !rot || !axes || !best || !which || !flipped || !pose ||
        !posed || B < 1 || N < 1 || N > MAX_ATOMS || n < 2) {
        mcg_set_error("mcg_shape_overlay_field: bad arguments (non-null buffers, B >= 1, 1 <= N <= %d, n >= 2)", MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    hipLaunchKernelGGL(k_shape_overlay, dim3(B), dim3(256), 0, (hipStream_t)stream, f, ref_xform, frames, xform, n_nodes_dev,
                       N, rot, axes, n, alpha, amplitude, score, best, which, flipped, pose, posed);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
