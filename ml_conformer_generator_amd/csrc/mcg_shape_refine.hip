// Refined pose on the reference ("Refined pose"): `mcg_shape_overlay`'s four principal-frame starts,
// each moved as a rigid body to maximise its first-order Gaussian overlap with the reference, then scored on the
// reference's grid; a refined candidate replaces the start pose only where its grid Tanimoto is strictly better.
//   k_overlay_refine:      one 256-lane workgroup per (candidate, orientation).  The start z_w is `mcg_shape::frame_start`,
//                          as `k_shape_overlay` builds it; the reference y and the start sit in LDS.  Objective
//                          O(y, z) = sum_ij A^2 (pi / 2 alpha)^1.5 exp(-(alpha / 2) |y_i - z_j|^2), rigid motion
//                          z' = (z - c) @ G + p (c the start's atom centroid, p where it is now).  Every step takes a
//                          normalised-gradient move (angle s_r about the torque, length s_t along the force:
//                          `rotate_about<false>` and `step_along` of mcg_rigid_step.h, G made orthonormal once, after
//                          the last step), keeps it
//                          only if O strictly increases (then both lengths x 1.2; else both x 0.5), for `steps` steps.
//                          Lane l owns the pairs q = l + 256 k of q = i * n + j; the seven sums (O, force, torque) are
//                          reduced by a fixed butterfly per wave and the tree (w0 + w1) + (w2 + w3), read by every lane,
//                          so every lane holds the same state and takes the same branch.  No atomics.
//   k_overlay_refine_pick: one 256-lane workgroup per candidate.  The four refined candidates z_w @ G_w + t_w are scored
//                          by `mcg_shape::overlap_scores<4>`, as `k_shape_overlay` scores the starts, so a candidate with
//                          G = I, t = 0 scores the bits its start scored.  The first maximum replaces the start only if
//                          strictly better; the pose is then Q = M_s' R_w G M_r^T, d = t_r + t_w @ M_r^T - t_s @ Q.
// Everything depends on the candidate's own atoms and the reference only: bit-identical whatever the batch, row or width.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"
#include "mcg_rigid_step.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;
using namespace mcg_rigid;     // the trial, the step lengths, the returned transform, the sums: one text for every walk

constexpr int RF_THREADS = GRID_THREADS;
constexpr int RF_WAVES = RF_THREADS / 64;
constexpr float RF_STEP_ROT = 0.2f;       // initial rotation step, rad
constexpr float RF_STEP_TRANS = 0.5f;     // initial translation step, Angstrom

// ws per (candidate, orientation): G row-major [9], then t [3] with z' = z @ G + t
constexpr int RF_WS = 12;

struct RefineShared {
    float y[MAX_ATOMS][3];        // the reference frame
    float r[MAX_ATOMS][3];        // the start minus its atom centroid
    float rr[MAX_ATOMS][3];       // r @ G of the pose being evaluated
    float red[RF_WAVES][7];
    float c[3];
};

// O / force / torque sums of the pose (G, p) into v[7]: sum e, sum e d, sum e (rr x (y - p)), d = y - p - rr; identical
// in every lane.
__device__ void evaluate(RefineShared& s, int n_ref, int na, const float* G, const float* p, float half_alpha, float* v) {
    const int tid = threadIdx.x;
    if (tid < na) rotate_row(s.r[tid][0], s.r[tid][1], s.r[tid][2], G, s.rr[tid]);
    __syncthreads();
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int total = n_ref * na;
    for (int q = tid; q < total; q += RF_THREADS) {
        const int i = q / na, j = q - i * na;
        const float yx = s.y[i][0] - p[0], yy = s.y[i][1] - p[1], yz = s.y[i][2] - p[2];
        const float rx = s.rr[j][0], ry = s.rr[j][1], rz = s.rr[j][2];
        const float dx = yx - rx, dy = yy - ry, dz = yz - rz;
        const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        const float e = __expf(-half_alpha * d2);
        acc[0] += e;
        acc[1] = __builtin_fmaf(e, dx, acc[1]);
        acc[2] = __builtin_fmaf(e, dy, acc[2]);
        acc[3] = __builtin_fmaf(e, dz, acc[3]);
        acc[4] = __builtin_fmaf(e, ry * yz - rz * yy, acc[4]);
        acc[5] = __builtin_fmaf(e, rz * yx - rx * yz, acc[5]);
        acc[6] = __builtin_fmaf(e, rx * yy - ry * yx, acc[6]);
    }
    block_sums<7>(acc, s.red, v);
}

__global__ __launch_bounds__(RF_THREADS) void k_overlay_refine(const float* __restrict__ ref_frame, int n_ref,
                                                               const float* __restrict__ frames,
                                                               const int* __restrict__ n_nodes, int N,
                                                               const float* __restrict__ rot /*[4][9]*/,
                                                               const int* __restrict__ flipped,
                                                               const int* __restrict__ which, int steps,
                                                               float half_alpha, float pref, float* __restrict__ ws,
                                                               float* __restrict__ objective) {
    __shared__ RefineShared s;
    const int b = blockIdx.x >> 2, w = blockIdx.x & 3, tid = threadIdx.x;
    float* out = ws + (size_t)blockIdx.x * RF_WS;
    if (which[b] < 0) {                       // failed in k_shape_overlay: the pick leaves the row alone
        if (tid < RF_WS) out[tid] = __builtin_nanf("");
        if (objective != nullptr && tid < 2) objective[(size_t)blockIdx.x * 2 + tid] = __builtin_nanf("");
        return;
    }
    const int na = atom_count(n_nodes[b], N);
    const bool flip = flipped[b] != 0;
    for (int i = tid; i < n_ref * 3; i += RF_THREADS) s.y[i / 3][i % 3] = ref_frame[i];
    if (tid < na) {                           // z_w
        const float* x = frames + ((size_t)b * N + tid) * 3;
        frame_start(x[0], x[1], x[2], flip, rot + w * 9, s.r[tid]);
    }
    __syncthreads();
    atom_centroid(&s.r[0][0], 3, na, max(na, 1), s.c);
    const float c[3] = {s.c[0], s.c[1], s.c[2]};
    __syncthreads();
    if (tid < na) {
        for (int k = 0; k < 3; ++k) s.r[tid][k] = s.r[tid][k] - c[k];
    }
    float G[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, p[3] = {c[0], c[1], c[2]};
    float cur[7];
    evaluate(s, n_ref, na, G, p, half_alpha, cur);
    const float o_start = cur[0];
    StepLengths len = {RF_STEP_ROT, RF_STEP_TRANS};
    for (int it = 0; it < steps; ++it) {
        float Gn[9], pn[3];
        const float fn = norm3(cur + 1), tn = norm3(cur + 4);
        if (tn > 0.f) {
            rotate_about<false>(G, cur[4] / tn, cur[5] / tn, cur[6] / tn, len.rot, Gn);
        } else {
            for (int k = 0; k < 9; ++k) Gn[k] = G[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) pn[k] = step_along(p[k], cur[1 + k], fn, fn > 0.f, len.trans);
        float nxt[7];
        evaluate(s, n_ref, na, Gn, pn, half_alpha, nxt);
        if (nxt[0] > cur[0]) {
            keep_trial<7>(G, p, cur, Gn, pn, nxt);
            len.grow();
        } else {
            len.shrink();
        }
    }
    orthonormalise(G);
    if (tid == 0) {
        write_transform(G, p, c[0], c[1], c[2], out);
        if (objective != nullptr) {
            objective[(size_t)blockIdx.x * 2] = pref * o_start;
            objective[(size_t)blockIdx.x * 2 + 1] = pref * cur[0];
        }
    }
}

// xform = M row-major [9], then t [3]: frames = (coords - t) @ M on the real rows (mcg_shape_frames_tf).
__global__ __launch_bounds__(RF_THREADS) void k_overlay_refine_pick(
    const float* __restrict__ f, const float* __restrict__ ref_xform, const float* __restrict__ frames,
    const float* __restrict__ xform, const int* __restrict__ n_nodes, int N, const float* __restrict__ rot /*[4][9]*/,
    const float* __restrict__ axes, int n, float alpha, float amp, const float* __restrict__ ws,
    const int* __restrict__ flipped, int* __restrict__ which, float* __restrict__ best, float* __restrict__ pose,
    float* __restrict__ posed, float* __restrict__ start_best, int* __restrict__ refined,
    float* __restrict__ refined_score) {
    __shared__ float c[4][MAX_ATOMS][3];      // the four refined candidates
    __shared__ float red[9][4];               // per wave: fg[4], gg[4], ff
    __shared__ float sc[4];
    __shared__ float zr[12];                  // M_r row-major, then t_r
    __shared__ int s_pick;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (which[b] < 0) {                       // failed in k_shape_overlay: left exactly as it was
        if (tid == 0) { start_best[b] = best[b]; refined[b] = 0; }
        if (refined_score != nullptr && tid < 4) refined_score[b * 4 + tid] = __builtin_nanf("");
        return;
    }
    const int na = atom_count(n_nodes[b], N);
    const bool flip = flipped[b] != 0;
    if (tid < 12) zr[tid] = ref_xform[tid];
    for (int i = tid; i < na; i += RF_THREADS) {
        const float* x = frames + ((size_t)b * N + i) * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float* gt = ws + ((size_t)b * 4 + w) * RF_WS;
            float z[3], g[3];
            frame_start(x0, x1, x2, flip, rot + w * 9, z);
            rotate_row(z[0], z[1], z[2], gt, g);
            c[w][i][0] = g[0] + gt[9]; c[w][i][1] = g[1] + gt[10]; c[w][i][2] = g[2] + gt[11];
        }
    }
    __syncthreads();
    const float sw = overlap_scores<4>(f, axes, n, c, na, alpha, amp, red);
    if (tid < 4) {
        sc[tid] = sw;
        if (refined_score != nullptr) refined_score[b * 4 + tid] = sw;
    }
    __syncthreads();
    if (tid == 0) {
        float sb;
        const int wb = first_max4(sc, &sb);
        const float start = best[b];
        const bool take = sb > start;                               // strictly better (NaN never is)
        start_best[b] = start;
        refined[b] = take ? 1 : 0;
        if (take) {
            const float* xs = xform + (size_t)b * 12;
            const float* gt = ws + ((size_t)b * 4 + wb) * RF_WS;
            const float* R = rot + wb * 9;
            float A[9], RG[9], Q[9], d[3];
            for (int i = 0; i < 3; ++i)                             // A = M_s' (diag(1, 1, -1) on the flipped rows)
                for (int k = 0; k < 3; ++k) A[i * 3 + k] = k == 2 && flip ? -xs[i * 3 + k] : xs[i * 3 + k];
            mat3_mul(R, gt, RG);
            float ARG[9];
            mat3_mul(A, RG, ARG);
            for (int i = 0; i < 3; ++i)                             // Q = A R G M_r^T
                for (int j = 0; j < 3; ++j)
                    Q[i * 3 + j] = __builtin_fmaf(ARG[i * 3 + 2], zr[j * 3 + 2],
                                                  __builtin_fmaf(ARG[i * 3], zr[j * 3], ARG[i * 3 + 1] * zr[j * 3 + 1]));
            for (int j = 0; j < 3; ++j) {                           // d = t_r + t_w @ M_r^T - t_s @ Q
                const float tw = __builtin_fmaf(gt[11], zr[j * 3 + 2], __builtin_fmaf(gt[9], zr[j * 3], gt[10] * zr[j * 3 + 1]));
                const float ts = __builtin_fmaf(xs[11], Q[6 + j], __builtin_fmaf(xs[9], Q[j], xs[10] * Q[3 + j]));
                d[j] = (zr[9 + j] + tw) - ts;
            }
            best[b] = sb;
            which[b] = wb;
            for (int k = 0; k < 9; ++k) pose[(size_t)b * 12 + k] = Q[k];
            for (int k = 0; k < 3; ++k) pose[(size_t)b * 12 + 9 + k] = d[k];
        }
        s_pick = take ? wb : -1;
    }
    __syncthreads();
    const int wb = s_pick;
    if (wb < 0) return;
    for (int i = tid; i < na; i += RF_THREADS)     // x_out = z' @ M_r^T + t_r; padded rows stay zero
        posed_row_pick(c[wb][i], zr, posed + ((size_t)b * N + i) * 3);
}

}  // namespace

extern "C" int mcg_shape_overlay_refined(const float* ref_frame, int n_ref, const float* ref_xform, const float* frames,
                                         const float* xform, const int32_t* n_nodes_dev, int B, int N, const float* rot,
                                         const float* axes, int n, float alpha, float amplitude, float* f_scratch,
                                         float* score, float* best, int32_t* which, int32_t* flipped, float* pose,
                                         float* posed, int steps, float* refine_ws, float* objective, float* start_best,
                                         int32_t* refined, float* refined_score, void* stream) {
    static_assert(WALK_MAX_STEPS == 1024, "the bound the message below states");
    const bool own_ok = refine_ws && start_best && refined && steps >= 0 && steps <= WALK_MAX_STEPS && alpha > 0.f;
    if (int rc = mcg_shape_overlay_launch("mcg_shape_overlay_refined", own_ok, ", 0 <= steps <= 1024, alpha > 0",
                                          ref_frame, n_ref, ref_xform, frames, xform, n_nodes_dev, B, N, rot, axes, n,
                                          alpha, amplitude, f_scratch, score, best, which, flipped, pose, posed, stream))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const double a = (double)alpha, amp = (double)amplitude;
    const float pref = (float)(amp * amp * pow(M_PI / (2.0 * a), 1.5));
    hipLaunchKernelGGL(k_overlay_refine, dim3(B * 4), dim3(RF_THREADS), 0, s, ref_frame, n_ref, frames, n_nodes_dev, N, rot,
                       flipped, which, steps, (float)(0.5 * a), pref, refine_ws, objective);
    hipLaunchKernelGGL(k_overlay_refine_pick, dim3(B), dim3(RF_THREADS), 0, s, f_scratch, ref_xform, frames, xform,
                       n_nodes_dev, N, rot, axes, n, alpha, amplitude, refine_ws, flipped, which, best, pose, posed,
                       start_best, refined, refined_score);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
