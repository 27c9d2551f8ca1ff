// Device pieces shared by the rigid-body accept / reject walks (`k_overlay_refine`, `k_receptor_relieve`,
// `k_receptor_optimise`; DESIGN.md section 6, "Shared device text"): the 3x3 product, the trial rotation and the
// Gram-Schmidt pass, the trial pose (`rotate_about`, `step_along`) and its shift test, the step lengths and their
// factors, the transform a walk returns, the atom centroid and the reduction of a pose's sums.  One text, so the three
// walks form, keep and return a trial with the same operations in the same order, and the walk that is pinned trial by
// trial pins the text the other two run (`k_receptor_optimise_flex` repeats `k_receptor_optimise`'s use of them).
// Contraction is off inside the bodies and every fused multiply-add is written out, as in mcg_shape_grid.h.  Scalars go
// in by value (the centroid, the rotation axis, the components of p): in that shape the helpers leave the kernels the
// instruction streams profiles/walk_share_isa.txt records.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "mcg_shape_grid.h"

namespace mcg_rigid {

// c = a @ b (row-major 3x3)
__device__ __forceinline__ void mat3_mul(const float* a, const float* b, float* c) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            c[i * 3 + j] = __builtin_fmaf(a[i * 3 + 2], b[6 + j], __builtin_fmaf(a[i * 3], b[j], a[i * 3 + 1] * b[3 + j]));
}

// Row-vector form (r' = r @ D) of the rotation by theta about the unit axis n: D = R^T with Rodrigues'
// R = I + sin(theta) K + (1 - cos(theta)) K^2, K v = n x v.
__device__ __forceinline__ void rodrigues_row(float nx, float ny, float nz, float theta, float* D) {
#pragma clang fp contract(off)
    const float s = sinf(theta), c1 = 1.f - cosf(theta);
    const float K[9] = {0.f, -nz, ny, nz, 0.f, -nx, -ny, nx, 0.f};
    const float K2[9] = {-(ny * ny + nz * nz), nx * ny, nx * nz, nx * ny, -(nx * nx + nz * nz), ny * nz,
                         nx * nz, ny * nz, -(nx * nx + ny * ny)};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            D[j * 3 + i] = ((i == j ? 1.f : 0.f) + s * K[i * 3 + j]) + c1 * K2[i * 3 + j];
}

// Rows of G made orthonormal (Gram-Schmidt, third row = first x second: det +1).  The identity stays exactly the identity.
__device__ __forceinline__ void orthonormalise(float* G) {
#pragma clang fp contract(off)
    float a[3] = {G[0], G[1], G[2]}, b[3] = {G[3], G[4], G[5]};
    const float na = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = a[k] / na;
    const float ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = b[k] - ab * a[k];
    const float nb = sqrtf((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = b[k] / nb;
    G[0] = a[0]; G[1] = a[1]; G[2] = a[2];
    G[3] = b[0]; G[4] = b[1]; G[5] = b[2];
    G[6] = a[1] * b[2] - a[2] * b[1];
    G[7] = a[2] * b[0] - a[0] * b[2];
    G[8] = a[0] * b[1] - a[1] * b[0];
}

// |v|, the squares summed as (v0^2 + v1^2) + v2^2
__device__ __forceinline__ float norm3(const float* v) {
#pragma clang fp contract(off)
    return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// Gn = G rotated by sr about the unit axis (nx, ny, nz), the torque over its length.  ORTHO: Gn is made orthonormal again
// as it is formed.  The caller decides whether the trial turns at all (else Gn is G's bits) and divides the torque.
template <bool ORTHO>
__device__ __forceinline__ void rotate_about(const float* G, float nx, float ny, float nz, float sr, float* Gn) {
#pragma clang fp contract(off)
    float D[9];
    rodrigues_row(nx, ny, nz, sr, D);
    mat3_mul(G, D, Gn);
    if (ORTHO) orthonormalise(Gn);
}

// One component of the trial position: p moved by st along the force (f its component, fn = |force|) where `moves`,
// else p's bits.  The caller decides `moves` from fn.
__device__ __forceinline__ float step_along(float p, float f, float fn, bool moves, float st) {
#pragma clang fp contract(off)
    return moves ? p + st * (f / fn) : p;
}

// Whether pn lies within max_shift of c = (cx, cy, cz); true for a NaN.
__device__ __forceinline__ bool within_shift(const float* pn, float cx, float cy, float cz, float max_shift) {
#pragma clang fp contract(off)
    const float sx = pn[0] - cx, sy = pn[1] - cy, sz = pn[2] - cz;
    return !(((sx * sx + sy * sy) + sz * sz) > max_shift * max_shift);
}

constexpr int WALK_MAX_STEPS = 1024;          // the largest step budget an entry takes
constexpr float WALK_GROW = 1.2f, WALK_SHRINK = 0.5f;

// The two step lengths of a walk: both grow after a trial that is kept and shrink after one that is not.
struct StepLengths {
    float rot, trans;                         // rad, Angstrom
    __device__ __forceinline__ void grow() { rot *= WALK_GROW; trans *= WALK_GROW; }
    __device__ __forceinline__ void shrink() { rot *= WALK_SHRINK; trans *= WALK_SHRINK; }
};

// The trial (Gn, pn) with its K sums becomes the pose that holds.
template <int K>
__device__ __forceinline__ void keep_trial(float* G, float* p, float* cur, const float* Gn, const float* pn,
                                           const float* nxt) {
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = Gn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = pn[k];
#pragma unroll
    for (int k = 0; k < K; ++k) cur[k] = nxt[k];
}

// out12 = G row-major, then p - c @ G, c = (cx, cy, cz): x' = (x - c) @ G + p = x @ G + (p - c @ G).  One lane writes it.
__device__ __forceinline__ void write_transform(const float* G, const float* p, float cx, float cy, float cz,
                                                float* out12) {
#pragma clang fp contract(off)
    float cg[3];
    mcg_shape::rotate_row(cx, cy, cz, G, cg);
    for (int k = 0; k < 9; ++k) out12[k] = G[k];
    for (int k = 0; k < 3; ++k) out12[9 + k] = p[k] - cg[k];
}

// out_c[k] = (sum over i < na of rows[i * stride + k]) / (float)den for k < 3, summed in atom order by lanes 0..2 of the
// workgroup.  The rows must be visible to those lanes already; ends with the barrier that makes out_c (LDS) visible to
// every lane.  Every lane calls it.
__device__ __forceinline__ void atom_centroid(const float* rows, int stride, int na, int den, float* out_c) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    if (tid < 3) {
        float acc = 0.f;
        for (int i = 0; i < na; ++i) acc += rows[i * stride + tid];
        out_c[tid] = acc / (float)den;
    }
    __syncthreads();
}

// v[k] = the sum of acc[k] over the 256 lanes of the workgroup, K sums at once: an xor butterfly per wave, then the tree
// (w0 + w1) + (w2 + w3) through red[4][K] in LDS, read by every lane.  Every lane calls it and gets the same bits.
template <int K>
__device__ __forceinline__ void block_sums(float* acc, float (*red)[K], float* v) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[tid >> 6][k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// out[3] = the point (x, y, z) turned right-handed by theta about the line through (bx, by, bz) along the unit vector
// (nx, ny, nz): the row-vector Rodrigues matrix applied to the difference to b, b added back.  For a walk that turns a part
// of a molecule about one of its bonds (`k_receptor_optimise_flex`); b itself comes back with its own bits.
__device__ __forceinline__ void turn_about_line(float x, float y, float z, float bx, float by, float bz, float nx, float ny,
                                                float nz, float theta, float* out) {
#pragma clang fp contract(off)
    float D[9], o[3];
    rodrigues_row(nx, ny, nz, theta, D);
    mcg_shape::rotate_row(x - bx, y - by, z - bz, D, o);
    out[0] = o[0] + bx; out[1] = o[1] + by; out[2] = o[2] + bz;
}

}  // namespace mcg_rigid
