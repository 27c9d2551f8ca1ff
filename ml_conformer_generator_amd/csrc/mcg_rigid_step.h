// Device pieces shared by the rigid-body accept / reject walks (`k_overlay_refine`, `k_receptor_relieve`,
// `k_receptor_optimise`): the 3x3 product, the trial rotation and the Gram-Schmidt pass.  One text, so the three walks form
// a trial rotation with the same operations in the same order.  Contraction is off inside the bodies and the one fused
// multiply-add is written out, as in mcg_shape_grid.h.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

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

}  // namespace mcg_rigid
