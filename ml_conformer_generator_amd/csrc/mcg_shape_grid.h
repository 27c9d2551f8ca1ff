// Device helpers shared by the grid-overlap kernels of mcg_shape.hip (`k_shape_overlap`, `k_shape_overlay`): the row-vector
// rotation and the Gaussian density at one grid point.  Every multiply-add is written out (fmaf where one is fused) and
// contraction is off inside the bodies, so the compiler has no choice left and both kernels produce the same bits for the
// same inputs, however it schedules or packs them.  The expressions are the ones the compiler chose for the original
// unannotated code, so `mcg_shape_tanimoto`'s outputs did not change when they moved here.
#pragma once

#include <hip/hip_runtime.h>

namespace mcg_shape {

constexpr int MAX_ATOMS = 64;

// out = x @ m  (row vector times row-major 3x3: rotate_coord, shape_similarity.py:448-463)
__device__ __forceinline__ void rotate_row(float x0, float x1, float x2, const float* m, float* out) {
#pragma clang fp contract(off)
    out[0] = __builtin_fmaf(x2, m[6], __builtin_fmaf(x0, m[0], x1 * m[3]));
    out[1] = __builtin_fmaf(x2, m[7], __builtin_fmaf(x0, m[1], x1 * m[4]));
    out[2] = __builtin_fmaf(x2, m[8], __builtin_fmaf(x0, m[2], x1 * m[5]));
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

}  // namespace mcg_shape
