// The pair arithmetic of the receptor interaction score ("Receptor interactions"; the definition is
// the module docstring of interactions.py), shared by the kernel that scores a pose (`k_receptor_interactions`) and the one
// that walks a pose downhill on the score (`k_receptor_optimise`): one text, so both produce the same bits for the same
// pair.  Contraction is off inside the bodies: every product and sum is rounded on its own.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "mcg_receptor_tiles.h"

namespace mcg_interaction {

constexpr int IX_THREADS = mcg_tiles::TILE_ATOMS;             // lanes per workgroup = receptor atoms per tile
constexpr int IX_WAVES = IX_THREADS / 64;
constexpr float IX_CUTOFF = 8.0f, IX_CUTOFF2 = 64.0f;
constexpr float W_G1 = -0.0356f, W_G2 = -0.00516f, W_REP = 0.840f, W_HYD = -0.0351f, W_HB = -0.587f, W_ROT = 0.0585f;
constexpr float HB_FULL = -0.7f;              // a hydrogen bond counts in full at or below this surface distance
constexpr unsigned T_DONOR = 1u, T_ACCEPTOR = 2u, T_HYDROPHOBIC = 4u;

// ((((w1 g1 + w2 g2) + w3 rep) + w4 hyd) + w5 hb): the weighted sum of five terms, in this order
__device__ __forceinline__ float weighted(const float* t) {
#pragma clang fp contract(off)
    return (((W_G1 * t[0] + W_G2 * t[1]) + W_REP * t[2]) + W_HYD * t[3]) + W_HB * t[4];
}

// r2 = dx*dx + dy*dy + dz*dz of ligand atom (x, y, z) and receptor atom q, rounded one by one in that order.
__device__ __forceinline__ float pair_r2(float x, float y, float z, const float4& q, float& dx, float& dy, float& dz) {
#pragma clang fp contract(off)
    dx = x - q.x; dy = y - q.y; dz = z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// The surface distance of a COUNTED pair: d = sqrtf(r2) - (R_i + R_j), the radius sum rounded first; r = sqrtf(r2).  The
// one text every threshold on d is decided from (`pair_terms` below, `k_receptor_contacts`).
__device__ __forceinline__ float pair_surface_distance(float r2, float ri, float rj, float& r) {
#pragma clang fp contract(off)
    r = sqrtf(r2);
    return r - (ri + rj);
}

// What a pair leaves behind for a caller that wants the derivative too: the surface distance, the centre distance, the two
// Gaussians and whether the pair is a donor facing an acceptor.
struct PairValues {
    float d, r, g1, g2;
    bool hb;
};

// The five terms of a COUNTED pair (r2 < IX_CUTOFF2 is the caller's decision) added to acc[5], the full hydrogen bonds to
// nhb: d = sqrtf(r2) - (R_i + R_j), the piecewise terms decided on that fp32 d.
__device__ __forceinline__ PairValues pair_terms(float r2, float ri, float rj, unsigned ti, unsigned tj, float* acc,
                                                 int& nhb) {
#pragma clang fp contract(off)
    PairValues v;
    const float d = pair_surface_distance(r2, ri, rj, v.r);
    const float a1 = d + d;                            // d / 0.5
    const float a2 = (d - 3.0f) * 0.5f;                // (d - 3) / 2
    v.d = d;
    v.g1 = expf(-(a1 * a1));
    v.g2 = expf(-(a2 * a2));
    acc[0] += v.g1;
    acc[1] += v.g2;
    if (d < 0.f) acc[2] += d * d;
    if ((ti & tj & T_HYDROPHOBIC) != 0u && d < 1.5f) acc[3] += d <= 0.5f ? 1.0f : 1.5f - d;
    v.hb = ((ti & T_DONOR) != 0u && (tj & T_ACCEPTOR) != 0u) || ((ti & T_ACCEPTOR) != 0u && (tj & T_DONOR) != 0u);
    if (v.hb && d < 0.f) {
        const bool full = d <= HB_FULL;
        acc[4] += full ? 1.0f : d / HB_FULL;
        nhb += full ? 1 : 0;
    }
    return v;
}

// dW/dd of a counted pair, W the weighted sum of the five terms, from the same fp32 d and the Gaussians `pair_terms`
// left: g1' = -8 d g1, g2' = -((d - 3) / 2) g2, rep' = 2 d where d < 0, hyd' = -1 on 0.5 < d < 1.5 (both hydrophobic),
// hb' = 1 / -0.7f on -0.7f < d < 0 (donor facing acceptor), 0 elsewhere; weighted in the order of `weighted`.
__device__ __forceinline__ float pair_slope(const PairValues& v, unsigned ti, unsigned tj) {
#pragma clang fp contract(off)
    const float d = v.d;
    float s[5];
    s[0] = (-8.0f * d) * v.g1;
    s[1] = -((d - 3.0f) * 0.5f) * v.g2;
    s[2] = d < 0.f ? d + d : 0.f;
    s[3] = ((ti & tj & T_HYDROPHOBIC) != 0u && d > 0.5f && d < 1.5f) ? -1.0f : 0.f;
    s[4] = (v.hb && d > HB_FULL && d < 0.f) ? 1.0f / HB_FULL : 0.f;
    return weighted(s);
}

}  // namespace mcg_interaction
