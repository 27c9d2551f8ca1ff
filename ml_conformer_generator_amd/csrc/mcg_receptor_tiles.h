// Device pieces shared by the kernels that reach a receptor through its 256-atom tiles (`k_receptor_interactions`,
// `k_receptor_optimise`, `k_receptor_relieve`; DESIGN.md section 6, "Shared device text"): a workgroup maximum and
// the list of the tiles whose bounding sphere comes within reach of the ligand.  One text, so the three
// kernels keep the same tiles in the same order.  Contraction is off inside the bodies: every product and sum is rounded
// on its own.  Every helper is called by all 256 lanes of the workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/mlconfgen_hip.h"

namespace mcg_tiles {

constexpr int TILE_ATOMS = 256;               // receptor atoms per tile = lanes per workgroup
constexpr int TILE_WAVES = TILE_ATOMS / 64;
constexpr int MAX_RECEPTOR_TILES = MCG_RECEPTOR_MAX_ATOMS / TILE_ATOMS;
// What the reach of the tile test adds to the exact bound: the centroid, rho and the test itself are rounded, G drifts
// from a rotation by a few ulp per accepted step and the shift test is itself rounded, all far below 1e-3 of the lengths
// involved.
constexpr float TILE_SLACK_ABS = 0.05f, TILE_SLACK_REL = 1e-3f;

static_assert(MCG_RECEPTOR_MAX_ATOMS % TILE_ATOMS == 0, "the tile list holds every tile of the largest receptor");
static_assert(TILE_WAVES == 4, "the trees below have four leaves");

// The kept tiles of one workgroup, in ascending order; sits in the kernel's shared struct.
template <int MAX_TILES>
struct TileList {
    int wave_tiles[TILE_WAVES];               // per wave: tiles kept in the round being compacted
    int n_tiles;
    unsigned short list[MAX_TILES];
};

// v[k] = the maximum of v[k] over the workgroup, K values at once: a butterfly per wave, then the four waves' values
// through red[4][K] in LDS.  A maximum is exact in any order.  `lane`, `wave`: the caller's threadIdx.x & 63 and >> 6.
// Ends past the barrier, with the result in every lane.
template <int K>
__device__ __forceinline__ void block_max4(float (*red)[K], float* v, int lane, int wave) {
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = fmaxf(v[k], __shfl_xor(v[k], o, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = fmaxf(fmaxf(red[0][k], red[1][k]), fmaxf(red[2][k], red[3][k]));
}

// The tiles t < T within reach of the ligand, in ascending order, into tl: tile t is kept unless
// |q_t - c| > lim, c = (cx, cy, cz), lim = reach + (ABS + REL * reach), reach = reach0 + radius_t, with
// (q_t, radius_t) = tile_sphere[t];
// without tile_sphere every tile is kept.  The caller states reach0, everything but the tile's own radius.  A ballot per
// wave over 256 tiles a round, the waves' counts prefix-summed through LDS.  Ends with the barrier that makes n_tiles
// visible.
template <int MAX_TILES>
__device__ __forceinline__ void build_tile_list(TileList<MAX_TILES>& tl, const float4* __restrict__ tile_sphere, int T,
                                                float cx, float cy, float cz, float reach0) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, a = tid & 63, w = tid >> 6;
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += TILE_ATOMS) {
        const int t = t0 + tid;
        bool keep = t < T;
        if (keep && tile_sphere != nullptr) {
            const float4 q = tile_sphere[t];
            const float dx = q.x - cx, dy = q.y - cy, dz = q.z - cz;
            const float reach = reach0 + q.w;
            const float lim = reach + (TILE_SLACK_ABS + TILE_SLACK_REL * reach);
            keep = !(((dx * dx + dy * dy) + dz * dz) > lim * lim);          // a NaN sphere keeps its tile
        }
        const unsigned long long m = __ballot(keep);
        if (a == 0) tl.wave_tiles[w] = __popcll(m);
        __syncthreads();
        int before = base;
        for (int v = 0; v < w; ++v) before += tl.wave_tiles[v];
        if (keep) tl.list[before + __popcll(m & ((1ull << a) - 1ull))] = (unsigned short)t;
        base += (tl.wave_tiles[0] + tl.wave_tiles[1]) + (tl.wave_tiles[2] + tl.wave_tiles[3]);
        __syncthreads();
    }
    if (tid == 0) tl.n_tiles = base;
    __syncthreads();
}

}  // namespace mcg_tiles
