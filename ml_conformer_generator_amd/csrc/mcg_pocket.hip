// Blocked-ray masks of a grid round a place on a receptor ("Pockets from the receptor"): per grid point,
// which of 26 rays of length `reach` meet a receptor atom's van der Waals sphere, and whether a probe sphere on the point
// would overlap one.  The definition is in include/mlconfgen_hip_pocket.h; the host grows the pocket from the masks.
//   k_pocket_masks:  one lane per grid point; a workgroup of 256 lanes covers a compact brick of 4 x 8 x 8 points (the last
//                    index fastest, so a wave stores runs of 8 consecutive masks), whose bounding sphere is small:
//                    `mcg_tiles::build_tile_list` keeps only the receptor tiles within half the brick's diagonal + the
//                    reach of a point of the brick's centre.  A kept tile is staged in LDS as float4 and every lane reads
//                    the same atom by broadcast.  blockIdx.y = part s of S = gridDim.y walks the kept tiles
//                    [s K / S, (s + 1) K / S) of its brick's K.  S = 1 stores the mask; S > 1 ORs the part into an output the
//                    launcher has zeroed on the same stream (a vector atomic; lanes whose part is 0 add nothing).
// An OR is exact in any order and each (point, atom) pair is decided from that pair alone, so a point's mask has the same
// bits whatever the receptor's order, the tile skipping and S.  fp32, contraction off, no inline assembly.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_receptor_tiles.h"
#include "../../include/mlconfgen_hip_pocket.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

using mcg_tiles::MAX_RECEPTOR_TILES;
using mcg_tiles::TILE_ATOMS;

constexpr int PK_BI = 4, PK_BJ = 8, PK_BL = 8;          // the brick: points per axis (i slowest, l fastest)
static_assert(PK_BI * PK_BJ * PK_BL == TILE_ATOMS, "one lane per point of a brick, one staged atom per lane");
// half the brick's diagonal in units of the spacing: sqrt(3^2 + 7^2 + 7^2) / 2 = 5.17204..., rounded up
constexpr float PK_HALF_DIAGONAL = 5.172041f;
// An atom farther than max(reach, probe) + r + PK_SKIP_PAD from a point cannot set a bit of it and is passed over before
// the 26 tests: a blocked ray needs |d| <= t_c + |e| <= reach + r, an occupied point |d| < r + probe.  The pad keeps the
// rounded test from passing over a pair the rounded ray test would still set: it widens the squared limit by
// 2e-3 (reach + r), the roundings of d2 and of e2 come to a few 2^-24 of them - smaller for every length under 1000 A.
// It changes no bit.
constexpr float PK_SKIP_PAD = 1e-3f;

struct Shared {
    float4 atom[TILE_ATOMS];
    mcg_tiles::TileList<MAX_RECEPTOR_TILES> tiles;
};

// The +u / -u pair of direction (A, B, C) (its index K < 13 in the header's order; -u is 25 - K): one dot product serves
// both rays, since t(-u) = -t(u).  A zero component of u leaves e's component equal to d's and is not multiplied out.
template <int A, int B, int C>
__device__ __forceinline__ unsigned ray_pair(float dx, float dy, float dz, float r2, float reach) {
    constexpr int K = (A + 1) * 9 + (B + 1) * 3 + (C + 1);
    static_assert(K < 13, "the first half of the directions; the second is their negatives");
    constexpr int NZ = (A != 0) + (B != 0) + (C != 0);
    constexpr float S = NZ == 1 ? 1.f : (NZ == 2 ? 0.70710678118654752f : 0.57735026918962576f);
    constexpr float ux = A * S, uy = B * S, uz = C * S;
    float t = 0.f;
    bool first = true;
    if constexpr (A != 0) { t = dx * ux; first = false; }
    if constexpr (B != 0) { t = first ? dy * uy : t + dy * uy; first = false; }
    if constexpr (C != 0) { t = first ? dz * uz : t + dz * uz; }
    const float tp = fminf(fmaxf(t, 0.f), reach), tm = fminf(fmaxf(-t, 0.f), reach);
    float px = dx, py = dy, pz = dz, mx = dx, my = dy, mz = dz;
    if constexpr (A != 0) { px = dx - tp * ux; mx = dx + tm * ux; }
    if constexpr (B != 0) { py = dy - tp * uy; my = dy + tm * uy; }
    if constexpr (C != 0) { pz = dz - tp * uz; mz = dz + tm * uz; }
    const float ep = (px * px + py * py) + pz * pz, em = (mx * mx + my * my) + mz * mz;
    return (ep <= r2 ? 1u << K : 0u) | (em <= r2 ? 1u << (25 - K) : 0u);
}

__device__ __forceinline__ unsigned atom_mask(float dx, float dy, float dz, float r2, float reach) {
    return ray_pair<-1, -1, -1>(dx, dy, dz, r2, reach) | ray_pair<-1, -1, 0>(dx, dy, dz, r2, reach) |
           ray_pair<-1, -1, 1>(dx, dy, dz, r2, reach) | ray_pair<-1, 0, -1>(dx, dy, dz, r2, reach) |
           ray_pair<-1, 0, 0>(dx, dy, dz, r2, reach) | ray_pair<-1, 0, 1>(dx, dy, dz, r2, reach) |
           ray_pair<-1, 1, -1>(dx, dy, dz, r2, reach) | ray_pair<-1, 1, 0>(dx, dy, dz, r2, reach) |
           ray_pair<-1, 1, 1>(dx, dy, dz, r2, reach) | ray_pair<0, -1, -1>(dx, dy, dz, r2, reach) |
           ray_pair<0, -1, 0>(dx, dy, dz, r2, reach) | ray_pair<0, -1, 1>(dx, dy, dz, r2, reach) |
           ray_pair<0, 0, -1>(dx, dy, dz, r2, reach);
}

__global__ __launch_bounds__(TILE_ATOMS) void k_pocket_masks(const float4* __restrict__ rec, int R,
                                                             const float4* __restrict__ tile_sphere, int n, float spacing,
                                                             float probe, float reach, unsigned* __restrict__ masks) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    const int nbj = (n + PK_BJ - 1) / PK_BJ, nbl = (n + PK_BL - 1) / PK_BL;
    const int brick = blockIdx.x;
    const int bi = brick / (nbj * nbl), bj = (brick / nbl) % nbj, bl = brick % nbl;
    const int i = bi * PK_BI + (tid >> 6), j = bj * PK_BJ + ((tid >> 3) & 7), l = bl * PK_BL + (tid & 7);
    const bool live = i < n && j < n && l < n;
    const float c = 0.5f * (float)(n - 1);                                   // a whole number or a half: exact
    const float px = ((float)i - c) * spacing, py = ((float)j - c) * spacing, pz = ((float)l - c) * spacing;
    // the brick's centre, its points beyond the grid included: the sphere only grows
    const float cx = ((float)(bi * PK_BI) + 0.5f * (PK_BI - 1) - c) * spacing;
    const float cy = ((float)(bj * PK_BJ) + 0.5f * (PK_BJ - 1) - c) * spacing;
    const float cz = ((float)(bl * PK_BL) + 0.5f * (PK_BL - 1) - c) * spacing;
    const float far = fmaxf(reach, probe);
    const int T = (R + TILE_ATOMS - 1) / TILE_ATOMS;
    mcg_tiles::build_tile_list(sh.tiles, tile_sphere, T, cx, cy, cz, PK_HALF_DIAGONAL * spacing + far);
    const int K = sh.tiles.n_tiles, S = gridDim.y, s = blockIdx.y;
    const int k0 = (int)((long)s * K / S), k1 = (int)((long)(s + 1) * K / S);
    unsigned m = 0u;
    for (int k = k0; k < k1; ++k) {
        const int a0 = (int)sh.tiles.list[k] * TILE_ATOMS, na = min(TILE_ATOMS, R - a0);
        __syncthreads();                                                     // the previous tile is read by every lane
        if (tid < na) sh.atom[tid] = rec[a0 + tid];
        __syncthreads();
        if (live) {
            for (int a = 0; a < na; ++a) {
                const float4 y = sh.atom[a];
                const float dx = y.x - px, dy = y.y - py, dz = y.z - pz;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                const float lim = (far + y.w) + PK_SKIP_PAD;
                if (d2 > lim * lim) continue;
                const float ro = y.w + probe;
                if (d2 < ro * ro) m |= MCG_POCKET_OCCUPIED;
                m |= atom_mask(dx, dy, dz, y.w * y.w, reach);
            }
        }
    }
    if (!live) return;
    unsigned* out = masks + ((size_t)i * n + j) * n + l;
    if (S == 1) *out = m;
    else if (m != 0u) atomicOr(out, m);
}

}  // namespace

extern "C" int mcg_pocket_masks(const float* rec_xyzr, int R, const float* tile_sphere, int n, float spacing, float probe,
                                float reach, int splits, uint32_t* masks, void* stream) {
    const auto positive = [](float v) { return isfinite(v) && v > 0.f; };
    if (!rec_xyzr || !masks || n < 1 || n > MCG_POCKET_MAX_N || R < 1 || R > MCG_RECEPTOR_MAX_ATOMS || !positive(spacing) ||
        !positive(probe) || !positive(reach) || splits < 1 || splits > MCG_POCKET_MAX_SPLITS) {
        mcg_set_error("mcg_pocket_masks: bad arguments (non-null rec_xyzr and masks, 1 <= n <= %d, 1 <= R <= %d, spacing, "
                      "probe and reach finite and > 0, 1 <= splits <= %d)", MCG_POCKET_MAX_N, MCG_RECEPTOR_MAX_ATOMS,
                      MCG_POCKET_MAX_SPLITS);
        return MCG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t P = (size_t)n * n * n;
    if (splits > 1) MCG_HIP(hipMemsetAsync(masks, 0, P * sizeof(uint32_t), s));
    const unsigned bricks = (unsigned)(((n + PK_BI - 1) / PK_BI) * ((n + PK_BJ - 1) / PK_BJ) * ((n + PK_BL - 1) / PK_BL));
    hipLaunchKernelGGL(k_pocket_masks, dim3(bricks, (unsigned)splits), dim3(TILE_ATOMS), 0, s,
                       reinterpret_cast<const float4*>(rec_xyzr), R, reinterpret_cast<const float4*>(tile_sphere), n, spacing,
                       probe, reach, reinterpret_cast<unsigned*>(masks));
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
