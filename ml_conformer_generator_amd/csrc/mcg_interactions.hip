// Receptor interactions ("Receptor interactions"; the definition is the module docstring of
// interactions.py): an empirical interaction score of every posed molecule against a typed receptor - the functional form
// of the AutoDock Vina scoring function on the package's own heavy-atom types, intermolecular terms only.
//   k_receptor_interactions: one 256-lane workgroup per molecule.  Lane l holds ligand atom a = l & 63 in registers
//                       (coordinates, radius, type); wave w = l >> 6 walks the receptor atoms j = w, w + 4, ... of each
//                       kept 256-atom tile, tiles and atoms in ascending order.  A tile is staged in LDS as float4
//                       (x, y, z, R_j) plus one type byte per atom and read by broadcast: every lane of a wave reads the
//                       same address.  Pair (i, j): r2 = dx*dx + dy*dy + dz*dz, rounded one by one in that order; the pair
//                       COUNTS iff r2 < 64; d = sqrtf(r2) - (R_i + R_j); the five terms of a counted pair go to the
//                       lane's five fp32 accumulators and one integer, a pair that does not count adds nothing.  The four
//                       waves' partials of an atom are combined as (w0 + w1) + (w2 + w3) through LDS, the molecule's sums
//                       are a fixed butterfly over the 64 atom slots in wave 0 (padded slots hold 0).  No atomics.
//   Tile list:          with `tile_sphere` the workgroup keeps only the tiles whose bounding sphere comes within the cut-off
//                       of the ligand's (`mcg_tiles::build_tile_list`, mcg_receptor_tiles.h), with the reach rho + 8: c
//                       the atom centroid, rho the ligand's radius about it.  Every pair of a tile left out has r2 >= 64
//                       and would add nothing, so the list changes no bit of the result.
// A molecule's outputs depend on its own atoms and the receptor arrays only: bit-identical whatever the batch, row or width.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"
#include "mcg_receptor_tiles.h"
#include "mcg_interaction_pair.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;
using namespace mcg_tiles;           // the centroid and the tile list, shared by every kernel that reaches a receptor
using namespace mcg_interaction;     // the pair arithmetic, shared with k_receptor_optimise

struct InteractionShared {
    float4 tile[IX_THREADS];                  // the staged receptor tile: x, y, z, R_j
    unsigned char type[IX_THREADS];
    float part[IX_WAVES][MAX_ATOMS][5];       // per wave and atom: g1, g2, rep, hyd, hb
    int hb_part[IX_WAVES][MAX_ATOMS];
    float c[3];
    float reach[IX_WAVES][1];                 // per wave: max |x_i - c|^2
    TileList<MAX_RECEPTOR_TILES> tiles;
};

__global__ __launch_bounds__(IX_THREADS) void k_receptor_interactions(
    const float* __restrict__ lig, const float* __restrict__ lig_r, const unsigned char* __restrict__ lig_t,
    const int* __restrict__ n_nodes, const int* __restrict__ n_rot, int N, const float4* __restrict__ rec,
    const unsigned char* __restrict__ rec_t, int R, const float4* __restrict__ tile_sphere,
    float* __restrict__ atom_terms, float* __restrict__ mol_terms, int* __restrict__ hbonds) {
    __shared__ InteractionShared s;
    const int b = blockIdx.x, tid = threadIdx.x, a = tid & 63, w = tid >> 6;
    const int na = atom_count(n_nodes[b], N);
    float* at = atom_terms + (size_t)b * N * 6;
    float* mt = mol_terms + (size_t)b * 8;
    const bool real = a < na;
    float x = 0.f, y = 0.f, z = 0.f, ri = 0.f;
    unsigned ti = 0u;
    if (real) {
        const float* p = lig + ((size_t)b * N + a) * 3;
        x = p[0]; y = p[1]; z = p[2];
        ri = lig_r[(size_t)b * N + a];
        ti = lig_t[(size_t)b * N + a];
    }
    const bool bad = real && !(isfinite(x) && isfinite(y) && isfinite(z));
    if (__syncthreads_or(bad) != 0 || na == 0) {                   // NaN floats and -1, or - no atoms - zeros
        const float v = na == 0 ? 0.f : __builtin_nanf("");
        for (int q = tid; q < N * 6; q += IX_THREADS) at[q] = q < na * 6 ? v : 0.f;
        if (tid < 8) mt[tid] = tid < 7 ? v : 0.f;
        if (tid == 0) hbonds[b] = na == 0 ? 0 : -1;
        return;
    }
    if (w == 0) s.part[0][a][0] = x, s.part[0][a][1] = y, s.part[0][a][2] = z;      // borrowed for the centroid
    __syncthreads();
    if (tid < 3) {                            // atom centroid, summed in atom order (inline: DESIGN.md section 6)
        float acc = 0.f;
        for (int i = 0; i < na; ++i) acc += s.part[0][i][tid];
        s.c[tid] = acc / (float)na;
    }
    __syncthreads();
    const float c[3] = {s.c[0], s.c[1], s.c[2]};
    float rho2 = 0.f;
    if (real) {
        const float ux = x - c[0], uy = y - c[1], uz = z - c[2];
        rho2 = (ux * ux + uy * uy) + uz * uz;
    }
    block_max4<1>(s.reach, &rho2, a, w);
    build_tile_list(s.tiles, tile_sphere, (R + IX_THREADS - 1) / IX_THREADS, c[0], c[1], c[2], sqrtf(rho2) + IX_CUTOFF);

    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int nhb = 0;
    const int nt = s.tiles.n_tiles;
    for (int k = 0; k < nt; ++k) {
        const int j0 = (int)s.tiles.list[k] * IX_THREADS;
        const int cnt = min(IX_THREADS, R - j0);                   // the last tile's tail
        if (tid < cnt) {
            s.tile[tid] = rec[j0 + tid];
            s.type[tid] = rec_t[j0 + tid];
        }
        __syncthreads();
        for (int jj = w; jj < cnt; jj += IX_WAVES) {
            const float4 q = s.tile[jj];
            float dx, dy, dz;
            const float r2 = pair_r2(x, y, z, q, dx, dy, dz);
            const bool counts = real && r2 < IX_CUTOFF2;
            if (__ballot(counts) == 0ull) continue;                // nobody in this wave: nothing is added
            if (counts) pair_terms(r2, ri, q.w, ti, s.type[jj], acc, nhb);
        }
        __syncthreads();                      // the tile is free again
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) s.part[w][a][k] = acc[k];
    s.hb_part[w][a] = nhb;
    __syncthreads();
    if (w != 0) return;
    float t[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] = (s.part[0][a][k] + s.part[1][a][k]) + (s.part[2][a][k] + s.part[3][a][k]);
    int hb = (s.hb_part[0][a] + s.hb_part[1][a]) + (s.hb_part[2][a] + s.hb_part[3][a]);
    if (a < N) {                              // a padded atom's terms are 0: its lanes added nothing
#pragma unroll
        for (int k = 0; k < 5; ++k) at[a * 6 + k] = t[k];
        at[a * 6 + 5] = real ? weighted(t) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
        for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_xor(t[k], o, 64);
    for (int o = 32; o > 0; o >>= 1) hb += __shfl_xor(hb, o, 64);
    if (a == 0) {
        const float sum = weighted(t);
        const float den = 1.0f + W_ROT * (float)max(n_rot[b], 0);
#pragma unroll
        for (int k = 0; k < 5; ++k) mt[k] = t[k];
        mt[5] = sum;
        mt[6] = sum / den;
        mt[7] = 0.f;
        hbonds[b] = hb;
    }
}

}  // namespace

extern "C" int mcg_receptor_interactions(const float* lig_xyz, const float* lig_radius, const uint8_t* lig_type,
                                         const int32_t* n_nodes_dev, const int32_t* n_rot_dev, int B, int N,
                                         const float* rec_xyzr, const uint8_t* rec_type, int R, const float* tile_sphere,
                                         float* atom_terms, float* mol_terms, int32_t* hbonds, void* stream) {
    static_assert(MAX_ATOMS == 64, "the bound the message below states");
    if (!lig_xyz || !lig_radius || !lig_type || !n_nodes_dev || !n_rot_dev || !rec_xyzr || !rec_type || !atom_terms ||
        !mol_terms || !hbonds || B < 1 || B > MCG_RECEPTOR_MAX_B || N < 1 || N > MAX_ATOMS || R < 1 ||
        R > MCG_RECEPTOR_MAX_ATOMS) {
        mcg_set_error("mcg_receptor_interactions: bad arguments (non-null buffers, 1 <= B <= %d, 1 <= N <= 64, "
                      "1 <= R <= %d)", MCG_RECEPTOR_MAX_B, MCG_RECEPTOR_MAX_ATOMS);
        return MCG_ERR_ARG;
    }
    hipLaunchKernelGGL(k_receptor_interactions, dim3(B), dim3(IX_THREADS), 0, (hipStream_t)stream, lig_xyz, lig_radius,
                       lig_type, n_nodes_dev, n_rot_dev, N, (const float4*)rec_xyzr, rec_type, R,
                       (const float4*)tile_sphere, atom_terms, mol_terms, hbonds);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
