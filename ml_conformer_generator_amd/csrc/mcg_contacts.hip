// Receptor contacts ("Receptor contacts"; the definition is the module docstring of contacts.py): which
// groups of receptor atoms - residues - a posed molecule touches, with which kind of contact, and how many of a reference
// fingerprint's bits it keeps.
//   k_receptor_contacts: one 256-lane workgroup per molecule, shaped like `k_receptor_interactions`.  Lane l holds ligand
//                       atom a = l & 63 in registers; wave w = l >> 6 walks the receptor atoms j = w, w + 4, ... of each kept
//                       256-atom tile.  A tile is staged in LDS as float4 (x, y, z, R_j), a type byte and the int32 group id.
//                       Pair (i, j): `pair_r2` and `pair_surface_distance` of mcg_interaction_pair.h - the bits the score is
//                       decided on; the four kind bits from that fp32 d.  Per receptor atom the wave's 64 lanes' bits are
//                       reduced by ballots to one wave-uniform value, recorded for the staged atom, and ORed into each lane's
//                       private per-ligand-atom byte.
//   After each tile:    the staged atoms with kinds != 0 are compacted - ballot, the waves' counts prefix-summed through LDS,
//                       as `build_tile_list` does - into the candidate list (group << 8 | kinds), in tile and atom order.
//   After the walk:     the candidates are sorted (a bitonic network over the next power of two, padded with ~0), the heads of
//                       the runs of one group are ranked by the same ballot compaction, and each head ORs its run together:
//                       at most 256 entries in ascending group order.  The four waves' per-atom bytes are ORed through LDS.
//   Reference join:     with `counts` each lane takes an entry and binary-searches the reference list; the three integer sums
//                       are a butterfly per wave and the four waves' values through LDS - exact in any order.
// No atomics anywhere: an OR and an integer sum do not depend on their order, and every list position is a prefix sum.
// A molecule's outputs depend on its own atoms and the receptor arrays only: bit-identical whatever the batch, row or width,
// with and without the tile list.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_shape_grid.h"
#include "mcg_receptor_tiles.h"
#include "mcg_interaction_pair.h"
#include "../../include/mlconfgen_hip_contacts.h"

#include <math.h>

#pragma clang fp contract(off)      // every product and sum rounded on its own: the compiler has no choice left

namespace {

using namespace mcg_shape;
using namespace mcg_tiles;
using namespace mcg_interaction;

constexpr int CT_CAP = MCG_CONTACT_MAX_CANDIDATES;
constexpr int CT_GROUPS = MCG_CONTACT_MAX_GROUPS;
constexpr float CT_CONTACT = 0.5f;            // the surface distance at or below which two atoms are in contact: the score's
//                                               `hyd` term is 1 exactly there
constexpr unsigned long long CT_PAD = ~0ull;  // sorts behind every candidate: a group id is >= 0

static_assert(CT_GROUPS == IX_THREADS, "one lane per entry in the epilogue");
static_assert((CT_CAP & (CT_CAP - 1)) == 0 && CT_CAP >= IX_THREADS, "the bitonic network runs over a power of two");

struct ContactShared {
    float4 tile[IX_THREADS];                  // the staged receptor tile: x, y, z, R_j
    int grp[IX_THREADS];
    unsigned char type[IX_THREADS];
    unsigned char tkinds[IX_THREADS];         // per staged atom: the OR of the kind bits over the ligand's atoms
    unsigned long long cand[CT_CAP];          // group << 8 | kinds of the contacting receptor atoms, then sorted
    int out_grp[CT_GROUPS];
    unsigned char out_kinds[CT_GROUPS];
    unsigned char atom_part[IX_WAVES][MAX_ATOMS];
    float xyz[MAX_ATOMS][3];                  // the centroid's summands
    float c[3];
    float reach[IX_WAVES][1];
    int wave_n[IX_WAVES];                     // per wave: kept in the round being compacted
    int sums[IX_WAVES][3];
    TileList<MAX_RECEPTOR_TILES> tiles;
};

// The kind bits of one counted pair, decided on the fp32 surface distance d.
__device__ __forceinline__ unsigned pair_kinds(float d, unsigned ti, unsigned tj) {
    unsigned k = 0u;
    if (d <= CT_CONTACT) {
        k = MCG_CONTACT_CONTACT;
        if ((ti & tj & T_HYDROPHOBIC) != 0u) k |= MCG_CONTACT_HYDROPHOBIC;
        if (d <= HB_FULL) {
            if ((ti & T_DONOR) != 0u && (tj & T_ACCEPTOR) != 0u) k |= MCG_CONTACT_HBOND_DONOR;
            if ((ti & T_ACCEPTOR) != 0u && (tj & T_DONOR) != 0u) k |= MCG_CONTACT_HBOND_ACCEPTOR;
        }
    }
    return k;
}

// Where lane (a, w) writes in a list that already holds `base` items, when the lanes with an item append theirs in lane
// order - the ballot and prefix of `build_tile_list`, for a list that grows across calls; `total`: the list's length
// afterwards.  Called by all 256 lanes; two barriers.
__device__ __forceinline__ int append_slot(int* wave_n, bool has_item, int a, int w, int base, int& total) {
    const unsigned long long m = __ballot(has_item);
    if (a == 0) wave_n[w] = __popcll(m);
    __syncthreads();
    int before = base;
    for (int v = 0; v < w; ++v) before += wave_n[v];
    total = base + ((wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]));
    __syncthreads();
    return before + __popcll(m & ((1ull << a) - 1ull));
}

__global__ __launch_bounds__(IX_THREADS) void k_receptor_contacts(
    const float* __restrict__ lig, const float* __restrict__ lig_r, const unsigned char* __restrict__ lig_t,
    const int* __restrict__ n_nodes, int N, const float4* __restrict__ rec, const unsigned char* __restrict__ rec_t,
    const int* __restrict__ rec_g, int R, const float4* __restrict__ tile_sphere, const int* __restrict__ ref_g,
    const unsigned char* __restrict__ ref_k, int K_ref, unsigned mask, int* __restrict__ groups,
    unsigned char* __restrict__ kinds, int* __restrict__ n_groups, unsigned char* __restrict__ atom_kinds,
    int* __restrict__ status, int* __restrict__ counts) {
    __shared__ ContactShared s;
    const int b = blockIdx.x, tid = threadIdx.x, a = tid & 63, w = tid >> 6;
    const int na = atom_count(n_nodes[b], N);
    int* og = groups + (size_t)b * CT_GROUPS;
    unsigned char* ok = kinds + (size_t)b * CT_GROUPS;
    unsigned char* oa = atom_kinds + (size_t)b * N;
    const bool real = a < na;
    float x = 0.f, y = 0.f, z = 0.f, ri = 0.f;
    unsigned ti = 0u;
    if (real) {
        const float* p = lig + ((size_t)b * N + a) * 3;
        x = p[0]; y = p[1]; z = p[2];
        ri = lig_r[(size_t)b * N + a];
        ti = lig_t[(size_t)b * N + a];
    }
    // what the reference holds over the mask: the same for every row, summed below with the row's own two counts
    int ref_bits = 0;
    if (counts != nullptr && tid < K_ref) ref_bits = __popc((unsigned)ref_k[tid] & mask);

    const bool bad = real && !(isfinite(x) && isfinite(y) && isfinite(z));
    int st = MCG_CONTACT_OK;
    if (__syncthreads_or(bad) != 0) st = MCG_CONTACT_NONFINITE;
    else if (na == 0) st = MCG_CONTACT_EMPTY;

    int n_cand = 0;
    unsigned akinds = 0u;
    if (st == MCG_CONTACT_OK) {               // (block-uniform)
        if (w == 0) s.xyz[a][0] = x, s.xyz[a][1] = y, s.xyz[a][2] = z;
        __syncthreads();
        if (tid < 3) {                        // atom centroid, summed in atom order, as the interaction kernel forms it
            float acc = 0.f;
            for (int i = 0; i < na; ++i) acc += s.xyz[i][tid];
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
        build_tile_list(s.tiles, tile_sphere, (R + IX_THREADS - 1) / IX_THREADS, c[0], c[1], c[2],
                        sqrtf(rho2) + IX_CUTOFF);

        const int nt = s.tiles.n_tiles;
        for (int k = 0; k < nt; ++k) {
            const int j0 = (int)s.tiles.list[k] * IX_THREADS;
            const int cnt = min(IX_THREADS, R - j0);               // the last tile's tail
            if (tid < cnt) {
                s.tile[tid] = rec[j0 + tid];
                s.type[tid] = rec_t[j0 + tid];
                s.grp[tid] = rec_g[j0 + tid];
            }
            s.tkinds[tid] = 0;
            __syncthreads();
            for (int jj = w; jj < cnt; jj += IX_WAVES) {
                const float4 q = s.tile[jj];
                float dx, dy, dz;
                const float r2 = pair_r2(x, y, z, q, dx, dy, dz);
                const bool looked = real && r2 < IX_CUTOFF2;
                if (__ballot(looked) == 0ull) continue;            // nobody in this wave: no bit is set
                unsigned kb = 0u;
                if (looked) {
                    float r;
                    kb = pair_kinds(pair_surface_distance(r2, ri, q.w, r), ti, s.type[jj]);
                }
                if (__ballot(kb != 0u) == 0ull) continue;
                akinds |= kb;
                const unsigned u = (__ballot((kb & 1u) != 0u) != 0ull ? 1u : 0u) | (__ballot((kb & 2u) != 0u) != 0ull ? 2u : 0u) |
                                   (__ballot((kb & 4u) != 0u) != 0ull ? 4u : 0u) | (__ballot((kb & 8u) != 0u) != 0ull ? 8u : 0u);
                if (a == 0) s.tkinds[jj] = (unsigned char)u;       // atom jj is this wave's alone
            }
            __syncthreads();
            const unsigned tk = tid < cnt ? s.tkinds[tid] : 0u;
            int total;
            const int slot = append_slot(s.wave_n, tk != 0u, a, w, n_cand, total);
            if (tk != 0u && slot < CT_CAP)
                s.cand[slot] = ((unsigned long long)(unsigned)s.grp[tid] << 8) | (unsigned long long)tk;
            n_cand = total;                   // (past append_slot's second barrier: the tile is free again)
            __syncthreads();
        }
        if (n_cand > CT_CAP) st = MCG_CONTACT_OVERFLOW;
    }

    int n_out = 0;
    if (st == MCG_CONTACT_OK) {
        // sort: a bitonic network over P = the power of two >= max(n_cand, 256), the tail padded with CT_PAD
        int P = IX_THREADS;
        while (P < n_cand) P <<= 1;
        for (int i = n_cand + tid; i < P; i += IX_THREADS) s.cand[i] = CT_PAD;
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (P >> 1); t += IX_THREADS) {
                    const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                    const int hi = lo | stride;
                    const bool up = (lo & size) == 0;
                    const unsigned long long v0 = s.cand[lo], v1 = s.cand[hi];
                    if ((v0 > v1) == up) s.cand[lo] = v1, s.cand[hi] = v0;
                }
                __syncthreads();
            }
        }
        // the heads of the runs of one group, ranked in order; each ORs its run together
        for (int i0 = 0; i0 < n_cand; i0 += IX_THREADS) {
            const int i = i0 + tid;
            bool head = false;
            int g = 0;
            if (i < n_cand) {
                g = (int)(s.cand[i] >> 8);
                head = i == 0 || (int)(s.cand[i - 1] >> 8) != g;
            }
            int total;
            const int slot = append_slot(s.wave_n, head, a, w, n_out, total);
            if (head && slot < CT_GROUPS) {
                unsigned u = 0u;
                for (int e = i; e < n_cand && (int)(s.cand[e] >> 8) == g; ++e) u |= (unsigned)(s.cand[e] & 0xffull);
                s.out_grp[slot] = g;
                s.out_kinds[slot] = (unsigned char)u;
            }
            n_out = total;
        }
        if (n_out > CT_GROUPS) st = MCG_CONTACT_OVERFLOW;
    }
    if (st != MCG_CONTACT_OK) n_out = 0, akinds = 0u;
    __syncthreads();

    // entries, zero behind the count; one lane per entry
    const int eg = tid < n_out ? s.out_grp[tid] : 0;
    const unsigned ek = tid < n_out ? (unsigned)s.out_kinds[tid] : 0u;
    og[tid] = eg;
    ok[tid] = (unsigned char)ek;
    s.atom_part[w][a] = (unsigned char)akinds;
    __syncthreads();
    if (w == 0 && a < N)
        oa[a] = (unsigned char)((s.atom_part[0][a] | s.atom_part[1][a]) | (s.atom_part[2][a] | s.atom_part[3][a]));
    if (tid == 0) {
        n_groups[b] = n_out;
        status[b] = st;
    }
    if (counts == nullptr) return;            // (a kernel argument: block-uniform)

    int v[3] = {(int)__popc(ek & mask), ref_bits, 0};
    if (tid < n_out && K_ref > 0) {           // binary search of the entry's group in the ascending reference list
        int lo = 0, hi = K_ref - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ref_g[mid] < eg) lo = mid + 1; else hi = mid;
        }
        if (ref_g[lo] == eg) v[2] = __popc(ek & (unsigned)ref_k[lo] & mask);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (a == 0) s.sums[w][0] = v[0], s.sums[w][1] = v[1], s.sums[w][2] = v[2];
    __syncthreads();
    if (tid < 3) {
        const bool failed = st == MCG_CONTACT_NONFINITE || st == MCG_CONTACT_OVERFLOW;
        counts[(size_t)b * 3 + tid] = failed ? -1 : (s.sums[0][tid] + s.sums[1][tid]) + (s.sums[2][tid] + s.sums[3][tid]);
    }
}

}  // namespace

extern "C" int mcg_receptor_contacts(const float* lig_xyz, const float* lig_radius, const uint8_t* lig_type,
                                     const int32_t* n_nodes_dev, int B, int N, const float* rec_xyzr,
                                     const uint8_t* rec_type, const int32_t* rec_group, int R, const float* tile_sphere,
                                     const int32_t* ref_group, const uint8_t* ref_kinds, int K_ref, int kinds_mask,
                                     int32_t* groups, uint8_t* kinds, int32_t* n_groups, uint8_t* atom_kinds,
                                     int32_t* status, int32_t* counts, void* stream) {
    static_assert(MAX_ATOMS == 64, "the bound the message below states");
    const bool reference = counts == nullptr || K_ref == 0 || (ref_group && ref_kinds);
    if (!lig_xyz || !lig_radius || !lig_type || !n_nodes_dev || !rec_xyzr || !rec_type || !rec_group || !groups || !kinds ||
        !n_groups || !atom_kinds || !status || !reference || B < 1 || B > MCG_RECEPTOR_MAX_B || N < 1 || N > MAX_ATOMS ||
        R < 1 || R > MCG_RECEPTOR_MAX_ATOMS || K_ref < 0 || K_ref > MCG_CONTACT_MAX_GROUPS || kinds_mask < 0 ||
        kinds_mask > MCG_CONTACT_ALL_KINDS) {
        mcg_set_error("mcg_receptor_contacts: bad arguments (non-null buffers, 1 <= B <= %d, 1 <= N <= 64, 1 <= R <= %d, "
                      "0 <= K_ref <= %d with its two lists where counts are asked for, 0 <= kinds_mask <= %d)",
                      MCG_RECEPTOR_MAX_B, MCG_RECEPTOR_MAX_ATOMS, MCG_CONTACT_MAX_GROUPS, MCG_CONTACT_ALL_KINDS);
        return MCG_ERR_ARG;
    }
    hipLaunchKernelGGL(k_receptor_contacts, dim3(B), dim3(IX_THREADS), 0, (hipStream_t)stream, lig_xyz, lig_radius,
                       lig_type, n_nodes_dev, N, (const float4*)rec_xyzr, rec_type, rec_group, R,
                       (const float4*)tile_sphere, ref_group, ref_kinds, K_ref, (unsigned)kinds_mask, groups, kinds,
                       n_groups, atom_kinds, status, counts);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
