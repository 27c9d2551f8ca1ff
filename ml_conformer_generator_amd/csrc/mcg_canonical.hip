// Exact canonical labelling of molecular graphs ("Canonical graphs and SMILES"): per molecule the
// atom order whose relabelled graph has the lexicographically smallest certificate over the leaves of a
// partition-refinement search.  The package's OWN definition - no toolkit's canonical order.  Integers only: ranks are
// counts, nothing is hashed on the way to a decision, so every output is exact.
//   k_canonical_order: one 64-lane workgroup (one wave) per molecule, lane = atom.  In LDS: the bond-code rows (68-byte
//                      stride, as k_graph_fingerprint), per code the 64-bit neighbour masks (the twin test is four
//                      XORs), the three key words of every lane, the current ranks, the search stack (per depth the
//                      rank vector, 64 bytes, and the mask of members still to try) and the two atom orders.
//                      Refinement round: a lane takes its neighbours' (rank, code) items in ascending order by repeated
//                      minimum passes over its neighbour mask (no per-lane array, no scratch) into rank + eight 9-bit
//                      items = 78 bits, three words; the new rank is the count of smaller keys among the other lanes'
//                      (LDS broadcasts).  A leaf is compared with the best so far without materialising either
//                      certificate: lane k finds the first difference in row k of the two relabelled graphs and a wave
//                      minimum takes the earliest.  Every loop bound is uniform in the wave or guarded by `real`.
#include "mcg_common.h"
#include "mcg_api_internal.h"

namespace {

constexpr int CN_MAXW = MCG_CANONICAL_MAX_ATOMS;       // atoms per molecule: one lane, one bit of a 64-bit mask
constexpr int CN_STRIDE = 68;                          // bytes per bond-code row in LDS (17 dwords: rows spread over banks)
constexpr int CN_MAXDEG = MCG_CANONICAL_MAX_DEGREE;    // items of a refinement key
constexpr uint32_t CN_BUDGET = MCG_CANONICAL_LEAF_BUDGET;
constexpr uint32_t CN_SEED = 0x6d636731u;              // the fingerprint's two seeds
constexpr uint32_t CN_SEED_HI = CN_SEED ^ 0x9e3779b9u;
constexpr uint32_t CN_NONE = 0xffffffffu;
static_assert(CN_MAXW == 64 && CN_MAXDEG == 8, "a key is a 6-bit rank and eight 9-bit items in three words");

__device__ __forceinline__ uint32_t cn_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// MurmurHash3_x86_32, one 4-byte block at a time (as csrc/mcg_fingerprint.hip)
__device__ __forceinline__ uint32_t cn_mix(uint32_t h, uint32_t k) {
    k *= 0xcc9e2d51u;
    k = cn_rotl32(k, 15);
    k *= 0x1b873593u;
    h ^= k;
    h = cn_rotl32(h, 13);
    return h * 5u + 0xe6546b64u;
}

__device__ __forceinline__ uint32_t cn_final(uint32_t h, uint32_t n_words) {
    h ^= 4u * n_words;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ uint32_t cn_val2(uint32_t c) {          // twice the bond order, aromatic = 1.5
    return c == 1 ? 2u : c == 2 ? 4u : c == 3 ? 6u : c == 4 ? 3u : 0u;
}

__device__ __forceinline__ unsigned long long cn_wave_or(unsigned long long v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    for (int off = 32; off > 0; off >>= 1) {
        lo |= __shfl_xor(lo, off);
        hi |= __shfl_xor(hi, off);
    }
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t cn_wave_min(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}

struct CnShared {
    __attribute__((aligned(16))) uint8_t code[CN_MAXW * CN_STRIDE];
    unsigned long long by_code[4][CN_MAXW];            // neighbours by bond code 1..4
    unsigned long long st_try[CN_MAXW];                // per depth: members of the target cell still to try
    int32_t z[CN_MAXW];
    uint32_t kw[3][CN_MAXW];                           // the refinement keys, most significant word first
    uint32_t row_hash[2][CN_MAXW];
    uint8_t st_rank[CN_MAXW][CN_MAXW];                 // per depth: the rank vector of the node
    uint8_t rk[CN_MAXW];                               // the ranks the keys are built from
    uint8_t ord_new[CN_MAXW], ord_best[CN_MAXW];       // position -> atom: the leaf at hand, the best leaf so far
};

// Refinement to the point where no rank changes (the number of distinct ranks has stopped growing: a key starts with the
// lane's rank, so cells only split).  "No rank changed" equals "no cell split" only because every rank vector that comes
// in is in count-of-smaller form - the initial colour's by construction, an individualised one because v keeps r and the
// rest of its cell takes r + 1, the count of atoms now in front of them.  Called by all 64 lanes; returns the lane's rank, which `s.rk` then holds too.
__device__ __forceinline__ uint32_t cn_refine(CnShared& s, uint32_t rank, const int a, const int n, const bool real,
                                              const unsigned long long mine, const uint32_t deg) {
    const uint8_t* row = s.code + a * CN_STRIDE;
    for (int it = 0; it <= n; ++it) {
        s.rk[a] = (uint8_t)rank;
        __syncthreads();
        unsigned long long hi = 0ull, lo = 0ull;       // items 0..3 and 4..7, 9 bits each: (rank of j) << 3 | code
        if (real) {
            uint32_t emitted = 0, last = 0;            // a real item is >= 1 (code >= 1)
            while (emitted < deg) {
                uint32_t best = CN_NONE, count = 0;
                for (unsigned long long f = mine; f != 0ull; f &= f - 1ull) {
                    const int j = __ffsll((long long)f) - 1;
                    const uint32_t item = ((uint32_t)s.rk[j] << 3) | row[j];
                    if (item > last) {
                        count = item < best ? 1u : count + (item == best ? 1u : 0u);
                        best = item < best ? item : best;
                    }
                }
                if (count == 0) break;                 // cannot happen: deg counts exactly the bits of `mine`
                for (uint32_t t = 0; t < count; ++t, ++emitted) {
                    if (emitted < 4) hi = (hi << 9) | best;
                    else lo = (lo << 9) | best;
                }
                last = best;
            }
        }
        const uint32_t k0 = (rank << 18) | (uint32_t)(hi >> 18);
        const uint32_t k1 = ((uint32_t)(hi & 0x3ffffull) << 9) | (uint32_t)(lo >> 27);
        const uint32_t k2 = (uint32_t)(lo & 0x7ffffffull);
        s.kw[0][a] = k0, s.kw[1][a] = k1, s.kw[2][a] = k2;
        __syncthreads();
        uint32_t smaller = 0;
        if (real) {
            for (int j = 0; j < n; ++j) {
                const uint32_t j0 = s.kw[0][j], j1 = s.kw[1][j], j2 = s.kw[2][j];
                smaller += (j0 < k0 || (j0 == k0 && (j1 < k1 || (j1 == k1 && j2 < k2)))) ? 1u : 0u;
            }
        }
        const bool changed = __any((real && smaller != rank) ? 1 : 0) != 0;
        if (real) rank = smaller;
        if (!changed) break;
    }
    return rank;
}

__global__ __launch_bounds__(CN_MAXW) void k_canonical_order(const int32_t* __restrict__ z,
                                                             const int8_t* __restrict__ bonds,
                                                             const int32_t* __restrict__ n_nodes, int W,
                                                             int32_t* __restrict__ order_out,
                                                             int32_t* __restrict__ status_out,
                                                             int32_t* __restrict__ leaves_out,
                                                             unsigned long long* __restrict__ key_out) {
    __shared__ CnShared s;
    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), W);
    const bool real = a < n;

    // the molecule's W x W codes -> LDS rows; the diagonal, the padding and anything that is no code 1..4 become 0
    const int8_t* src = bonds + (size_t)b * W * W;
    for (int idx = a; idx < W * W; idx += CN_MAXW) {
        const int i = idx / W, j = idx - i * W;
        const int c = src[idx];
        s.code[i * CN_STRIDE + j] = (i < n && j < n && i != j && c >= 1 && c <= 4) ? (uint8_t)c : (uint8_t)0;
    }
    const int32_t za = real ? z[(size_t)b * W + a] : 0;
    s.z[a] = za;
    __syncthreads();

    const uint8_t* row = s.code + a * CN_STRIDE;
    unsigned long long mine = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull, m4 = 0ull;
    uint32_t deg = 0, val2 = 0;
    if (real) {
        for (int j = 0; j < n; ++j) {
            const uint32_t c = row[j];
            const unsigned long long bit = 1ull << j;
            m1 |= c == 1 ? bit : 0ull;
            m2 |= c == 2 ? bit : 0ull;
            m3 |= c == 3 ? bit : 0ull;
            m4 |= c == 4 ? bit : 0ull;
            deg += c != 0 ? 1u : 0u;
            val2 += cn_val2(c);
        }
        mine = m1 | m2 | m3 | m4;
    }
    s.by_code[0][a] = m1, s.by_code[1][a] = m2, s.by_code[2][a] = m3, s.by_code[3][a] = m4;

    int status = 0;
    if (n == 0) status = MCG_CANONICAL_EMPTY;
    else if (__any((real && deg > (uint32_t)CN_MAXDEG) ? 1 : 0) != 0) status = MCG_CANONICAL_DEGREE;
    uint32_t leaves = 0;

    if (status == 0) {                                   // uniform in the workgroup
        // the initial colour (Z, degree, v2), ranked by counting
        const uint32_t c0 = (uint32_t)za, c1 = (deg << 8) | val2;
        s.kw[0][a] = c0, s.kw[1][a] = c1;
        __syncthreads();
        uint32_t rank = 0;
        if (real) {
            for (int j = 0; j < n; ++j) {
                const uint32_t j0 = s.kw[0][j], j1 = s.kw[1][j];
                rank += ((int32_t)j0 < za || (j0 == c0 && j1 < c1)) ? 1u : 0u;
            }
        }
        __syncthreads();
        rank = cn_refine(s, rank, a, n, real, mine, deg);

        int d = 0;                                       // nodes on the stack
        bool have_best = false;
        while (true) {
            const unsigned long long present = cn_wave_or(real ? 1ull << rank : 0ull);
            if (__popcll(present) == n) {                // every cell a singleton: a leaf
                ++leaves;
                if (real) s.ord_new[rank] = (uint8_t)a;
                __syncthreads();
                bool better = !have_best;
                if (have_best) {
                    // the first difference of the two certificates: the Z sequence (position a), then row a of the
                    // relabelled graphs (position 64 + 64 a + j); the low bit says which side is larger there
                    uint32_t diff = CN_NONE;
                    const int p = real ? s.ord_new[a] : 0, q = real ? s.ord_best[a] : 0;
                    if (real && s.z[p] != s.z[q]) diff = ((uint32_t)a << 1) | (s.z[p] < s.z[q] ? 0u : 1u);
                    for (int j = 0; j < n; ++j) {
                        if (real && j < a && diff == CN_NONE) {
                            const uint32_t cn = s.code[p * CN_STRIDE + s.ord_new[j]];
                            const uint32_t cb = s.code[q * CN_STRIDE + s.ord_best[j]];
                            if (cn != cb) diff = ((uint32_t)(64 + 64 * a + j) << 1) | (cn < cb ? 0u : 1u);
                        }
                    }
                    const uint32_t first = cn_wave_min(diff);
                    better = first != CN_NONE && (first & 1u) == 0u;
                }
                __syncthreads();
                if (better) {
                    if (real) s.ord_best[a] = s.ord_new[a];
                    have_best = true;
                }
                __syncthreads();
                if (leaves == CN_BUDGET) {               // a branch still unexplored behind the last leaf allowed?
                    unsigned long long left = 0ull;
                    for (int l = 0; l < d; ++l) left |= s.st_try[l];
                    if (left != 0ull) {
                        status = MCG_CANONICAL_BUDGET;
                        break;
                    }
                }
            } else {
                // the target cell: the non-singleton cell of smallest rank (a cell of rank r ends at the next rank present)
                int target = -1;
                for (unsigned long long rest = present; rest != 0ull;) {
                    const int r = __ffsll((long long)rest) - 1;
                    rest &= rest - 1ull;
                    const int next = rest != 0ull ? __ffsll((long long)rest) - 1 : n;
                    if (next - r > 1) {
                        target = r;
                        break;
                    }
                }
                const bool member = real && (int)rank == target;
                const unsigned long long cell = __ballot(member ? 1 : 0);
                // the twin rule: skip a member that has a twin among the members in front of it
                bool skip = false;
                const unsigned long long me = 1ull << a;
                for (unsigned long long f = cell; f != 0ull; f &= f - 1ull) {
                    const int u = __ffsll((long long)f) - 1;
                    if (member && u < a && s.z[u] == za) {
                        const unsigned long long others = ~(me | (1ull << u));
                        const unsigned long long x = (s.by_code[0][u] ^ m1) | (s.by_code[1][u] ^ m2) |
                                                     (s.by_code[2][u] ^ m3) | (s.by_code[3][u] ^ m4);
                        skip = skip || (x & others) == 0ull;
                    }
                }
                const unsigned long long to_try = cell & ~__ballot(skip ? 1 : 0);
                s.st_rank[d][a] = (uint8_t)rank;
                if (a == 0) s.st_try[d] = to_try;
                __syncthreads();
                ++d;
            }
            // the next branch: the deepest node that still has a member to try
            while (d > 0 && s.st_try[d - 1] == 0ull) --d;
            if (d == 0) break;
            const unsigned long long t = s.st_try[d - 1];
            const int v = __ffsll((long long)t) - 1;
            const uint32_t r = s.st_rank[d - 1][v];
            rank = s.st_rank[d - 1][a];
            if (rank == r && a != v) rank = r + 1u;      // v keeps the cell's rank, the other members move up by one
            __syncthreads();
            if (a == 0) s.st_try[d - 1] = t & (t - 1ull);
            __syncthreads();
            rank = cn_refine(s, rank, a, n, real, mine, deg);
        }
    }

    // 64 bits of the best certificate, for grouping: row k of the relabelled graph hashed under both seeds by lane k,
    // then the row hashes with n by two lanes
    unsigned long long key = 0ull;
    if (status == 0) {
        if (real) {
            const int p = s.ord_best[a];
            uint32_t h0 = cn_mix(CN_SEED, (uint32_t)s.z[p]), h1 = cn_mix(CN_SEED_HI, (uint32_t)s.z[p]);
            for (int j = 0; j < a; ++j) {
                const uint32_t c = s.code[p * CN_STRIDE + s.ord_best[j]];
                h0 = cn_mix(h0, c);
                h1 = cn_mix(h1, c);
            }
            s.row_hash[0][a] = cn_final(h0, (uint32_t)a + 1u);
            s.row_hash[1][a] = cn_final(h1, (uint32_t)a + 1u);
        }
        __syncthreads();
        uint32_t hk = 0;
        if (a < 2) {                                     // lane 0: the low half, lane 1: the high half
            hk = cn_mix(a == 0 ? CN_SEED : CN_SEED_HI, (uint32_t)n);
            for (int j = 0; j < n; ++j) hk = cn_mix(hk, s.row_hash[a][j]);
            hk = cn_final(hk, (uint32_t)n + 1u);
        }
        const uint32_t key_hi = __shfl(hk, 1);
        key = ((unsigned long long)key_hi << 32) | hk;
    }
    if (a < W) order_out[(size_t)b * W + a] = (status == 0 && real) ? (int32_t)s.ord_best[a] : -1;
    if (a == 0) {
        status_out[b] = status;
        leaves_out[b] = (int32_t)leaves;
        key_out[b] = key;
    }
}

}  // namespace

extern "C" int mcg_canonical_order(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                                   int32_t* order_out, int32_t* status_out, int32_t* leaves_out, uint64_t* key_out,
                                   void* stream) {
    if (!z || !bonds || !n_nodes_dev || !order_out || !status_out || !leaves_out || !key_out || B < 0 ||
        B > MCG_CANONICAL_MAX_B || W < 1 || W > CN_MAXW) {
        mcg_set_error("mcg_canonical_order: bad arguments (non-null z, bonds, n_nodes, order_out, status_out, leaves_out "
                      "and key_out, 0 <= B <= %d, 1 <= W <= %d)", MCG_CANONICAL_MAX_B, CN_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_canonical_order, dim3((unsigned)B), dim3(CN_MAXW), 0, (hipStream_t)stream, z, bonds, n_nodes_dev,
                       W, order_out, status_out, leaves_out, reinterpret_cast<unsigned long long*>(key_out));
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
