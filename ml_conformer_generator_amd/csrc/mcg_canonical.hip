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
//   k_canonical_order<true>: the same search text with the stereo leaf policy ("Stereo identity").
//                      Prepass, once: a lane works out from fp32 coordinates whether its atom is a tetrahedral candidate
//                      or an end of a double-bond candidate, its up to four neighbours in ascending input index, the
//                      sign s(a) and - the end of lower index - the cis / trans bits of the up to 2 x 2 substituent pairs;
//                      bytes in LDS.  At a leaf everything is an integer: lane a takes 4 tet + db of its atom from the
//                      ranks of its neighbours (an inversion count, two comparisons and a bit lookup) into v[rank]; where
//                      the certificate equals the best one, one more wave minimum takes the first difference of v.  The
//                      twin rule skips only twins of degree <= 1: swapping them moves no descriptor.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_graph_rules.h"
#include "mcg_hash.h"

namespace {

constexpr int CN_MAXW = MCG_CANONICAL_MAX_ATOMS;       // atoms per molecule: one lane, one bit of a 64-bit mask
constexpr int CN_MAXDEG = MCG_CANONICAL_MAX_DEGREE;    // items of a refinement key
constexpr uint32_t CN_BUDGET = MCG_CANONICAL_LEAF_BUDGET;
constexpr uint32_t CN_NONE = 0xffffffffu;
static_assert(CN_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");
static_assert(CN_MAXDEG == 8, "a key is a 6-bit rank and eight 9-bit items in three words");

struct CnShared {
    __attribute__((aligned(16))) uint8_t code[CN_MAXW * MCG_CODE_STRIDE];
    unsigned long long by_code[4][CN_MAXW];            // neighbours by bond code 1..4
    unsigned long long st_try[CN_MAXW];                // per depth: members of the target cell still to try
    int32_t z[CN_MAXW];
    uint32_t kw[3][CN_MAXW];                           // the refinement keys, most significant word first
    uint32_t row_hash[2][CN_MAXW];
    uint8_t st_rank[CN_MAXW][CN_MAXW];                 // per depth: the rank vector of the node
    uint8_t rk[CN_MAXW];                               // the ranks the keys are built from
    uint8_t ord_new[CN_MAXW], ord_best[CN_MAXW];       // position -> atom: the leaf at hand, the best leaf so far
};

// What the stereo leaf policy keeps beside the search state; nothing for the graph search.
template <bool STEREO> struct CnStereoShared {};
template <> struct CnStereoShared<true> {
    float x[3][CN_MAXW];
    uint32_t nb[CN_MAXW];                              // four bytes, 0xff = none: a tetrahedral candidate's neighbours in
                                                       // ascending index; an end of a double bond: its one or two
                                                       // substituents, then (byte 2) the other end
    uint8_t deg[CN_MAXW];
    uint8_t end_ok[CN_MAXW];                           // the atom qualifies as an end of a double-bond candidate
    uint8_t db_bits[CN_MAXW];                          // written by the end of lower index: 0x80 defined | bit 2 i + j set
                                                       // where its substituent i and the other end's j are cis
    uint8_t v_new[CN_MAXW], v_best[CN_MAXW];           // position -> 4 tet + db: the leaf at hand, the best leaf so far
};

constexpr float CN_STEREO_MIN = 0.1f;                  // |chi| and |cos| below it: undefined (part of the definition)
constexpr uint32_t CN_KIND_TET_POS = 1, CN_KIND_TET_NEG = 2, CN_KIND_DB = 3;

// The stereo prepass of one molecule, called by all 64 lanes: returns the lane's kind (0, or CN_KIND_*: a DEFINED
// descriptor), its packed neighbours in `nbp` and its double bond's bits in `dbs`; `counts` (uniform): the defined
// tetrahedral descriptors, the defined double bonds, the undefined candidates.  Coordinates are read for real atoms only.
__device__ __forceinline__ uint32_t cn_stereo_prepass(const CnShared& s, CnStereoShared<true>& t,
                                                      const float* __restrict__ xyz, const int a, const bool real,
                                                      const int32_t za, const uint32_t deg, const unsigned long long mine,
                                                      const unsigned long long m1, const unsigned long long m2,
                                                      const unsigned long long m34, uint32_t& nbp, uint32_t& dbs,
                                                      int32_t (&counts)[3]) {
    t.x[0][a] = real ? xyz[3 * a] : 0.0f;
    t.x[1][a] = real ? xyz[3 * a + 1] : 0.0f;
    t.x[2][a] = real ? xyz[3 * a + 2] : 0.0f;
    t.deg[a] = (uint8_t)(deg < 255u ? deg : 255u);
    __syncthreads();
    const uint8_t* row = s.code + a * MCG_CODE_STRIDE;
    bool twins = false;                                // two terminal twins among the neighbours
    if (real) {
        for (unsigned long long f = mine; f != 0ull; f &= f - 1ull) {
            const int j = low_bit(f);
            for (unsigned long long g = f & (f - 1ull); g != 0ull; g &= g - 1ull) {
                const int k = low_bit(g);
                twins = twins || (t.deg[j] == 1 && t.deg[k] == 1 && s.z[j] == s.z[k] && row[j] == row[k]);
            }
        }
    }
    const bool tet = real && (za == 6 || za == 14) && (m2 | m34) == 0ull && (deg == 3u || deg == 4u) && !twins;
    const bool end = real && (za == 6 || za == 7) && __popcll(m2) == 1 && m34 == 0ull && (deg == 2u || deg == 3u) && !twins;
    nbp = 0xffffffffu;
    if (tet || end) {
        int at = 0;
        for (unsigned long long f = m1; f != 0ull; f &= f - 1ull, at += 8)
            nbp = (nbp & ~(0xffu << at)) | ((uint32_t)(low_bit(f)) << at);
        if (end) nbp = (nbp & 0xff00ffffu) | ((uint32_t)(low_bit(m2)) << 16);
    }
    t.nb[a] = nbp;
    t.end_ok[a] = end ? 1 : 0;
    __syncthreads();

    uint32_t kind = 0;
    if (tet) {
        const int i0 = nbp & 0xffu, i1 = (nbp >> 8) & 0xffu, i2 = (nbp >> 16) & 0xffu, o = deg == 4u ? (int)(nbp >> 24) : a;
        const float ox = t.x[0][o], oy = t.x[1][o], oz = t.x[2][o];
        const float ax = t.x[0][i0] - ox, ay = t.x[1][i0] - oy, az = t.x[2][i0] - oz;
        const float bx = t.x[0][i1] - ox, by = t.x[1][i1] - oy, bz = t.x[2][i1] - oz;
        const float cx = t.x[0][i2] - ox, cy = t.x[1][i2] - oy, cz = t.x[2][i2] - oz;
        const float det = ax * (by * cz - bz * cy) - ay * (bx * cz - bz * cx) + az * (bx * cy - by * cx);
        const float len = sqrtf(ax * ax + ay * ay + az * az) * sqrtf(bx * bx + by * by + bz * bz) *
                          sqrtf(cx * cx + cy * cy + cz * cz);
        const float chi = det / len;
        if (len > 0.0f && fabsf(chi) >= CN_STEREO_MIN) kind = chi > 0.0f ? CN_KIND_TET_POS : CN_KIND_TET_NEG;
    }
    const int b = end ? (int)((nbp >> 16) & 0xffu) : a;
    const bool bond = end && t.end_ok[b] != 0 && (int)((t.nb[b] >> 16) & 0xffu) == a;   // a candidate, seen from this end
    uint32_t bits = 0;
    if (bond && a < b) {
        const uint32_t other = t.nb[b];
        const float ex = t.x[0][b] - t.x[0][a], ey = t.x[1][b] - t.x[1][a], ez = t.x[2][b] - t.x[2][a];
        const float ee = ex * ex + ey * ey + ez * ez;
        bool ok = ee > 0.0f;
        uint32_t cis = 0;
        for (int i = 0; i < 2; ++i) {
            const int x = (nbp >> (8 * i)) & 0xffu;
            for (int j = 0; j < 2; ++j) {
                const int y = (other >> (8 * j)) & 0xffu;
                if (x != 0xff && y != 0xff) {
                    const float dx = t.x[0][x] - t.x[0][a], dy = t.x[1][x] - t.x[1][a], dz = t.x[2][x] - t.x[2][a];
                    const float fx = t.x[0][y] - t.x[0][b], fy = t.x[1][y] - t.x[1][b], fz = t.x[2][y] - t.x[2][b];
                    const float tx = (dx * ex + dy * ey + dz * ez) / ee, ty = (fx * ex + fy * ey + fz * ez) / ee;
                    const float px = dx - tx * ex, py = dy - tx * ey, pz = dz - tx * ez;
                    const float qx = fx - ty * ex, qy = fy - ty * ey, qz = fz - ty * ez;
                    const float len = sqrtf(px * px + py * py + pz * pz) * sqrtf(qx * qx + qy * qy + qz * qz);
                    const float c = (px * qx + py * qy + pz * qz) / len;
                    ok = ok && len > 0.0f && fabsf(c) >= CN_STEREO_MIN;
                    cis |= c > 0.0f ? 1u << (2 * i + j) : 0u;
                }
            }
        }
        // two substituents of one end lie on opposite sides of every substituent of the other end
        const bool two_x = ((nbp >> 8) & 0xffu) != 0xffu, two_y = ((other >> 8) & 0xffu) != 0xffu;
        if (two_x) ok = ok && ((cis ^ (cis >> 2)) & 1u) != 0u && (!two_y || ((cis ^ (cis >> 2)) & 2u) != 0u);
        if (two_y) ok = ok && ((cis ^ (cis >> 1)) & 1u) != 0u && (!two_x || ((cis ^ (cis >> 1)) & 4u) != 0u);
        bits = ok ? 0x80u | cis : 0u;
    }
    t.db_bits[a] = (uint8_t)bits;
    __syncthreads();
    if (bond && a > b) bits = t.db_bits[b];
    dbs = bits & 0xfu;
    if (bond && (bits & 0x80u) != 0u) kind = CN_KIND_DB;
    const bool tet_open = tet && kind == 0, bond_low = bond && a < b;
    counts[0] = __popcll(__ballot((tet && kind != 0) ? 1 : 0));
    counts[1] = __popcll(__ballot((bond_low && kind != 0) ? 1 : 0));
    counts[2] = __popcll(__ballot(tet_open ? 1 : 0)) + __popcll(__ballot((bond_low && kind == 0) ? 1 : 0));
    return kind;
}

// 4 tet + db of the lane's atom at the labelling in `s.rk` (a leaf: every rank distinct).  Integers only.
__device__ __forceinline__ uint32_t cn_stereo_value(const CnShared& s, const CnStereoShared<true>& t, const uint32_t kind,
                                                    const uint32_t nbp, const uint32_t dbs, const int a,
                                                    const uint32_t rank) {
    if (kind == CN_KIND_TET_POS || kind == CN_KIND_TET_NEG) {
        // the parity of the permutation that sorts the neighbours by rank: its inversions (the implicit H is last)
        const uint32_t r0 = s.rk[nbp & 0xffu], r1 = s.rk[(nbp >> 8) & 0xffu], r2 = s.rk[(nbp >> 16) & 0xffu];
        uint32_t inv = (r0 > r1 ? 1u : 0u) + (r0 > r2 ? 1u : 0u) + (r1 > r2 ? 1u : 0u);
        if ((nbp >> 24) != 0xffu) {
            const uint32_t r3 = s.rk[nbp >> 24];
            inv += (r0 > r3 ? 1u : 0u) + (r1 > r3 ? 1u : 0u) + (r2 > r3 ? 1u : 0u);
        }
        return ((kind == CN_KIND_TET_NEG) != ((inv & 1u) != 0u)) ? 8u : 4u;
    }
    if (kind == CN_KIND_DB) {
        const int b = (nbp >> 16) & 0xffu;
        if (rank < s.rk[b]) return 0u;                 // stored at the end of larger rank
        const uint32_t other = t.nb[b];
        const uint32_t x1 = (nbp >> 8) & 0xffu, y1 = (other >> 8) & 0xffu;
        const uint32_t i = (x1 != 0xffu && s.rk[x1] < s.rk[nbp & 0xffu]) ? 1u : 0u;
        const uint32_t j = (y1 != 0xffu && s.rk[y1] < s.rk[other & 0xffu]) ? 1u : 0u;
        const uint32_t bit = a < b ? 2u * i + j : 2u * j + i;
        return ((dbs >> bit) & 1u) != 0u ? 1u : 2u;
    }
    return 0u;
}

// Refinement to the point where no rank changes (the number of distinct ranks has stopped growing: a key starts with the
// lane's rank, so cells only split).  "No rank changed" equals "no cell split" only because every rank vector that comes
// in is in count-of-smaller form - the initial colour's by construction, an individualised one because v keeps r and the
// rest of its cell takes r + 1, the count of atoms now in front of them.  Called by all 64 lanes; returns the lane's rank, which `s.rk` then holds too.
__device__ __forceinline__ uint32_t cn_refine(CnShared& s, uint32_t rank, const int a, const int n, const bool real,
                                              const unsigned long long mine, const uint32_t deg) {
    const uint8_t* row = s.code + a * MCG_CODE_STRIDE;
    for (int it = 0; it <= n; ++it) {
        s.rk[a] = (uint8_t)rank;
        __syncthreads();
        unsigned long long hi = 0ull, lo = 0ull;       // items 0..3 and 4..7, 9 bits each: (rank of j) << 3 | code
        if (real) {
            uint32_t emitted = 0, last = 0;            // a real item is >= 1 (code >= 1)
            while (emitted < deg) {
                uint32_t best = CN_NONE, count = 0;
                for (unsigned long long f = mine; f != 0ull; f &= f - 1ull) {
                    const int j = low_bit(f);
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

// STEREO: the leaf tie-break policy.  false: the first leaf with the smallest certificate wins (the graph search, whose
// four trailing arguments are not read); true: among those leaves the smallest stereo vector wins.
template <bool STEREO>
__global__ __launch_bounds__(CN_MAXW) void k_canonical_order(const int32_t* __restrict__ z,
                                                             const int8_t* __restrict__ bonds,
                                                             const int32_t* __restrict__ n_nodes, int W,
                                                             int32_t* __restrict__ order_out,
                                                             int32_t* __restrict__ status_out,
                                                             int32_t* __restrict__ leaves_out,
                                                             unsigned long long* __restrict__ key_out,
                                                             const float* __restrict__ coords,
                                                             int8_t* __restrict__ stereo_out,
                                                             unsigned long long* __restrict__ stereo_key_out,
                                                             int32_t* __restrict__ counts_out) {
    __shared__ CnShared s;
    __shared__ CnStereoShared<STEREO> t;
    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), W);
    const bool real = a < n;

    mcg_stage_codes(s.code, bonds + (size_t)b * W * W, W, n, a, CN_MAXW);
    const int32_t za = real ? z[(size_t)b * W + a] : 0;
    s.z[a] = za;
    __syncthreads();

    const McgBondTally tally = mcg_bond_tally(s.code + a * MCG_CODE_STRIDE, real ? n : 0);
    const unsigned long long mine = tally.mask, m1 = tally.m1, m2 = tally.m2, m3 = tally.m3, m4 = tally.m4;
    const uint32_t deg = tally.deg, val2 = tally.v2;
    s.by_code[0][a] = m1, s.by_code[1][a] = m2, s.by_code[2][a] = m3, s.by_code[3][a] = m4;

    uint32_t kind = 0, nbp = 0, dbs = 0;                 // the lane's stereo state: a few bits, kept in registers
    int32_t counts[3] = {0, 0, 0};
    if constexpr (STEREO)
        kind = cn_stereo_prepass(s, t, coords + (size_t)b * W * 3, a, real, za, deg, mine, m1, m2, m3 | m4, nbp, dbs,
                                 counts);

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
            const unsigned long long present = wave_or(real ? 1ull << rank : 0ull);
            if (__popcll(present) == n) {                // every cell a singleton: a leaf
                ++leaves;
                if (real) s.ord_new[rank] = (uint8_t)a;
                if constexpr (STEREO) {
                    if (real) t.v_new[rank] = (uint8_t)cn_stereo_value(s, t, kind, nbp, dbs, a, rank);
                }
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
                            const uint32_t cn = s.code[p * MCG_CODE_STRIDE + s.ord_new[j]];
                            const uint32_t cb = s.code[q * MCG_CODE_STRIDE + s.ord_best[j]];
                            if (cn != cb) diff = ((uint32_t)(64 + 64 * a + j) << 1) | (cn < cb ? 0u : 1u);
                        }
                    }
                    const uint32_t first = wave_min(diff);
                    better = first != CN_NONE && (first & 1u) == 0u;
                    if constexpr (STEREO) {
                        if (first == CN_NONE) {          // the same certificate: the smaller stereo vector wins
                            const uint32_t vn = real ? t.v_new[a] : 0u, vb = real ? t.v_best[a] : 0u;
                            const uint32_t at = wave_min(vn != vb ? ((uint32_t)a << 1) | (vn < vb ? 0u : 1u) : CN_NONE);
                            better = at != CN_NONE && (at & 1u) == 0u;
                        }
                    }
                }
                __syncthreads();
                if (better) {
                    if (real) s.ord_best[a] = s.ord_new[a];
                    if constexpr (STEREO) {
                        if (real) t.v_best[a] = t.v_new[a];
                    }
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
                    const int r = low_bit(rest);
                    rest &= rest - 1ull;
                    const int next = rest != 0ull ? low_bit(rest) : n;
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
                    const int u = low_bit(f);
                    if (member && u < a && s.z[u] == za) {
                        const unsigned long long others = ~(me | (1ull << u));
                        const unsigned long long x = (s.by_code[0][u] ^ m1) | (s.by_code[1][u] ^ m2) |
                                                     (s.by_code[2][u] ^ m3) | (s.by_code[3][u] ^ m4);
                        // the stereo search skips terminal twins only: swapping others moves their neighbours' descriptors
                        skip = skip || ((x & others) == 0ull && (!STEREO || deg <= 1u));
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
            const int v = low_bit(t);
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
            uint32_t h0 = mm3_mix(MCG_HASH_SEED, (uint32_t)s.z[p]), h1 = mm3_mix(MCG_HASH_SEED_HI, (uint32_t)s.z[p]);
            for (int j = 0; j < a; ++j) {
                const uint32_t c = s.code[p * MCG_CODE_STRIDE + s.ord_best[j]];
                h0 = mm3_mix(h0, c);
                h1 = mm3_mix(h1, c);
            }
            s.row_hash[0][a] = mm3_final(h0, (uint32_t)a + 1u);
            s.row_hash[1][a] = mm3_final(h1, (uint32_t)a + 1u);
        }
        __syncthreads();
        uint32_t hk = 0;
        if (a < 2) {                                     // lane 0: the low half, lane 1: the high half
            hk = mm3_mix(a == 0 ? MCG_HASH_SEED : MCG_HASH_SEED_HI, (uint32_t)n);
            for (int j = 0; j < n; ++j) hk = mm3_mix(hk, s.row_hash[a][j]);
            hk = mm3_final(hk, (uint32_t)n + 1u);
        }
        const uint32_t key_hi = __shfl(hk, 1);
        key = ((unsigned long long)key_hi << 32) | hk;
    }
    if constexpr (STEREO) {
        // the same mixing over (n, the row hashes, v[0..n-1])
        unsigned long long skey = 0ull;
        if (status == 0) {
            uint32_t hk = 0;
            if (a < 2) {
                hk = mm3_mix(a == 0 ? MCG_HASH_SEED : MCG_HASH_SEED_HI, (uint32_t)n);
                for (int j = 0; j < n; ++j) hk = mm3_mix(hk, s.row_hash[a][j]);
                for (int j = 0; j < n; ++j) hk = mm3_mix(hk, (uint32_t)t.v_best[j]);
                hk = mm3_final(hk, 2u * (uint32_t)n + 1u);
            }
            const uint32_t key_hi = __shfl(hk, 1);
            skey = ((unsigned long long)key_hi << 32) | hk;
        }
        if (a < W) stereo_out[(size_t)b * W + a] = (status == 0 && real) ? (int8_t)t.v_best[a] : (int8_t)0;
        if (a == 0) stereo_key_out[b] = skey;
        if (a < 3) counts_out[(size_t)b * 3 + a] = a == 0 ? counts[0] : a == 1 ? counts[1] : counts[2];
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
    hipLaunchKernelGGL(k_canonical_order<false>, dim3((unsigned)B), dim3(CN_MAXW), 0, (hipStream_t)stream, z, bonds,
                       n_nodes_dev, W, order_out, status_out, leaves_out, reinterpret_cast<unsigned long long*>(key_out),
                       (const float*)nullptr, (int8_t*)nullptr, (unsigned long long*)nullptr, (int32_t*)nullptr);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_stereo_order(const float* coords, const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                                int B, int W, int32_t* order_out, int32_t* status_out, int32_t* leaves_out,
                                uint64_t* key_out, int8_t* stereo_out, uint64_t* stereo_key_out, int32_t* counts_out,
                                void* stream) {
    if (!coords || !z || !bonds || !n_nodes_dev || !order_out || !status_out || !leaves_out || !key_out || !stereo_out ||
        !stereo_key_out || !counts_out || B < 0 || B > MCG_CANONICAL_MAX_B || W < 1 || W > CN_MAXW) {
        mcg_set_error("mcg_stereo_order: bad arguments (non-null coords, z, bonds, n_nodes, order_out, status_out, "
                      "leaves_out, key_out, stereo_out, stereo_key_out and counts_out, 0 <= B <= %d, 1 <= W <= %d)",
                      MCG_CANONICAL_MAX_B, CN_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_canonical_order<true>, dim3((unsigned)B), dim3(CN_MAXW), 0, (hipStream_t)stream, z, bonds,
                       n_nodes_dev, W, order_out, status_out, leaves_out, reinterpret_cast<unsigned long long*>(key_out),
                       coords, stereo_out, reinterpret_cast<unsigned long long*>(stereo_key_out), counts_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
