// Substructure patterns ("Substructure patterns"): every embedding of each of P query graphs in each of
// B molecular graphs - a subgraph-monomorphism search, exact in integers.  The package's OWN definition - no toolkit's
// substructure matcher.
//   k_substructure_match: one 64-lane workgroup (one wave) per (molecule, chunk of the patterns).  Once per molecule, lane =
//                      atom, in LDS: the bond-code rows (68-byte stride, as k_graph_fingerprint), per code the 64-bit
//                      neighbour masks (as k_canonical_order), and per atom the mask of its ring-bond neighbours - a bond
//                      is a ring bond iff a flood over the neighbour masks from one end, that bond left out, reaches the
//                      other.  Per pattern: its bond bytes (the earlier-position half only), per position the mask of the
//                      earlier positions it has a query bond with, and its domain - a ballot.  Then lane = ROOT atom: every
//                      lane runs its own depth-first search over an explicit stack in LDS, per depth the 64-bit mask of
//                      candidates still to try ([depth][lane]: lanes on different banks) and the lane's assignment byte.
//                      The candidates of position k are one AND chain: domain, ~used, and per earlier bonded position the
//                      OR of the allowed per-code masks of its image, filtered by the ring mask.  The search is
//                      lane-divergent on purpose: roots are the parallelism the problem offers.  It is bounded by
//                      construction: every pass of the loop pops a candidate (a node, at most NODE_BUDGET) or leaves a
//                      level a node opened; an explicit pass cap derived from the two sits on top.  count is a wave sum,
//                      covered a wave OR, first the lowest lane's that found one.  No recursion, no scratch, no atomics.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_graph_rules.h"
#include "mcg_ring_bonds.h"

namespace {

constexpr int SS_MAXW = MCG_SUBSTRUCTURE_MAX_ATOMS;           // atoms per molecule: one lane, one bit of a 64-bit mask
constexpr int SS_MAXM = MCG_SUBSTRUCTURE_MAX_PATTERN_ATOMS;   // query atoms per pattern: the depth of the stack
constexpr uint32_t SS_BUDGET = MCG_SUBSTRUCTURE_NODE_BUDGET;
// a pass takes a node (<= SS_BUDGET, plus the one that trips the budget) or leaves a level (<= one per node that opened it)
constexpr uint32_t SS_PASS_CAP = 2u * SS_BUDGET + 2u * SS_MAXM + 2u;
constexpr int SS_TARGET_GROUPS = 2048;                        // workgroups to aim for when B is small: 8 per CU
static_assert(SS_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");
static_assert(SS_MAXM == 32, "32-bit position masks");

struct SsShared {
    __attribute__((aligned(16))) uint8_t code[SS_MAXW * MCG_CODE_STRIDE];
    unsigned long long by_code[4][SS_MAXW];            // neighbours by bond code 1..4
    unsigned long long nbr[SS_MAXW];                   // all neighbours
    unsigned long long ring_nb[SS_MAXW];               // neighbours over a ring bond
    unsigned long long cand[SS_MAXM][SS_MAXW];         // per depth and lane: the candidates still to try
    unsigned long long dom[SS_MAXM];                   // per position: the atoms that satisfy its query atom
    uint32_t earlier[SS_MAXM];                         // per position: the earlier positions it has a query bond with
    uint8_t pbond[SS_MAXM][SS_MAXM];                   // the pattern's bond bytes, [k][q] for q < k, else 0
    uint8_t asg[SS_MAXM][SS_MAXW];                     // per depth and lane: the atom assigned
    uint8_t first[SS_MAXM][SS_MAXW];                   // per lane: the first embedding it found
};

// the atoms position k of lane a's search may take: in its domain, unused, and bonded as the pattern asks to the image of
// every earlier position k has a query bond with
__device__ __forceinline__ unsigned long long ss_candidates(const SsShared& s, int k, int a, unsigned long long used) {
    unsigned long long c = s.dom[k] & ~used;
    for (uint32_t e = s.earlier[k]; e != 0u && c != 0ull; e &= e - 1u) {
        const int q = __ffs((int)e) - 1;
        const uint32_t pb = s.pbond[k][q];
        const int u = s.asg[q][a];                     // < 64: written from a bit index
        unsigned long long ok = 0ull;
        ok |= (pb & 1u) ? s.by_code[0][u] : 0ull;
        ok |= (pb & 2u) ? s.by_code[1][u] : 0ull;
        ok |= (pb & 4u) ? s.by_code[2][u] : 0ull;
        ok |= (pb & 8u) ? s.by_code[3][u] : 0ull;
        const unsigned long long rb = s.ring_nb[u];
        ok &= (pb & 0x10u) ? rb : ~0ull;
        ok &= (pb & 0x20u) ? ~rb : ~0ull;
        c &= ok;
    }
    return c;
}

__global__ __launch_bounds__(SS_MAXW) void k_substructure_match(
        const int32_t* __restrict__ z, const int8_t* __restrict__ bonds, const int32_t* __restrict__ n_nodes,
        const int32_t* __restrict__ nh_in, int W, const int32_t* __restrict__ pat_n,
        const unsigned long long* __restrict__ pat_atoms, const uint8_t* __restrict__ pat_bonds, int P,
        int32_t* __restrict__ count_out, int32_t* __restrict__ status_out, int32_t* __restrict__ first_out,
        unsigned long long* __restrict__ covered_out) {
    __shared__ SsShared s;
    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), W);
    const bool real = a < n;
    const unsigned long long me = 1ull << a;

    mcg_stage_codes(s.code, bonds + (size_t)b * W * W, W, n, a, SS_MAXW);
    const int za = real ? z[(size_t)b * W + a] : 0;
    __syncthreads();

    const McgBondTally tally = mcg_bond_tally(s.code + a * MCG_CODE_STRIDE, real ? n : 0);
    const unsigned long long mine = tally.mask, m1 = tally.m1, m2 = tally.m2, m3 = tally.m3, m4 = tally.m4;
    s.by_code[0][a] = m1, s.by_code[1][a] = m2, s.by_code[2][a] = m3, s.by_code[3][a] = m4;
    s.nbr[a] = mine;
    __syncthreads();

    // ring bonds: (a, j) is one iff j is reached from a's other neighbours (mcg_ring_bonds.h)
    const unsigned long long ring_nb = mcg_ring_bonds_of(s.nbr, a, mine, n).mask;
    s.ring_nb[a] = ring_nb;
    const int deg = tally.deg;
    const bool arom = m4 != 0ull, ring = ring_nb != 0ull;
    const int nh = !real ? 0 : nh_in ? nh_in[(size_t)b * W + a] : max(0, (2 * mcg_valence0(za) - tally.v2) / 2);

    for (int p = blockIdx.y; p < P; p += gridDim.y) {            // uniform in the workgroup
        const int m = min(max(pat_n[p], 0), SS_MAXM);
        __syncthreads();                                         // the tables of the pattern before are no longer read
        const uint8_t* pb_src = pat_bonds + (size_t)p * SS_MAXM * SS_MAXM;
        for (int idx = a; idx < SS_MAXM * SS_MAXM; idx += SS_MAXW) {
            const int k = idx >> 5, q = idx & 31;
            s.pbond[k][q] = (q < k && k < m) ? pb_src[idx] : (uint8_t)0;
        }
        const unsigned long long* pa = pat_atoms + (size_t)p * SS_MAXM * 2;
        for (int k = 0; k < m; ++k) {
            const unsigned long long zm = pa[2 * k], w = pa[2 * k + 1];
            const int dmin = (int)(w & 255ull), dmax = (int)(w >> 8 & 255ull), hmin = (int)(w >> 16 & 255ull),
                      hmax = (int)(w >> 24 & 255ull), rq = (int)(w >> 32 & 255ull), aq = (int)(w >> 40 & 255ull);
            const bool z_ok = zm == ~0ull || (za >= 0 && za < 64 && (zm >> za & 1ull) != 0ull);
            const bool ok = real && z_ok && deg >= dmin && deg <= dmax && nh >= hmin && nh <= hmax &&
                            (rq == 1 ? ring : rq == 2 ? !ring : true) && (aq == 1 ? arom : aq == 2 ? !arom : true);
            const unsigned long long d = __ballot(ok ? 1 : 0);
            if (a == 0) s.dom[k] = d;
        }
        __syncthreads();
        if (a < SS_MAXM) {
            uint32_t e = 0u;
            for (int q = 0; q < a; ++q) e |= s.pbond[a][q] != 0 ? 1u << q : 0u;
            s.earlier[a] = e;
        }
        __syncthreads();

        uint32_t cnt = 0u;
        unsigned long long cov = 0ull;
        bool over = false;
        if (m >= 1 && real && (s.dom[0] & me) != 0ull) {         // lane = root
            uint32_t nodes = 1u;
            unsigned long long used = me;
            s.asg[0][a] = (uint8_t)a;
            if (m == 1) {
                cnt = 1u, cov = me;
                s.first[0][a] = (uint8_t)a;
            } else {
                int d = 1;
                s.cand[1][a] = ss_candidates(s, 1, a, used);
                for (uint32_t pass = 0u; d >= 1; ++pass) {
                    if (pass >= SS_PASS_CAP) {                   // the belt: cannot happen, see SS_PASS_CAP
                        over = true;
                        break;
                    }
                    const unsigned long long c = s.cand[d][a];
                    if (c == 0ull) {                             // level d is exhausted: free the atom of the level below
                        --d;
                        if (d >= 1) used &= ~(1ull << s.asg[d][a]);
                        continue;
                    }
                    if (nodes == SS_BUDGET) {                    // this would be node NODE_BUDGET + 1
                        over = true;
                        break;
                    }
                    ++nodes;
                    const int v = low_bit(c);
                    s.cand[d][a] = c & (c - 1ull);
                    s.asg[d][a] = (uint8_t)v;
                    if (d == m - 1) {                            // an embedding
                        if (cnt == 0u)
                            for (int q = 0; q < m; ++q) s.first[q][a] = s.asg[q][a];
                        ++cnt;
                        cov |= used | (1ull << v);
                    } else {
                        used |= 1ull << v;
                        ++d;
                        s.cand[d][a] = ss_candidates(s, d, a, used);
                    }
                }
            }
        }
        __syncthreads();
        const uint32_t total = wave_sum(cnt);
        const unsigned long long covered = wave_or(cov);
        const unsigned long long found = __ballot(cnt != 0u ? 1 : 0);
        const bool budget = __any(over ? 1 : 0) != 0;
        const size_t at = (size_t)b * P + p;
        if (a < SS_MAXM) {
            int32_t f = -1;
            if (found != 0ull && a < m) f = (int32_t)s.first[a][low_bit(found)];
            first_out[at * SS_MAXM + a] = f;
        }
        if (a == 0) {
            count_out[at] = (int32_t)total;
            status_out[at] = budget ? MCG_SUBSTRUCTURE_BUDGET : 0;
            covered_out[at] = covered;
        }
    }
}

}  // namespace

extern "C" int mcg_substructure_match(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                                      const int32_t* nh_or_null, int B, int W, const int32_t* pat_n,
                                      const uint64_t* pat_atoms, const uint8_t* pat_bonds, int P, int32_t* count,
                                      int32_t* status, int32_t* first, uint64_t* covered, void* stream) {
    if (!z || !bonds || !n_nodes_dev || !pat_n || !pat_atoms || !pat_bonds || !count || !status || !first || !covered ||
        B < 0 || B > MCG_SUBSTRUCTURE_MAX_B || W < 1 || W > SS_MAXW || P < 1 || P > MCG_SUBSTRUCTURE_MAX_PATTERNS) {
        mcg_set_error("mcg_substructure_match: bad arguments (non-null z, bonds, n_nodes, pat_n, pat_atoms, pat_bonds, "
                      "count, status, first and covered, 0 <= B <= %d, 1 <= W <= %d, 1 <= P <= %d)",
                      MCG_SUBSTRUCTURE_MAX_B, SS_MAXW, MCG_SUBSTRUCTURE_MAX_PATTERNS);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    const int want = SS_TARGET_GROUPS / B;
    const int chunks = want < 1 ? 1 : want > P ? P : want;     // split the patterns over more workgroups when B is small
    hipLaunchKernelGGL(k_substructure_match, dim3((unsigned)B, (unsigned)chunks), dim3(SS_MAXW), 0, (hipStream_t)stream, z,
                       bonds, n_nodes_dev, nh_or_null, W, pat_n, reinterpret_cast<const unsigned long long*>(pat_atoms),
                       pat_bonds, P, count, status, first, reinterpret_cast<unsigned long long*>(covered));
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
