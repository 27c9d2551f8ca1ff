// Standardised graphs ("Standardised graphs"): the largest fragment of a molecular graph, the checks
// that make it a molecule, and a Kekule form of its aromatic bonds.  The package's OWN definition - not RDKit's
// FragmentParent / Kekulize / SanitizeMol: no charges, no normalisation, no agreement with RDKit claimed.
//   k_standardize_graphs: one 64-lane workgroup (one wave) per molecule, lane = atom, the layout of k_hydrogens_place:
//     stage     bond codes (68-byte rows, read through the lower triangle so the masks are symmetric whatever came in) and
//               atomic numbers -> LDS; the diagonal, the padding and every code outside 1..4 become 0.
//     masks     per lane the 64-bit neighbour mask, the code-4 mask, the half-bond sum of the valence check and sigma.
//     fragments every lane closes its own mask under the neighbour masks (frontier by frontier: each atom's mask is read
//               once), so a component is one mask and its label the lowest set bit; size and Z sum are the lane's own loop.
//               The parent is a shuffle reduction on (size, Z sum, -label); the keep mask is one ballot.
//     compact   new index = popcount of the keep mask below the lane; the inverse map goes to LDS.
//     bridges   the parent's code-4 bonds are listed in LDS (offsets by a wave scan); lanes stride over the list, each
//               closing one end's mask with that bond taken out until the other end turns up or nothing is new.
//     Kekule    the eligible graph's masks -> LDS, its components by the same closure; the lane that is a component's
//               lowest atom runs the backtracking search of the definition on 64-bit matched / skipped masks with an
//               explicit stack.  All stacks share one 64-entry LDS array: a component's depth is at most its size, the
//               sizes sum to at most 64, and a lane's slice starts at the sum of the sizes before it (a wave scan).
//     write     plain vector stores of every element of every output: compacted coordinates (copied as 32-bit words, bit
//               for bit), Z, codes, Kekule orders, atom map and the four per-row integers.
//   The closures and the search are divergent integer work on a handful of LDS words: latency-bound by nature, nowhere
//   near a roofline; a batch fills the machine with one wave per molecule.  Every loop bound is the molecule's own n, bond
//   count or the step budget: a molecule's outputs have the same bits whatever the batch, its row and the padded widths.
//   No atomics, no inline assembly, no private arrays (no scratch), no floating-point arithmetic.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_elements.h"
#include "mcg_graph_rules.h"

namespace {

typedef unsigned long long u64;

constexpr int SG_MAXW = MCG_STANDARDIZE_MAX_ATOMS;   // atoms per molecule: one lane and one mask bit each
constexpr int SG_MAX_BONDS = SG_MAXW * (SG_MAXW - 1) / 2;
constexpr int SG_BUDGET = MCG_STANDARDIZE_KEKULE_BUDGET;
constexpr int SG_SKIP = 64;                          // a stack entry's choice: "the atom was skipped"
static_assert(SG_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");

enum : int { SG_EMPTY = 1, SG_OVER_VALENCE = 2, SG_AROMATIC_BRIDGE = 4, SG_NOT_KEKULIZABLE = 8, SG_SEARCH_BUDGET = 16 };

__constant__ McgElementTable c_std_elements = MCG_ELEMENTS;

__device__ __forceinline__ int high_bit(u64 m) { return 63 - __clzll((long long)m); }

__global__ __launch_bounds__(SG_MAXW) void k_standardize_graphs(
    const uint32_t* __restrict__ coords, const int32_t* __restrict__ z, const int8_t* __restrict__ bonds,
    const int32_t* __restrict__ n_nodes, int N, int W, uint32_t* __restrict__ coords_out, int32_t* __restrict__ z_out,
    int8_t* __restrict__ bonds_out, int8_t* __restrict__ kekule_out, int32_t* __restrict__ atom_map_out,
    int32_t* __restrict__ n_out, int32_t* __restrict__ n_fragments_out, int32_t* __restrict__ removed_out,
    int32_t* __restrict__ status_out) {
    __shared__ __attribute__((aligned(16))) uint8_t code[SG_MAXW * MCG_CODE_STRIDE];
    __shared__ u64 adj[SG_MAXW];                      // every bond
    __shared__ u64 eadj[SG_MAXW];                     // the eligible graph
    __shared__ int32_t zs[SG_MAXW];
    __shared__ uint16_t blist[SG_MAX_BONDS];          // the parent's code-4 bonds: i | j << 8, i < j
    __shared__ uint16_t stack[SG_MAXW];               // the searches' frames: atom | choice << 8
    __shared__ uint8_t inv[SG_MAXW];                  // new index -> old
    __shared__ uint8_t partner[SG_MAXW];              // old index -> the atom it shares its double bond with; 0xff none

    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), min(N, W));
    const bool real = a < n;
    const u64 me = 1ull << a;

    // mcg_stage_codes' rule, read through the lower triangle: entry (i, j) is the code at (max, min)
    const int8_t* src = bonds + (size_t)b * W * W;
    for (int idx = a; idx < W * W; idx += SG_MAXW) {
        const int i = idx / W, j = idx - i * W;
        uint8_t c = 0;
        if (i < n && j < n && i != j) {
            c = (uint8_t)src[max(i, j) * W + min(i, j)];
            if (c < 1 || c > 4) c = 0;
        }
        code[i * MCG_CODE_STRIDE + j] = c;
    }
    const int za = real ? z[(size_t)b * W + a] : 0;
    zs[a] = za;
    partner[a] = 0xff;
    inv[a] = 0;
    __syncthreads();

    const McgBondTally tally = mcg_bond_tally(code + a * MCG_CODE_STRIDE, real ? n : 0);
    const u64 mine = tally.mask, arom = tally.m4;
    const int half = tally.v2 - tally.narom;          // half-bonds of the valence check: an aromatic bond counts 2
    const int sigma = tally.n1 + 2 * tally.n2 + 3 * tally.n3 + tally.narom;      // sigma of the Kekule rule
    adj[a] = mine;
    __syncthreads();

    // fragments: this lane's component, its label, size and Z sum
    const u64 comp = real ? mcg_flood(adj, me, 0ull, n) : 0ull;
    int label = real ? low_bit(comp) : SG_MAXW, size = real ? __popcll(comp) : -1;
    long long zsum = 0;
    for (u64 m = comp; m != 0ull; m &= m - 1ull) zsum += zs[low_bit(m)];
    const int n_fragments = __popcll(__ballot(real && label == a));
    int best = label;
    for (int off = 32; off > 0; off >>= 1) {          // most atoms, then the larger Z sum, then the lowest label
        const int o_size = __shfl_xor(size, off), o_label = __shfl_xor(best, off);
        const int o_lo = __shfl_xor((int)(zsum & 0xffffffffll), off), o_hi = __shfl_xor((int)(zsum >> 32), off);
        const long long o_z = ((long long)o_hi << 32) | (unsigned int)o_lo;
        if (o_size > size || (o_size == size && (o_z > zsum || (o_z == zsum && o_label < best))))
            size = o_size, zsum = o_z, best = o_label;
    }
    const bool kept = real && label == best;
    const u64 keep = __ballot(kept);
    const int m_out = __popcll(keep);
    const int rank = __popcll(keep & low_bits(a));
    if (kept) inv[rank] = (uint8_t)a;

    int status = n == 0 ? SG_EMPTY : 0;
    {
        const int maxv = za >= 0 && za < MCG_N_ELEMENT_Z ? c_std_elements.max_valence[za] : 0;
        if (__ballot(kept && half > 2 * maxv) != 0ull) status |= SG_OVER_VALENCE;
    }

    // the parent's code-4 bonds, listed by their lower atom
    const u64 up = kept ? arom & ~low_bits(a) & ~me : 0ull;
    const int n_up = __popcll(up);
    int incl = n_up;
    for (int off = 1; off < SG_MAXW; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (a >= off) incl += v;
    }
    const int n_arom = __shfl(incl, SG_MAXW - 1);
    {
        int slot = incl - n_up;
        for (u64 m = up; m != 0ull; m &= m - 1ull) blist[slot++] = (uint16_t)(a | (low_bit(m) << 8));
    }
    __syncthreads();                                  // blist, inv
    bool bridge = false;
    for (int k = a; k < n_arom; k += SG_MAXW) {
        const int i = blist[k] & 0xff, j = blist[k] >> 8;
        const u64 bi = 1ull << i, bj = 1ull << j;
        u64 reach = bi, front = bi;
        while (front != 0ull && (reach & bj) == 0ull) {
            u64 nxt = reach;
            while (front != 0ull) {
                const int t = low_bit(front);
                front &= front - 1ull;
                u64 m = adj[t];
                if (t == i) m &= ~bj;
                if (t == j) m &= ~bi;
                nxt |= m;
            }
            front = nxt & ~reach;
            reach = nxt;
        }
        bridge = bridge || (reach & bj) == 0ull;
    }
    if (__ballot(bridge) != 0ull) status |= SG_AROMATIC_BRIDGE;

    // Kekule form: the eligible graph, its components, one search per component
    const bool elig = kept && arom != 0ull && mcg_valence0(za) - sigma >= 1;
    const u64 m_elig = __ballot(elig);
    const u64 m_optional = __ballot(elig && (za == 7 || za == 15 || za == 33));
    eadj[a] = elig ? arom & m_elig : 0ull;
    __syncthreads();
    const bool searching = (status & (SG_EMPTY | SG_OVER_VALENCE | SG_AROMATIC_BRIDGE)) == 0;
    const u64 ecomp = (searching && elig) ? mcg_flood(eadj, me, 0ull, n) : 0ull;
    const bool leader = ecomp != 0ull && low_bit(ecomp) == a;
    const int esize = leader ? __popcll(ecomp) : 0;
    int base = esize;
    for (int off = 1; off < SG_MAXW; off <<= 1) {
        const int v = __shfl_up(base, off);
        if (a >= off) base += v;
    }
    base -= esize;
    bool failed = false, spent = false;
    if (leader) {
        u64 matched = 0ull, skipped = 0ull;
        int depth = 0, steps = 0;
        bool enter = true;
        for (;;) {
            int atom = 0;
            u64 cand = 0ull;
            if (enter) {                              // one entry into the procedure of the definition: one step
                if (++steps > SG_BUDGET) {
                    spent = true;
                    break;
                }
                const u64 avail = ecomp & ~matched & ~skipped;
                if (avail == 0ull) break;             // every atom matched or skipped: this component has its form
                atom = high_bit(avail);
                cand = eadj[atom] & avail;
            } else {                                  // the recursion below the top frame failed: undo it, go on behind it
                if (depth == 0) {
                    failed = true;
                    break;
                }
                const int f = stack[base + --depth];
                atom = f & 0xff;
                const int choice = f >> 8;
                if (choice == SG_SKIP) {
                    skipped &= ~(1ull << atom);
                    continue;                         // behind the skip there is nothing: this frame fails too
                }
                matched &= ~((1ull << atom) | (1ull << choice));
                cand = eadj[atom] & ecomp & ~matched & ~skipped & low_bits(choice);
            }
            if (cand != 0ull) {
                const int p = high_bit(cand);
                matched |= (1ull << atom) | (1ull << p);
                stack[base + depth++] = (uint16_t)(atom | (p << 8));
                enter = true;
            } else if ((m_optional >> atom & 1ull) != 0ull) {
                skipped |= 1ull << atom;
                stack[base + depth++] = (uint16_t)(atom | (SG_SKIP << 8));
                enter = true;
            } else {
                enter = false;
            }
        }
        if (!failed && !spent)
            for (int d = 0; d < depth; ++d) {
                const int f = stack[base + d], i = f & 0xff, p = f >> 8;
                if (p != SG_SKIP) partner[i] = (uint8_t)p, partner[p] = (uint8_t)i;
            }
    }
    if (__ballot(failed) != 0ull) status |= SG_NOT_KEKULIZABLE;
    if (__ballot(spent) != 0ull) status |= SG_SEARCH_BUDGET;
    __syncthreads();                                  // partner

    // every element of every output
    const uint32_t* xin = coords + (size_t)b * N * 3;
    uint32_t* xout = coords_out + (size_t)b * N * 3;
    for (int r = a; r < N; r += SG_MAXW) {
        const bool w = r < m_out;
        const int s = w ? inv[r] : 0;
        xout[r * 3] = w ? xin[s * 3] : 0u;
        xout[r * 3 + 1] = w ? xin[s * 3 + 1] : 0u;
        xout[r * 3 + 2] = w ? xin[s * 3 + 2] : 0u;
    }
    if (a < W) {
        const bool w = a < m_out;
        z_out[(size_t)b * W + a] = w ? zs[inv[a]] : 0;
        atom_map_out[(size_t)b * W + a] = w ? (int32_t)inv[a] : -1;
    }
    int8_t* bout = bonds_out + (size_t)b * W * W;
    int8_t* kout = kekule_out + (size_t)b * W * W;
    for (int idx = a; idx < W * W; idx += SG_MAXW) {
        const int ri = idx / W, rj = idx - ri * W;
        int c = 0, k = 0;
        if (ri < m_out && rj < m_out) {
            const int i = inv[ri], j = inv[rj];
            c = code[i * MCG_CODE_STRIDE + j];
            if (status == 0) k = c == 4 ? (partner[i] == j ? 2 : 1) : c;
        }
        bout[idx] = (int8_t)c;
        kout[idx] = (int8_t)k;
    }
    if (a == 0) {
        n_out[b] = m_out;
        n_fragments_out[b] = n_fragments;
        removed_out[b] = n - m_out;
        status_out[b] = status;
    }
}

}  // namespace

extern "C" int mcg_standardize_graphs(const float* coords, const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                                      int B, int N, int W, float* coords_out, int32_t* z_out, int8_t* bonds_out,
                                      int8_t* kekule_out, int32_t* atom_map_out, int32_t* n_out, int32_t* n_fragments_out,
                                      int32_t* atoms_removed_out, int32_t* status_out, void* stream) {
    if (!coords || !z || !bonds || !n_nodes_dev || !coords_out || !z_out || !bonds_out || !kekule_out || !atom_map_out ||
        !n_out || !n_fragments_out || !atoms_removed_out || !status_out || B < 0 || B > MCG_STANDARDIZE_MAX_B || N < 1 ||
        W < 1 || W > SG_MAXW) {
        mcg_set_error("mcg_standardize_graphs: bad arguments (non-null coords, z, bonds, n_nodes and outputs, "
                      "0 <= B <= %d, N >= 1, 1 <= W <= %d)", MCG_STANDARDIZE_MAX_B, SG_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_standardize_graphs, dim3((unsigned)B), dim3(SG_MAXW), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(coords), z, bonds, n_nodes_dev, N, W,
                       reinterpret_cast<uint32_t*>(coords_out), z_out, bonds_out, kekule_out, atom_map_out, n_out,
                       n_fragments_out, atoms_removed_out, status_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
