// Rings and scaffolds ("Rings and scaffolds"): the ring bonds, ring systems, ring sizes, linker and exo
// atoms and the Murcko-type scaffold of each of B molecular graphs, and the induced sub-graph of an atom mask - exact in
// integers.  The package's OWN definitions - not RDKit's ring perception, SSSR or MurckoScaffold.
//   k_ring_scaffold:   one 64-lane workgroup (one wave) per molecule, lane = atom.  In LDS the bond-code rows (68-byte
//                      stride, as k_canonical_order) and per atom the 64-bit neighbour mask, then the ring-bond neighbour
//                      mask.  Ring bonds and their sizes: per lane, per bond, the flood of mcg_ring_bonds.h (lane-divergent
//                      on purpose: it holds no ballot).  Ring systems: per lane the closure of its ring-bond neighbourhood
//                      over the ring-bond masks in LDS, again the lane's own loop; the label is the lowest bit.  Pruning:
//                      the wave-uniform mask `alive` loses, per round, the ballot of the lanes with fewer than two live
//                      neighbours; the loop ends on that ballot being empty, so every lane takes the same trip count (a
//                      chain of n atoms: n / 2 rounds).  Linker, exo and scaffold masks are ballots.
//   k_induced_subgraph: one wave per molecule, lane = atom.  A kept atom's new index is the number of kept atoms below it
//                      (a popcount of the mask under its bit), so the kept atoms stay in ascending order; the new index ->
//                      old index table goes through LDS, and the W x W output is written by all lanes from the staged codes.
// No recursion, no scratch, no atomics: a molecule's outputs have the same bits whatever the batch, its row and the width.
#include "mcg_common.h"
#include "mcg_api_internal.h"
#include "mcg_graph_rules.h"
#include "mcg_ring_bonds.h"

namespace {

constexpr int SC_MAXW = MCG_SCAFFOLD_MAX_ATOMS;               // atoms per molecule: one lane, one bit of a 64-bit mask
static_assert(SC_MAXW == 64 && MCG_CODE_STRIDE == 68, "one wave per molecule: lane = atom, 68-byte code rows");

struct ScShared {
    __attribute__((aligned(16))) uint8_t code[SC_MAXW * MCG_CODE_STRIDE];
    unsigned long long nbr[SC_MAXW];                   // all neighbours
    unsigned long long ring_nb[SC_MAXW];               // neighbours over a ring bond
};

struct SgShared {
    __attribute__((aligned(16))) uint8_t code[SC_MAXW * MCG_CODE_STRIDE];
    int32_t src[SC_MAXW];                              // new index -> old index
};

__global__ __launch_bounds__(SC_MAXW) void k_ring_scaffold(
        const int32_t* __restrict__ z, const int8_t* __restrict__ bonds, const int32_t* __restrict__ n_nodes, int W,
        unsigned long long* __restrict__ ring_nb_out, int32_t* __restrict__ ring_size_out,
        int32_t* __restrict__ ring_system_out, unsigned long long* __restrict__ masks_out,
        int32_t* __restrict__ counts_out) {
    __shared__ ScShared s;
    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), W);
    const bool real = a < n;
    const unsigned long long me = 1ull << a;

    mcg_stage_codes(s.code, bonds + (size_t)b * W * W, W, n, a, SC_MAXW);
    __syncthreads();

    const McgBondTally tally = mcg_bond_tally(s.code + a * MCG_CODE_STRIDE, real ? n : 0);
    const unsigned long long mine = tally.mask, m2 = tally.m2;        // neighbours; neighbours over a code-2 bond
    s.nbr[a] = mine;
    __syncthreads();

    // ring bonds and the smallest cycle through each: the lane's own floods
    const McgRingBonds rb = mcg_ring_bonds_of(s.nbr, a, mine, n);
    s.ring_nb[a] = rb.mask;
    __syncthreads();
    const bool in_ring = rb.mask != 0ull;
    const unsigned long long ring = __ballot(in_ring ? 1 : 0);

    // ring systems: the closure of {a} under the ring-bond masks, the lane's own flood; the label is the lowest bit
    const unsigned long long comp = in_ring ? mcg_flood(s.ring_nb, me, 0ull, n) : 0ull;
    const int label = low_bit(comp);
    const unsigned long long heads = __ballot(in_ring && label == a ? 1 : 0);

    const int n_ring_bonds = wave_sum(__popcll(rb.mask)) / 2;
    const int n_ring_atoms = __popcll(ring), n_systems = __popcll(heads);
    const int smallest = wave_min(in_ring ? rb.smallest : 0x7fffffff);
    const int largest = wave_max(rb.largest);

    // pruning: every atom with fewer than two live neighbours leaves, round after round.  `alive` and `leave` are the same
    // in every lane, so the loop's end is wave-uniform; a round removes at least one atom: <= n rounds, + 1 to see the end.
    unsigned long long alive = low_bits(n);
    for (int round = 0; round <= n; ++round) {
        const bool out = (alive & me) != 0ull && __popcll(mine & alive) < 2;
        const unsigned long long leave = __ballot(out ? 1 : 0);
        if (leave == 0ull) break;
        alive &= ~leave;
    }
    const unsigned long long linker = alive & ~ring;
    const unsigned long long core = ring | linker;
    const unsigned long long exo = __ballot(real && (core & me) == 0ull && (m2 & core) != 0ull ? 1 : 0);

    if (a < W) {
        const size_t at = (size_t)b * W + a;
        ring_nb_out[at] = rb.mask;                     // 0 for a lane without an atom: the documented fill
        ring_size_out[at] = rb.smallest;
        ring_system_out[at] = label;
    }
    if (a < 4) masks_out[(size_t)b * 4 + a] = a == 0 ? ring : a == 1 ? linker : a == 2 ? exo : (core | exo);
    if (a < 8) {
        const int v = a == 0 ? n_ring_bonds - n_ring_atoms + n_systems : a == 1 ? n_systems
                      : a == 2 ? (n_ring_bonds != 0 ? smallest : 0) : a == 3 ? largest : a == 4 ? n_ring_atoms
                      : a == 5 ? __popcll(linker) : a == 6 ? __popcll(exo) : n_ring_bonds;
        counts_out[(size_t)b * 8 + a] = v;
    }
}

__global__ __launch_bounds__(SC_MAXW) void k_induced_subgraph(
        const int32_t* __restrict__ z, const int8_t* __restrict__ bonds, const int32_t* __restrict__ n_nodes,
        const unsigned long long* __restrict__ mask, int W, int mode, int32_t* __restrict__ z_out,
        int8_t* __restrict__ bonds_out, int32_t* __restrict__ n_out, int32_t* __restrict__ map_out) {
    __shared__ SgShared s;
    const int b = blockIdx.x, a = threadIdx.x;
    const int n = min(max(n_nodes[b], 0), W);
    const unsigned long long me = 1ull << a;
    const unsigned long long keep = mask[b] & low_bits(n);
    const int m = __popcll(keep);

    mcg_stage_codes(s.code, bonds + (size_t)b * W * W, W, n, a, SC_MAXW);
    const bool kept = (keep & me) != 0ull;             // implies a < n <= W
    const int pos = __popcll(keep & (me - 1ull));      // < m
    if (kept) s.src[pos] = a;
    __syncthreads();

    if (a < W) {
        const size_t at = (size_t)b * W + a;           // lane = NEW index from here on
        const int from = a < m ? s.src[a] : -1;
        map_out[at] = from;
        z_out[at] = from < 0 ? 0 : mode == 1 ? 6 : z[(size_t)b * W + from];
    }
    int8_t* dst = bonds_out + (size_t)b * W * W;
    for (int idx = a; idx < W * W; idx += SC_MAXW) {
        const int i = idx / W, j = idx - i * W;
        uint8_t c = 0;
        if (i < m && j < m) {
            c = s.code[s.src[i] * MCG_CODE_STRIDE + s.src[j]];
            if (mode == 1 && c != 0) c = 1;
        }
        dst[idx] = (int8_t)c;
    }
    if (a == 0) n_out[b] = m;
}

}  // namespace

extern "C" int mcg_ring_scaffold(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev, int B, int W,
                                 uint64_t* ring_nb_out, int32_t* ring_size_out, int32_t* ring_system_out,
                                 uint64_t* masks_out, int32_t* counts_out, void* stream) {
    if (!z || !bonds || !n_nodes_dev || !ring_nb_out || !ring_size_out || !ring_system_out || !masks_out || !counts_out ||
        B < 0 || B > MCG_SCAFFOLD_MAX_B || W < 1 || W > SC_MAXW) {
        mcg_set_error("mcg_ring_scaffold: bad arguments (non-null z, bonds, n_nodes, ring_nb_out, ring_size_out, "
                      "ring_system_out, masks_out and counts_out, 0 <= B <= %d, 1 <= W <= %d)", MCG_SCAFFOLD_MAX_B, SC_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_ring_scaffold, dim3((unsigned)B), dim3(SC_MAXW), 0, (hipStream_t)stream, z, bonds, n_nodes_dev, W,
                       reinterpret_cast<unsigned long long*>(ring_nb_out), ring_size_out, ring_system_out,
                       reinterpret_cast<unsigned long long*>(masks_out), counts_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}

extern "C" int mcg_induced_subgraph(const int32_t* z, const int8_t* bonds, const int32_t* n_nodes_dev,
                                    const uint64_t* mask, int mode, int B, int W, int32_t* z_out, int8_t* bonds_out,
                                    int32_t* n_out, int32_t* map_out, void* stream) {
    if (!z || !bonds || !n_nodes_dev || !mask || !z_out || !bonds_out || !n_out || !map_out || B < 0 ||
        B > MCG_SCAFFOLD_MAX_B || W < 1 || W > SC_MAXW || mode < 0 || mode > 1) {
        mcg_set_error("mcg_induced_subgraph: bad arguments (non-null z, bonds, n_nodes, mask, z_out, bonds_out, n_out and "
                      "map_out, mode 0 or 1, 0 <= B <= %d, 1 <= W <= %d)", MCG_SCAFFOLD_MAX_B, SC_MAXW);
        return MCG_ERR_ARG;
    }
    if (B == 0) return MCG_OK;
    hipLaunchKernelGGL(k_induced_subgraph, dim3((unsigned)B), dim3(SC_MAXW), 0, (hipStream_t)stream, z, bonds, n_nodes_dev,
                       reinterpret_cast<const unsigned long long*>(mask), W, mode, z_out, bonds_out, n_out, map_out);
    MCG_HIP(hipGetLastError());
    return MCG_OK;
}
