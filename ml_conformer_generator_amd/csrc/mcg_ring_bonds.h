// The ring-bond rule that more than one kernel reads ("Rings and scaffolds"): bond (a, j) is a ring
// bond iff j is reachable from a with that bond left out.  Device code for kernels that run one 64-lane wave per molecule
// with lane = atom and keep every atom's 64-bit neighbour mask in LDS (k_substructure_match, k_ring_scaffold,
// k_torsion_tree, k_graph_fingerprint).  The flood is one lane's own: it holds no ballot and no cross-lane read, so lanes
// may take different trip counts.  Integer work only.
#pragma once
#include <stdint.h>
#include "mcg_wave.h"

// The length of the smallest cycle through bond (a, j), 0 where there is none: a breadth-first flood over `nbr` (LDS, one
// mask per atom; written and synchronised by the caller) from a's other neighbours.  `mine` = nbr[a], j a bit of it.  The
// frontier never holds a, and starts without j: the bond left out is not walked.  A round adds at least one atom: <= n
// rounds.  j enters the frontier in round d - 1 when the shortest way round has d bonds; the cycle then has d + 1.
__device__ __forceinline__ int mcg_ring_bond_size(const unsigned long long* nbr, int a, unsigned long long mine, int j,
                                                  int n) {
    const unsigned long long target = 1ull << j;
    unsigned long long reach = 1ull << a, frontier = mine & ~target;
    for (int it = 0; it < n && frontier != 0ull; ++it) {
        reach |= frontier;
        if ((reach & target) != 0ull) return it + 2;
        unsigned long long next = 0ull;
        for (unsigned long long g = frontier; g != 0ull; g &= g - 1ull) next |= nbr[low_bit(g)];
        frontier = next & ~reach;
    }
    return 0;
}

struct McgRingBonds {
    unsigned long long mask;                         // bit j: (a, j) is a ring bond
    int smallest, largest;                           // over a's ring bonds, the smallest cycle through each; 0, 0 without one
};

// every ring bond of atom a (`mine` = nbr[a]; 0 for a lane without an atom)
__device__ __forceinline__ McgRingBonds mcg_ring_bonds_of(const unsigned long long* nbr, int a, unsigned long long mine,
                                                          int n) {
    McgRingBonds r{0ull, 0, 0};
    for (unsigned long long f = mine; f != 0ull; f &= f - 1ull) {
        const int j = low_bit(f);
        const int size = mcg_ring_bond_size(nbr, a, mine, j, n);
        if (size != 0) {
            r.mask |= 1ull << j;
            r.smallest = r.smallest == 0 || size < r.smallest ? size : r.smallest;
            r.largest = size > r.largest ? size : r.largest;
        }
    }
    return r;
}
