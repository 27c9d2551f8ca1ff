// The prologue and the per-atom count and class rules of a molecular graph that the graph kernels share (DESIGN.md section
// 6, "The shared prologue of the graph kernels" and "Explicit hydrogens": Count and Parent): staging the bond codes, the bond
// tally of an atom's row of codes, the flood over neighbour masks, an atom's hydrogens nH - the pharmacophore perception's
// count plus the one aromatic N-H per 5-ring - and whether it is linear, planar or tetrahedral.  Device code for kernels
// that run one 64-lane wave per molecule with lane = atom: what a rule asks of OTHER atoms arrives as a ballot mask.
// Integer work only.
#pragma once
#include <stdint.h>
#include "mcg_wave.h"

enum : int { MCG_CLASS_TETRAHEDRAL = 0, MCG_CLASS_PLANAR = 1, MCG_CLASS_LINEAR = 2 };

constexpr int MCG_CODE_STRIDE = 68;                  // bytes per bond-code row in LDS (17 dwords)

// v0 of pharmacophore.py: B 3, C 4, N 3, O 2, F 1, Si 4, P 3, S 2, Cl 1, As 3, Se 2, Br 1, I 1; any other element 0
__device__ __forceinline__ int mcg_valence0(int z) {
    switch (z) {
        case 6: case 14: return 4;
        case 5: case 7: case 15: case 33: return 3;
        case 8: case 16: case 34: return 2;
        case 9: case 17: case 35: case 53: return 1;
        default: return 0;
    }
}

// a molecule's W x W codes -> LDS rows of MCG_CODE_STRIDE bytes, by the `lanes` lanes of one wave; the diagonal, everything at
// or beyond n and every code outside 1..4 become 0
__device__ __forceinline__ void mcg_stage_codes(uint8_t* code, const int8_t* src, int W, int n, int lane, int lanes) {
    for (int idx = lane; idx < W * W; idx += lanes) {
        const int i = idx / W, j = idx - i * W;
        const uint8_t c = (uint8_t)src[idx];
        code[i * MCG_CODE_STRIDE + j] = (i < n && j < n && i != j && c >= 1 && c <= 4) ? c : (uint8_t)0;
    }
}

struct McgBondTally {
    unsigned long long mask;                         // bit j: bonded to atom j
    unsigned long long m1, m2, m3, m4;               // the same per bond code 1 2 3 4
    int deg, v2, n1, n2, n3, narom;                  // bonded atoms; twice the bond-order sum (codes 1 2 3 4 add 2 4 6 3); code counts
};

// the tally of one atom's staged row over the molecule's n atoms; n = 0 for a lane without an atom: the empty tally
__device__ __forceinline__ McgBondTally mcg_bond_tally(const uint8_t* row, int n) {
    McgBondTally t{};
    for (int j = 0; j < n; ++j) {
        const int c = row[j];
        const unsigned long long bit = 1ull << j;
        t.m1 |= c == 1 ? bit : 0ull;
        t.m2 |= c == 2 ? bit : 0ull;
        t.m3 |= c == 3 ? bit : 0ull;
        t.m4 |= c == 4 ? bit : 0ull;
    }
    t.mask = t.m1 | t.m2 | t.m3 | t.m4;
    t.n1 = __popcll(t.m1), t.n2 = __popcll(t.m2), t.n3 = __popcll(t.m3), t.narom = __popcll(t.m4);
    t.deg = t.n1 + t.n2 + t.n3 + t.narom;
    t.v2 = 2 * t.n1 + 4 * t.n2 + 6 * t.n3 + 3 * t.narom;
    return t;
}

// every atom reachable from the atoms of `start` without entering an atom of `blocked`: a breadth-first flood over `nbr`
// (LDS, one mask per atom; written and synchronised by the caller), frontier by frontier, so every member's mask is read
// once.  One lane's own: no ballot, no cross-lane read.  A round adds at least one atom: <= n rounds.
__device__ __forceinline__ unsigned long long mcg_flood(const unsigned long long* nbr, unsigned long long start,
                                                        unsigned long long blocked, int n) {
    unsigned long long reach = start, frontier = start;
    for (int it = 0; it < n && frontier != 0ull; ++it) {
        unsigned long long next = 0ull;
        for (unsigned long long g = frontier; g != 0ull; g &= g - 1ull) next |= nbr[low_bit(g)];
        frontier = next & ~reach & ~blocked;
        reach |= frontier;
    }
    return reach;
}

__device__ __forceinline__ bool mcg_has_code_2_or_4(const McgBondTally& t) { return t.n2 >= 1 || t.narom >= 1; }

// linear: a code-3 bond or two code-2 bonds; planar: a code-2 or code-4 bond, or an N / O next to an atom that has one
// (`m_has24`: the ballot of mcg_has_code_2_or_4 over the molecule's atoms); tetrahedral otherwise
__device__ __forceinline__ int mcg_parent_class(int z, const McgBondTally& t, unsigned long long m_has24) {
    return (t.n3 >= 1 || t.n2 >= 2) ? MCG_CLASS_LINEAR
           : (mcg_has_code_2_or_4(t) || ((z == 7 || z == 8) && (t.mask & m_has24) != 0ull)) ? MCG_CLASS_PLANAR
                                                                                             : MCG_CLASS_TETRAHEDRAL;
}

// whether atom a may take the aromatic N-H of a 5-ring: an aromatic N of degree 2 carrying the perception's donor bit
__device__ __forceinline__ bool mcg_ring_nh_candidate(int z, const McgBondTally& t, int type_bits) {
    return z == 7 && t.narom >= 1 && t.deg == 2 && (type_bits & 1) != 0;
}

// nH of atom `a`: max(0, (2 v0 - v2) / 2), plus the one aromatic N-H per 5-ring - the kept rings (`rings[0..nr)`, ascending
// masks) walked in list order, the same walk in every lane; `m_ring_n`: the ballot of mcg_ring_nh_candidate
__device__ __forceinline__ int mcg_implicit_hydrogens(bool real, int a, int z, const McgBondTally& t,
                                                      const unsigned long long* rings, int nr,
                                                      unsigned long long m_ring_n) {
    int nh = real ? max(0, (2 * mcg_valence0(z) - t.v2) / 2) : 0;
    unsigned long long given = 0ull;
    for (int r = 0; r < nr; ++r) {
        const unsigned long long m = rings[r];
        const unsigned long long cand = m & m_ring_n;
        if (__popcll(m) == 5 && (m & given) == 0ull && cand != 0ull) given |= cand & (~cand + 1ull);
    }
    if ((given >> a & 1ull) != 0ull) nh = 1;
    return nh;
}
