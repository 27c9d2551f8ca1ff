// The per-atom count and class rules of a molecular graph that more than one kernel reads ("Explicit
// hydrogens": Count and Parent): the bond tally of an atom's row of codes, its hydrogens nH - the pharmacophore perception's
// count plus the one aromatic N-H per 5-ring - and whether it is linear, planar or tetrahedral.  Device code for kernels
// that run one 64-lane wave per molecule with lane = atom (k_hydrogens_place, k_charges_peoe): what a rule asks of OTHER
// atoms arrives as a ballot mask.  Integer work only.
#pragma once
#include <stdint.h>

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
    int deg, v2, n2, n3, narom;                      // bonded atoms; twice the bond-order sum (codes 1 2 3 4 add 2 4 6 3); code counts
};

// the tally of one atom's staged row over the molecule's n atoms
__device__ __forceinline__ McgBondTally mcg_bond_tally(const uint8_t* row, int n) {
    McgBondTally t{0ull, 0, 0, 0, 0, 0};
    for (int j = 0; j < n; ++j) {
        const int c = row[j];
        if (c != 0) {
            t.mask |= 1ull << j;
            ++t.deg;
            t.v2 += c == 1 ? 2 : c == 2 ? 4 : c == 3 ? 6 : 3;
            t.n2 += c == 2 ? 1 : 0;
            t.n3 += c == 3 ? 1 : 0;
            t.narom += c == 4 ? 1 : 0;
        }
    }
    return t;
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
