// Elements a caller's atom decoder may name, by atomic number (the Python side's config.ELEMENTS):
// single-bond covalent radius (Angstrom, Cordero et al. 2008) for the covalent-radius connectivity of the hand-off, and
// the maximum valence of the validity proxy behind the GCN.  A zero radius marks a Z the library does not know; such a Z
// keeps maximum valence 0.  The eight default elements (C N O F P S Cl Br) carry the values the kernels always used.
#pragma once

constexpr int MCG_N_ELEMENT_Z = 36;          // = the GCN's element embedding rows (config.GCN_NUM_EMBEDDINGS)
constexpr int MCG_N_ATOM_CLASSES = 8;

struct McgElementTable {
    double rcov[MCG_N_ELEMENT_Z];
    int max_valence[MCG_N_ELEMENT_Z];
};

constexpr McgElementTable MCG_ELEMENTS = {
    //  Z: 0    1    2    3    4    5 B   6 C   7 N   8 O   9 F   10   11   12   13   14 Si  15 P  16 S  17 Cl
    {0.0, 0.0, 0.0, 0.0, 0.0, 0.84, 0.76, 0.71, 0.66, 0.57, 0.0, 0.0, 0.0, 0.0, 1.11, 1.07, 1.05, 1.02,
    //  18   19   20   21   22   23   24   25   26   27   28   29   30   31   32  33 As  34 Se  35 Br
     0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.19, 1.20, 1.20},
    {0, 0, 0, 0, 0, 3, 4, 4, 2, 1, 0, 0, 0, 0, 4, 5, 6, 1,
     0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 6, 1},
};

// class -> atomic number, passed by value to the hand-off kernel
struct McgClassZ {
    int z[MCG_N_ATOM_CLASSES];
};

constexpr McgClassZ MCG_DEFAULT_CLASS_Z = {{6, 7, 8, 9, 15, 16, 17, 35}};     // config.py:20-29 (sorted PERMITTED_ELEMENTS)
