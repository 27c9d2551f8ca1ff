"""Fixtures of the receptor-interaction tests: hand-computable pairs, the named molecules whose types and rotatable bonds
the definition pins, and a synthetic PDB string typed atom by atom."""
import math
import random

import numpy as np

import canonical_cases as CC
import canonical_ref as CR
import interactions_ref as R
import pharmacophore_cases as PC

D, A, H = R.DONOR, R.ACCEPTOR, R.HYDROPHOBIC
E225 = math.exp(-2.25)


def _pair(r, zi, ti, zj, tj):
    """One ligand atom at the origin and one receptor atom at distance r on the x axis."""
    return dict(x=np.zeros((1, 3), dtype=np.float32), z=[zi], t=[ti], y=np.array([[r, 0.0, 0.0]], dtype=np.float32),
                zr=[zj], tr=[tj])


# the largest fp32 below 8 and the smallest above it, whose squares round to fp32 values below and above 64
BELOW_8 = float(np.nextafter(np.float32(8.0), np.float32(0.0)))
ABOVE_8 = float(np.nextafter(np.float32(8.0), np.float32(9.0)))
assert np.float32(BELOW_8) * np.float32(BELOW_8) < np.float32(64.0) < np.float32(ABOVE_8) * np.float32(ABOVE_8)

# name -> (the pair, the expected values by hand: g1, g2, rep, hyd, hb, hbonds; None = not pinned here)
HAND = {
    "C...C at 3.8 A": (_pair(3.8, 6, H, 6, H), dict(g1=1.0, g2=E225, rep=0.0, hyd=1.0, hb=0.0, hbonds=0)),
    "donor O to acceptor O at 2.7 A": (_pair(2.7, 8, D, 8, A), dict(rep=0.49, hyd=0.0, hb=1.0, hbonds=1)),
    "acceptor O to donor O at 2.7 A": (_pair(2.7, 8, A, 8, D), dict(rep=0.49, hyd=0.0, hb=1.0, hbonds=1)),
    "two donors at 2.7 A": (_pair(2.7, 8, D, 8, D), dict(rep=0.49, hyd=0.0, hb=0.0, hbonds=0)),
    "just inside the cut-off": (_pair(BELOW_8, 6, H, 6, H), dict(rep=0.0, hyd=0.0, hb=0.0, hbonds=0, counted=True)),
    "just outside the cut-off": (_pair(ABOVE_8, 6, H, 6, H), dict(g1=0.0, g2=0.0, rep=0.0, hyd=0.0, hb=0.0, hbonds=0,
                                                                  counted=False)),
}
# 3.8 - (1.9 + 1.9) and 2.7 - (1.7 + 1.7) are not exactly 0 and -0.7 in fp32: the fp32 d is within an ulp of 4 of them, and
# the ramps and g1 are continuous there, so the hand values hold to 1e-6 - except the decision d <= -0.7f itself, which the
# restatement takes from the same fp32 d and the hand table states for it


def hand_args(pair, n_rot=0):
    return (pair["x"], R.radii(pair["z"]), pair["t"], pair["y"], R.radii(pair["zr"]), pair["tr"], n_rot)


# ----------------------------------------------------------------------------------------------- ligand typing
TOLUENE = CC.NAMED["toluene"][0]
ACETAMIDE = PC.PINNED["acetamide"][0]             # C C(=O) N: atoms 0 CH3, 1 C=O, 2 O, 3 N
BUTANE = CR.mol([6] * 4, CC._chain(4))
ETHANE = CR.mol([6] * 2, CC._chain(2))
CHAIN64 = CC.EDGES["64-atom chain"]
# name -> (molecule, hydrophobic flags or None, n_rot)
MOLECULES = {
    "toluene": (TOLUENE, [True] * 7, 0),
    "acetamide": (ACETAMIDE, [True, False, False, False], 0),
    "chlorobenzene": (PC.PINNED["chlorobenzene"][0], [True] * 7, 0),
    "pyridine": (PC.PINNED["pyridine"][0], [False, False, True, True, True, False], 0),
    "ethanol": (PC.PINNED["ethanol"][0], [True, False, False], 0),
    "butane": (BUTANE, [True] * 4, 1),
    "biphenyl": (CC.NAMED["biphenyl"][0], [True] * 12, 1),
    "decalin": (CC.NAMED["decalin"][0], [True] * 10, 0),
    "ethane": (ETHANE, [True] * 2, 0),
    "64-atom chain": (CHAIN64, [True] * 64, 61),
}


def renumberings(mol, count=4, seed=5):
    """`mol` itself and count - 1 seeded renumberings of it, each with the permutation p (new atom k = old atom p[k])."""
    rng = random.Random(seed)
    out = [(mol, list(range(mol[2])))]
    for _ in range(count - 1):
        p = list(range(mol[2]))
        rng.shuffle(p)
        out.append((CR.permute(*mol, p), p))
    return out


def pharm_types(mol):
    import pharmacophore_ref as PR
    return PR.perceive(*mol)[0]


# ----------------------------------------------------------------------------------------------- the PDB string
def _line(rec, serial, atom, res, seq, x, y, z, el):
    name = atom.ljust(4) if len(el) == 2 else (" " + atom).ljust(4)
    return "%-6s%5d %4s %3s A%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s" % (rec, serial, name, res, seq, x, y, z, el)


# (record, atom, residue, sequence number, xyz, element, expected type)
PDB_ATOMS = [
    ("ATOM", "N", "GLY", 1, (0.000, 0.000, 0.000), "N", D),
    ("ATOM", "CA", "GLY", 1, (1.458, 0.000, 0.000), "C", 0),                # 1.458 A from its N
    ("ATOM", "C", "GLY", 1, (2.009, 1.420, 0.000), "C", 0),                 # bonded to O and to SER N
    ("ATOM", "O", "GLY", 1, (1.251, 2.390, 0.000), "O", A),
    ("ATOM", "N", "SER", 2, (3.332, 1.536, 0.000), "N", D),
    ("ATOM", "CA", "SER", 2, (3.988, 2.839, 0.000), "C", 0),
    ("ATOM", "C", "SER", 2, (5.504, 2.693, 0.000), "C", 0),
    ("ATOM", "O", "SER", 2, (6.018, 1.573, 0.000), "O", A),
    ("ATOM", "CB", "SER", 2, (3.540, 3.650, 1.220), "C", 0),                # bonded to OG
    ("ATOM", "OG", "SER", 2, (3.900, 5.020, 1.100), "O", D | A),
    ("ATOM", "N", "ASP", 3, (6.217, 3.818, 0.000), "N", D),
    ("ATOM", "CA", "ASP", 3, (7.672, 3.830, 0.000), "C", 0),
    ("ATOM", "C", "ASP", 3, (8.190, 5.260, 0.000), "C", 0),
    ("ATOM", "O", "ASP", 3, (7.420, 6.220, 0.000), "O", A),
    ("ATOM", "CB", "ASP", 3, (8.210, 3.080, 1.220), "C", H),                # no N or O within 1.75 A
    ("ATOM", "CG", "ASP", 3, (9.730, 3.060, 1.250), "C", 0),
    ("ATOM", "OD1", "ASP", 3, (10.340, 3.650, 0.330), "O", A),
    ("ATOM", "OD2", "ASP", 3, (10.290, 2.450, 2.190), "O", A),
    ("ATOM", "OXT", "ASP", 3, (9.420, 5.430, 0.000), "O", A),
    ("HETATM", "O", "HOH", 4, (14.000, 3.000, 1.000), "O", D | A),
    ("HETATM", "ZN", "ZN", 5, (12.000, 4.000, 1.500), "ZN", D),
]
PDB = "\n".join(_line(rec, k + 1, atom, res, seq, *xyz, el)
                for k, (rec, atom, res, seq, xyz, el, _) in enumerate(PDB_ATOMS)) + "\nEND\n"
PDB_UNTEMPLATED = 1                               # the zinc

# a proline, a HETATM ligand with an N, an O, a C, an S and a Cl, and a hydrogen that is dropped
EXTRA_ATOMS = [
    ("ATOM", "N", "PRO", 6, (20.000, 0.000, 0.000), "N", 0),
    ("ATOM", "CD", "PRO", 6, (20.900, 1.150, 0.000), "C", 0),
    ("ATOM", "H", "GLY", 1, (-0.500, 0.800, 0.000), "H", None),
    ("HETATM", "N1", "LIG", 7, (30.000, 0.000, 0.000), "N", D | A),
    ("HETATM", "O1", "LIG", 7, (30.000, 5.000, 0.000), "O", D | A),
    ("HETATM", "C1", "LIG", 7, (30.000, 10.000, 0.000), "C", H),
    ("HETATM", "S1", "LIG", 7, (30.000, 15.000, 0.000), "S", 0),
    ("HETATM", "CL1", "LIG", 7, (30.000, 20.000, 0.000), "CL", H),
    ("ATOM", "OD1", "GLY", 8, (40.000, 0.000, 0.000), "O", D | A),          # a name the residue's template does not know
]
PDB_EXTRA = "\n".join(_line(rec, k + 1, atom, res, seq, *xyz, el)
                      for k, (rec, atom, res, seq, xyz, el, _) in enumerate(PDB_ATOMS + EXTRA_ATOMS)) + "\nEND\n"
EXTRA_UNTEMPLATED = PDB_UNTEMPLATED + 3           # the ligand's N and O, and the misnamed O
