"""The named embedded molecules of the stereo-identity tests ("Stereo identity"), built by
construction from ideal directions - or by swapping two substituents' positions to invert one centre -, their
renumberings and proper rigid motions, the seeded molecule-like fuzz set and the padded-batch builder.  A molecule is
(z, adj, n, xyz) as in `stereo_ref`.

Leaf counts of the stereo search, by hand: it skips only twins of degree <= 1, so a pair of non-terminal twins costs one
leaf per order.  CHFClBr, CFClBrI and 2-butanol have no automorphism (1 leaf), nor have the gem-dimethyl, CF3 and planar
cases once their terminal twins are skipped (1); the 2,3-dichlorobutanes' graph has the swap of its halves (2), as have
3-pentanol (its two ethyls), the dichloroethenes, cyclohexene and hexa-2,4-diene (2 each); 1,3-dimethylcyclobutane: the
swap of the two ring CH2 - twins, skipped by the graph search - times the swap of the two CH(CH3) (4 against the graph
search's 2); 1,4-dimethylcyclohexane: the ring's two reflections (4)."""
import math
import random

import canonical_ref as R

_T = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]
BOND = 1.5


def _tet(k, sign=1, at=(0.0, 0.0, 0.0)):
    """The point one bond along the k-th ideal tetrahedral direction (of the inverted tetrahedron for sign = -1)."""
    s = sign * BOND / math.sqrt(3.0)
    return (at[0] + s * _T[k][0], at[1] + s * _T[k][1], at[2] + s * _T[k][2])


def _mol(z, bonds, xyz):
    zz, adj, n = R.mol(z, bonds)
    assert len(xyz) == n
    return zz, adj, n, [tuple(float(v) for v in p) for p in xyz]


def mirror(mol):
    z, adj, n, xyz = mol
    return z, adj, n, [(-p[0], p[1], p[2]) for p in xyz]


def swapped(mol, a, b):
    """The molecule with the positions of atoms a and b exchanged: inverts the centre both are bonded to."""
    z, adj, n, xyz = mol
    xyz = list(xyz)
    xyz[a], xyz[b] = xyz[b], xyz[a]
    return z, adj, n, xyz


def renumbered(rng, mol):
    z, adj, n, xyz = mol
    p = list(range(n))
    rng.shuffle(p)
    zz, aa, _ = R.permute(z, adj, n, p)
    return zz, aa, n, [xyz[a] for a in p]


def moved(rng, mol):
    """A random PROPER rotation (a unit quaternion's) and a translation."""
    z, adj, n, xyz = mol
    q = [rng.gauss(0, 1) for _ in range(4)]
    s = math.sqrt(sum(v * v for v in q))
    w, x, y, zq = (v / s for v in q)
    rot = [[1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * w), 2 * (x * zq + y * w)],
           [2 * (x * y + zq * w), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * w)],
           [2 * (x * zq - y * w), 2 * (y * zq + x * w), 1 - 2 * (x * x + y * y)]]
    t = [rng.uniform(-5, 5) for _ in range(3)]
    return z, adj, n, [tuple(sum(rot[i][k] * p[k] for k in range(3)) + t[i] for i in range(3)) for p in xyz]


# ------------------------------------------------------------------------------------------------- the named cases
CHFCLBR = _mol([6, 9, 17, 35], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], [(0, 0, 0), _tet(0), _tet(1), _tet(2)])
CFCLBRI = _mol([6, 9, 17, 35, 53], [(0, k, 1) for k in range(1, 5)], [(0, 0, 0), _tet(0), _tet(1), _tet(2), _tet(3)])
# C0 - C1(O2) - C3 - C4
BUTAN_2_OL = _mol([6, 6, 8, 6, 6], [(0, 1, 1), (1, 2, 1), (1, 3, 1), (3, 4, 1)],
                  [_tet(0), (0, 0, 0), _tet(1), _tet(2), _tet(3, -1, _tet(2))])
# C0 - C1 - C2(O5) - C3 - C4
PENTAN_3_OL = _mol([6, 6, 6, 6, 6, 8], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (2, 5, 1)],
                   [_tet(3, -1, _tet(0)), _tet(0), (0, 0, 0), _tet(1), _tet(3, -1, _tet(1)), _tet(2)])
# C0 - C1(Cl4) - C2(Cl5) - C3: C2's other three directions are those of the inverted tetrahedron
_DCB = _mol([6, 6, 6, 6, 17, 17], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (1, 4, 1), (2, 5, 1)],
            [_tet(0), (0, 0, 0), _tet(2), _tet(0, -1, _tet(2)), _tet(1), _tet(1, -1, _tet(2))])
DICHLOROBUTANES = [_DCB, swapped(_DCB, 0, 4), swapped(_DCB, 3, 5), swapped(swapped(_DCB, 0, 4), 3, 5)]


def _dichloroethene(side):
    return _mol([17, 6, 6, 17], [(0, 1, 1), (1, 2, 2), (2, 3, 1)],
                [(-0.87, 1.5, 0), (0, 0, 0), (1.34, 0, 0), (2.21, 1.5 * side, 0)])


def _dimethylcyclobutane(side):
    return _mol([6] * 6, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1), (0, 4, 1), (2, 5, 1)],
                [(1.1, 0, 0), (0, 1.1, 0), (-1.1, 0, 0), (0, -1.1, 0), (1.9, 0, 1.2), (-1.9, 0, 1.2 * side)])


def _dimethylcyclohexane(side):
    ring = [(1.45 * math.cos(k * math.pi / 3), 1.45 * math.sin(k * math.pi / 3), 0.25 * (-1) ** k) for k in range(6)]
    return _mol([6] * 8, [(k, (k + 1) % 6, 1) for k in range(6)] + [(0, 6, 1), (3, 7, 1)],
                ring + [(2.25, 0, 1.45), (-2.25, 0, -0.25 + 1.2 * side)])


def _ring_in_plane(n, radius=1.4):
    return [(radius * math.cos(2 * k * math.pi / n), radius * math.sin(2 * k * math.pi / n), 0.0) for k in range(n)]


CIS_DCE, TRANS_DCE = _dichloroethene(1), _dichloroethene(-1)
CIS_DMCB, TRANS_DMCB = _dimethylcyclobutane(1), _dimethylcyclobutane(-1)
CIS_DMCH, TRANS_DMCH = _dimethylcyclohexane(1), _dimethylcyclohexane(-1)
CYCLOHEXENE = _mol([6] * 6, [(k, (k + 1) % 6, 2 if k == 0 else 1) for k in range(6)], _ring_in_plane(6))
GEM_DIMETHYL = _mol([6, 6, 6, 9, 17], [(0, k, 1) for k in range(1, 5)], [(0, 0, 0), _tet(0), _tet(1), _tet(2), _tet(3)])
CF3_PARENT = _mol([6, 9, 9, 9, 6, 17], [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (4, 5, 1)],
                  [(0, 0, 0), _tet(0), _tet(1), _tet(2), _tet(3), _tet(0, -1, _tet(3))])
PLANAR_CENTRE = _mol([6, 9, 17, 35], [(0, 1, 1), (0, 2, 1), (0, 3, 1)],
                     [(0, 0, 0), (1.5, 0, 0), (-0.75, 1.3, 0), (-0.75, -1.3, 0)])
# hexa-2,4-diene, all trans: two double bonds that share the single bond C2-C3
HEXADIENE = _mol([6] * 6, [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 5, 1)],
                 [(-0.75, 1.3, 0), (0, 0, 0), (1.34, 0, 0), (2.09, -1.3, 0), (3.43, -1.3, 0), (4.18, -2.6, 0)])
HEXADIENE_CIS_TRANS = _mol(HEXADIENE[0], [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 5, 1)],
                           [(-0.75, -1.3, 0)] + HEXADIENE[3][1:])
# trans-cyclooctene: the ring is the only thing on either end of the double bond
_OCT = [(0, 0, 0), (1.34, 0, 0), (2.1, -1.3, 0.3), (2.0, -2.0, 1.7), (1.2, -1.2, 2.8), (0.1, -0.2, 2.9), (-1.0, 0.6, 2.0),
        (-0.76, 1.3, 0.6)]
TRANS_CYCLOOCTENE = _mol([6] * 8, [(k, (k + 1) % 8, 2 if k == 0 else 1) for k in range(8)], _OCT)

# name -> (molecule, (defined tet, defined db, undefined), the leaves of the stereo search, equal to its mirror image?)
NAMED = {
    "CHFClBr": (CHFCLBR, (1, 0, 0), 1, False),
    "CFClBrI": (CFCLBRI, (1, 0, 0), 1, False),
    "2-butanol": (BUTAN_2_OL, (1, 0, 0), 1, False),
    "3-pentanol": (PENTAN_3_OL, (1, 0, 0), 2, True),
    "2,3-dichlorobutane a": (DICHLOROBUTANES[0], (2, 0, 0), 2, None),
    "2,3-dichlorobutane b": (DICHLOROBUTANES[1], (2, 0, 0), 2, None),
    "cis-1,2-dichloroethene": (CIS_DCE, (0, 1, 0), 2, True),
    "trans-1,2-dichloroethene": (TRANS_DCE, (0, 1, 0), 2, True),
    "cis-1,3-dimethylcyclobutane": (CIS_DMCB, (2, 0, 0), 4, True),
    "trans-1,3-dimethylcyclobutane": (TRANS_DMCB, (2, 0, 0), 4, True),
    "cis-1,4-dimethylcyclohexane": (CIS_DMCH, (2, 0, 0), 4, True),
    "trans-1,4-dimethylcyclohexane": (TRANS_DMCH, (2, 0, 0), 4, True),
    "cyclohexene": (CYCLOHEXENE, (0, 1, 0), 2, True),
    "gem-dimethyl parent": (GEM_DIMETHYL, (0, 0, 0), 1, True),
    "CF3 parent": (CF3_PARENT, (0, 0, 0), 1, True),
    "planar centre": (PLANAR_CENTRE, (0, 0, 1), 1, True),
    "hexa-2,4-diene": (HEXADIENE, (0, 2, 0), 2, True),
}


def sixty_four():
    """A 64-atom chain whose only stereocentre is atom 1: neighbours 0 (F), 2 and 63 (Cl, the last lane)."""
    z = [9] + [6] * 62 + [17]
    bonds = [(0, 1, 1)] + [(k, k + 1, 1) for k in range(1, 62)] + [(1, 63, 1)]
    xyz = [_tet(0), (0, 0, 0), _tet(1)] + [(_tet(1)[0] + 1.3 * (k - 2), _tet(1)[1] - 0.4 * ((k - 2) % 2), _tet(1)[2])
                                          for k in range(3, 63)] + [_tet(2)]
    return _mol(z, bonds, xyz)


def over_degree():
    """Atom 0 with nine neighbours: DEGREE."""
    rng = random.Random(9)
    return _mol([6] * 10, [(0, k, 1) for k in range(1, 10)], [tuple(rng.uniform(-2, 2) for _ in range(3)) for _ in range(10)])


# ------------------------------------------------------------------------------------------------- fuzz
FUZZ_SEED = 20261020


def molecule_like(rng, n):
    """A random tree of degree <= 4 with a few ring closures, mostly single bonds, C with some N O F Cl; terminal atoms
    are often halogens so that terminal twins and real centres both occur."""
    z = [rng.choice((6, 6, 6, 6, 6, 7, 8)) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    deg = [0] * n

    def room(a):
        return deg[a] < (4 if z[a] == 6 else 3 if z[a] == 7 else 2)
    for a in range(1, n):
        parents = [p for p in range(a) if room(p)]
        if not parents:
            continue
        p = rng.choice(parents[-6:])
        adj[a][p] = adj[p][a] = 1
        deg[a] += 1
        deg[p] += 1
    for _ in range(rng.randint(0, 3)):
        a, b = rng.randrange(n), rng.randrange(n)
        if a != b and adj[a][b] == 0 and room(a) and room(b):
            adj[a][b] = adj[b][a] = 1
            deg[a] += 1
            deg[b] += 1
    for a in range(n):
        if deg[a] == 1 and rng.random() < 0.5:
            z[a] = rng.choice((9, 9, 17, 8, 6))
    for _ in range(rng.randint(0, 4)):                       # some double bonds where both ends have a valence left
        a = rng.randrange(n)
        nb = [j for j in range(n) if adj[a][j] == 1]
        if nb:
            b = rng.choice(nb)
            if z[a] in (6, 7) and z[b] in (6, 7) and room(a) and room(b) and all(c != 2 for c in adj[a] + adj[b]):
                adj[a][b] = adj[b][a] = 2
                deg[a] += 1                                   # a valence, not a neighbour: keeps `room` honest
                deg[b] += 1
    return z, adj, n


def doubled(rng, n):
    """Two copies of one `molecule_like` fragment joined through a bond between their first atoms (and, for odd n, a
    carbon between them): an automorphism that swaps the halves, so leaves tie on the certificate and the stereo vector
    decides - meso forms and enantiomer-like halves under random coordinates."""
    h = n // 2
    z, adj, _ = molecule_like(rng, h)
    zz = z + z + [6] * (n - 2 * h)
    out = [[0] * n for _ in range(n)]
    for a in range(h):
        for b in range(h):
            out[a][b] = out[h + a][h + b] = adj[a][b]
    free = sum(1 for c in adj[0] if c) + sum(1 for c in adj[0] if c == 2) < (4 if z[0] == 6 else 3 if z[0] == 7 else 2)
    if n > 2 * h:
        out[0][n - 1] = out[n - 1][0] = out[h][n - 1] = out[n - 1][h] = 1 if free else 0
    elif free:
        out[0][h] = out[h][0] = 1
    return zz, out, n


def fuzz_set(count=256, seed=FUZZ_SEED, low=0.05, high=0.2):
    """`count` molecule-like graphs of 1..42 atoms (every third one `doubled`) with random coordinates, redrawn until -
    in fp64 - every candidate's |chi| and every |cos| lies outside [low, high]: fp32 and fp64 cannot disagree on a sign
    or on the threshold."""
    import numpy
    import stereo_ref
    rng = random.Random(seed)
    out = []
    for k in range(count):
        n = 1 + (k * 5) % 42
        z, adj, n = doubled(rng, n) if k % 3 == 2 and n >= 4 else molecule_like(rng, n)
        while True:
            xyz = [tuple(float(numpy.float32(rng.uniform(-4, 4))) for _ in range(3)) for _ in range(n)]   # fp32 values
            if all(not (low <= m <= high) for m in stereo_ref.margins(z, adj, n, xyz)):
                break
        out.append((z, adj, n, xyz))
    return out


def pad_batch(mols, width=None, junk=None):
    """(coords [B,W,3] fp32, z [B,W] int32, bonds [B,W,W] int8, n [B] int32) torch tensors; `junk`: a `random.Random`
    that fills the diagonal and everything at or beyond a molecule's atoms with values the kernel must ignore - NaN and
    infinities in the coordinates."""
    import canonical_cases
    import torch
    z, bonds, n = canonical_cases.pad_batch([m[:3] for m in mols], width, junk)
    W = int(bonds.shape[1])
    x = torch.zeros(len(mols), W, 3)
    if junk is not None:
        x[:] = torch.tensor([float("nan"), float("inf"), -1e30])
    for b, m in enumerate(mols):
        if m[2]:
            x[b, : m[2]] = torch.tensor(m[3], dtype=torch.float64).to(torch.float32)
    return x, z, bonds, n
