"""Molecules and score cases shared by the pharmacophore tests: the pinned set of DESIGN.md section 6 ("Pharmacophore
overlap") with its types, rings and nH written out by hand, seeded molecule-like graphs with aromatic rings, and the
posed candidates the score is checked on.  A molecule is (z, adj, n) as in `pharmacophore_ref`."""
import functools
import math
import random

import numpy as np

import pharmacophore_ref as R
from pharmacophore_ref import A, D, H, N, P


def _ring(n, code, first=0):
    return [(first + i, first + (i + 1) % n, code) for i in range(n)]


_INDOLE = [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 8, 4), (8, 0, 4), (3, 4, 4), (4, 5, 4), (5, 6, 4), (6, 7, 4), (7, 8, 4)]
_NAPHTHALENE = _ring(6, 4) + [(5, 6, 4), (6, 7, 4), (7, 8, 4), (8, 9, 4), (9, 4, 4)]

# name -> (molecule, types, ring masks, nH), all by hand from the definition
PINNED = {
    "ethanol": (R.mol([6, 6, 8], [(0, 1, 1), (1, 2, 1)]), [H, 0, D | A], [], [3, 2, 1]),
    "dimethyl ether": (R.mol([6, 8, 6], [(0, 1, 1), (1, 2, 1)]), [0, A, 0], [], [3, 0, 3]),
    "acetic acid": (R.mol([6, 6, 8, 8], [(0, 1, 1), (1, 2, 2), (1, 3, 1)]), [H, N, A, D | A], [], [3, 0, 0, 1]),
    "methanesulfonic acid": (R.mol([6, 16, 8, 8, 8], [(0, 1, 1), (1, 2, 2), (1, 3, 2), (1, 4, 1)]),
                             [0, N, A, A, D | A], [], [3, 0, 0, 0, 1]),
    "acetamide": (R.mol([6, 6, 8, 7], [(0, 1, 1), (1, 2, 2), (1, 3, 1)]), [H, 0, A, D], [], [3, 0, 0, 2]),
    "N,N-dimethylacetamide": (R.mol([6, 6, 8, 7, 6, 6], [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1), (3, 5, 1)]),
                              [H, 0, A, 0, 0, 0], [], [3, 0, 0, 0, 3, 3]),
    "trimethylamine": (R.mol([7, 6, 6, 6], [(0, 1, 1), (0, 2, 1), (0, 3, 1)]), [P, 0, 0, 0], [], [0, 3, 3, 3]),
    "aniline": (R.mol([6] * 6 + [7], _ring(6, 4) + [(0, 6, 1)]), [0] * 6 + [D], [63], [0, 1, 1, 1, 1, 1, 2]),
    "acetamidine": (R.mol([6, 6, 7, 7], [(0, 1, 1), (1, 2, 2), (1, 3, 1)]), [H, 0, D | A, D | P], [], [3, 0, 1, 2]),
    "acetonitrile": (R.mol([6, 6, 7], [(0, 1, 1), (1, 2, 3)]), [H, 0, A], [], [3, 0, 0]),
    "benzene": (R.mol([6] * 6, _ring(6, 4)), [0] * 6, [63], [1] * 6),
    "chlorobenzene": (R.mol([6] * 6 + [17], _ring(6, 4) + [(0, 6, 1)]), [0] * 6 + [H], [63], [0, 1, 1, 1, 1, 1, 0]),
    "pyridine": (R.mol([7] + [6] * 5, _ring(6, 4)), [A, 0, 0, 0, 0, 0], [63], [0, 1, 1, 1, 1, 1]),
    "pyrrole": (R.mol([7] + [6] * 4, _ring(5, 4)), [D, 0, 0, 0, 0], [31], [0, 1, 1, 1, 1]),
    "N-methylpyrrole": (R.mol([7] + [6] * 5, _ring(5, 4) + [(0, 5, 1)]), [0] * 6, [31], [0, 1, 1, 1, 1, 3]),
    "imidazole": (R.mol([7, 6, 7, 6, 6], _ring(5, 4)), [D | A, 0, D | A, 0, 0], [31], [0, 1, 0, 1, 1]),
    "oxazole": (R.mol([8, 6, 7, 6, 6], _ring(5, 4)), [0, 0, A, 0, 0], [31], [0, 1, 0, 1, 1]),
    # N0 C1 C2 C3 (3a) C4 C5 C6 C7 C8 (7a): the five-ring 0 1 2 3 8 and the six-ring 3 4 5 6 7 8 share the bond 3-8
    "indole": (R.mol([7] + [6] * 8, _INDOLE), [D] + [0] * 8, [271, 504], [0, 1, 1, 0, 1, 1, 1, 1, 0]),
    # two six-rings 0-1-2-3-4-5 and 4-5-6-7-8-9 sharing the bond 4-5
    "naphthalene": (R.mol([6] * 10, _NAPHTHALENE), [0] * 10, [63, 1008], [1, 1, 1, 1, 0, 0, 1, 1, 1, 1]),
    "cyclohexane": (R.mol([6] * 6, _ring(6, 1)), [H] * 6, [], [2] * 6),
    "methane": (R.mol([6], []), [H], [], [4]),
    "no atoms": (R.mol([], []), [], [], []),
}


def molecule_like(rng, n):
    """The recipe of `fingerprint_cases.molecule_like` - a random tree with degree <= 3 plus 0-3 ring closures, elements
    from C N O F S, codes from 1 2 4 - grown from 0-3 aromatic rings (code 4, five or six atoms of C N O S, sometimes
    fused to the previous one) so that ring features occur."""
    z, bonds, deg = [], {}, []

    def atom(el):
        z.append(el)
        deg.append(0)
        return len(z) - 1

    def bond(i, j, c):
        bonds[(min(i, j), max(i, j))] = c
        deg[i] += 1
        deg[j] += 1

    last = None
    for _ in range(rng.randint(0, 3)):
        size = rng.choice([5, 6, 6])
        fused = last is not None and rng.random() < 0.5
        if len(z) + size - (2 if fused else 0) > n:
            break
        members = list(last[:2]) if fused else []
        while len(members) < size:
            members.append(atom(rng.choice([6, 6, 6, 6, 7, 7, 8, 16])))
        for k in range(size):
            i, j = members[k], members[(k + 1) % size]
            if (min(i, j), max(i, j)) not in bonds:
                bond(i, j, 4)
        last = members
    while len(z) < n:
        a = atom(rng.choice([6, 6, 6, 7, 8, 9, 16]))
        open_ = [j for j in range(a) if deg[j] < 3]
        if open_:
            bond(a, rng.choice(open_), rng.choice([1, 1, 2, 4]))
    for _ in range(rng.randint(0, 3)):
        if n < 3:
            break
        i, j = rng.sample(range(n), 2)
        if (min(i, j), max(i, j)) not in bonds:
            bond(i, j, rng.choice([1, 1, 2, 4]))
    return R.mol(z, [(i, j, c) for (i, j), c in bonds.items()])


@functools.lru_cache(maxsize=None)
def molecule_like_set(count=504, seed=20261018):
    """`count` molecule-like graphs of 1..42 atoms, every size present."""
    rng = random.Random(seed)
    return [molecule_like(rng, 1 + k % 42) for k in range(count)]


def big_molecules():
    """n = 63 and n = 64 (the last lane, the top mask bit): a molecule-like graph each, and each with a pyridine ring on
    its last six atoms."""
    rng = random.Random(6364)
    out = [molecule_like(rng, 63), molecule_like(rng, 64)]
    for n in (63, 64):
        z, adj, _ = molecule_like(rng, n - 6)
        z = z + [6] * 5 + [7]
        bonds = [(i, j, adj[i][j]) for i in range(n - 6) for j in range(i) if adj[i][j]]
        out.append(R.mol(z, bonds + _ring(6, 4, n - 6) + [(0, n - 6, 1)]))
    return out


def junk_graph(rng, n):
    """A dense junk graph, as `fingerprint_cases.junk_graph`: every code uniform in 0..4."""
    z = [rng.randint(1, 35) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    for a in range(n):
        for j in range(a):
            adj[a][j] = adj[j][a] = rng.randint(0, 4)
    return z, adj, n


def sparse_aromatic_junk(rng, n):
    """Junk the ring walk cannot skip: a random graph of code-4 bonds with at most three per atom, so every atom of
    degree 2 or 3 is ring-eligible and the paths branch as often as the definition lets them."""
    z = [rng.choice([6, 7, 8, 16]) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    deg = [0] * n
    for _ in range(4 * n):
        i, j = rng.sample(range(n), 2)
        if adj[i][j] == 0 and deg[i] < 3 and deg[j] < 3:
            adj[i][j] = adj[j][i] = 4
            deg[i] += 1
            deg[j] += 1
    return z, adj, n


def petersen_field():
    """Six Petersen graphs of aromatic bonds (60 atoms, every atom with three): 12 five-cycles and 10 six-cycles each,
    132 rings - more than the 32 that are kept."""
    bonds = []
    for g in range(6):
        o = 10 * g
        for k in range(5):
            bonds += [(o + k, o + (k + 1) % 5, 4), (o + k, o + 5 + k, 4), (o + 5 + k, o + 5 + (k + 2) % 5, 4)]
    return R.mol([6] * 60, bonds)


def k33():
    """K(3,3) of aromatic bonds: six closed paths of six atoms, all over the same six atoms - one ring."""
    return R.mol([6] * 6, [(i, j, 4) for i in range(3) for j in range(3, 6)])


def random_permutation(rng, mol):
    p = list(range(mol[2]))
    rng.shuffle(p)
    return p, R.permute(*mol, p)


# ---- score cases ---------------------------------------------------------------------------------------------------
CANDIDATE_SIZES = (1, 2, 27, 42, 64)
MARGIN = 1e-3                                   # every same-type reference-candidate distance is this far from 1.5 A


def _margin_ok(fr, fm):
    for t in range(6):
        a = np.array([p for k, p in fr if k == t], dtype=np.float64).reshape(-1, 1, 3)
        b = np.array([p for k, p in fm if k == t], dtype=np.float64).reshape(1, -1, 3)
        if a.size and b.size and (np.abs(np.sqrt(((a - b) ** 2).sum(-1)) - 1.5) < MARGIN).any():
            return False
    return True


def _rotation(rng):
    q = np.array([rng.gauss(0, 1) for _ in range(4)])
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# benzene 0-5; a carboxylic acid on 0 (C6, =O7, OH 8); CH2 10 - NH2 9 on 3; Cl 11 on 2; an ethyl (12, 13) on 4: ten features -
# R, N, A, D A, D P, H (Cl), H H (the ethyl)
REFERENCE_MOLECULE = R.mol([6] * 7 + [8, 8, 7, 6, 17, 6, 6],
                           _ring(6, 4) + [(0, 6, 1), (6, 7, 2), (6, 8, 1), (3, 10, 1), (10, 9, 1), (2, 11, 1), (4, 12, 1),
                                          (12, 13, 1)])


def _rich_molecule(n):
    """The first molecule-like graph of n atoms (seeds 100 + n, 1100 + n, ...) that has features to score: for the large
    sizes a ring and four different atom types."""
    if n == 1:
        return R.mol([8], [])                   # one atom that carries features: water's O
    for seed in range(100 + n, 100000, 1000):
        m = molecule_like(random.Random(seed), n)
        t, rings, _ = R.perceive(*m)
        kinds = {k for bits in t for k in range(5) if bits >> k & 1}
        if n < 27 and kinds or rings and len(kinds) >= 4:
            return m
    raise AssertionError(n)


@functools.lru_cache(maxsize=None)
def score_cases():
    """(references, cases): `references` name -> feature list [(type index, fp32 xyz)] of 1 feature, of a 14-atom molecule
    (about 10) and of the maximum 352; `cases` a list of dicts (ref, name, mol, coords fp32 [n,3]) - every candidate size
    at an identical, a shifted and a rotated pose against every reference, the 14-atom reference molecule on itself, and
    a candidate without features.  The generator redraws a pose until every same-type reference-candidate distance is at
    least `MARGIN` from 1.5 A, and asserts it: `matches` then does not hang on the last place of a distance."""
    rng = random.Random(1510)

    def cloud(n, sigma):
        return np.array([[rng.gauss(0, sigma) for _ in range(3)] for _ in range(n)], dtype=np.float32).reshape(n, 3)

    ref_mol = REFERENCE_MOLECULE
    ref_xyz = cloud(14, 1.8)
    t, rings, _ = R.perceive(*ref_mol)
    refs = {"one": [(0, np.array([0.3, -0.2, 0.1], dtype=np.float32))],
            "molecule": R.features(ref_xyz, t, rings),
            "max": [(rng.randrange(6), p) for p in cloud(R.MAX_FEATURES, 3.0)]}
    assert len(refs["molecule"]) >= 6 and len(refs["max"]) == R.MAX_FEATURES
    cases = [dict(ref="molecule", name="reference on itself", mol=ref_mol, coords=ref_xyz)]
    mols = {n: _rich_molecule(n) for n in CANDIDATE_SIZES}
    for rname, fr in refs.items():
        for n in CANDIDATE_SIZES:
            t, rings, _ = R.perceive(*mols[n])
            base = cloud(n, 2.0)
            for pose in ("identical", "shifted", "rotated"):
                for _ in range(200):
                    if pose == "identical":
                        xyz = base
                    elif pose == "shifted":
                        xyz = (base + np.array([rng.gauss(0, 0.8) for _ in range(3)], dtype=np.float32)).astype(np.float32)
                    else:
                        xyz = (base.astype(np.float64) @ _rotation(rng).T).astype(np.float32)
                    if _margin_ok(fr, R.features(xyz, t, rings)):
                        break
                    base = cloud(n, 2.0) if pose == "identical" else base
                cases.append(dict(ref=rname, name=f"{n} atoms, {pose}", mol=mols[n], coords=xyz))
    cases.append(dict(ref="molecule", name="no features", mol=R.mol([9, 9], [(0, 1, 1)]), coords=cloud(2, 1.0)))
    for c in cases:
        t, rings, _ = R.perceive(*c["mol"])
        assert _margin_ok(refs[c["ref"]], R.features(c["coords"], t, rings)), c["name"]
    return refs, cases
