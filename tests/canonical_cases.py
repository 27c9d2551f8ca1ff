"""The named graphs of the canonical-labelling tests ("Canonical graphs and SMILES"), their expected
leaf counts and canonical strings, seeded random graphs and the padded-batch builder.  A molecule is (z, adj, n) as in
`canonical_ref`.

Leaf counts, by hand: without twins the search visits one leaf per automorphism when the refinement is as fine as the
orbits (benzene 12 = D6, naphthalene 4, decalin 4, cube 48, Wagner graph 16 = D8, toluene 2: the two ring directions).
Twins - atoms of one element with the same bonds to everyone else - collapse to one branch each: neopentane's four
methyls, isolated atoms and the atoms of K5 are one twin class (1 leaf); the two ends of an ethane or of a propane are
twins, so k disjoint ones give k! leaves (4 ethanes 24, 5 / 6 / 7 propanes 120 / 720 / 5 040 > the budget);
hexamethylbenzene's methyls are no twins of each other (different ring atoms) and keep the ring's 12; biphenyl 8 = the
swap of the rings times each ring's flip; bicyclopentyl likewise 8; tri-tert-butylmethane's methyls are twins within a
tert-butyl, which leaves the 3! orders of the three tert-butyls."""
import random

import canonical_ref as R


def _ring(n, code, at=0):
    return [(at + i, at + (i + 1) % n, code) for i in range(n)]


def _chain(n, at=0):
    return [(at + i, at + i + 1, 1) for i in range(n - 1)]


def _propanes(k):
    return R.mol([6] * (3 * k), [b for i in range(k) for b in _chain(3, 3 * i)])


def _tri_tert_butylmethane():
    bonds = []
    for t in range(3):
        q = 1 + 4 * t
        bonds += [(0, q, 1)] + [(q, q + 1 + m, 1) for m in range(3)]
    return R.mol([6] * 13, bonds)


CUBE = R.mol([6] * 8, [(a, a ^ bit, 1) for a in range(8) for bit in (1, 2, 4) if a < a ^ bit])
WAGNER = R.mol([6] * 8, _ring(8, 1) + [(i, i + 4, 1) for i in range(4)])

# name -> (molecule, leaves, canonical string or None = not pinned by the definition's table)
NAMED = {
    "benzene": (R.mol([6] * 6, _ring(6, 4)), 12, "c1ccccc1"),
    "toluene": (R.mol([6] * 7, _ring(6, 4) + [(0, 6, 1)]), 2, None),
    "biphenyl": (R.mol([6] * 12, _ring(6, 4) + _ring(6, 4, 6) + [(0, 6, 1)]), 8, "c1ccc(cc1)-c1ccccc1"),
    "naphthalene": (R.mol([6] * 10, _ring(6, 4) + [(5, 6, 4), (6, 7, 4), (7, 8, 4), (8, 9, 4), (9, 4, 4)]), 4,
                    "c1ccc2ccccc2c1"),
    "neopentane": (R.mol([6] * 5, [(0, k, 1) for k in range(1, 5)]), 1, None),
    "16 isolated C": (R.mol([6] * 16, []), 1, None),
    "four disjoint ethanes": (R.mol([6] * 8, [(2 * i, 2 * i + 1, 1) for i in range(4)]), 24, None),
    "hexamethylbenzene": (R.mol([6] * 12, _ring(6, 4) + [(i, 6 + i, 1) for i in range(6)]), 12, None),
    "tri-tert-butylmethane skeleton": (_tri_tert_butylmethane(), 6, None),
    "decalin": (R.mol([6] * 10, _ring(6, 1) + [(5, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 4, 1)]), 4, None),
    "bicyclopentyl": (R.mol([6] * 10, _ring(5, 1) + _ring(5, 1, 5) + [(0, 5, 1)]), 8, None),
    "cube": (CUBE, 48, "C12C3C4C1C1C2C3C41"),
    "Wagner graph": (WAGNER, 16, None),
    "K5": (R.mol([6] * 5, [(a, b, 1) for a in range(5) for b in range(a)]), 1, "C123C45C11C24C351"),
    "5 disjoint propanes": (_propanes(5), 120, None),
    "6 disjoint propanes": (_propanes(6), 720, None),
}
OVER_BUDGET = _propanes(7)                      # 5 040 leaves: more than the budget

# beyond the table: the sizes at which the kernel takes its edges
EDGES = {
    "no atoms": R.mol([], []),
    "one atom": R.mol([8], []),
    "two atoms": R.mol([6, 7], [(0, 1, 3)]),
    "64-atom chain": R.mol([6] * 64, _chain(64)),
    "64 isolated atoms": R.mol([6] * 64, []),
}

# the mutation pair: every atom of 1,3,5-cyclohexatriene (alternating 2 / 1) has the initial colour (C, 2, 6), so only the
# bond code in the refinement key tells an individualised atom's two neighbours apart: 6 leaves (its symmetry D3) with
# it, the 12 of benzene's ring without it
CYCLOHEXATRIENE = R.mol([6] * 6, [(i, (i + 1) % 6, 2 - i % 2) for i in range(6)])
BENZENE = R.mol([6] * 6, _ring(6, 4))

PYRROLE = R.mol([7, 6, 6, 6, 6], _ring(5, 4))
IMIDAZOLE_4_METHYL = R.mol([7, 6, 7, 6, 6, 6], _ring(5, 4) + [(3, 5, 1)])     # N0 C1 N2 C3(-C5) C4: the two N differ
METHYLSILANE = R.mol([6, 14], [(0, 1, 1)])


def renumbered(rng, mol):
    p = list(range(mol[2]))
    rng.shuffle(p)
    return R.permute(*mol, p)


def nested_rings(m):
    """A chain of m atoms with atom i bonded to atom m - 1 - i: every such ring is open across the middle of the chain."""
    return R.mol([6] * m, _chain(m) + [(i, m - 1 - i, 1) for i in range(m // 2 - 1)])


def random_graph(rng, n, max_degree=4):
    """A random graph of n atoms (C N O), codes 1 / 2 / 4, every degree at most `max_degree`; sparse or symmetric enough
    that a good share of them need a search."""
    adj = [[0] * n for _ in range(n)]
    deg = [0] * n
    if rng.random() < 0.4:                      # all carbon, built from rings, chains and stars: symmetric on purpose
        z, at = [6] * n, 0
        while at < n:
            k = min(rng.randint(1, 6), n - at)
            kind = rng.choice(["ring", "chain", "star"])
            if kind == "ring" and k >= 3:
                pairs = [(at + i, at + (i + 1) % k) for i in range(k)]
            elif kind == "star" and k <= 5:
                pairs = [(at, at + i) for i in range(1, k)]
            else:
                pairs = [(at + i, at + i + 1) for i in range(k - 1)]
            code = rng.choice([1, 1, 2, 4]) if kind != "star" else 1
            for a, b in pairs:
                adj[a][b] = adj[b][a] = code
                deg[a] += 1
                deg[b] += 1
            at += k
        extra = rng.randint(0, 2)
    else:
        z = [rng.choice([6, 6, 6, 6, 7, 8]) for _ in range(n)]
        extra = rng.randint(0, 2 * n)
    for _ in range(extra):
        a, b = rng.randrange(n), rng.randrange(n)
        if a != b and adj[a][b] == 0 and deg[a] < max_degree and deg[b] < max_degree:
            adj[a][b] = adj[b][a] = rng.choice([1, 1, 1, 2, 4])
            deg[a] += 1
            deg[b] += 1
    return z, adj, n


FUZZ_SEED = 20261019


def fuzz_set(count=256, seed=FUZZ_SEED):
    rng = random.Random(seed)
    return [random_graph(rng, 1 + k % 24) for k in range(count)]


def over_degree(rng, n=12):
    """A dense random graph in which atom 0 has 9 neighbours."""
    z, adj, n = random_graph(rng, n)
    for j in range(1, 10):
        adj[0][j] = adj[j][0] = adj[0][j] or 1
    return z, adj, n


def pad_batch(mols, width=None, junk=None):
    """(z [B,W] int32, bonds [B,W,W] int8, n [B] int32) as nested lists -> torch tensors; `junk`: a `random.Random` that
    fills the diagonal and everything at or beyond a molecule's atoms with values the kernel must ignore."""
    import torch
    W = width if width is not None else max([m[2] for m in mols] + [1])
    z = torch.zeros(len(mols), W, dtype=torch.int32)
    bonds = torch.zeros(len(mols), W, W, dtype=torch.int8)
    if junk is not None:
        z = torch.tensor([[junk.randint(-3, 90) for _ in range(W)] for _ in mols], dtype=torch.int32).reshape(len(mols), W)
        bonds = torch.tensor([[[junk.randint(-128, 127) for _ in range(W)] for _ in range(W)] for _ in mols],
                             dtype=torch.int8).reshape(len(mols), W, W)
    for b, (zs, adj, n) in enumerate(mols):
        if n:
            z[b, :n] = torch.tensor(zs, dtype=torch.int32)
            block = torch.tensor(adj, dtype=torch.int8)
            if junk is not None:
                block = block + torch.diag(bonds[b, :n, :n].diagonal())
            bonds[b, :n, :n] = block
    return z, bonds, torch.tensor([m[2] for m in mols], dtype=torch.int32)
