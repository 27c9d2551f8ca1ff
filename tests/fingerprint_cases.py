"""Molecular graphs shared by the fingerprint tests: the pinned molecules of DESIGN.md section 6 ("Chemical
fingerprints") and seeded random graphs.  A molecule is (z, adj, n) as in `fingerprint_ref`."""
import random

import fingerprint_ref as R


def _ring(n, code):
    return [(i, (i + 1) % n, code) for i in range(n)]


def _chain(n):
    return [(i, i + 1, 1) for i in range(n - 1)]


# name -> (molecule, set bits, key): the pins of the definition
PINNED = {
    "ethanol": (R.mol([6, 6, 8], [(0, 1, 1), (1, 2, 1)]), [161, 171, 250, 735, 1017, 1212, 1503, 1740, 1900],
                0x2c3bb7c6ee92483a),
    "dimethyl ether": (R.mol([6, 8, 6], [(0, 1, 1), (1, 2, 1)]), [136, 140, 1326, 1503, 1813, 2035], 0x225947b9e5e093c9),
    "benzene": (R.mol([6] * 6, _ring(6, 4)), [673, 684, 1291], 0xfe498f7719e699cc),
    "pyridine": (R.mol([7] + [6] * 5, _ring(6, 4)), [634, 673, 684, 1129, 1164, 1291, 1761, 1872, 1874],
                 0xd232d5191a40baba),
    "cyclohexane": (R.mol([6] * 6, _ring(6, 1)), [153, 1428, 1823], 0x2250b17d5ebcb05e),
    "n-hexane": (R.mol([6] * 6, _chain(6)), [928, 947, 1017, 1112, 1503, 1717, 1740, 1778], 0x272a2e0b0df30834),
    "methane": (R.mol([6], []), [27, 294, 1144], 0xf5228d710df3c2ee),
    "ethene": (R.mol([6, 6], [(0, 1, 2)]), [563, 1221, 1508], 0x4b01b2ef8c38e8b4),
    "no atoms": (R.mol([], []), [], 0x2056f3754d76c94e),
    # two six-rings sharing the bond 4-5: 0-1-2-3-4-5 and 4-5-6-7-8-9
    "decalin": (R.mol([6] * 10, _ring(6, 1) + [(5, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 4, 1)]),
                [153, 279, 450, 699, 711, 778, 798, 1428], 0x1598aacb0beba1fa),
    # two five-rings 0-1-2-3-4 and 5-6-7-8-9 joined by the bond 0-5
    "bicyclopentyl": (R.mol([6] * 10, [(i, (i + 1) % 5, 1) for i in range(5)]
                            + [(5 + i, 5 + (i + 1) % 5, 1) for i in range(5)] + [(0, 5, 1)]),
                      [585, 593, 635, 693, 865, 1046, 1616, 1884], 0x3e5a348fb0cfe580),
}


def molecule_like(rng, n):
    """A random tree with degree <= 3 plus 0-3 ring closures; elements from C N O F S, codes from 1 2 4."""
    z = [rng.choice([6, 6, 6, 7, 8, 9, 16]) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    deg = [0] * n
    for a in range(1, n):
        open_ = [j for j in range(a) if deg[j] < 3]
        j = rng.choice(open_)
        adj[a][j] = adj[j][a] = rng.choice([1, 1, 2, 4])
        deg[a] += 1
        deg[j] += 1
    for _ in range(rng.randint(0, 3)):
        if n < 3:
            break
        a, j = rng.sample(range(n), 2)
        if adj[a][j] == 0:
            adj[a][j] = adj[j][a] = rng.choice([1, 1, 2, 4])
    return z, adj, n


def molecule_like_set(count=520, seed=20261016):
    """`count` molecule-like graphs of 1..42 atoms, every size present."""
    rng = random.Random(seed)
    return [molecule_like(rng, 1 + k % 42) for k in range(count)]


def junk_graph(rng, n):
    """A dense junk graph: every code uniform in 0..4 (about 50 neighbours per atom at n = 64)."""
    z = [rng.randint(1, 35) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    for a in range(n):
        for j in range(a):
            adj[a][j] = adj[j][a] = rng.randint(0, 4)
    return z, adj, n


def random_permutation(rng, mol):
    p = list(range(mol[2]))
    rng.shuffle(p)
    return R.permute(*mol, p)
