"""The named molecules of the ring and scaffold tests ("Rings and scaffolds") with their expected
values WRITTEN OUT BY HAND - the smallest shapes at which each stage can go wrong -, the seeded fuzz and the identity
examples.  A molecule is (z, adj, n) as in `canonical_ref`; `canonical_cases.pad_batch` builds the padded batches.

An expectation names, by hand: the ring systems as (atoms, label, ring size of those atoms) - several entries may share a
label where a system's atoms have different sizes -, the linker and exo atoms, n_rings, the ring bonds, min / max ring size.
`expected(name)` only spreads that over the per-atom lists the kernel writes; it computes nothing from the graph."""
import random

import canonical_cases as C
import canonical_ref as R


def _ring(n, code=1, at=0):
    return [(at + i, at + (i + 1) % n, code) for i in range(n)]


def _chain(n, at=0):
    return [(at + i, at + i + 1, 1) for i in range(n - 1)]


def _r(lo, hi):
    return tuple(range(lo, hi + 1))


_TWO_PHENYLS = _ring(6, 4) + _ring(6, 4, 6)
_NAPHTHALENE = _ring(6, 4) + [(5, 6, 4), (6, 7, 4), (7, 8, 4), (8, 9, 4), (9, 4, 4)]

# name -> (molecule, dict(systems=[(atoms, label, size)], linker, exo, n_rings, ring_bonds, min_size, max_size))
NAMED = {
    "butane": (R.mol([6] * 4, _chain(4)),
               dict(systems=[], linker=(), exo=(), n_rings=0, ring_bonds=0, min_size=0, max_size=0)),
    "benzene": (R.mol([6] * 6, _ring(6, 4)),
                dict(systems=[(_r(0, 5), 0, 6)], linker=(), exo=(), n_rings=1, ring_bonds=6, min_size=6, max_size=6)),
    # the methyl, atom 6, is pruned; a single bond makes no exo atom
    "toluene": (R.mol([6] * 7, _ring(6, 4) + [(0, 6, 1)]),
                dict(systems=[(_r(0, 5), 0, 6)], linker=(), exo=(), n_rings=1, ring_bonds=6, min_size=6, max_size=6)),
    # the bond 0-6 joins two ring atoms and is no ring bond: two systems, no linker atom
    "biphenyl": (R.mol([6] * 12, _TWO_PHENYLS + [(0, 6, 1)]),
                 dict(systems=[(_r(0, 5), 0, 6), (_r(6, 11), 6, 6)], linker=(), exo=(), n_rings=2, ring_bonds=12,
                      min_size=6, max_size=6)),
    "diphenylmethane": (R.mol([6] * 13, _TWO_PHENYLS + [(0, 12, 1), (6, 12, 1)]),
                        dict(systems=[(_r(0, 5), 0, 6), (_r(6, 11), 6, 6)], linker=(12,), exo=(), n_rings=2,
                             ring_bonds=12, min_size=6, max_size=6)),
    # the two methyls 13, 14 on the linker atom are pruned
    "2,2-diphenylpropane": (R.mol([6] * 15, _TWO_PHENYLS + [(0, 12, 1), (6, 12, 1), (12, 13, 1), (12, 14, 1)]),
                            dict(systems=[(_r(0, 5), 0, 6), (_r(6, 11), 6, 6)], linker=(12,), exo=(), n_rings=2,
                                 ring_bonds=12, min_size=6, max_size=6)),
    # the carbonyl O, atom 13, is doubly bonded to the linker atom
    "benzophenone": (R.mol([6] * 13 + [8], _TWO_PHENYLS + [(0, 12, 1), (6, 12, 1), (12, 13, 2)]),
                     dict(systems=[(_r(0, 5), 0, 6), (_r(6, 11), 6, 6)], linker=(12,), exo=(13,), n_rings=2,
                          ring_bonds=12, min_size=6, max_size=6)),
    "cyclohexanone": (R.mol([6] * 6 + [8], _ring(6) + [(0, 6, 2)]),
                      dict(systems=[(_r(0, 5), 0, 6)], linker=(), exo=(6,), n_rings=1, ring_bonds=6, min_size=6,
                           max_size=6)),
    # atom 0 is the spiro atom: the five-ring 0 1 2 3 4, the six-ring 0 5 6 7 8 9; ONE system
    "spiro[4.5]decane": (R.mol([6] * 10, _ring(5) + [(0, 5, 1), (5, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 0, 1)]),
                         dict(systems=[(_r(0, 4), 0, 5), (_r(5, 9), 0, 6)], linker=(), exo=(), n_rings=2, ring_bonds=11,
                              min_size=5, max_size=6)),
    "naphthalene": (R.mol([6] * 10, _NAPHTHALENE),
                    dict(systems=[(_r(0, 9), 0, 6)], linker=(), exo=(), n_rings=2, ring_bonds=11, min_size=6,
                         max_size=6)),
    # bridgeheads 0 and 3; bridges 0-1-2-3, 0-4-5-3 and 0-6-3: every bond lies on a five-ring
    "norbornane": (R.mol([6] * 7, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 4, 1), (4, 5, 1), (5, 3, 1), (0, 6, 1), (6, 3, 1)]),
                   dict(systems=[(_r(0, 6), 0, 5)], linker=(), exo=(), n_rings=2, ring_bonds=8, min_size=5, max_size=5)),
    # bridgeheads 0 and 1; three two-atom bridges
    "bicyclo[2.2.2]octane": (R.mol([6] * 8, [(0, 2, 1), (2, 3, 1), (3, 1, 1), (0, 4, 1), (4, 5, 1), (5, 1, 1),
                                             (0, 6, 1), (6, 7, 1), (7, 1, 1)]),
                             dict(systems=[(_r(0, 7), 0, 6)], linker=(), exo=(), n_rings=2, ring_bonds=9, min_size=6,
                                  max_size=6)),
    "cubane": (C.CUBE, dict(systems=[(_r(0, 7), 0, 4)], linker=(), exo=(), n_rings=5, ring_bonds=12, min_size=4,
                            max_size=4)),
    # the 8-ring with its four diagonals: ring bond i, i+1 closes over i+4, i+5; a diagonal likewise: all 4
    "Wagner graph": (C.WAGNER, dict(systems=[(_r(0, 7), 0, 4)], linker=(), exo=(), n_rings=5, ring_bonds=12, min_size=4,
                                    max_size=4)),
    "14-ring": (R.mol([6] * 14, _ring(14)),
                dict(systems=[(_r(0, 13), 0, 14)], linker=(), exo=(), n_rings=1, ring_bonds=14, min_size=14, max_size=14)),
    # phenyl 0..5, chain 6..15 (6 on atom 0), cyclopropane 16 17 18 (15 on 16)
    "phenyl-C10-cyclopropane": (R.mol([6] * 19, _ring(6, 4) + [(0, 6, 1)] + _chain(10, 6) + [(15, 16, 1)] + _ring(3, 1, 16)),
                                dict(systems=[(_r(0, 5), 0, 6), (_r(16, 18), 16, 3)], linker=_r(6, 15), exo=(),
                                     n_rings=2, ring_bonds=9, min_size=3, max_size=6)),
    "benzene . cyclopropane . C": (R.mol([6] * 10, _ring(6, 4) + _ring(3, 1, 6)),
                                   dict(systems=[(_r(0, 5), 0, 6), (_r(6, 8), 6, 3)], linker=(), exo=(), n_rings=2,
                                        ring_bonds=9, min_size=3, max_size=6)),
    "64-ring": (R.mol([6] * 64, _ring(64)),                                    # bit 63
                dict(systems=[(_r(0, 63), 0, 64)], linker=(), exo=(), n_rings=1, ring_bonds=64, min_size=64, max_size=64)),
    "64-chain": (R.mol([6] * 64, _chain(64)),                                  # 32 pruning rounds, nothing left
                 dict(systems=[], linker=(), exo=(), n_rings=0, ring_bonds=0, min_size=0, max_size=0)),
    # chain 0..60, triangle 61 62 63 (60 on 61): 61 pruning rounds from one side
    "61-chain-triangle": (R.mol([6] * 64, _chain(61) + [(60, 61, 1)] + _ring(3, 1, 61)),
                          dict(systems=[(_r(61, 63), 61, 3)], linker=(), exo=(), n_rings=1, ring_bonds=3, min_size=3,
                               max_size=3)),
    "no atoms": (R.mol([], []), dict(systems=[], linker=(), exo=(), n_rings=0, ring_bonds=0, min_size=0, max_size=0)),
    "one atom": (R.mol([8], []), dict(systems=[], linker=(), exo=(), n_rings=0, ring_bonds=0, min_size=0, max_size=0)),
}


def _mask(atoms):
    return sum(1 << a for a in atoms)


def expected(name):
    """The hand-written expectation of a named case in `scaffold_ref.perceive`'s layout.  `ring_nb`: two bonded atoms of
    one system are joined by a ring bond (were the bond a bridge, its ends would lie in different systems)."""
    (z, adj, n), e = NAMED[name]
    size, system = [0] * n, [-1] * n
    for atoms, label, s in e["systems"]:
        for a in atoms:
            size[a], system[a] = s, label
    ring = [a for a in range(n) if system[a] >= 0]
    ring_nb = [_mask(j for j in range(n) if adj[a][j] and system[a] >= 0 and system[a] == system[j]) for a in range(n)]
    n_systems = len({label for _, label, _ in e["systems"]})
    return dict(ring_nb=ring_nb, ring_size=size, ring_system=system,
                masks=[_mask(ring), _mask(e["linker"]), _mask(e["exo"]), _mask(list(ring) + list(e["linker"]) + list(e["exo"]))],
                counts=[e["n_rings"], n_systems, e["min_size"], e["max_size"], len(ring), len(e["linker"]), len(e["exo"]),
                        e["ring_bonds"]])


def molecules():
    return {name: mol for name, (mol, _) in NAMED.items()}


# which named case must see each planted mistake of `scaffold_ref.MUTATIONS`
CATCHES = {"flood_keeps_bond": "toluene", "prune_one_round": "61-chain-triangle", "exo_code_1": "toluene",
           "split_spiro": "spiro[4.5]decane"}

FUZZ_SEED = 20261020


def _joined(rng, mol):
    """`mol` with its fragments strung together by single bonds between atoms of degree < 4: chains between rings."""
    z, adj, n = mol
    label = list(range(n))
    for _ in range(n):
        for a in range(n):
            for j in range(n):
                if adj[a][j]:
                    label[a] = label[j] = min(label[a], label[j])
    last = None
    for head in sorted(set(label)):
        free = [a for a in range(n) if label[a] == head and sum(1 for c in adj[a] if c) < 4]
        if not free:
            continue
        a = rng.choice(free)
        if last is not None and sum(1 for c in adj[last] if c) < 4:
            adj[a][last] = adj[last][a] = 1
        last = rng.choice(free)
    return z, adj, n


def fuzz_set(count=320, seed=FUZZ_SEED):
    """Seeded random graphs of 1..64 atoms, every degree at most 4 (`canonical_cases.random_graph`): each size five times;
    every other one has its fragments joined, which is where linker atoms come from."""
    rng = random.Random(seed)
    mols = [C.random_graph(rng, 1 + k % 64) for k in range(count)]
    return [_joined(rng, m) if (k // 64) % 2 else m for k, m in enumerate(mols)]


# the identity examples: (z, adj, n)
ETHYLBENZENE = R.mol([6] * 8, _ring(6, 4) + [(0, 6, 1), (6, 7, 1)])
PYRIDINE = R.mol([7] + [6] * 5, _ring(6, 4))
CYCLOHEXANE = R.mol([6] * 6, _ring(6))
