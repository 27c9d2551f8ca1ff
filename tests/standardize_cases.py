"""Named molecular graphs shared by the standardisation tests, each with the answer derived BY HAND from the words of the
definition ("Standardised graphs"), and the padded batch the kernel is run on.

A case is a dict: mol (z, codes, n), xyz fp32 [n,3] (arbitrary: the coordinates play no part in the verdict; one case
carries a NaN), and the expected status, atom_map, n_fragments, doubles (pairs of NEW indices that get order 2; None
where the status is not 0).  Indices are those of the definition: the search takes the highest unmatched atom first and
tries its neighbours from the highest down."""
import functools

import numpy as np

import standardize_ref as SR


def mol(z, bonds):
    n = len(z)
    codes = [[0] * n for _ in range(n)]
    for i, j, c in bonds:
        assert i != j and codes[i][j] == 0
        codes[i][j] = codes[j][i] = c
    return list(z), codes, n


def ring(size, code=4, first=0):
    return [(first + i, first + (i + 1) % size, code) for i in range(size)]


def chain(atoms, code=1):
    return [(a, b, code) for a, b in zip(atoms, atoms[1:])]


def benzenoid(hexagons, order="yx"):
    """The carbon skeleton of fused hexagons, all bonds aromatic: `hexagons` are (q, r) axial coordinates of ring centres;
    the atoms are the distinct corners, numbered by ascending (y, x) (or (x, y)); a bond joins corners one bond length
    apart."""
    pts = {}
    for q, r in hexagons:
        cx, cy = 3 ** 0.5 * (q + r / 2.0), 1.5 * r
        for k in range(6):
            a = np.pi / 6 + k * np.pi / 3
            x, y = cx + np.cos(a), cy + np.sin(a)
            pts[(round(x, 3), round(y, 3))] = (x, y)
    keys = sorted(pts, key=(lambda p: (p[1], p[0])) if order == "yx" else (lambda p: (p[0], p[1])))
    xy = np.array([pts[k] for k in keys])
    bonds = [(i, j, 4) for i in range(len(keys)) for j in range(i) if abs(np.hypot(*(xy[i] - xy[j])) - 1.0) < 1e-3]
    return mol([6] * len(keys), bonds)


def triangle(k):
    """The triangular benzenoid with k hexagons on a side (k = 2: phenalenyl, 3: triangulene): one sublattice holds k - 1
    more atoms than the other, so no Kekule structure exists."""
    return [(q, r) for q in range(k) for r in range(k - q)]


def shuffled(m, seed):
    """The same graph with its atoms renumbered by a seeded permutation: the geometric numbering of `benzenoid` lets the
    highest-first search see a dead end at once, an arbitrary one does not."""
    z, codes, n = m
    perm = np.random.RandomState(seed).permutation(n).tolist()
    return mol([z[perm.index(a)] for a in range(n)],
               [(perm[i], perm[j], codes[i][j]) for i in range(n) for j in range(i) if codes[i][j]])


def _case(m, status=0, atom_map=None, n_fragments=1, doubles=None):
    z, codes, n = m
    return dict(mol=m, status=status, atom_map=list(range(n)) if atom_map is None else list(atom_map),
                n_fragments=n_fragments, doubles=None if status else sorted(doubles or []))


BICYCLE = ring(10) + [(4, 9, 4)]                    # naphthalene's skeleton: the perimeter 0..9 and the fusion bond 4-9
FIVE_SIX = chain(list(range(9)), 4) + [(8, 3, 4), (8, 0, 4)]     # indole's: N0 C1 C2 C3a C4 C5 C6 C7 C7a
INTERLEAVED = mol([8 if a == 63 else 6 for a in range(64)],
                  [(1 + 2 * i, 1 + 2 * ((i + 1) % 6), 4) for i in range(6)]
                  + chain(list(range(11, 64, 2))) + chain(list(range(0, 64, 2))))


def _named():
    c = {}
    # ---- valid, with the double bonds the highest-first search leaves
    c["benzene"] = _case(mol([6] * 6, ring(6)), doubles=[(4, 5), (2, 3), (0, 1)])
    c["pyridine"] = _case(mol([7] + [6] * 5, ring(6)), doubles=[(4, 5), (2, 3), (0, 1)])
    c["pyrrole"] = _case(mol([7] + [6] * 4, ring(5)), doubles=[(3, 4), (1, 2)])                 # N0 stays unmatched
    c["furan"] = _case(mol([8] + [6] * 4, ring(5)), doubles=[(3, 4), (1, 2)])                   # O0 is not eligible
    c["imidazole"] = _case(mol([7, 6, 7, 6, 6], ring(5)), doubles=[(3, 4), (1, 2)])             # N0 stays unmatched
    c["pyrazine"] = _case(mol([7, 6, 6, 7, 6, 6], ring(6)), doubles=[(4, 5), (2, 3), (0, 1)])
    # N0, C1 (=O6), C2..C5: C1 spends its fourth valence on the oxygen and is not eligible
    c["2-pyridone"] = _case(mol([7, 6, 6, 6, 6, 6, 8], ring(6) + [(1, 6, 2)]), doubles=[(4, 5), (2, 3)])
    c["naphthalene"] = _case(mol([6] * 10, BICYCLE), doubles=[(8, 9), (6, 7), (4, 5), (2, 3), (0, 1)])
    c["indole"] = _case(mol([7] + [6] * 8, FIVE_SIX), doubles=[(7, 8), (5, 6), (3, 4), (1, 2)])
    c["benzimidazole"] = _case(mol([7, 6, 7] + [6] * 6, FIVE_SIX), doubles=[(7, 8), (5, 6), (3, 4), (1, 2)])
    # azulene: the perimeter 0..9 and the bond 3-9: a 5-ring (0 1 2 3 9) and a 7-ring, still a perfect matching
    c["azulene"] = _case(mol([6] * 10, ring(10) + [(3, 9, 4)]), doubles=[(8, 9), (6, 7), (4, 5), (2, 3), (0, 1)])
    # ---- no Kekule form
    c["cyclopentadienyl"] = _case(mol([6] * 5, ring(5)), status=SR.NOT_KEKULIZABLE)
    c["N-methylpyridine"] = _case(mol([7] + [6] * 6, ring(6) + [(0, 6, 1)]), status=SR.NOT_KEKULIZABLE)
    # ---- an aromatic bond outside every ring
    c["aromatic biphenyl"] = _case(mol([6] * 12, ring(6) + ring(6, first=6) + [(0, 6, 4)]), status=SR.AROMATIC_BRIDGE)
    # ---- fragments
    c["benzene and water"] = _case(mol([6] * 6 + [8], ring(6)), atom_map=range(6), n_fragments=2,
                                   doubles=[(4, 5), (2, 3), (0, 1)])
    c["propane and ethanol"] = _case(mol([6, 6, 6, 6, 6, 8], chain([0, 1, 2]) + chain([3, 4, 5])), atom_map=[3, 4, 5],
                                     n_fragments=2)
    c["two ethanes"] = _case(mol([6] * 4, [(0, 1, 1), (2, 3, 1)]), atom_map=[0, 1], n_fragments=2)
    # F7 with two bonds, in the fragment that goes
    c["benzene and a bad fragment"] = _case(mol([6] * 6 + [6, 9, 6], ring(6) + chain([6, 7, 8])), atom_map=range(6),
                                            n_fragments=2, doubles=[(4, 5), (2, 3), (0, 1)])
    c["five-bonded carbon"] = _case(mol([6] * 6, [(0, k, 1) for k in range(1, 6)]), status=SR.OVER_VALENCE)
    c["no atoms"] = _case(mol([], []), status=SR.EMPTY, n_fragments=0)
    c["one atom"] = _case(mol([6], []))
    # 64 atoms, two fragments interleaved by index: the odd atoms (an aromatic ring 1 3 5 7 9 11 with a tail ending in O63)
    # outweigh the even ones (a chain of 32 carbons)
    c["interleaved 64"] = _case(INTERLEAVED, atom_map=range(1, 64, 2), n_fragments=2, doubles=[(4, 5), (2, 3), (0, 1)])
    # ---- the search budget (chosen on the CPU with the restatement: see `test_standardize_host.py`)
    c["decacene"] = dict(_case(benzenoid([(q, 0) for q in range(10)])), doubles=None)           # 42 atoms, valid, cheap
    c["triangular 46"] = _case(benzenoid(triangle(5)), status=SR.NOT_KEKULIZABLE)                # 383 steps as numbered ...
    c["triangular 46 shuffled"] = _case(shuffled(benzenoid(triangle(5)), 0), status=SR.SEARCH_BUDGET)      # ... > 16384 renumbered
    return c


@functools.lru_cache(maxsize=None)
def cases():
    named = _named()
    rng = np.random.RandomState(11)
    for name, c in named.items():
        c["xyz"] = (rng.standard_normal((c["mol"][2], 3)) * 3.0).astype(np.float32)
    named["pyrrole"]["xyz"][2, 1] = np.nan              # a non-finite coordinate is copied like any other
    return named


@functools.lru_cache(maxsize=None)
def references():
    """name -> `standardize_ref.standardize` of the case: computed once, shared, never written to."""
    return {name: SR.standardize(*c["mol"], coords=c["xyz"]) for name, c in cases().items()}


def eligible_count(m):
    z, codes, n = m
    return len(SR.eligible_graph(z, SR.clean(codes, n), range(n))[0])


def pad_batch(items, W, N, garbage_seed=None):
    """(coords [B,N,3] fp32, z [B,W] int32, bonds [B,W,W] int8, n [B] int32) as numpy arrays from cases; with
    `garbage_seed` everything at or beyond a row's atom count - coordinates, elements, codes - and the diagonal holds
    junk (symmetric junk: the matrix stays symmetric)."""
    B = len(items)
    rng = np.random.RandomState(garbage_seed or 0)
    if garbage_seed is None:
        xyz, z, bonds = np.zeros((B, N, 3), np.float32), np.zeros((B, W), np.int32), np.zeros((B, W, W), np.int8)
    else:
        xyz = (rng.standard_normal((B, N, 3)) * 50).astype(np.float32)
        xyz[:, ::3] = np.nan
        z = rng.randint(-3, 60, size=(B, W)).astype(np.int32)
        bonds = rng.randint(-2, 7, size=(B, W, W)).astype(np.int8)
        bonds = np.maximum(bonds, bonds.transpose(0, 2, 1))
    n = np.zeros(B, np.int32)
    for b, c in enumerate(items):
        zz, codes, k = c["mol"]
        n[b] = k
        if k:
            xyz[b, :k] = c["xyz"]
            z[b, :k] = zz
            block = np.array(codes, dtype=np.int8).reshape(k, k)
            if garbage_seed is not None:
                block[np.arange(k), np.arange(k)] = rng.randint(1, 5, size=k)
            bonds[b, :k, :k] = block
    return xyz, z, bonds, n
