"""Molecules shared by the electrostatic tests: every fixture of `hydrogens_cases` (methane, water, ethanol, acetamide,
acetonitrile, pyridine, pyrrole, imidazole, phenol, "grown 64" with every lane real, the one-atom and the zero-atom
molecule among them) plus the ones the charge table needs - acetic acid, a sulfone, a thioether, a chloro / bromo /
fluoro compound, a phosphate, a molecule with Si (no parameters: status 1) and one with a hydrogen the placement has no
direction for - and the point clouds of the overlap kernel's shape cases.  A fixture is `hydrogens_cases`' dict: mol (z,
adj, n), xyz fp32 [n,3]."""
import functools
import math

import numpy as np

import electrostatics_ref as ER
import hydrogens_cases as C
import hydrogens_ref as HR

_T = [np.array(v) / math.sqrt(3.0) for v in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]     # tetrahedral directions


def _star(lengths):
    """A centre at the origin with neighbours along the tetrahedral directions at the given bond lengths."""
    return [[0.0, 0.0, 0.0]] + [list(_T[k] * r) for k, r in enumerate(lengths)]


def _added():
    f = {}
    # C0 methyl, C1 carboxyl carbon, O2 carbonyl, O3 hydroxyl
    f["acetic acid"] = C._fixture([6, 6, 8, 8], [(0, 1, 1), (1, 2, 2), (1, 3, 1)],
                                  [C._polar(C.CC, 180), [0, 0, 0], C._polar(1.21, 60), C._polar(1.36, -60)])
    f["dimethyl sulfone"] = C._fixture([16, 8, 8, 6, 6], [(0, 1, 2), (0, 2, 2), (0, 3, 1), (0, 4, 1)],
                                       _star([1.44, 1.44, 1.78, 1.78]))
    bent = np.array(C._hand_written()["propane"]["xyz"], dtype=np.float64)
    f["dimethyl sulfide"] = dict(mol=C.R.mol([6, 16, 6], [(0, 1, 1), (1, 2, 1)]),
                                 xyz=((bent - bent[1]) * (1.81 / C.CC) + bent[1]).astype(np.float32), hydrogens=None,
                                 degenerate=False)
    f["bromochlorofluoromethane"] = C._fixture([6, 9, 17, 35], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], _star([1.36, 1.77, 1.94]))
    # P0 with a phosphoryl O1 and three hydroxyl O
    f["phosphoric acid"] = C._fixture([15, 8, 8, 8, 8], [(0, 1, 2), (0, 2, 1), (0, 3, 1), (0, 4, 1)],
                                      _star([1.48, 1.57, 1.57, 1.57]))
    f["methylsilane"] = C._fixture([6, 14], [(0, 1, 1)], [[0, 0, 0], [1.87, 0, 0]])
    # ethanol beside an oxygen bonded to nothing: in a larger molecule its two hydrogens have no direction
    base = C._hand_written()["ethanol"]
    stray = base["xyz"].astype(np.float64).mean(0) + np.array([0.0, 0.0, 4.0])
    f["ethanol and a stray oxygen"] = dict(mol=C.R.mol([6, 6, 8, 8], [(0, 1, 1), (1, 2, 1)]),
                                           xyz=np.vstack([base["xyz"], stray.astype(np.float32)]), hydrogens=None,
                                           degenerate=False)
    return f


@functools.lru_cache(maxsize=None)
def fixtures():
    f = dict(C.fixtures())
    f.update(_added())
    return f


UNCHARGED = "methylsilane"
UNPLACED = "ethanol and a stray oxygen"
REQUIRED = ("methane", "water", "ethanol", "acetic acid", "acetamide", "acetonitrile", "pyridine", "pyrrole", "imidazole",
            "phenol", "dimethyl sulfone", "dimethyl sulfide", "bromochlorofluoromethane", "phosphoric acid", "grown 64",
            "no atoms", UNCHARGED, UNPLACED)


@functools.lru_cache(maxsize=None)
def references():
    """name -> dict(placed, charges, points): `hydrogens_ref.place`, `electrostatics_ref.charges` and
    `electrostatics_ref.points` of the fixture: computed once, shared, never written to."""
    out = {}
    for name, fx in fixtures().items():
        z, adj, n = fx["mol"]
        placed = HR.place(z, adj, n, fx["xyz"])
        ch = ER.charges(z, adj, n)
        out[name] = dict(placed=placed, charges=ch, points=ER.points(n, fx["xyz"], ch, placed))
    return out


def fp32_points(name):
    """(xyz [P,3] fp32, q [P] fp32) of a fixture: the restatement's charge points rounded to what a kernel is given."""
    x, q = references()[name]["points"]
    return x.astype(np.float32), q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def cloud(k, shift=0.0):
    """(xyz [k,3] fp32, q [k] fp32): the first k charge points of copies of "grown 64" set side by side 30 A apart - a
    point cloud with a molecule's distances and charges at any size up to 256 and beyond."""
    x, q = fp32_points("grown 64")
    copies = -(-k // len(q))
    xs = np.vstack([x + np.float32([30.0 * c + shift, 0.25 * shift, 0.0]) for c in range(copies)])[:k]
    qs = np.concatenate([q * np.float32(1.0 - 0.1 * c) for c in range(copies)])[:k]
    return np.ascontiguousarray(xs, dtype=np.float32), np.ascontiguousarray(qs, dtype=np.float32)


def pad_points(items, PW, garbage_seed=None):
    """(xyz [B,PW,3] fp32, q [B,PW] fp32, n [B] int32) from (xyz, q) pairs; with `garbage_seed` everything at or beyond a
    row's points holds junk, NaN included."""
    B = len(items)
    rng = np.random.RandomState(garbage_seed or 0)
    if garbage_seed is None:
        xyz, q = np.zeros((B, PW, 3), np.float32), np.zeros((B, PW), np.float32)
    else:
        xyz = (rng.standard_normal((B, PW, 3)) * 50).astype(np.float32)
        xyz[:, ::3] = np.nan
        q = rng.standard_normal((B, PW)).astype(np.float32)
        q[:, 1::4] = np.inf
    n = np.zeros(B, np.int32)
    for b, (x, c) in enumerate(items):
        n[b] = len(c)
        xyz[b, : len(c)] = x
        q[b, : len(c)] = c
    return xyz, q, n
