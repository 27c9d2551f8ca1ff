"""Molecules with 3D heavy atoms shared by the explicit-hydrogen tests: hand-written graphs with idealised geometry and
their known hydrogen counts, fixtures written to hit the degenerate fallbacks, a hindered hydroxyl, a 64-atom molecule
and the padded batch the kernel is run on.  A fixture is a dict: mol (z, adj, n as in `pharmacophore_ref`), xyz fp32
[n,3], hydrogens (the known count, or None), degenerate (written to sit exactly on a degenerate fallback)."""
import functools
import math
import random

import numpy as np

import hydrogens_ref as HR
import pharmacophore_ref as R

CC, CO, CN, CAR = 1.52, 1.43, 1.47, 1.39


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


GENERIC = _rot(0.41, -0.87, 1.23)                  # no fixture axis stays on a coordinate axis
SHIFT = np.array([0.7, -1.1, 0.4])
MOTION = (_rot(-1.1, 0.6, 2.2), np.array([1.5, 2.0, -0.5]))      # the rigid motion of the equivariance test


def _polar(r, deg, z=0.0):
    return [r * math.cos(math.radians(deg)), r * math.sin(math.radians(deg)), z]


def _ring_xyz(size, r, start=90.0):
    return [_polar(r, start + 360.0 * k / size) for k in range(size)]


def _ring_bonds(size, code, first=0):
    return [(first + i, first + (i + 1) % size, code) for i in range(size)]


def _fixture(z, bonds, xyz, hydrogens=None, degenerate=False, generic=True):
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    if generic:
        p = p @ GENERIC.T + SHIFT
    return dict(mol=R.mol(z, bonds), xyz=p.astype(np.float32), hydrogens=hydrogens, degenerate=degenerate)


R6 = CAR                                            # circumradius of a regular hexagon of side CAR
R5 = 1.38 / (2 * math.sin(math.pi / 5))             # of a regular pentagon of side 1.38
_TET = 109.4712


def _hand_written():
    f = {}
    f["methane"] = _fixture([6], [], [[0.3, -0.2, 0.1]], 4, generic=False)
    # C0 - C1 - O2, zig-zag in the xy-plane
    ethanol = [[0, 0, 0], [CC, 0, 0], [CC + CO * math.cos(math.radians(180 - _TET)), CO * math.sin(math.radians(180 - _TET)), 0]]
    f["ethanol"] = _fixture([6, 6, 8], [(0, 1, 1), (1, 2, 1)], ethanol, 6)
    f["benzene"] = _fixture([6] * 6, _ring_bonds(6, 4), _ring_xyz(6, R6), 6)
    f["pyridine"] = _fixture([7] + [6] * 5, _ring_bonds(6, 4), _ring_xyz(6, R6), 5)
    f["pyrrole"] = _fixture([7] + [6] * 4, _ring_bonds(5, 4), _ring_xyz(5, R5), 5)
    f["imidazole"] = _fixture([7, 6, 7, 6, 6], _ring_bonds(5, 4), _ring_xyz(5, R5), 4)
    # C0 methyl, C1 carbonyl at the origin, O2, N3: the three substituents of C1 at 120 degrees
    f["acetamide"] = _fixture([6, 6, 8, 7], [(0, 1, 1), (1, 2, 2), (1, 3, 1)],
                              [_polar(CC, 180), [0, 0, 0], _polar(1.23, 60), _polar(1.35, -60)], 5)
    f["acetonitrile"] = _fixture([6, 6, 7], [(0, 1, 1), (1, 2, 3)], [[0, 0, 0], [1.46, 0, 0], [2.62, 0, 0]], 3,
                                 degenerate=True)       # w of the methyl rotor lies on its axis: p = 0
    f["propyne"] = _fixture([6, 6, 6], [(0, 1, 1), (1, 2, 3)], [[0, 0, 0], [1.46, 0, 0], [2.66, 0, 0]], 4, degenerate=True)
    # benzene with O6 on C0
    f["phenol"] = _fixture([6] * 6 + [8], _ring_bonds(6, 4) + [(0, 6, 1)], _ring_xyz(6, R6) + [_polar(R6 + 1.36, 90)], 6)
    f["formaldehyde"] = _fixture([6, 8], [(0, 1, 2)], [[0, 0, 0], [1.21, 0, 0]], 2)
    f["ethane"] = _fixture([6, 6], [(0, 1, 1)], [[0, 0, 0], [CC, 0, 0]], 6)
    # isobutane: C0 with three methyls, tetrahedral k = 3
    t = math.radians(_TET - 90.0)
    iso = [[0, 0, 0]] + [[CC * math.cos(t) * math.cos(math.radians(a)), CC * math.cos(t) * math.sin(math.radians(a)),
                          -CC * math.sin(t)] for a in (0, 120, 240)]
    f["isobutane"] = _fixture([6] * 4, [(0, 1, 1), (0, 2, 1), (0, 3, 1)], iso, 10)
    # propane, k = 2 tetrahedral in the middle; dimethylamine likewise with h = 1
    bent = [[-CC * math.sin(math.radians(_TET / 2)), CC * math.cos(math.radians(_TET / 2)), 0], [0, 0, 0],
            [CC * math.sin(math.radians(_TET / 2)), CC * math.cos(math.radians(_TET / 2)), 0]]
    f["propane"] = _fixture([6, 6, 6], [(0, 1, 1), (1, 2, 1)], bent, 8)
    f["dimethylamine"] = _fixture([6, 7, 6], [(0, 1, 1), (1, 2, 1)], bent, 7)
    # hydrogen cyanide's carbon: linear k = 1; carbon dioxide has none
    f["hydrogen cyanide"] = _fixture([6, 7], [(0, 1, 3)], [[0, 0, 0], [1.16, 0, 0]], 1)
    f["water"] = _fixture([8], [], [[-1.0, 2.0, 0.5]], 2, generic=False)
    f["no atoms"] = dict(mol=R.mol([], []), xyz=np.zeros((0, 3), dtype=np.float32), hydrogens=0, degenerate=False)
    return f


def _degenerate():
    """Exactly degenerate geometries, on the coordinate axes so that they are exact in fp32 too."""
    f = {}
    # a tetrahedral C between two neighbours on one line: u1 + u2 = 0 exactly
    f["straight propane"] = _fixture([6, 6, 6], [(0, 1, 1), (1, 2, 1)], [[-1.5, 0, 0], [0, 0, 0], [1.5, 0, 0]], 8,
                                     degenerate=True, generic=False)
    # a planar C (one aromatic bond each way) between two neighbours on one line
    f["straight aromatic"] = _fixture([6, 6, 6], [(0, 1, 4), (1, 2, 4)], [[0, -1.5, 0.25], [0, 0, 0.25], [0, 1.5, 0.25]],
                                      5, degenerate=True, generic=False)
    # a tetrahedral C whose three neighbours lie in a plane with it, along exact directions that sum to zero
    f["flat isobutane"] = _fixture([6] * 4, [(0, 1, 1), (0, 2, 1), (0, 3, 1)],
                                   [[0, 0, 0], [1.5, 0, 0], [-0.75, 1.2990381, 0], [-0.75, -1.2990381, 0]], 10, degenerate=True,
                                   generic=False)
    return f


def _hindered():
    """Ethanol with an unbonded fluorine 2.0 A beyond the default (delta = 0) hydroxyl hydrogen, on the O-H line."""
    base = _hand_written()["ethanol"]
    ref = HR.place(*base["mol"], base["xyz"])
    assert ref["rotor_delta"][2] == 0
    h = ref["coords"][ref["parents"].index(2)]
    o = base["xyz"][2].astype(np.float64)
    far = h + 2.0 * (h - o) / np.linalg.norm(h - o)
    z, adj, n = base["mol"]
    mol = R.mol(z + [9], [(0, 1, 1), (1, 2, 1)])
    return dict(mol=mol, xyz=np.vstack([base["xyz"], far.astype(np.float32)]), hydrogens=None, degenerate=False)


def _grown(seed, n=64):
    """A 64-atom tree with molecule-like geometry: every new atom 1.5 A from an earlier one of degree < 3 (one code-2 bond
    now and then), at 100..125 degrees from that atom's other bonds and at least 2.7 A from every atom it is not bonded
    to; terminal atoms become O, N, F or stay C."""
    rng = random.Random(seed)
    for _ in range(200):
        xyz, z, bonds, deg = [np.zeros(3)], [6], [], [0]
        tries = 0
        while len(z) < n and tries < 20000:
            tries += 1
            p = rng.randrange(len(z))
            if deg[p] >= 3:
                continue
            d = np.array([rng.gauss(0, 1) for _ in range(3)])
            d /= np.linalg.norm(d)
            q = xyz[p] + 1.5 * d
            ok = np.linalg.norm(q) < 14.0
            for i, j, _ in bonds:
                other = j if i == p else i if j == p else None
                if other is not None:
                    c = d.dot((xyz[other] - xyz[p]) / 1.5)
                    ok = ok and math.cos(math.radians(125)) <= c <= math.cos(math.radians(100))
            for i, r in enumerate(xyz):
                if i != p:
                    near = any((a == i and b == p) or (a == p and b == i) for a, b, _ in bonds)
                    ok = ok and np.linalg.norm(q - r) >= (2.3 if near else 2.7)
            if ok:
                xyz.append(q)
                z.append(6)
                bonds.append((p, len(z) - 1, 1))
                deg[p] += 1
                deg.append(1)
        if len(z) == n:
            break
    assert len(z) == n
    for a in range(n):
        if deg[a] == 1:
            z[a] = rng.choice([8, 7, 9, 8, 17, 6])
        elif deg[a] == 2 and rng.random() < 0.3:
            z[a] = rng.choice([7, 8])
    # a few double bonds between carbons of degree <= 2 that have none yet
    used = set()
    for k, (i, j, c) in enumerate(bonds):
        if z[i] == 6 and z[j] == 6 and deg[i] <= 2 and deg[j] <= 2 and i not in used and j not in used and rng.random() < 0.25:
            bonds[k] = (i, j, 2)
            used.update((i, j))
    return dict(mol=R.mol(z, bonds), xyz=np.array(xyz).astype(np.float32), hydrogens=None, degenerate=False)


def grown(seed, n):
    """A grown molecule of n atoms that is in no fixture list: for bit comparisons, not for the restatement."""
    return _grown(seed, n)


GROWN_SEED = 33                                     # the first seed whose molecule meets the conditions test_hydrogens_gpu.py asserts


@functools.lru_cache(maxsize=None)
def fixtures():
    f = _hand_written()
    f.update(_degenerate())
    f["hindered ethanol"] = _hindered()
    f["grown 64"] = _grown(GROWN_SEED)
    return f


KNOWN_COUNTS = {"methane": 4, "ethanol": 6, "benzene": 6, "pyridine": 5, "pyrrole": 5, "imidazole": 4, "acetamide": 5,
                "acetonitrile": 3, "propyne": 4}


@functools.lru_cache(maxsize=None)
def references():
    """name -> `hydrogens_ref.place` of the fixture: computed once, shared, never written to."""
    return {name: HR.place(*fx["mol"], fx["xyz"]) for name, fx in fixtures().items()}


def pad_batch(items, W, N, garbage_seed=None):
    """(coords [B,N,3] fp32, z [B,W] int32, bonds [B,W,W] int8, n [B] int32) as numpy arrays from fixtures; with
    `garbage_seed` everything at or beyond a row's atom count - coordinates, elements, codes, the diagonal - holds junk."""
    B = len(items)
    rng = np.random.RandomState(garbage_seed or 0)
    if garbage_seed is None:
        xyz, z, bonds = np.zeros((B, N, 3), np.float32), np.zeros((B, W), np.int32), np.zeros((B, W, W), np.int8)
    else:
        xyz = (rng.standard_normal((B, N, 3)) * 50).astype(np.float32)
        xyz[:, ::3] = np.nan                                       # junk coordinates include NaN
        z = rng.randint(-3, 60, size=(B, W)).astype(np.int32)
        bonds = rng.randint(-2, 7, size=(B, W, W)).astype(np.int8)
    n = np.zeros(B, np.int32)
    for b, fx in enumerate(items):
        zz, adj, k = fx["mol"]
        n[b] = k
        if k:
            xyz[b, :k] = fx["xyz"]
            z[b, :k] = zz
            block = np.array(adj, dtype=np.int8).reshape(k, k)
            if garbage_seed is not None:
                block[np.arange(k), np.arange(k)] = rng.randint(1, 5, size=k)       # junk on the diagonal too
            bonds[b, :k, :k] = block
    return xyz, z, bonds, n
