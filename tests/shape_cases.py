"""The smallest geometries at which the shape-moment and frame kernels can go wrong, for `tests/test_shape_stages_host.py` and
`tests/test_shape_stages_gpu.py`.  Each builder asserts its own condition, so a later edit cannot hollow a case out.

Every case is built in fp64, rotated by one fixed orthogonal matrix with no zero entry (`ROT`) and shifted by `SHIFT` (about
1 A), then rounded to fp32.  Exceptions, each forced by its own condition: the bare single atom; the two threshold pairs,
which need an EXACT fp32 distance and therefore lie along x, shifted only (1.0 and fl32(5.4) share their binade's grid, so
the sum, the difference and the centred coordinates are all exact); the far hexagon, which is moved on by (200, -150, 90)."""
from __future__ import annotations

import math
import os
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

import shape_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shape_quadrupole.npz")
THRESHOLD = 2 * R.AMPLITUDE                       # the default neighbour threshold, 5.4
WIDTH = 64


def _rot() -> np.ndarray:
    a, b, c = 0.7, -1.1, 0.4
    rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    m = rx @ ry @ rz
    assert float(np.abs(m.T @ m - np.eye(3)).max()) < 1e-15 and float(np.abs(m).min()) > 0.1       # orthogonal, no axis kept
    return m


ROT = _rot()
SHIFT = np.array([0.9, -1.1, 1.05])
FAR = np.array([200.0, -150.0, 90.0])


class Case(NamedTuple):
    name: str
    points: np.ndarray            # [n,3] fp32
    degenerate: str               # "none", "top2" (two largest moments equal), "low2", "all3", "near" - asserted below
    centre_only: bool = False     # values are compared with centre_atoms = 1 only


def _place(p) -> np.ndarray:
    return (np.asarray(p, dtype=np.float64).reshape(-1, 3) @ ROT + SHIFT).astype(np.float32)


def _ring(n: int, r: float) -> np.ndarray:
    a = 2 * math.pi * np.arange(n) / n
    return np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1)


def _adj(p, centre=False):
    return R.neighbour_matrix(R.centre_atoms_fp32(p)[0] if centre else p, THRESHOLD)


def _moments(p) -> np.ndarray:
    return R.restate(p, centre_atoms=True)["moments"]


def _gap(m: np.ndarray) -> Tuple[float, float]:
    return (m[0] - m[1]) / m[0], (m[1] - m[2]) / m[1]


# fp32 rounding of the coordinates splits an exactly degenerate pair of moments by a few 1e-8 relative (2e-6 for the far
# hexagon, whose coordinates of about 200 are rounded to 1.5e-5)
_EQUAL, _APART = 1e-5, 0.01


def _assert_degeneracy(name: str, p: np.ndarray, kind: str) -> None:
    if p.shape[0] == 0:
        return
    top, low = _gap(_moments(p))
    want = {"none": (top > _APART and low > _APART), "top2": (top < _EQUAL and low > _APART),
            "low2": (top > _APART and low < _EQUAL), "all3": (top < _EQUAL and low < _EQUAL),
            "near": (_EQUAL < min(top, low) < 1e-2)}[kind]
    assert want, (name, kind, top, low)


def single_atom() -> Case:
    p = np.array([[0.0, 0.0, 0.0]], dtype=np.float32)
    assert p.shape == (1, 3)
    return Case("single_atom", p, "all3")


def pair() -> Case:
    p = _place([[0, 0, 0], [1.5, 0, 0]])
    d = R.fp32_distances(p)[0, 1]
    assert abs(float(d) - 1.5) < 1e-6 and bool(_adj(p)[0, 1])
    return Case("pair", p, "low2")


def coincident_triple() -> Case:
    p = _place([[0, 0, 0], [0, 0, 0], [1.5, 0, 0]])
    for centre in (False, True):
        q = R.centre_atoms_fp32(p)[0] if centre else p
        a = _adj(p, centre)
        assert np.array_equal(q[0], q[1]) and float(R.fp32_distances(q)[0, 1]) == 0.0        # bit-identical atoms
        assert not a[0, 1] and a[0, 2] and a[1, 2]                                            # and NOT neighbours
    return Case("coincident_triple", p, "low2")


def _threshold_pair(name: str, d32: np.float32, neighbours: bool) -> Case:
    x0 = np.float32(1.0)
    p = np.array([[x0, -1.1, 1.05], [x0 + d32, -1.1, 1.05]], dtype=np.float32)
    thr = np.float32(THRESHOLD)
    for centre in (False, True):
        q = R.centre_atoms_fp32(p)[0] if centre else p
        got = R.fp32_distances(q)[0, 1]
        assert got == d32, (name, centre, got, d32)                                           # the distance is exact
        assert bool(_adj(p, centre)[0, 1]) == neighbours
    assert (d32 == thr) != neighbours
    return Case(name, p, "low2")


def pair_at_threshold() -> Case:
    return _threshold_pair("pair_at_threshold", np.float32(THRESHOLD), False)


def pair_below_threshold() -> Case:
    thr = np.float32(THRESHOLD)
    below = np.nextafter(thr, np.float32(0))
    assert below < thr and np.nextafter(below, np.float32(10)) == thr
    return _threshold_pair("pair_below_threshold", below, True)


def hexagon() -> Case:
    p = _place(_ring(6, 1.39))
    assert int(_adj(p).sum()) == 30                                                           # complete graph
    return Case("hexagon", p, "top2")


def tetrahedron() -> Case:
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) * (1.54 / math.sqrt(3))
    p = _place(np.concatenate([np.zeros((1, 3)), v]))
    assert p.shape[0] == 5 and int(_adj(p).sum()) == 20
    return Case("tetrahedron", p, "all3")


def cube() -> Case:
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * (1.57 / 2)
    p = _place(v)
    assert p.shape[0] == 8 and int(_adj(p).sum()) == 56
    return Case("cube", p, "all3")


def chain5() -> Case:
    p = _place(np.arange(5)[:, None] * np.array([1.5, 0, 0]))
    a = _adj(p)
    assert a[0, 3] and not a[0, 4]                                                            # 4.5 < 5.4 < 6.0
    return Case("chain5", p, "low2")


def ring12() -> Case:
    p = _place(_ring(12, 2.9))
    a = _adj(p)
    assert a[0, 3] and a[0, 4] and not a[0, 5] and not a[0, 6]             # chords 4.10, 5.02 | 5.60, 5.80: not complete
    return Case("ring12", p, "top2")


def _golden(name: str) -> np.ndarray:
    return np.load(GOLDEN, allow_pickle=False)[f"xyz_{name}"].astype(np.float64)


def crown_6() -> Case:
    p = _place(_golden("crown_6"))
    assert p.shape[0] == 18
    return Case("crown_6", p, "near")


def two_hexagons() -> Case:
    p = _place(np.concatenate([_ring(6, 1.39), _ring(6, 1.39) + np.array([30.0, 0, 0])]))
    a = _adj(p)
    assert int(a[:6, :6].sum()) == 30 and int(a[6:, 6:].sum()) == 30 and int(a[:6, 6:].sum()) == 0       # disconnected
    return Case("two_hexagons", p, "none")


def chain12_no_edges() -> Case:
    p = _place(np.arange(12)[:, None] * np.array([6.0, 0, 0]))
    assert int(_adj(p).sum()) == 0 and int(_adj(p, True).sum()) == 0
    return Case("chain12_no_edges", p, "low2")


def far_hexagon() -> Case:
    p = ((_ring(6, 1.39) @ ROT + SHIFT) + FAR).astype(np.float32)
    assert float(np.linalg.norm(p.astype(np.float64).mean(axis=0))) > 250.0 and int(_adj(p, True).sum()) == 30
    return Case("far_hexagon", p, "top2", centre_only=True)


def paba() -> Case:
    p = _place(_golden("paba"))
    assert p.shape[0] == 10
    return Case("paba", p, "none")


def walk12() -> Case:
    p = _place(_golden("walk12"))
    assert p.shape[0] == 12
    return Case("walk12", p, "none")


def helix64() -> Case:
    """64 atoms on a tight helix (radius 1.5, rise 0.6 per atom, 100 degrees per atom): every atom neighbours the 8 atoms
    after it, and any 9 consecutive atoms are mutual neighbours."""
    i = np.arange(64)
    th = np.deg2rad(100.0) * i
    p = _place(np.stack([1.5 * np.cos(th), 1.5 * np.sin(th), 0.6 * i], axis=1))
    for centre in (False, True):
        cl = R.find_cliques(_adj(p, centre), 8)
        for k in range(2, 9):
            assert bool((cl[k] == 63).any()), (k, "atom 63 in no clique of this order")
        assert cl[2].shape[0] > 64                                       # the prefix scan's chunk of edges per lane is > 1
        assert cl[3].shape[0] > 1024                                     # more triangles than lanes: the stride loop runs
        assert sum(v.shape[0] for v in cl.values()) <= 50_000
    return Case("helix64", p, "none")


BUILDERS = (single_atom, pair, coincident_triple, pair_at_threshold, pair_below_threshold, hexagon, tetrahedron, cube,
            chain5, ring12, crown_6, two_hexagons, chain12_no_edges, far_hexagon, paba, walk12, helix64)
COMPACT = ("hexagon", "tetrahedron", "cube")
_CASES: List[Case] = []


def cases() -> List[Case]:
    """All cases, built (and their conditions asserted) once."""
    if not _CASES:
        for b in BUILDERS:
            c = b()
            assert c.points.dtype == np.float32 and c.points.shape[1] == 3 and c.points.shape[0] <= WIDTH
            _assert_degeneracy(c.name, c.points, c.degenerate)
            _CASES.append(c)
    return list(_CASES)


def case(name: str) -> Case:
    return {c.name: c for c in cases()}[name]


# (atom radius, amplitude, neighbour threshold): the defaults, and a second set so that no constant is only ever its default
PARAMS = {"default": (R.ATOM_RADIUS, R.AMPLITUDE, THRESHOLD), "second": (1.2, 2.0, 3.0)}
ORDERS = (2, 3, 6, 8)
_REFS: Dict[tuple, dict] = {}


def reference(name: str, n_terms: int = 6, centre_atoms: bool = False, params: str = "default") -> dict:
    """`shape_ref.restate` of a case, computed once and shared; treat the result as read-only."""
    key = (name, n_terms, bool(centre_atoms), params)
    if key not in _REFS:
        radius, amp, thr = PARAMS[params]
        _REFS[key] = R.restate(case(name).points, n_terms=n_terms, amplitude=amp, atom_radius=radius, threshold=thr,
                               centre_atoms=centre_atoms)
    return _REFS[key]


EMPTY_ROW = 8         # the n_nodes = 0 row sits here, in the middle of the batch


def ragged_batch() -> Tuple[np.ndarray, np.ndarray, Dict[str, int]]:
    """(coords [B, 64, 3] fp32 zero-padded, n_nodes [B] int32, {case name: row}) holding every case, with an n_nodes = 0 row at
    EMPTY_ROW whose coordinates are NOT zero (a kernel that ignored its count would show)."""
    cs = cases()
    rows: List[np.ndarray] = [c.points for c in cs]
    rows.insert(EMPTY_ROW, np.zeros((0, 3), dtype=np.float32))
    x = np.zeros((len(rows), WIDTH, 3), dtype=np.float32)
    n = np.array([r.shape[0] for r in rows], dtype=np.int32)
    for b, r in enumerate(rows):
        x[b, : r.shape[0]] = r
    x[EMPTY_ROW, :6] = case("hexagon").points
    where = {c.name: (i if i < EMPTY_ROW else i + 1) for i, c in enumerate(cs)}
    assert int(n[EMPTY_ROW]) == 0 and 0 < EMPTY_ROW < len(rows) - 1 and EMPTY_ROW not in where.values()
    return x, n, where
