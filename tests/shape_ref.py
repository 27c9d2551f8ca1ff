"""Plain fp64 restatement of the Gaussian-volume shape stage: `mcg_shape_moments`, `mcg_shape_frames` / `_tf` and the grid
Tanimoto behind `mcg_shape_tanimoto`.  Host only (numpy), no import of the package's kernels or of its tensor path; written
from the formulas in the header comment of `csrc/mcg_shape_frames.hip` and from `oracle/shape_oracle.py`.

What is restated, per molecule of n atoms with fp32 coordinates p:
  * optional centring (`centre_atoms`): the mean as the kernel computes it, bit for bit - an fp32 sum in atom order, divided
    by n in fp32, subtracted in fp32 (`centre_atoms_fp32`);
  * the neighbour rule (`neighbour_matrix`): fp32 direct-difference distance d = sqrt((dx dx + dy dy) + dz dz), every
    operation rounded on its own, i ~ j iff 0 < d < fl32(threshold).  A decision, not arithmetic: the only other fp32 step;
  * every clique (mutually neighbouring i1 < ... < ik) of order k = 1 .. n_terms, by a plain recursive search;
  * everything else in fp64.  A clique of order k with members c_i contributes, with sign (-1)^(k-1),
        w = A^k exp(-alpha gamma) (pi / (k alpha))^1.5,   gamma = sum |c_i|^2 - |sum c_i|^2 / k = sum |c_i - m|^2,
        m = mean c_i,   volume += w,   first += w m,   second_ab += w (m_a m_b + delta_ab / (2 k alpha));
    shape centre = first / volume; tensor = second moments of the points minus the shape centre, over the volume; the
    principal moments are its eigenvalues (`numpy.linalg.eigvalsh`), descending.

Error unit.  The kernel and the project's tensor path evaluate each term in fp32 and sum in fp64, so their distance from this
restatement scales with the magnitude of the terms, not of the result (inclusion-exclusion cancels).  Per quantity:
    u_volume  = 2^-24 sum_terms |w| kappa                                   (absolute)
    u_centre  = 2^-24 sum_terms max_d |w m_d| kappa / volume                (first moments over volume)
    u_tensor  = 2^-24 sum_terms max_ab |w (m_a m_b + delta_ab h_k)| kappa / volume
    u_moments = u_tensor + 2^-24 lambda_max                                 (the fp32 `eigh` and rotation on top)
    kappa     = 1 for a single atom, 1 + alpha (q + |s|^2 / k) for a clique of order k >= 2, q = sum |c_i|^2, s = sum c_i,
                in the coordinates the pass is evaluated in.
kappa is the condition of the fp32 weight: gamma is formed as q - |s|^2 / k, each of the two rounded at its own size, so
gamma is off by about 2^-24 (q + |s|^2 / k) and w = A^k exp(-alpha gamma) by alpha times that, relatively.  Without kappa
(the `*_plain` units, also returned) the counts below are single digits for every case whose atoms lie within a few
angstroms of the origin the pass evaluates in, but 197 (tensor) for the two hexagons 30 A apart taken as they stand, 74
after centring (atoms 15 A out) and 25 for the 38 A long helix: the cancellation that makes the uncentred far hexagon 4e-3 off
in volume, at a smaller distance.  With kappa the worst count of every case lies between 0.1 and 3.2, so the unit follows
the error and one constant per quantity serves all cases.  A tolerance is a count of these units.

Measured counts, and the constants that follow from them.  `tests/test_shape_stages_host.py` runs the project's fp32 tensor
path (`_grow_cliques` / `_shape_moments` / `_moment_tensor` / `shape_quadrupole_batch`, device="cpu") over every case of
`tests/shape_cases.py` for n_terms in {2, 3, 6, 8}, both centring modes and the default and the second parameter set, and
prints its worst error in these units:

    python -m pytest tests/test_shape_stages_host.py -k tensor_path -s

gave (x86-64 host, torch CPU with its bundled LAPACK):

    volume        0.99 units at single_atom        n_terms=2 centre=0 default
    centre        0.67 units at chain12_no_edges   n_terms=2 centre=0 default
    tensor        2.15 units at chain5             n_terms=2 centre=0 default
    moments       3.16 units at chain5             n_terms=2 centre=0 default
    offdiag       0.74 units at coincident_triple  n_terms=2 centre=0 second
    diag          2.32 units at chain5             n_terms=2 centre=0 default
    frame_centre  0.98 units at chain5             n_terms=2 centre=0 default

(MEASURED_UNITS below; the far hexagon without centring is left out of the counts: fp32 gamma cancels there for any
evaluation order, the tensor path is 4.3e-3 relative off in volume and 7.4e-3 absolute in the tensor.)

The GPU tolerance of a quantity is 4 x its measured count (TOL_UNITS): the kernel and the tensor path are two fp32
evaluations that may lie on opposite sides of fp64 (x 2), and LAPACK and expf differ between machines (x 2).  The host test
holds the tensor path within HALF of TOL_UNITS, the GPU test holds the kernels within TOL_UNITS.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

ATOM_RADIUS = 1.60
AMPLITUDE = 2.70
EPS32 = 2.0 ** -24


def get_alpha(atom_radius: float = ATOM_RADIUS, amplitude: float = AMPLITUDE) -> float:
    lam = 4 * math.pi / 3 / amplitude
    return (math.pi / lam ** (2 / 3)) / atom_radius ** 2


# Worst error of the fp32 tensor path against this restatement, in the units above (see the module docstring for the
# command).  "offdiag", "diag" and "frame_centre" are the frame checker's quantities 3, 4 and 5, in u_moments / u_moments /
# u_frame_centre of the frame points.
MEASURED_UNITS = {"volume": 0.99, "centre": 0.67, "tensor": 2.15, "moments": 3.16, "offdiag": 0.74, "diag": 2.32,
                  "frame_centre": 0.98}
TOL_UNITS = {k: 4.0 * v for k, v in MEASURED_UNITS.items()}

MUTATIONS: Tuple[str, ...] = (
    "drop_2", "drop_3", "drop_4", "drop_5", "drop_6",      # one whole order of the inclusion-exclusion missing
    "even_sign",                                           # even orders added instead of subtracted
    "half_alpha",                                          # 1 / (2 alpha) instead of 1 / (2 k alpha)
    "le_threshold",                                        # d <= threshold
    "coincident",                                          # d == 0 (distinct atoms) counted as neighbours
    "atom_mean_centre",                                    # the atoms' mean instead of first moment over volume
)


# ------------------------------------------------------------------------------------------------- the two fp32 steps
def centre_atoms_fp32(points: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(points - mean, mean) as `load_and_build` computes them: acc += p[i] in atom order in fp32, acc / n, p - mean."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    acc = np.zeros(3, dtype=np.float32)
    for i in range(n):
        acc = (acc + p[i]).astype(np.float32)
    mean = (acc / np.float32(max(n, 1))).astype(np.float32)
    return (p - mean).astype(np.float32), mean


def fp32_distances(points: np.ndarray) -> np.ndarray:
    """d[i, j] = sqrtf((dx dx + dy dy) + dz dz) in fp32, every product and sum rounded on its own."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    d = (p[:, None, :] - p[None, :, :]).astype(np.float32)
    sq = (d * d).astype(np.float32)
    return np.sqrt(((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32)).astype(np.float32)


def neighbour_matrix(points: np.ndarray, threshold: float, mutation: Optional[str] = None) -> np.ndarray:
    d = fp32_distances(points)
    thr = np.float32(threshold)
    below = d <= thr if mutation == "le_threshold" else d < thr
    if mutation == "coincident":
        above = ~np.eye(d.shape[0], dtype=bool)
    else:
        above = d > np.float32(0)
    return below & above


def find_cliques(adj: np.ndarray, max_order: int) -> Dict[int, np.ndarray]:
    """{k: int array [C_k, k]} of all i1 < ... < ik with every pair adjacent, k = 1 .. max_order, lexicographic."""
    n = adj.shape[0]
    found: Dict[int, List[List[int]]] = {k: [] for k in range(1, max_order + 1)}

    def grow(members: List[int], cand: List[int]) -> None:
        for v in cand:
            m = members + [v]
            found[len(m)].append(m)
            if len(m) < max_order:
                grow(m, [u for u in cand if u > v and adj[v, u]])

    grow([], list(range(n)))
    return {k: np.asarray(v, dtype=np.int64).reshape(-1, k) for k, v in found.items()}


# ------------------------------------------------------------------------------------------------- fp64 moments
_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def _order_terms(p: np.ndarray, idx: np.ndarray, k: int, alpha: float, amplitude: float, mutation: Optional[str]):
    """Signed per-clique terms of order k about the origin of `p` (fp64): w [C], w m [C,3], second [C,6] (xx yy zz xy xz yz)."""
    c = p[idx]                                           # [C, k, 3]
    m = c.mean(axis=1)
    gamma = ((c - m[:, None, :]) ** 2).sum(axis=(1, 2))
    sign = 1.0 if (k % 2 == 1 or mutation == "even_sign") else -1.0
    w = sign * amplitude ** k * np.exp(-alpha * gamma) * (math.pi / (k * alpha)) ** 1.5
    h = 1.0 / (2.0 * alpha) if mutation == "half_alpha" else 1.0 / (2.0 * k * alpha)
    second = np.stack([w * (m[:, a] * m[:, b] + (h if a == b else 0.0)) for a, b in _PAIRS], axis=1)
    # how far an fp32 gamma = q - |s|^2 / k can be off, relative to the weight it feeds: alpha * 2^-24 * (q + |s|^2 / k)
    cond = 1.0 + (alpha * ((c ** 2).sum(axis=(1, 2)) + k * (m ** 2).sum(axis=1)) if k > 1 else 0.0)
    return w, w[:, None] * m, second, cond


def moments_about(p: np.ndarray, cliques: Dict[int, np.ndarray], n_terms: int, alpha: float, amplitude: float,
                  mutation: Optional[str] = None) -> dict:
    """Sums over all cliques of order <= n_terms for the fp64 points `p`: volume, first [3], second [6], the per-order signed
    sums of each, and the absolute sums behind the error units."""
    out = {"volume": 0.0, "first": np.zeros(3), "second": np.zeros(6), "abs_w": 0.0, "abs_first": 0.0, "abs_second": 0.0,
           "plain_w": 0.0, "plain_second": 0.0, "per_order": {}}
    for k in range(1, n_terms + 1):
        idx = cliques.get(k)
        if idx is None or idx.shape[0] == 0 or mutation == f"drop_{k}":
            out["per_order"][k] = {"volume": 0.0, "first": np.zeros(3), "second": np.zeros(6)}
            continue
        w, f, s, cond = _order_terms(p, idx, k, alpha, amplitude, mutation)
        po = {"volume": float(w.sum()), "first": f.sum(axis=0), "second": s.sum(axis=0)}
        out["per_order"][k] = po
        out["volume"] += po["volume"]
        out["first"] = out["first"] + po["first"]
        out["second"] = out["second"] + po["second"]
        out["abs_w"] += float((np.abs(w) * cond).sum())
        out["abs_first"] += float((np.abs(f).max(axis=1) * cond).sum())
        out["abs_second"] += float((np.abs(s).max(axis=1) * cond).sum())
        out["plain_w"] += float(np.abs(w).sum())
        out["plain_second"] += float(np.abs(s).max(axis=1).sum())
    return out


def _sym(second: np.ndarray) -> np.ndarray:
    xx, yy, zz, xy, xz, yz = second
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def restate(points: np.ndarray, n_terms: int = 6, amplitude: float = AMPLITUDE, atom_radius: float = ATOM_RADIUS,
            threshold: Optional[float] = None, centre_atoms: bool = False, mutation: Optional[str] = None,
            cliques: Optional[Dict[int, np.ndarray]] = None) -> dict:
    """The shape stage of one molecule.  `points` [n,3] fp32.  Returns
      mean [3] fp32 (zeros without centre_atoms), points32 [n,3] fp32 (after centring), cliques, counts [n_terms-1],
      volume, centre [3] (shape centre, in the coordinates of points32), tensor [3,3], moments [3] descending,
      per_order {k: signed sums of volume / first / second about the input origin},
      u_volume, u_centre, u_tensor, u_moments (the error units of the module docstring).
    `cliques`: reuse these instead of searching (the frame checker: the frame points keep the input's cliques)."""
    threshold = 2 * amplitude if threshold is None else threshold
    alpha = get_alpha(atom_radius, amplitude)
    p32 = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    mean = np.zeros(3, dtype=np.float32)
    if centre_atoms:
        p32, mean = centre_atoms_fp32(p32)
    if cliques is None:
        cliques = find_cliques(neighbour_matrix(p32, threshold, mutation), n_terms)
    res = {"mean": mean, "points32": p32, "cliques": cliques, "n_terms": n_terms, "alpha": alpha, "amplitude": amplitude,
           "atom_radius": atom_radius,
           "counts": np.array([cliques[k].shape[0] if k in cliques else 0 for k in range(2, n_terms + 1)], dtype=np.int64)}
    res.update(from_points(p32.astype(np.float64), cliques, n_terms, alpha, amplitude, mutation))
    return res


def from_points(p: np.ndarray, cliques: Dict[int, np.ndarray], n_terms: int, alpha: float, amplitude: float,
                mutation: Optional[str] = None) -> dict:
    """The fp64 part of `restate`: everything behind the neighbour decision, for fp64 points `p` and given cliques."""
    one = moments_about(p, cliques, n_terms, alpha, amplitude, mutation)
    vol = one["volume"]
    res = {"volume": vol, "per_order": one["per_order"], "u_volume": EPS32 * one["abs_w"],
           "u_volume_plain": EPS32 * one["plain_w"]}
    if p.shape[0] == 0:
        nan3 = np.full(3, np.nan)
        res.update(centre=nan3, tensor=np.full((3, 3), np.nan), moments=nan3, u_centre=0.0, u_tensor=0.0, u_moments=0.0)
        return res
    centre = p.mean(axis=0) if mutation == "atom_mean_centre" else one["first"] / vol
    two = moments_about(p - centre, cliques, n_terms, alpha, amplitude, mutation)
    tensor = _sym(two["second"]) / vol
    moments = np.linalg.eigvalsh(tensor)[::-1].copy()
    res.update(centre=centre, tensor=tensor, moments=moments, first_centred=two["first"] / vol,
               u_centre=EPS32 * one["abs_first"] / abs(vol), u_tensor=EPS32 * two["abs_second"] / abs(vol),
               u_tensor_plain=EPS32 * two["plain_second"] / abs(vol))
    res["u_moments"] = res["u_tensor"] + EPS32 * float(np.abs(moments).max())
    return res


def ratio(err: float, tol: float) -> float:
    """err / tol; an exact quantity (tol == 0) must be met exactly."""
    if tol > 0.0:
        return err / tol
    return 0.0 if err == 0.0 else math.inf


# ------------------------------------------------------------------------------------------------- frame checker
ORTHO_TOL = 32 * EPS32       # fp32 LAPACK eigenvectors of a 3x3: orthonormal to a small multiple of 2^-24


def check_frame(points: np.ndarray, frames: np.ndarray, xform: Optional[np.ndarray], moments: np.ndarray, ref: dict,
                tol_units: Optional[Dict[str, float]] = None) -> Dict[str, float]:
    """Invariants of a returned frame that hold whatever basis a degenerate eigenspace was given.  `points` [n,3] fp32 (the
    kernel's input, before any centring), `frames` [N,3] (N >= n, padded rows), `xform` [12] (M row-major, then t) or None
    (the tensor path has none: invariants 1 and 2 are skipped), `moments` [3], `ref` = `restate(points, ...)` with the same
    parameters (its cliques are reused: the frame points keep the molecule's neighbour graph).
    Returns {name: measured / allowed}; a frame passes when every value is <= 1.
      1 "ortho", "det": M^T M = I and |det M| = 1 within ORTHO_TOL (3 ORTHO_TOL for the determinant).
      2 "rigid": frames == (points - t) @ M on the real rows, within the fp32 rounding of the kernel's own evaluation
        ((p - mean) - centre, a three-term dot product, t = mean + centre rounded once):
        2^-24 * 2 * (max|p| + 2 max|t| + 4 max|p - t|); "padding": 0 where padded rows are exactly 0, else inf.
      3 "offdiag": off-diagonals of the fp64 tensor of the frame points, in TOL_UNITS["offdiag"] u_moments.
      4 "diag": its diagonal against `moments`, in TOL_UNITS["diag"] u_moments; "descending": 0 or inf.
      5 "frame_centre": first moments over volume of the frame points, in TOL_UNITS["frame_centre"] u_frame_centre with
        u_frame_centre = u_centre of the frame points + 2^-24 (max|p| + max|t|) (t's rounding moves the whole frame)."""
    tol_units = TOL_UNITS if tol_units is None else tol_units
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    n = p.shape[0]
    fr = np.asarray(frames, dtype=np.float64).reshape(-1, 3)
    mom = np.asarray(moments, dtype=np.float64).reshape(3)
    out: Dict[str, float] = {}
    t_abs = 0.0
    if xform is not None:
        xf = np.asarray(xform, dtype=np.float64).reshape(12)
        M, t = xf[:9].reshape(3, 3), xf[9:]
        t_abs = float(np.abs(t).max())
        out["ortho"] = ratio(float(np.abs(M.T @ M - np.eye(3)).max()), ORTHO_TOL)
        out["det"] = ratio(abs(abs(float(np.linalg.det(M))) - 1.0), 3 * ORTHO_TOL)
        want = (p - t) @ M
        rigid_tol = EPS32 * 2 * (float(np.abs(p).max()) + 2 * t_abs + 4 * float(np.abs(p - t).max()))
        out["rigid"] = ratio(float(np.abs(fr[:n] - want).max()), rigid_tol)
    out["padding"] = 0.0 if (fr.shape[0] == n or float(np.abs(fr[n:]).max()) == 0.0) else math.inf
    again = restate(fr[:n].astype(np.float32), n_terms=ref["n_terms"], amplitude=ref["amplitude"],
                    atom_radius=ref["atom_radius"], cliques=ref["cliques"])
    T = again["tensor"]
    u_m = again["u_moments"]
    out["offdiag"] = ratio(float(np.abs(T - np.diag(np.diag(T))).max()), tol_units["offdiag"] * u_m)
    out["diag"] = ratio(float(np.abs(np.diag(T) - mom).max()), tol_units["diag"] * u_m)
    out["descending"] = 0.0 if (mom[0] >= mom[1] >= mom[2]) else math.inf
    u_fc = again["u_centre"] + EPS32 * (float(np.abs(p).max()) + t_abs)
    out["frame_centre"] = ratio(float(np.abs(again["centre"]).max()), tol_units["frame_centre"] * u_fc)
    return out


# ------------------------------------------------------------------------------------------------- grid half
def grid_density(coords: np.ndarray, axes: np.ndarray, alpha: float, amplitude: float) -> np.ndarray:
    """1 - prod_atoms (1 - A exp(-alpha d^2)) at every point of meshgrid(axes[0], axes[1], axes[2], indexing="ij"), fp64."""
    ax = np.asarray(axes, dtype=np.float64)
    gx, gy, gz = np.meshgrid(ax[0], ax[1], ax[2], indexing="ij")
    pts = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    c = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    prod = np.ones(pts.shape[0])
    for a in range(c.shape[0]):
        prod *= 1.0 - amplitude * np.exp(-alpha * ((pts - c[a]) ** 2).sum(axis=1))
    return 1.0 - prod


def grid_tanimoto(ref: np.ndarray, cand: np.ndarray, rot: np.ndarray, axes: np.ndarray, alpha: float, amplitude: float,
                  f: Optional[np.ndarray] = None) -> float:
    """<f,g> / (<f,f> + <g,g> - <f,g>) on the grid of `axes` [3,n], f and g the densities (`grid_density`) of `ref` [n_ref,3]
    and of `cand` [n,3] @ `rot` [3,3], all in fp64.  An empty candidate has g = 0 and scores 0.  `f`: the reference's
    density where the caller already has it."""
    if f is None:
        f = grid_density(ref, axes, alpha, amplitude)
    g = grid_density(np.asarray(cand, dtype=np.float64).reshape(-1, 3) @ np.asarray(rot, dtype=np.float64).reshape(3, 3),
                     axes, alpha, amplitude)
    fg = float((f * g).sum())
    return fg / (float((f * f).sum()) + float((g * g).sum()) - fg)
