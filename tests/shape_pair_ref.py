"""Plain fp64 restatement of `mcg_shape_pair_tanimoto` (csrc/mcg_shape_pair.hip), stage by stage.  Host only (numpy), written
from the formulas in that file's header; no import of the package.

  density   F[b][g] = 1 - prod_a (1 - A exp(-alpha |p_g - y_a|^2)),  y = (x - t) @ M, p_g point g of
            meshgrid(axes[0], axes[1], axes[2], indexing="ij") in flatten order; NaN over the real columns of a row without
            atoms; +0 on the padded columns n^3 <= g < Gp.
  Gram      G = F F^T.  The kernel cuts Gp into 4 ranges of L = Gp / 4 (one per wave), walks a range in blocks of 32 and
            combines the four range sums as (p0 + p1) + (p2 + p3); `gram_parts` states the four range sums so that the
            mutations below can be planted, `gram` adds them.
  Tanimoto  T = G / (G_ii + G_jj - G).

Error unit of the density.  A point's fp32 density is off by the rounding of every factor 1 - A e_a (e_a = exp(-alpha d_a^2)),
carried by the product of the others:
    unit(p) = 2^-24 (1 + sum_a (3 + alpha d_a^2) A e_a prod_{b != a} |1 - A e_b|).
The 3 is one ulp for the factor's own rounding and two for the hardware exponential; alpha d_a^2 is the condition of the
exponential on its fp32 argument; the leading 1 the final 1 - prod (densities are of order 1).

Measured count.  `tests/test_shape_pair_stages_host.py::test_density_error_unit_is_measured_on_the_host` evaluates the density
in numpy float32 in the operation order of `mcg_shape::rotate_row` and `density_at` (fused products emulated in fp64, the
exponential correctly rounded) over both grids of `shape_pair_cases.GRIDS`, every grid size, both transforms and the
molecules of `shape_pair_cases.STAGE_BATCH`, and prints max |fp32 - fp64| / unit per grid:

    python -m pytest tests/test_shape_pair_stages_host.py -k measured -s

MEASURED_UNITS records it; the GPU tolerance is 4 x that (`shape_ref.TOL_UNITS`' convention: two fp32 evaluations may lie on
opposite sides of fp64, and the hardware exponential differs from the host's).  The measurement is of the emulation against
this restatement, never of the kernel.  It gave
    box     1.07 under "identity", 1.41 under "moved" (the rounding of x - t at coordinates of a few angstroms, which the unit
            does not model, adds to it);
    cloud   3.88 under both: atoms up to 8 A from a point, where alpha d^2 reaches 50 and the roundings of d^2 itself (three
            differences, three products, two sums and the product with alpha: about 5 x 2^-24 of it) outweigh the one
            2^-24 alpha d^2 that the unit grants.
"pair_density" is the maximum over all cases, 3.89; the checks on the box use the box's own, smaller count ("pair_density_box",
1.42), so the wide grid does not loosen them.

Gram bound.  Against the fp64 Gram of the SAME fp32 densities: every element is an fp32 sum of Gp unfused or fused products in
some order of depth at most L + 2 (a chain of L, then two adds), so
    |G_ij - sum_k F_ik F_jk| <= 2 (L + 2) 2^-24 sum_k |F_ik F_jk|         (`gram_bound`)
whatever the order: one rounding per product, L + 1 per partial sum chain, first order doubled.  Nothing is measured.

Measured on an MI355X (worst error / allowed, `tests/test_shape_pair_stages_gpu.py -s`): see GPU_WORST below."""
from __future__ import annotations

import functools
from typing import Optional, Tuple

import numpy as np

import shape_pair_cases as C
from shape_ref import AMPLITUDE, get_alpha

ALPHA = get_alpha()

EPS32 = 2.0 ** -24

# max |fp32 emulation - fp64| / unit over all cases (see the module docstring for the command).
MEASURED_UNITS = {"pair_density": 3.89, "pair_density_box": 1.42}
TOL_UNITS = {k: 4.0 * v for k, v in MEASURED_UNITS.items()}



def density_tol_units(grid: str) -> float:
    """The GPU tolerance of a density on `grid`, in units of `density_unit`."""
    return TOL_UNITS["pair_density_box" if grid == "box" else "pair_density"]


# Worst error / allowed printed by the GPU stage tests on an MI355X (gfx950).
GPU_WORST = {
    "density / tolerance, box": 0.254,            # n = 13 and 16, "moved"; 0.191 under "identity"
    "density / tolerance, cloud": 0.250,          # n = 13, "moved"; 0.249 under "identity"
    "gram / bound, stage batch, box": 0.0348,     # n = 5 (L = 32); 0.0036 at n = 16 (L = 1024)
    "gram / bound, stage batch, cloud": 0.0634,   # n = 5; 0.0126 at n = 16
    "gram / bound, tile-edge batches": 0.0496,    # n = 5; 0.0104 at n = 13
    "gram / bound, natural batches": 0.0562,      # B = 992; 0.0503 at 993, 0.0514 at 1985
    "field kernel / quotient bound": 0.0197,      # n = 5
    "pair kernel / quotient bound": 0.0281,       # n = 5
}

DENSITY_MUTATIONS: Tuple[str, ...] = (
    "swap_iy_iz",            # grid point idx takes axes[1][iz] and axes[2][iy]
    "drop_last_atom",        # a row scored on its first n - 1 atoms
    "keep_t",                # y = x @ M: t not subtracted
    "transpose_m",           # y = (x - t) @ M^T
    "pad_nonzero",           # the padded columns repeat the row's last real column
)
GRAM_MUTATIONS: Tuple[str, ...] = (
    "drop_kblock",           # one 32-point block of one wave's range left out         (which = (wave, block))
    "drop_wave",             # one wave's whole range left out                         (which = wave)
    "combine_twice",         # the combine reads slot `src` where it should read `dst` (which = (dst, src))
    "unmirrored",            # (i, j), i > j, of a diagonal tile keeps what the buffer held (which = (tile rows, i, j))
)
MUTATIONS = DENSITY_MUTATIONS + GRAM_MUTATIONS


# ------------------------------------------------------------------------------------------------- density
def grid_points(axes: np.ndarray, mutation: Optional[str] = None) -> np.ndarray:
    """[n^3, 3] fp64: the points of meshgrid(indexing="ij") in flatten order."""
    ax = np.asarray(axes, dtype=np.float64)
    ix, iy, iz = (k.ravel() for k in np.meshgrid(*(np.arange(ax.shape[1]),) * 3, indexing="ij"))
    if mutation == "swap_iy_iz":
        iy, iz = iz, iy
    return np.stack([ax[0][ix], ax[1][iy], ax[2][iz]], axis=1)


def frame_coords(x: np.ndarray, M: np.ndarray, t: np.ndarray, mutation: Optional[str] = None) -> np.ndarray:
    """y = (x - t) @ M in fp64 from the fp32 values the kernel is given."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    if mutation == "keep_t":
        t = np.zeros(3)
    if mutation == "transpose_m":
        M = M.T
    return (x - t) @ M


def _factors(y: np.ndarray, pts: np.ndarray, alpha: float, amp: float) -> Tuple[np.ndarray, np.ndarray]:
    """(d2 [atoms, points], A exp(-alpha d2)) in fp64."""
    d2 = ((pts[None, :, :] - y[:, None, :]) ** 2).sum(axis=2)
    return d2, amp * np.exp(-alpha * d2)


def density(x: np.ndarray, M: np.ndarray, t: np.ndarray, axes: np.ndarray, alpha: float, amp: float,
            mutation: Optional[str] = None) -> np.ndarray:
    """[n^3] fp64 density of the atoms x [n_atoms, 3] (at least one) on the grid of `axes`."""
    y = frame_coords(x, M, t, mutation)
    if mutation == "drop_last_atom":
        y = y[:-1]
    _, e = _factors(y, grid_points(axes, mutation), alpha, amp)
    return 1.0 - np.prod(1.0 - e, axis=0)


def density_unit(x: np.ndarray, M: np.ndarray, t: np.ndarray, axes: np.ndarray, alpha: float, amp: float) -> np.ndarray:
    """[n^3] fp64: unit(p) of the module docstring."""
    y = frame_coords(x, M, t)
    d2, e = _factors(y, grid_points(axes), alpha, amp)
    f = np.abs(1.0 - e)
    before = np.ones_like(f)                               # prod_{b < a} and prod_{b > a}: the product without factor a
    after = np.ones_like(f)
    for a in range(1, f.shape[0]):
        before[a] = before[a - 1] * f[a - 1]
        after[-1 - a] = after[-a] * f[-a]
    return EPS32 * (1.0 + ((3.0 + alpha * d2) * e * before * after).sum(axis=0))


def density_rows(x: np.ndarray, n_nodes: np.ndarray, M: np.ndarray, t: np.ndarray, axes: np.ndarray, alpha: float,
                 amp: float, mutation: Optional[str] = None) -> np.ndarray:
    """F [B, Gp] fp64 as `k_pair_density` is to write it: rows x[b, : n_nodes[b]], NaN over the real columns of a row
    without atoms, +0 on the padded columns."""
    n = np.asarray(axes).shape[1]
    total, Gp = n ** 3, C.padded(n)
    F = np.zeros((x.shape[0], Gp))
    for b in range(x.shape[0]):
        k = int(n_nodes[b])
        if k == 0 or (mutation == "drop_last_atom" and k == 1):
            F[b, :total] = np.nan if k == 0 else 0.0
        else:
            F[b, :total] = density(x[b, :k], M, t, axes, alpha, amp, mutation)
        if mutation == "pad_nonzero":
            F[b, total:] = F[b, total - 1]
    return F


@functools.lru_cache(maxsize=None)
def stage_reference(n: int, name: str, grid: str = "box") -> dict:
    """The molecules of `shape_pair_cases.STAGE_BATCH` under transform `name` on the n-point grid `grid`, computed once and shared
    (read only): x [B, 64, 3], n_nodes [B], F [B, Gp] fp64 (`density_rows`), unit [B, n^3] (0 on the empty rows)."""
    x, n_nodes = C.rows(C.STAGE_BATCH, name)
    M, t = C.transform(name)
    ax = C.axes(n, grid)
    unit = np.zeros((len(C.STAGE_BATCH), n ** 3))
    for b, k in enumerate(n_nodes):
        if k > 0:
            unit[b] = density_unit(x[b, :k], M, t, ax, ALPHA, AMPLITUDE)
    out = {"x": x, "n_nodes": n_nodes, "F": density_rows(x, n_nodes, M, t, ax, ALPHA, AMPLITUDE), "unit": unit}
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------- the fp32 emulation
def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding
    that differs from fmaf in about one case in 2^29: immaterial to a measured maximum)."""
    return (_f32(a).astype(np.float64) * _f32(b).astype(np.float64) + _f32(c).astype(np.float64)).astype(np.float32)


def density_fp32(x: np.ndarray, M: np.ndarray, t: np.ndarray, axes: np.ndarray, alpha: float, amp: float) -> np.ndarray:
    """[n^3] float32: the density in the operation order of `mcg_shape::rotate_row` and `density_at`, every operation
    rounded to fp32 on its own, the exponential correctly rounded (the hardware's is not: the unit's 3 allows for it)."""
    x, m, t = _f32(x).reshape(-1, 3), _f32(M).reshape(9), _f32(t).reshape(3)
    alpha32, amp32 = np.float32(alpha), np.float32(amp)
    x0, x1, x2 = x[:, 0] - t[0], x[:, 1] - t[1], x[:, 2] - t[2]
    c = [_fma32(x2, m[6 + k], _fma32(x0, m[k], x1 * m[3 + k])) for k in range(3)]
    pts = grid_points(axes).astype(np.float32)
    prod = np.ones(pts.shape[0], dtype=np.float32)
    for a in range(x.shape[0]):
        dx, dy, dz = pts[:, 0] - c[0][a], pts[:, 1] - c[1][a], pts[:, 2] - c[2][a]
        d2 = _fma32(dy, dy, dx * dx) + dz * dz
        e = np.exp((-d2 * alpha32).astype(np.float64)).astype(np.float32)
        prod = prod * _fma32(-amp32, e, np.float32(1.0))
    assert prod.dtype == np.float32 and d2.dtype == np.float32
    return np.float32(1.0) - prod


# ------------------------------------------------------------------------------------------------- Gram and Tanimoto
def gram_parts(F: np.ndarray, mutation: Optional[str] = None, which=None) -> np.ndarray:
    """[4, B, B] fp64: the sums of F_ik F_jk over the four k ranges of L = Gp / 4."""
    F = np.asarray(F, dtype=np.float64)
    B, Gp = F.shape
    L = Gp // C.KSPLIT
    parts = np.empty((C.KSPLIT, B, B))
    for w in range(C.KSPLIT):
        lo, hi = w * L, (w + 1) * L
        keep = np.ones(L, dtype=bool)
        if mutation == "drop_kblock" and which[0] == w:
            keep[which[1] * C.KBLOCK:(which[1] + 1) * C.KBLOCK] = False
        if mutation == "drop_wave" and which == w:
            keep[:] = False
        Fw = F[:, lo:hi][:, keep]
        parts[w] = Fw @ Fw.T
    return parts


def gram(F: np.ndarray, mutation: Optional[str] = None, which=None) -> np.ndarray:
    """G [B, B] fp64 = F F^T, (p0 + p1) + (p2 + p3)."""
    p = gram_parts(F, mutation, which)
    slots = [0, 1, 2, 3]
    if mutation == "combine_twice":
        slots[which[0]] = which[1]
    G = (p[slots[0]] + p[slots[1]]) + (p[slots[2]] + p[slots[3]])
    if mutation == "unmirrored":
        rows, i, j = which
        assert i > j and i // rows == j // rows
        G[i, j] = np.nan                                      # what the tests fill the buffer with before the call
    return G


def gram_abs(F: np.ndarray) -> np.ndarray:
    """sum_k |F_ik F_jk| [B, B] fp64."""
    A = np.abs(np.asarray(F, dtype=np.float64))
    return A @ A.T


def gram_bound(F: np.ndarray) -> np.ndarray:
    """[B, B]: the most an fp32 Gram of these densities may differ from the fp64 one (module docstring)."""
    L = np.asarray(F).shape[1] // C.KSPLIT
    return 2.0 * (L + 2) * EPS32 * gram_abs(F)


def tanimoto(G: np.ndarray) -> np.ndarray:
    """T = G / (G_ii + G_jj - G), in the dtype of G."""
    d = np.diagonal(G)
    with np.errstate(invalid="ignore", divide="ignore"):
        return G / ((d[:, None] + d[None, :]) - G)


def tanimoto_bound(a: float, c: float, d: float, da: float, dc: float, dd: float) -> float:
    """How far an fp32 quotient a' / ((c' + d') - a') may lie from a / (c + d - a) when |a' - a| <= da, |c' - c| <= dc,
    |d' - d| <= dd: the worst quotient over the corners of that box (T rises with a and falls with c and d where all are
    positive), plus the quotient's own three fp32 roundings: c + d (relative to c + d = (1 + T) times the denominator), the
    subtraction and the division, (3 + T) 2^-24 of T in all, taken as 4 x 2^-24 max(T, 1)."""
    den_lo, den_hi = (c - dc) + (d - dd) - (a + da), (c + dc) + (d + dd) - (a - da)
    assert den_lo > 0.0 and a - da > 0.0
    T = a / (c + d - a)
    spread = max((a + da) / den_lo - T, T - (a - da) / den_hi)
    return spread + 4.0 * EPS32 * max(abs(T) + spread, 1.0)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """fp32 arrays equal bit for bit, any NaN counting as equal to any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
