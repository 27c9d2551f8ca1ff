"""An fp64 numpy restatement of the blocked-ray masks of include/mlconfgen_hip_pocket.h, written from the definition and
nothing else, with the margin of every (point, test) pair: how far, in squared angstrom, the nearest atom's decision is from
flipping.  `Rules` plants the mistakes tests/test_pocket_host.py must catch."""
import dataclasses

import numpy as np

OCCUPIED = np.uint32(1 << 31)


@dataclasses.dataclass(frozen=True)
class Rules:
    clamp: bool = True            # t_c = min(max(t, 0), reach); False: t_c = t (an infinite line)
    probe_in_occupancy: bool = True
    dropped_direction: int = -1   # a direction whose bit is never set


def directions():
    d = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)],
                 dtype=np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def grid_points(n, spacing):
    ax = (np.arange(n, dtype=np.float64) - (n - 1) / 2) * spacing
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


FAR_MARGIN = 0.5              # squared angstrom: what every margin is capped at (see `masks`)
_NEAR_PAD = 0.25              # angstrom


def masks(xyz, r, n, spacing, probe, reach, rules=Rules(), chunk=128):
    """(masks [n^3] uint32, margin [n^3,27] fp64) of the grid of n^3 points round the origin against atoms `xyz` [R,3]
    (centre-relative) of radii `r` [R]: columns 0..25 of the margin are min over atoms of | |e|^2 - r^2 | per direction,
    column 26 is min over atoms of | |d|^2 - (r + probe)^2 |, each capped at FAR_MARGIN.
    Only the pairs with |d| <= max(reach, probe) + r + 0.25 are evaluated.  A pair beyond sets no bit (a blocked ray needs
    |d| <= reach + r, an occupied point |d| < r + probe) and its margins exceed (r + 0.25)^2 - r^2 > FAR_MARGIN for r >= 1,
    so the capped minimum is exact.  (The planted `clamp=False` line is infinite: its far pairs are left out too, which only
    makes the planted mistake smaller.)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    U = directions()
    pts = grid_points(n, spacing)
    P = pts.shape[0]
    out = np.zeros(P, dtype=np.uint32)
    margin = np.full((P, 27), FAR_MARGIN)
    if xyz.shape[0] == 0:
        return out, margin
    assert float(r.min()) >= 1.0
    ro = r + (probe if rules.probe_in_occupancy else 0.0)
    lim = max(reach, probe) + r + _NEAR_PAD
    bits = (np.uint32(1) << np.arange(26, dtype=np.uint32))
    if rules.dropped_direction >= 0:
        bits[rules.dropped_direction] = 0
    for s in range(0, P, chunk):
        p = pts[s: s + chunk]
        d_all = xyz[None, :, :] - p[:, None, :]                               # [p,R,3]
        near = (d_all * d_all).sum(-1) <= (lim * lim)[None, :]
        pi, ai = np.nonzero(near)                                             # sorted by point
        if pi.size == 0:
            continue
        d = d_all[pi, ai]                                                     # [m,3]
        d2 = (d * d).sum(-1)
        mo = d2 - ro[ai] ** 2
        t = d @ U.T                                                           # [m,26]
        tc = np.clip(t, 0.0, reach) if rules.clamp else t
        e = d[:, None, :] - tc[:, :, None] * U[None, :, :]                    # [m,26,3]: |e|^2 from e, never expanded
        mr = (e * e).sum(-1) - (r[ai] ** 2)[:, None]
        first = np.flatnonzero(np.r_[True, pi[1:] != pi[:-1]])                # segment starts: one per point with pairs
        rows = s + pi[first]
        margin[rows, :26] = np.minimum(np.minimum.reduceat(np.abs(mr), first, axis=0), FAR_MARGIN)
        margin[rows, 26] = np.minimum(np.minimum.reduceat(np.abs(mo), first), FAR_MARGIN)
        blocked = np.logical_or.reduceat(mr <= 0, first, axis=0)              # [rows,26]
        occ = np.logical_or.reduceat(mo < 0, first)
        out[rows] = (blocked * bits[None, :]).sum(axis=1, dtype=np.uint32) | np.where(occ, OCCUPIED, np.uint32(0))
    return out, margin


def differing_pairs(a, b):
    """[P,27] bool: which (point, test) pairs two mask arrays disagree on (column 26: the occupied bit)."""
    x = np.asarray(a).astype(np.uint32) ^ np.asarray(b).astype(np.uint32)
    cols = [(x >> np.uint32(k)) & np.uint32(1) for k in range(26)] + [(x >> np.uint32(31)) & np.uint32(1)]
    return np.stack(cols, axis=1).astype(bool)


def compare(got, want, margin, eps):
    """(wrong, left_out): the number of (point, test) pairs with a margin of at least `eps` on which `got` differs from the
    restatement's `want`, and the share of all pairs whose margin is below `eps` (not compared)."""
    checked = np.asarray(margin) >= eps
    return int((differing_pairs(got, want) & checked).sum()), float(1.0 - checked.mean())
