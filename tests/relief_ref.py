"""Clash relief (`receptor.relieve_clashes`, DESIGN.md section 6 "Clash relief"): the definition restated in fp64, the
synthetic cases of the tests and the rule by which an fp32 penalty, force or torque passes against the restatement.

Cases: a ligand is a self-avoiding 1.5 A random walk, centred; the receptor a jittered cubic lattice (spacing 2.6 A,
sigma 0.3 A) with the points within 3.8 A of a ligand atom removed - the pocket - and those beyond 12 A of the origin
dropped, all carbon; the ligand is then rotated by 0.25 rad about a random axis and shifted by 0.8-2.0 A so that it
clashes.  Seeds are fixed; every array is fp32, and the restatement reads those fp32 values in fp64.

The pass rule (`bounds`): with u = 2^-24 the unit roundoff, a pair's contact depth h = s - d, s = (r_i - margin) + r_j,
carries the absolute fp32 error
    delta = u (2 sqrt(3) M + (sqrt(3) + 2) D + 3 S)
  - the pose is formed as (x - c) + p: two roundings per component, each at most u M with M the largest coordinate
    magnitude present (ligand, its centroid, the receptor atoms in reach), so a component of x' is off by <= 2 u M, and so
    is, after the rounded subtraction x' - y (one more u |d_c|), a component of the difference: the distance moves by at
    most the norm of that, sqrt(3) (2 u M + u D), D the largest distance of a counted pair;
  - d^2 is three rounded products and two rounded sums, (1 + u)^3 on every term, and the square root halves the relative
    error and adds its own u / 2: 2 u D;
  - s is two rounded sums of magnitudes <= S = max r_i + max r_j, and h = s - d one more: 3 u S.
The pairs counted are those with h > -delta (a pair the fp32 code may see in contact).  A penalty term h^2 is then off by
at most 2 h delta + delta^2; a force term 2 h e (e the unit vector, whose components move by at most 2 delta / d) by
2 delta + 4 h delta / d + 6 u h (three more roundings: h + h over d, times the component); a torque term a x f, |a| <= rho
the ligand's radius about its centroid, by 2 rho times the force term's bound plus 2 |f| da + 4 u rho |f|, where
da = u (2 rho + (n + 2) M) covers the fp32 centroid (n rounded additions of magnitudes <= n M, over n) and the roundings of
a.  To the sum of these the summation error is added: every term goes through at most K = (counted pairs) + 8 rounded
additions - a lane's own chain, the six butterfly levels of its wave and the two levels of the tree - so K u sum |term|.
"""
import math

import numpy as np
import torch

from ml_conformer_generator_amd import receptor as RC

U = 2.0 ** -24
MARGIN = float(np.float32(RC.RELIEF_MARGIN))          # what the kernel is handed
CARBON = float(np.float32(RC.vdw_radius(6)))
STEP_ROT, STEP_TRANS, GROW, SHRINK = float(np.float32(0.05)), 0.25, float(np.float32(1.2)), 0.5
TILE = 256


# ----------------------------------------------------------------------------------------------- the cases
def ligand(n, g):
    """n points of a self-avoiding random walk with 1.5 A steps (no two points closer than 1.3 A but neighbours), centred."""
    pts = [np.zeros(3)]
    while len(pts) < n:
        for _ in range(200):
            v = g.normal(size=3)
            q = pts[-1] + 1.5 * v / np.linalg.norm(v)
            if all(np.linalg.norm(q - p) >= 1.3 for p in pts[:-1]):
                pts.append(q)
                break
        else:                                  # boxed in: start over from the first point outwards
            pts = [np.zeros(3)]
    x = np.array(pts)
    return x - x.mean(0)


def pocket(lig, g, extent=12.0):
    """The carved lattice around `lig`: [R,3], a few hundred points."""
    k = int(math.ceil(extent / 2.6)) + 1
    axis = np.arange(-k, k + 1) * 2.6
    pts = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3) + g.normal(size=((2 * k + 1) ** 3, 3)) * 0.3
    pts = pts[np.linalg.norm(pts, axis=1) <= extent]
    near = np.linalg.norm(pts[:, None, :] - lig[None, :, :], axis=2).min(axis=1)
    return pts[near > 3.8]


def displaced(lig, g):
    """`lig` rotated by 0.25 rad about a random axis through the origin and shifted by 0.8-2.0 A in a random direction."""
    a = g.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    rot = np.eye(3) + math.sin(0.25) * K + (1 - math.cos(0.25)) * (K @ K)
    v = g.normal(size=3)
    return lig @ rot.T + g.uniform(0.8, 2.0) * v / np.linalg.norm(v)


class Case:
    """One ligand in one receptor: `x` [n,3] fp32, `z` [n], `rec` [R,3] fp32, `rec_z` [R] (all carbon)."""
    def __init__(self, name, seed, n, R=None, slab=False):
        g = np.random.default_rng(seed)
        lig = ligand(n, g)
        rec = pocket(lig, g)
        x = displaced(lig, g)
        if R is not None:                      # the R pocket atoms nearest to the displaced ligand
            near = np.linalg.norm(rec[:, None, :] - x[None, :, :], axis=2).min(axis=1)
            rec = rec[np.argsort(near, kind="stable")[:R]]
            assert rec.shape[0] == R, (name, rec.shape)
        if slab:                               # a far slab, 40 A away: whole tiles of it are out of reach
            ax = np.arange(-10, 10) * 2.6
            far = np.stack(np.meshgrid(ax, ax, np.array([40.0, 42.6]), indexing="ij"), -1).reshape(-1, 3)
            rec = np.concatenate([rec[: len(rec) // 2], far + g.normal(size=far.shape) * 0.3, rec[len(rec) // 2:]])
        self.name, self.n = name, n
        self.x = x.astype(np.float32)
        self.z = np.full(n, 6, dtype=np.int64)
        self.rec = rec.astype(np.float32)
        self.rec_z = np.full(len(rec), 6, dtype=np.int64)

    @property
    def receptor(self):
        return torch.from_numpy(self.rec), torch.from_numpy(self.rec_z)

    def radii(self):
        return np.full(self.n, CARBON), np.full(len(self.rec), CARBON)

    def __repr__(self):
        return f"Case({self.name}: n={self.n}, R={len(self.rec)})"


def cases():
    """The cases of the tests: ligand sizes 1, 3, 41, 64 and more, receptor sizes 1, 255, 256, 257 and a multi-tile one;
    "clean" is displaced like the others and happens to touch nothing (P = 0 at the start), every other case clashes."""
    return [Case("n1", 108, 1), Case("n3", 201, 3), Case("n41", 301, 41), Case("n64", 401, 64),
            Case("R1", 506, 12, R=1), Case("R255", 601, 20, R=255), Case("R256", 701, 20, R=256),
            Case("R257", 801, 20, R=257), Case("multi", 901, 30, slab=True), Case("clean", 1005, 5),
            Case("n8", 1101, 8), Case("n17", 1201, 17), Case("n26", 1301, 26), Case("n39", 1401, 39)]


def pad(case_list, width):
    """(coords [B,width,3] fp32 with junk in the padded rows, n_nodes [B] int32, atomic numbers [B,width]) of cases."""
    B = len(case_list)
    x = np.full((B, width, 3), 7.5, dtype=np.float32)
    z = np.full((B, width), 8, dtype=np.int64)
    for b, c in enumerate(case_list):
        x[b, : c.n], z[b, : c.n] = c.x, c.z
    return torch.from_numpy(x), torch.tensor([c.n for c in case_list], dtype=torch.int32), torch.from_numpy(z)


# ----------------------------------------------------------------------------------------------- the restatement
def pairs(x, ri, y, rj, margin=MARGIN):
    """(h [n,R] signed depth s - d, d [n,R], diff [n,R,3] = x_i - y_j) in fp64; s = (r_i - margin) + r_j."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    diff = x[:, None, :] - y[None, :, :]
    d = np.sqrt((diff ** 2).sum(-1))
    return ((np.asarray(ri, dtype=np.float64)[:, None] - margin) + np.asarray(rj, dtype=np.float64)[None, :]) - d, d, diff


def seven(x, ri, y, rj, p=None, margin=MARGIN):
    """[7] fp64: P, net force, torque about `p` (default: the atom centroid of x)."""
    x = np.asarray(x, dtype=np.float64)
    h, d, diff = pairs(x, ri, y, rj, margin)
    h = np.maximum(h, 0.0)
    unit = np.divide(diff, d[..., None], out=np.zeros_like(diff), where=d[..., None] > 0)
    f = (2.0 * h[..., None] * unit).sum(1)                       # F_i
    p = x.mean(0) if p is None else p
    return np.concatenate([[(h ** 2).sum()], f.sum(0), np.cross(x - p, f).sum(0)])


def _rodrigues_row(axis, theta):
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return (np.eye(3) + math.sin(theta) * K + (1 - math.cos(theta)) * (K @ K)).T


def _orthonormal(G):
    a = G[0] / np.linalg.norm(G[0])
    b = G[1] - (a @ G[1]) * a
    b /= np.linalg.norm(b)
    return np.stack([a, b, np.cross(a, b)])


def walk(x, ri, y, rj, steps, max_shift=RC.RELIEF_MAX_SHIFT, margin=MARGIN):
    """The descent in fp64: dict(coords, rotation, translation, penalty [P after every trial, the start first], accepted,
    trials).  x' = (x - c) @ G + p from G = I, p = c; the step rule of `receptor.py`'s docstring."""
    x = np.asarray(x, dtype=np.float64)
    c = x.mean(0)
    r = x - c
    G, p = np.eye(3), c.copy()
    cur = seven(r @ G + p, ri, y, rj, p, margin)
    sr, st, accepted, trials, hist = STEP_ROT, STEP_TRANS, 0, 0, [cur[0]]
    for _ in range(steps):
        if cur[0] == 0.0:
            break
        trials += 1
        fn, tn = np.linalg.norm(cur[1:4]), np.linalg.norm(cur[4:7])
        Gn = _orthonormal(G @ _rodrigues_row(cur[4:7] / tn, sr)) if tn > 0 else G
        pn = p + st * cur[1:4] / fn if fn > 0 else p
        take = np.linalg.norm(pn - c) <= max_shift
        if take:
            nxt = seven(r @ Gn + pn, ri, y, rj, pn, margin)
            take = nxt[0] < cur[0]
        if take:
            G, p, cur, sr, st, accepted = Gn, pn, nxt, sr * GROW, st * GROW, accepted + 1
        else:
            sr, st = sr * SHRINK, st * SHRINK
        hist.append(cur[0])
    return dict(coords=r @ G + p, rotation=G, translation=p - c @ G, penalty=hist, accepted=accepted, trials=trials)


# ----------------------------------------------------------------------------------------------- the pass rule
def bounds(x, ri, y, rj, margin=MARGIN):
    """[7] fp64: how far the fp32 sums (P, force, torque) of the pose `x` may lie from `seven(x, ...)`, by the derivation
    of this module's docstring."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    h, d, _ = pairs(x, ri, y, rj, margin)
    S = float(np.max(ri) + np.max(rj))
    reach = d <= S + 1.0                                           # what can come into contact at all
    if not reach.any():
        return np.zeros(7)
    M = max(float(np.abs(x).max()), float(np.abs(y[reach.any(axis=0)]).max()))
    D = S + 1.0
    delta = U * (2 * math.sqrt(3) * M + (math.sqrt(3) + 2) * D + 3 * S)
    on = h > -delta
    hp, dd = np.maximum(h[on], 0.0), d[on]
    K = int(on.sum()) + 8
    rho = float(np.linalg.norm(x - x.mean(0), axis=1).max())
    da = U * (2 * rho + (n + 2) * M)
    p_term = 2 * hp * delta + delta ** 2
    f_term = 2 * delta + 4 * hp * delta / dd + 6 * U * hp
    t_term = 2 * rho * f_term + 2 * (2 * hp) * da + 4 * U * rho * (2 * hp)
    bp = p_term.sum() + K * U * (hp ** 2).sum()
    bf = f_term.sum() + K * U * (2 * hp).sum()
    bt = t_term.sum() + K * U * (2 * rho * 2 * hp).sum()
    return np.array([bp, bf, bf, bf, bt, bt, bt])


def check(got, x, ri, y, rj, what=""):
    """Assert the fp32 sums `got` - all seven, or the penalty alone - of the pose `x` lie inside the rule; prints the
    figures first.  Returns (err, bound)."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    want, bound = seven(x, ri, y, rj), bounds(x, ri, y, rj)
    err = np.abs(got - want[: len(got)])
    bound = bound[: len(got)]
    print(f"RELIEF {what}: P={want[0]:.6g} |F|={np.linalg.norm(want[1:4]):.4g} |tau|={np.linalg.norm(want[4:]):.4g} "
          f"err={err.max():.3g} (P {err[0]:.3g}) bound {bound.tolist()}")
    assert (err <= bound).all(), (what, err.tolist(), bound.tolist())
    return err, bound


def passes(got, x, ri, y, rj):
    return bool((np.abs(np.asarray(got, dtype=np.float64) - seven(x, ri, y, rj)) <= bounds(x, ri, y, rj)).all())
