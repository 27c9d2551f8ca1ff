"""Pose search (`interactions.search_pose`, kernels `mcg_pose_starts` and `mcg_pose_search_select`; DESIGN.md section 6 "Pose
search"): the keyed starts and the choice among the walked starts restated in fp64 numpy from the DESIGN words, and the
rules by which the kernels' values pass against the restatement.  Importing this module needs no GPU.

What is exact here (judged by equality): the Philox words (`seeding.philox4x32_10`) and the uniforms u = (w >> 8) 2^-24;
start 0; the objective J = W_after + 0.840f CLASH_after (one fp32 product, one fp32 sum); the winner; the gathered bits.

What is fp64 here and judged by a bound: the start coordinates, transform and angles; the composed transform; the RMSDs.
The bounds are linear error counts with u = 2^-24, derived below in the way `flex_pose_ref.drift_bound` and `gemm_ref`
derive theirs; no number in them is fitted.  The library functions' errors are HIP's documented maxima for the device
math functions: sinf 1 ulp and cosf 1 ulp (the rule uses `pose_optimise_ref.SINCOS_ULP` = 2, no smaller), cbrtf 2 ulp,
sqrtf and the division correctly rounded.  One ulp of a value v is at most 2 u |v|.

A point of the sphere   z = 2 u0 - 1 is exact (u0 has 24 bits).  phi = 2 pi u1: one rounding, |phi| <= 2 pi, so cos and sin
                        carry 2 pi u from phi, 2 SINCOS_ULP u of their own.  r = sqrt(max(1 - z^2, 0)): z^2 and the
                        difference one rounding each (2 u absolute), the root halves the relative error and adds u:
                        e_r = 2 u / max(2 r, sqrt(2 u)) + u.  A component r cos(phi): e_r + r (2 pi + 2 SINCOS_ULP + 1) u.
                        E_POINT(u0) is the largest of the three.
The rotation R_s        theta = max_turn u2: u pi.  An entry of D = (delta + s K) + c1 K2 (`rodrigues_row`), |s| <= 1,
                        c1 <= 2: s K carries (pi + 2 SINCOS_ULP + 1) u + E_POINT, c1 K2 carries (pi + 2 SINCOS_ULP + 1) u
                        for c1 and 2 (2 E_POINT + 3 u) for K2 (two products and a sum of axis components), the two sums
                        2 u more: E_D.  I @ D is exact but for the signs of zero; Gram-Schmidt of a matrix within E_D of a
                        rotation moves an entry by at most 6 E_D + 12 u (two normalisations, one projection, one cross
                        product): E_R = 7 E_D + 12 u.
The shift               len = spread cbrt(u2): (2 CBRT_ULP + 1) u spread; p = c + len dir: spread (E_POINT + (2 CBRT_ULP
                        + 2) u) + u |p| + e_c, e_c = (n + 1) u max|x| the centroid's own error (n - 1 sums, a division).
A torsion turn          theta_k = 2 pi u - pi: a rounded product and a rounded difference, 3 pi u.  The turn is
                        `turn_about_line`: for a point at distance r from b, the difference u r, the axis 3.5 u per
                        component (`pose_optimise_ref`), an entry of D (3 pi + 2 SINCOS_ULP + 1) u (1 + 2) + 3.5 u (1 + 4)
                        + 11 u =: E_TURN_D, the row product 3 r E_TURN_D + 3 u r, the sum with b u (r + |b|):
                        TURN = 3 E_TURN_D / u + 5 roundings of the lever.  As `flex_pose_ref.drift_bound`, the bound is
                        LINEAR: lever = 2 rho0 the largest distance inside the molecule, times the torsions used (every
                        earlier turn also moves the axis of a later one); the amplification of an earlier error by a later
                        axis is second order in u and left out, as there.
A start's coordinate    x_s = q' @ R_s + p: eps_q = e_c + u max|x| + TURN u lever used; the row product 3 rho (E_R + u);
                        the sum u |x_s|: `start_bound`.  The transform: R by E_R, t = p - c @ R_s by the shift's bound +
                        3 |c|_max (E_R + u) + u |t|.  The angles: 3 pi u.
The composed transform  R = R_s @ G_w, t = t_s @ G_w + t_w from the DEVICE'S OWN fp32 factors: three rounded products and
                        two rounded sums per entry.  The entries of a rotation are at most 1: 3 u for the products, 2 x 2 u
                        for the sums, 7 u.  For t the products are at most |t_s|_max each (3 u |t_s|), the partial sums 2
                        and 3 |t_s| (5 u |t_s|) and the last sum 3 |t_s| + |t_w|: u (11 |t_s|_max + |t_w|_max).
The RMSDs               a difference of coordinates u (|a| + |b|), squares and sums (n + 4) u relative, the root: against
                        the fp64 value from the device's own coordinates, 2 u (max|x_out| + max|x_in|) + (n + 6) u rms.
                        The conformer RMSD first takes x_out back through the composed map: 3 products and sums of
                        components of (x_out - t): 6 u (|x_out|_max + |t|_max) more per component, sqrt(3) of it in the
                        norm."""
import math

import numpy as np

import flex_pose_ref as FR
import pose_optimise_ref as PR
from ml_conformer_generator_amd import seeding

U = FR.U
F32 = np.float32
MAX_TORSIONS = FR.MAX_TORSIONS
MAX_STARTS = 64
PARAMS = 24
COUNTER_WORD = 0xFFFFFFFE
SINCOS_ULP = PR.SINCOS_ULP
CBRT_ULP = 2.0
W_REP32 = F32(0.840)
E_TURN_D = ((3 * math.pi + 2 * SINCOS_ULP + 1) * 3 + 3.5 * 5 + 11) * U
TURN = 3 * E_TURN_D / U + 5
# worst error / bound at factor 1 on the MI355X over tests/test_pose_search_gpu.py ("Pose search"); recorded, not
# used by any rule: the rules are the bounds themselves
MEASURED = dict(start_xyz=0.0426, start_R=0.0125, start_t=0.0079, start_angles=0.556, composed=0.192, rmsd=0.080,
                conformer_rmsd=0.0096)


class Rules:
    """The choices of the definition; the planted mistakes change one at a time."""
    def __init__(self, **kw):
        self.counter_word = COUNTER_WORD
        self.torsion_order = "ascending"
        self.axes = "current"             # a torsion turns about its axis as the earlier turns left it ("input": as it came)
        self.compose = "ts@Gw"            # t = t_s @ G_w + t_w
        self.tie = "lowest"
        self.nan_wins = False
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


RULES = Rules()


# ----------------------------------------------------------------------------------------------- the uniforms
def words(seed, sample_id, s, rules=RULES):
    """[6,4] uint32: the Philox words of start s of sample `sample_id` under `seed`."""
    key = seeding.philox_key(seed)
    counters = [[int(sample_id), int(s), j, rules.counter_word] for j in range(6)]
    return seeding.philox4x32_10(counters, key)


def uniforms(seed, sample_id, s, rules=RULES):
    """[24] fp32: u = (w >> 8) 2^-24, draw j in 4 j .. 4 j + 3; zeros for start 0."""
    if s == 0:
        return np.zeros(PARAMS, dtype=F32)
    w = words(seed, sample_id, s, rules).reshape(-1)
    return ((w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(F32)


def sphere_point(u0, u1):
    z = 2.0 * float(u0) - 1.0
    phi = 2.0 * math.pi * float(u1)
    r = math.sqrt(max(1.0 - z * z, 0.0))
    return np.array([r * math.cos(phi), r * math.sin(phi), z])


def rotation_row_form(axis, theta):
    """D with r' = r @ D: the transpose of Rodrigues' matrix about the unit `axis`."""
    n = np.asarray(axis, dtype=np.float64)
    Km = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return (np.eye(3) + math.sin(theta) * Km + (1 - math.cos(theta)) * (Km @ Km)).T


# ----------------------------------------------------------------------------------------------- one start
def start(x, t, seed, sample_id, s, spread, max_turn, rules=RULES):
    """Start s of the row x [n,3] fp32 with the tree t (`flex_pose_ref.tree`): dict coords [n,3], R [3,3], t [3], angles
    [16] in fp64 and u [24] fp32.  Start 0 is the input."""
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    n = len(x)
    u = uniforms(seed, sample_id, s, rules)
    if n == 0 or not np.isfinite(x).all():
        return dict(coords=x.astype(np.float64), R=np.full((3, 3), np.nan), t=np.full(3, np.nan),
                    angles=np.full(MAX_TORSIONS, np.nan), u=u)
    if s == 0:
        return dict(coords=x.astype(np.float64), R=np.eye(3), t=np.zeros(3), angles=np.zeros(MAX_TORSIONS), u=u)
    xd = x.astype(np.float64)
    c = xd.mean(axis=0)
    q = xd - c
    used = t["used"]
    theta = np.zeros(MAX_TORSIONS)
    theta[:used] = 2.0 * math.pi * u[8: 8 + used].astype(np.float64) - math.pi
    order = range(used) if rules.torsion_order == "ascending" else range(used - 1, -1, -1)
    q_in = q.copy()
    for k in order:
        one = np.zeros(MAX_TORSIONS)
        one[k] = theta[k]
        if rules.axes == "current":
            q = FR.twist(q, one, t)
        else:                             # the planted mistake: the axis and its foot taken from the input
            a, b = t["torsions"][k]
            n = (q_in[b] - q_in[a]) / np.linalg.norm(q_in[b] - q_in[a])
            D = rotation_row_form(n, theta[k])
            for i in sorted(t["sides"][k]):
                q[i] = (q[i] - q_in[b]) @ D + q_in[b]
    R = rotation_row_form(sphere_point(u[0], u[1]), float(max_turn) * float(u[2]))
    d = float(spread) * float(u[6]) ** (1.0 / 3.0) * sphere_point(u[4], u[5])
    p = c + d
    return dict(coords=q @ R + p, R=R, t=p - c @ R, angles=theta, u=u)


def e_point(u0):
    z = 2.0 * float(u0) - 1.0
    r = math.sqrt(max(1.0 - z * z, 0.0))
    e_r = 2 * U / max(2 * r, math.sqrt(2 * U)) + U
    return max(e_r + r * (2 * math.pi + 2 * SINCOS_ULP + 1) * U, U)


def start_bound(x, t, u, spread, s):
    """dict of bounds (coords, R, t, angles) for start s >= 1 of the row x with the uniforms u - the docstring's counts."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    if s == 0 or len(x) == 0 or not np.isfinite(x).all():
        return dict(coords=0.0, R=0.0, t=0.0, angles=0.0)
    n = len(x)
    xmax = float(np.abs(x).max())
    c = x.mean(axis=0)
    rho = float(np.sqrt(((x - c) ** 2).sum(axis=1)).max())
    ep_axis, ep_dir = e_point(u[0]), e_point(u[4])
    e_d = ((math.pi + 2 * SINCOS_ULP + 1) * U + ep_axis) + ((math.pi + 2 * SINCOS_ULP + 1) * U + 2 * (2 * ep_axis + 3 * U)) \
        + 2 * U
    e_r = 7 * e_d + 12 * U
    e_c = (n + 1) * U * xmax
    pmax = float(np.abs(c).max()) + float(spread)
    e_p = float(spread) * (ep_dir + (2 * CBRT_ULP + 2) * U) + U * pmax + e_c
    eps_q = e_c + U * xmax + TURN * U * (2 * rho) * t["used"]
    e_x = eps_q + 3 * rho * (e_r + U) + e_p + U * (rho + pmax)
    e_t = e_p + 3 * float(np.abs(c).max()) * (e_r + U) + U * (pmax + 3 * float(np.abs(c).max()))
    return dict(coords=e_x, R=e_r, t=e_t, angles=3 * math.pi * U)


# ----------------------------------------------------------------------------------------------- the choice
def objective(w_after, c_after):
    """J = W_after + 0.840f CLASH_after: one fp32 product, one fp32 sum."""
    with np.errstate(all="ignore"):
        return F32(F32(w_after) + F32(W_REP32 * F32(c_after)))


def choose(J, rules=RULES):
    """The winner among J [S] fp32: the smallest finite one, a tie to the lowest s; -1 where none is finite."""
    best, jb = -1, None
    for s, j in enumerate(np.asarray(J, dtype=F32)):
        if not np.isfinite(j) and not (rules.nan_wins and np.isnan(j)):
            continue
        if best < 0 or (np.isnan(j) and rules.nan_wins) or j < jb or (rules.tie == "highest" and j == jb):
            best, jb = s, j
    return best


def compose(start_xform, walk_xform, rules=RULES):
    """[12] fp64: the start's map followed by the walk's, R = R_s @ G_w, t = t_s @ G_w + t_w."""
    a, b = np.asarray(start_xform, dtype=np.float64), np.asarray(walk_xform, dtype=np.float64)
    Rs, ts, Gw, tw = a[:9].reshape(3, 3), a[9:], b[:9].reshape(3, 3), b[9:]
    t = ts @ Gw + tw if rules.compose == "ts@Gw" else tw @ Rs + ts
    return np.concatenate([(Rs @ Gw).reshape(9), t])


def compose_bound(start_xform, walk_xform):
    """(bound on an entry of R, bound on an entry of t) - the docstring's counts."""
    ts = float(np.abs(np.asarray(start_xform, dtype=np.float64)[9:]).max())
    tw = float(np.abs(np.asarray(walk_xform, dtype=np.float64)[9:]).max())
    return 7 * U, U * (11 * ts + tw)


def rmsds(x_in, x_out, xform):
    """(rmsd, conformer_rmsd) in fp64 of the input against the output, the second with the output taken back through
    x' = x @ R + t."""
    a, b = np.asarray(x_in, dtype=np.float64).reshape(-1, 3), np.asarray(x_out, dtype=np.float64).reshape(-1, 3)
    m = np.asarray(xform, dtype=np.float64)
    back = (b - m[9:]) @ m[:9].reshape(3, 3).T
    return math.sqrt(float(((b - a) ** 2).sum() / len(a))), math.sqrt(float(((back - a) ** 2).sum() / len(a)))


def rmsd_bounds(x_in, x_out, xform, rms, crms):
    a, b = np.asarray(x_in, dtype=np.float64), np.asarray(x_out, dtype=np.float64)
    n = len(a.reshape(-1, 3))
    size = float(np.abs(a).max()) + float(np.abs(b).max())
    tmax = float(np.abs(np.asarray(xform, dtype=np.float64)[9:]).max())
    plain = math.sqrt(3) * 2 * U * size + (n + 6) * U * rms
    return plain, plain + math.sqrt(3) * 6 * U * (float(np.abs(b).max()) + tmax) + (n + 6) * U * crms


def select(walk_coords, walk_xform, walk_stats, walk_angles, start_xform, start_angles, x_in, n, rules=RULES):
    """The choice restated: dict best, scores [S] fp32, and for the winner coords (bits), xform, angles, stats (fp64 where the
    kernel computes, the walk's own values where it gathers)."""
    S = len(walk_stats)
    J = np.array([objective(walk_stats[s][1], walk_stats[s][7]) for s in range(S)], dtype=F32)
    best = choose(J, rules)
    w = max(best, 0)
    if best <= 0:
        return dict(best=best, scores=J, coords=walk_coords[w], xform=np.asarray(walk_xform[w], dtype=np.float64),
                    angles=np.asarray(walk_angles[w], dtype=np.float64), stats=np.asarray(walk_stats[w], dtype=np.float64),
                    gathered=True)
    xf = compose(start_xform[w], walk_xform[w], rules)
    st = np.asarray(walk_stats[w], dtype=np.float64).copy()
    st[0], st[6] = walk_stats[0][0], walk_stats[0][6]
    st[4], st[9] = rmsds(np.asarray(x_in)[:n], np.asarray(walk_coords[w])[:n], xf)
    st[10] = st[11] = 0.0
    return dict(best=best, scores=J, coords=walk_coords[w], xform=xf, stats=st, gathered=False,
                angles=np.asarray(start_angles[w], dtype=np.float64) + np.asarray(walk_angles[w], dtype=np.float64))


# ----------------------------------------------------------------------------------------------- the pass rules
def starts_pass(got, want, bound):
    """Every violation (strings; empty = passes) of one start's device values `got` (coords [n,3], xform [12], angles [16])
    against `want` = start(...) under `bound` = start_bound(...); also the worst error / bound per value."""
    bad, ratios = [], {}

    def judge(key, g, w, b):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        if np.isnan(w).all() and w.size:
            if not np.isnan(g).all():
                bad.append(f"{key}: NaN expected")
            return
        if not np.isfinite(w).all():          # a row with a non-finite coordinate comes back as it came
            if not np.array_equal(g, w, equal_nan=True):
                bad.append(f"{key}: the row did not come back as it came")
            return
        err = float(np.abs(g - w).max()) if g.size else 0.0
        ratios[key] = err / b if b > 0 else (0.0 if err == 0 else math.inf)
        if not err <= b:
            bad.append(f"{key}: off by {err:.3e}, bound {b:.3e}")

    n = len(want["coords"])
    judge("start_xyz", np.asarray(got["coords"])[:n], want["coords"], bound["coords"])
    judge("start_R", np.asarray(got["xform"])[:9], np.asarray(want["R"]).reshape(9), bound["R"])
    judge("start_t", np.asarray(got["xform"])[9:], want["t"], bound["t"])
    judge("start_angles", got["angles"], want["angles"], bound["angles"])
    return bad, ratios
