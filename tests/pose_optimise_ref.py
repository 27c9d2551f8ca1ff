"""Optimised pose (`interactions.optimise_pose`, kernel `mcg_receptor_optimise`; DESIGN.md section 6 "Optimised pose"): the
procedure restated from the DESIGN words, and the rules by which the kernel's fp32 values pass against the restatement.

What is fp32 here, as in the definition: the pose -> coordinates step (x - c, the row-vector product with its fused
multiply-adds in the stated order, + p; the centroid summed in atom order), r2, the cut-off decision and d
(`interactions_ref.surface_distances`), the step lengths (x 1.2f / x 0.5f), the shift test and the comparison W' < W.
Everything else is fp64: the terms, their slopes, the forces, the torque, the trial formula (Rodrigues, the product, the
Gram-Schmidt pass) and the flags.

The pass rules, u = 2^-24.
  W             `interactions_ref.bounds(...)["weighted"]`, unchanged: the same sums by the same kernel text.
  F and torque  (`force_bounds`) a derived fp32 forward-error bound built like the interaction rule.  Per counted pair,
                with delta = u (8 + S) the one rounding of its size granted to d (S the largest radius sum):
                  1. delta through each slope's own largest slope: g1' = -8 d g1 has |d/dd| <= 8 (at d = 0); g2' =
                     -((d - 3) / 2) g2 has |d/dd| <= 1/2 (at d = 3); rep' = 2 d has 2; hyd' and hb' are constants between
                     their kinks, and the kinks are decided on the fp32 d the restatement reproduces bit for bit.
                  2. the roundings of the slope's own evaluation: g1 carries u / e (its squared argument) + 2 EXPF_ULP u g1
                     (expf, nominal 1 ulp) and the product one more rounding: 8 |d| (u / e + 2 EXPF_ULP u g1) + u |g1'|;
                     g2 carries 3 u / e + 2 EXPF_ULP u g2, its factor (d - 3) / 2 one rounding and the product one:
                     |a| (3 u / e + 2 EXPF_ULP u g2) + 2 u |g2'|; 2 d is exact; 1 / -0.7f is one rounding, u / 0.7.  The
                     weighted sum adds five products and four sums: 6 u sum |w_k s_k|.
                  3. g = -(dW/dd) / r and the three products g dx: r is the square root of five rounded operations on three
                     rounded differences (3 u relative), the division, dx and the product one rounding each: 6 u |dW/dd|.
                So a pair's contribution to F_ik is off by at most (|dx_k| / r) (e_slope + 6 u |dW/dd|).
                  4. the summation term K u sum |contribution|, K = (the counted pairs of one atom) + 8, as in the
                     interaction rule: the lane's chain, the waves' tree, the butterfly.
                The torque u_i x F_i reads the same fp32 lever u_i on both sides: per atom and component two levers times
                the two force bounds, 2 u (|u_y F_z| + |u_z F_y|) for its own three roundings, and 6 u sum_i of the same
                magnitude for the butterfly.
                ROCm documents no accuracy for expf, so EXPF_ULP = 1 is nominal and the bound carries the explicit factor
                FORCE_FACTOR = 4 x the worst ratio error / bound measured on the MI355X over the trace rows of
                tests/test_pose_optimise_gpu.py: 0.0085 (the net force of the one-atom receptor's case), so FORCE_FACTOR =
                0.034 - the margin `interactions_ref.FACTOR` has.
  Trial pose    (`trial_bounds`) G', p' from GIVEN fp32 F, torque, s_r, s_t, G, p, by the operation count at the magnitudes
                present.  Axis n = torque / |torque|: the norm is the root of five rounded operations (2.5 u relative), the
                division one more: 3.5 u per component.  sinf and cosf: SINCOS_ULP = 2 ulp nominal each.  An entry of D =
                (delta_ij + s K_ij) + c1 K2_ij: |s| (3.5 + 2 SINCOS_ULP + 1) u for s K; for c1 K2, c1 = 1 - cos off by
                (2 SINCOS_ULP + 1) u and K2 (products and a sum of axis components) by 9 u: c1 9 u + (2 SINCOS_ULP + 1) u
                + u; two sums: 2 u.  An entry of G @ D: sum_k |G_ik| e_D + 3 u.  Gram-Schmidt maps its input to its output
                with a Lipschitz constant of at most 4 per entry (the normalisation, the projection and the cross product
                each read two rows) and adds at most 12 roundings of quantities of size <= 1: e_G' = 4 e_GD + 12 u.
                p'_k = p_k + s_t (F_k / |F|): s_t 4.5 u + u |p'_k|.  A part of the move that is skipped is exact.
  Rotation      every entry of R R^T - I within ORTHO = 16 u: a Gram-Schmidt output in fp32 - unit rows within 4 u each,
                the projection's residue within 5 u, the cross product's three roundings and its norm within 8 u.
"""
import math
from fractions import Fraction

import numpy as np

import interactions_ref as IR

U = IR.U
EXPF_ULP = IR.EXPF_ULP
SINCOS_ULP = 2.0
MEASURED_WORST = 0.0085       # worst error / bound of F and the torque at factor 1 on the MI355X ("Optimised pose"):
#                               the net force of the one-atom receptor's case, first trial
FORCE_FACTOR = 0.034          # 4 x MEASURED_WORST
ORTHO = 16 * U
F32 = np.float32
STEP_ROT, STEP_TRANS = F32(0.05), F32(0.25)
GROW, SHRINK = F32(1.2), F32(0.5)
MIN_TRANS = F32(2.0 ** -8)
TRACE_WIDTH = 24
KINKS = (-0.7, 0.0, 0.5, 1.5)


class Walk:
    """The constants and choices of the walk; the planted mistakes change one at a time."""
    def __init__(self, **kw):
        self.torque_sign = 1.0
        self.grow = GROW
        self.orthonormalise = True
        self.torque_about = "p"
        self.g2_factor = 0.5          # the 1 / 2 of g2' = -((d - 3) / 2) g2
        self.strict = True
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


WALK = Walk()


# ----------------------------------------------------------------------------------------------- fp32 pieces
def _round32(s: Fraction) -> np.float32:
    """The exact rational `s` correctly rounded to fp32 (ties to even)."""
    f = F32(float(s))
    best = None
    for c in (f, np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))):
        if not np.isfinite(c):
            continue
        err = abs(Fraction(float(c)) - s)
        even = (int(np.asarray(c).view(np.int32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, c, even)
    return best[1]


def _fma32(a, b, c) -> np.float32:
    """fp32 fused multiply-add, a * b + c rounded once."""
    return _round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def rotate_row(r, G):
    """r @ G as the kernels form it: out[k] = fma(r2, G[2][k], fma(r0, G[0][k], r1 * G[1][k])), fp32."""
    r, G = np.asarray(r, dtype=F32), np.asarray(G, dtype=F32).reshape(3, 3)
    return np.array([_fma32(r[2], G[2, k], _fma32(r[0], G[0, k], r[1] * G[1, k])) for k in range(3)], dtype=F32)


def centroid(x):
    """The atom centroid summed in atom order, fp32."""
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    acc = np.zeros(3, dtype=F32)
    for row in x:
        acc = acc + row
    return (acc / F32(len(x))).astype(F32)


def pose_coords(x, c, G, p):
    """(coords [n,3], levers [n,3]) fp32 of the pose (G, p): u_i = (x_i - c) @ G, x'_i = u_i + p."""
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    r = (x - np.asarray(c, dtype=F32)[None, :]).astype(F32)
    u = np.stack([rotate_row(row, G) for row in r]) if len(r) else np.zeros((0, 3), dtype=F32)
    return (u + np.asarray(p, dtype=F32)[None, :]).astype(F32), u.astype(F32)


def start_pose(x):
    """(coords, levers) of evaluation 0: the input rows as they came, seen from c."""
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    return x, (x - centroid(x)[None, :]).astype(F32)


def shift_rejects(p_new, c, max_shift):
    """The fp32 shift test: ((sx*sx + sy*sy) + sz*sz) > max_shift * max_shift."""
    s = (np.asarray(p_new, dtype=F32) - np.asarray(c, dtype=F32)).astype(F32)
    m = F32(max_shift)
    return bool(((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) > m * m)


# ----------------------------------------------------------------------------------------------- terms, forces, torque
def _pairs(xp, ri, ti, y, rj, tj, defn, smooth):
    xp, y = np.asarray(xp).reshape(-1, 3), np.asarray(y).reshape(-1, 3)
    if smooth:                                  # d in fp64 throughout: the differentiable W the forces are checked against
        diff = xp.astype(np.float64)[:, None, :] - y.astype(np.float64)[None, :, :]
        r = np.sqrt((diff ** 2).sum(axis=2))
        counted = (diff ** 2).sum(axis=2) < defn.cutoff2
        d = r - (np.asarray(ri, dtype=np.float64)[:, None] + np.asarray(rj, dtype=np.float64)[None, :])
    else:
        counted, d = IR.surface_distances(xp, ri, y, rj, defn.cutoff2)
        diff = xp.astype(F32).astype(np.float64)[:, None, :] - y.astype(F32).astype(np.float64)[None, :, :]
        r = np.sqrt((diff ** 2).sum(axis=2))
    ti, tj = np.asarray(ti, dtype=np.int64)[:, None], np.asarray(tj, dtype=np.int64)[None, :]
    both = ((ti & IR.HYDROPHOBIC) != 0) & ((tj & IR.HYDROPHOBIC) != 0)
    facing = (((ti & IR.DONOR) != 0) & ((tj & IR.ACCEPTOR) != 0)) | (((ti & IR.ACCEPTOR) != 0) & ((tj & IR.DONOR) != 0))
    return counted, d, diff, r, both, facing


def _terms(d, counted, both, facing, defn):
    g1 = np.exp(-(d / defn.width1) ** 2)
    g2 = np.exp(-((d - defn.offset2) / defn.width2) ** 2)
    rep = np.where(d < 0, d * d, 0.0)
    hyd = np.where(d <= defn.hyd_full, 1.0, np.where(d >= defn.hyd_zero, 0.0,
                                                     (defn.hyd_zero - d) / (defn.hyd_zero - defn.hyd_full)))
    hb = np.where(d <= defn.hb_full, 1.0, np.where(d >= defn.hb_zero, 0.0,
                                                   (defn.hb_zero - d) / (defn.hb_zero - defn.hb_full)))
    return np.stack([g1, g2, rep, np.where(both, hyd, 0.0), np.where(facing, hb, 0.0)]) * counted[None]


def _slopes(d, counted, both, facing, defn, walk):
    """d(term)/dd of every pair [5,n,R], zero where the pair does not count."""
    g1 = np.exp(-(d / defn.width1) ** 2)
    g2 = np.exp(-((d - defn.offset2) / defn.width2) ** 2)
    s1 = -(2.0 / defn.width1 ** 2) * d * g1                                        # -8 d g1
    s2 = -(walk.g2_factor * 4.0 / defn.width2 ** 2) * (d - defn.offset2) * g2      # -((d - 3) / 2) g2
    s3 = np.where(d < 0, 2.0 * d, 0.0)
    s4 = np.where(both & (d > defn.hyd_full) & (d < defn.hyd_zero), -1.0 / (defn.hyd_zero - defn.hyd_full), 0.0)
    s5 = np.where(facing & (d > defn.hb_full) & (d < defn.hb_zero), -1.0 / (defn.hb_zero - defn.hb_full), 0.0)
    return np.stack([s1, s2, s3, s4, s5]) * counted[None]


def evaluate(xp, lever, ri, ti, y, rj, tj, defn=IR.DEFINITION, walk=WALK, smooth=False):
    """dict of one pose: terms [5], weighted W, atom_forces [n,3], force [3], torque [3] about the point the levers are
    seen from, in fp64 from the fp32 r2 / cut-off / d (`smooth`: from fp64 ones)."""
    counted, d, diff, r, both, facing = _pairs(xp, ri, ti, y, rj, tj, defn, smooth)
    w = np.array([defn.w[k] for k in IR.TERMS])
    t = _terms(d, counted, both, facing, defn)
    dw = np.tensordot(w, _slopes(d, counted, both, facing, defn, walk), axes=1)     # dW/dd [n,R]
    direction = np.divide(diff, r[:, :, None], out=np.zeros_like(diff), where=r[:, :, None] > 0)
    f_atoms = -(dw[:, :, None] * direction).sum(axis=1)
    lever = np.asarray(lever, dtype=np.float64).reshape(-1, 3)
    terms = t.sum(axis=(1, 2))
    return dict(terms=terms, weighted=float(w @ terms), atom_forces=f_atoms, force=f_atoms.sum(axis=0),
                torque=walk.torque_sign * np.cross(lever, f_atoms).sum(axis=0), d=d, counted=counted)


def force_bounds(xp, lever, ri, ti, y, rj, tj, defn=IR.DEFINITION, factor=None):
    """(force [3], torque [3]): how far the kernel's fp32 net force and torque may lie from `evaluate(...)` - by the
    derivation of this module's docstring."""
    factor = FORCE_FACTOR if factor is None else factor
    counted, d, diff, r, both, facing = _pairs(xp, ri, ti, y, rj, tj, defn, False)
    w = np.abs(np.array([defn.w[k] for k in IR.TERMS]))
    s = _slopes(d, counted, both, facing, defn, WALK)
    g1 = np.exp(-(d / defn.width1) ** 2) * counted
    g2 = np.exp(-((d - defn.offset2) / defn.width2) ** 2) * counted
    a2 = np.abs(d - defn.offset2) / defn.width2
    S = float(np.max(ri) + np.max(rj)) if len(np.atleast_1d(ri)) and len(np.atleast_1d(rj)) else 0.0
    delta = U * (8.0 + S)
    e_s = np.stack([8.0 * delta + 8.0 * np.abs(d) * (U / math.e + 2 * EXPF_ULP * U * g1) + U * np.abs(s[0]),
                    0.5 * delta + a2 * (3 * U / math.e + 2 * EXPF_ULP * U * g2) + 2 * U * np.abs(s[1]),
                    np.where(d < 0, 2.0 * delta, 0.0),
                    np.zeros_like(d),
                    np.where(s[4] != 0, U / 0.7, 0.0)]) * counted[None]
    dw_abs = np.tensordot(w, np.abs(s), axes=1)
    e_dw = np.tensordot(w, e_s, axes=1) + 6 * U * dw_abs + 6 * U * dw_abs          # parts 2 and 3
    direction = np.divide(np.abs(diff), r[:, :, None], out=np.zeros_like(diff), where=r[:, :, None] > 0)
    K = (int(counted.sum(axis=1).max()) if counted.size else 0) + 8
    contrib = dw_abs[:, :, None] * direction
    e_atoms = (e_dw[:, :, None] * direction).sum(axis=1) + K * U * contrib.sum(axis=1)          # [n,3]
    f_abs = contrib.sum(axis=1)
    lev = np.abs(np.asarray(lever, dtype=np.float64).reshape(-1, 3))
    e_tau, mag = np.zeros(3), np.zeros(3)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        e_tau[k] = (lev[:, a] * e_atoms[:, b] + lev[:, b] * e_atoms[:, a]).sum()
        mag[k] = (lev[:, a] * f_abs[:, b] + lev[:, b] * f_abs[:, a]).sum()
    return factor * e_atoms.sum(axis=0), factor * (e_tau + (2 + 6) * U * mag)


def weighted_bound(xp, ri, ti, y, rj, tj):
    """How far the kernel's W may lie from `evaluate(...)["weighted"]`: the interaction rule's, unchanged."""
    return float(IR.bounds(xp, ri, ti, y, rj, tj, 0)["weighted"])


# ----------------------------------------------------------------------------------------------- the trial formula
def _usable(v):
    n = math.sqrt(float(v[0]) ** 2 + float(v[1]) ** 2 + float(v[2]) ** 2) if np.all(np.isfinite(v)) else math.inf
    return n > 0 and math.isfinite(n), n


def gram_schmidt(G):
    a, b = G[0] / np.linalg.norm(G[0]), G[1].copy()
    b = b - (a @ b) * a
    b = b / np.linalg.norm(b)
    return np.stack([a, b, np.cross(a, b)])


def trial(F, tau, sr, st, G, p, walk=WALK):
    """(G' [3,3], p' [3], turns, moves) in fp64 from the given values: rotation by s_r about tau / |tau| in row-vector
    form (D = R^T of Rodrigues' R = I + sin K + (1 - cos) K^2, K v = n x v), G' = G @ D made orthonormal by Gram-Schmidt
    (third row = first x second); p' = p + s_t F / |F|.  A zero or non-finite vector skips its part."""
    F, tau = np.asarray(F, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    G, p = np.asarray(G, dtype=np.float64).reshape(3, 3), np.asarray(p, dtype=np.float64)
    turns, tn = _usable(tau)
    moves, fn = _usable(F)
    Gn, pn = G.copy(), p.copy()
    if turns:
        n = tau / tn
        Km = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
        Rm = np.eye(3) + math.sin(float(sr)) * Km + (1 - math.cos(float(sr))) * (Km @ Km)
        Gn = G @ Rm.T
        if walk.orthonormalise:
            Gn = gram_schmidt(Gn)
    if moves:
        pn = p + float(st) * F / fn
    return Gn, pn, turns, moves


def trial_bounds(F, tau, sr, st, G, p):
    """(e_G scalar, e_p [3]): how far the kernel's fp32 G', p' may lie from `trial(...)` of the same given values."""
    Gn, pn, turns, moves = trial(F, tau, sr, st, G, p)
    e_G = 0.0
    if turns:
        s, c1 = abs(math.sin(float(sr))), 1 - math.cos(float(sr))
        e_D = U * (s * (3.5 + 2 * SINCOS_ULP + 1) + c1 * 9 + (2 * SINCOS_ULP + 1) + 1 + 2)
        e_GD = float(np.abs(np.asarray(G, dtype=np.float64).reshape(3, 3)).sum(axis=1).max()) * e_D + 3 * U
        e_G = 4 * e_GD + 12 * U
    e_p = (float(st) * 4.5 * U + U * np.abs(pn)) if moves else np.zeros(3)
    return e_G, e_p


def trial_passes(G_new, p_new, F, tau, sr, st, G, p):
    """Whether a trial pose lies inside the rule for the given fp32 F, tau, s_r, s_t, G, p."""
    Gn, pn, turns, moves = trial(F, tau, sr, st, G, p)
    e_G, e_p = trial_bounds(F, tau, sr, st, G, p)
    G_new, p_new = np.asarray(G_new, dtype=np.float64).reshape(3, 3), np.asarray(p_new, dtype=np.float64)
    return bool((np.abs(G_new - Gn) <= e_G).all() and (np.abs(p_new - pn) <= e_p).all())


# ----------------------------------------------------------------------------------------------- the walk
def run_walk(x, ri, ti, y, rj, tj, steps, max_shift, walk=WALK, defn=IR.DEFINITION, state=F32):
    """The restatement's own walk.  `state`: the type G, p, W, F and the torque are held in between trials - np.float32
    gives what the kernel holds (the trace then is the restatement ROUNDED TO fp32), np.float64 the walk of the DESIGN
    table.  Returns dict: coords [n,3] fp32, G, p, trace [steps,24], w_before, w_after, trials, kept, rmsd, st."""
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    n = len(x)
    c = centroid(x)
    G, p = np.eye(3, dtype=state), c.astype(state)
    coords, lever = start_pose(x)

    def ev(xp, lv, pp):
        if walk.torque_about == "c":
            lv = (xp.astype(np.float64) - c.astype(np.float64))
        return evaluate(xp, lv, ri, ti, y, rj, tj, defn, walk)

    cur = ev(coords, lever, p)
    w_cur, F, tau = state(cur["weighted"]), cur["force"].astype(state), cur["torque"].astype(state)
    w_before = w_cur
    sr, st = STEP_ROT, STEP_TRANS
    trace = np.zeros((steps, TRACE_WIDTH), dtype=np.float64)
    trials = kept = 0
    while trials < steps and not (st < MIN_TRANS):
        Gn, pn, turns, moves = trial(F, tau, sr, st, G, p, walk)
        if not turns and not moves:
            break
        Gn, pn = Gn.astype(state), pn.astype(state)
        evaluated = not shift_rejects(pn, c, max_shift)
        w_new, take = state(0.0), False
        if evaluated:
            xp, lv = pose_coords(x, c, Gn, pn)
            nxt = ev(xp, lv, pn)
            w_new = state(nxt["weighted"])
            take = bool(w_new < w_cur) if walk.strict else bool(w_new <= w_cur)
        trace[trials] = np.concatenate([F, tau, [sr, st], Gn.reshape(9), pn, [w_new, float(evaluated), float(take), w_cur]])
        if take:
            G, p, w_cur, F, tau = Gn, pn, w_new, nxt["force"].astype(state), nxt["torque"].astype(state)
            coords = xp
            sr, st = F32(sr * walk.grow), F32(st * walk.grow)
            kept += 1
        else:
            sr, st = F32(sr * SHRINK), F32(st * SHRINK)
        trials += 1
    rmsd = math.sqrt(float(((coords.astype(np.float64) - x) ** 2).sum() / n)) if n else 0.0
    return dict(coords=coords, G=np.asarray(G), p=np.asarray(p), trace=trace, w_before=float(w_before),
                w_after=float(w_cur), trials=trials, kept=kept, rmsd=rmsd, st=float(st), c=c)


# ----------------------------------------------------------------------------------------------- the rule over a trace
def check_trace(trace, x, ri, ti, y, rj, tj, steps, max_shift, stats=None, coords=None, factor=None, ratios=None):
    """Every violation (a list of strings, empty = passes) of a walk's trace [steps,24] (fp32 values; the kernel's, or the
    restatement's rounded to fp32) against the restatement, TEACHER-FORCED: each row is judged from the pose the trace
    itself says is current, so no comparison depends on two walks taking the same branch.  `stats` [8] and `coords` [n,3]:
    the kernel's, checked against the trace where given.  `ratios`: a dict that collects the worst error / bound at
    factor 1 of the force ("force"), the torque ("torque"), W ("weighted") and the trial pose ("trial")."""
    bad = []
    ratios = ratios if ratios is not None else {}
    fac = FORCE_FACTOR if factor is None else factor

    def note(key, err, bound):
        err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
        r = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
        ratios[key] = max(ratios.get(key, 0.0), float(r.max()) if r.size else 0.0)

    tr = np.asarray(trace, dtype=F32).reshape(steps, TRACE_WIDTH)
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    c = centroid(x)
    used = [k for k in range(steps) if tr[k].any()]
    trials = (used[-1] + 1) if used else 0
    if tr[trials:].any():
        bad.append("rows beyond the last trial are not zero")
    G, p = np.eye(3, dtype=F32), c.copy()
    xp, lever = start_pose(x)
    sr, st = STEP_ROT, STEP_TRANS
    w_cur_bits = None
    kept = 0
    for k in range(trials):
        row = tr[k]
        F, tau, G_new, p_new = row[0:3], row[3:6], row[8:17].reshape(3, 3), row[17:20]
        w_new, evaluated, take, w_cur = row[20], row[21] == 1, row[22] == 1, row[23]
        if row[21] not in (0, 1) or row[22] not in (0, 1):
            bad.append(f"row {k}: flags {row[21]}, {row[22]}")
        want = evaluate(xp, lever, ri, ti, y, rj, tj)
        bF, bT = force_bounds(xp, lever, ri, ti, y, rj, tj, factor=1.0)
        bW = weighted_bound(xp, ri, ti, y, rj, tj)
        note("force", np.abs(F - want["force"]), bF)
        note("torque", np.abs(tau - want["torque"]), bT)
        note("weighted", abs(float(w_cur) - want["weighted"]), bW / IR.FACTOR)
        if not (np.abs(F - want["force"]) <= fac * bF).all():
            bad.append(f"row {k}: force {F} vs {want['force']} (bound {fac * bF})")
        if not (np.abs(tau - want["torque"]) <= fac * bT).all():
            bad.append(f"row {k}: torque {tau} vs {want['torque']} (bound {fac * bT})")
        if not abs(float(w_cur) - want["weighted"]) <= bW:
            bad.append(f"row {k}: W_cur {w_cur} vs {want['weighted']} (bound {bW})")
        if w_cur_bits is not None and np.asarray(w_cur).view(np.int32) != w_cur_bits:
            bad.append(f"row {k}: W_cur is not the W that held")
        if row[6] != sr or row[7] != st:
            bad.append(f"row {k}: step lengths {row[6]}, {row[7]} are not {sr}, {st}")
        sr, st = row[6], row[7]
        Gw, pw, turns, moves = trial(F, tau, sr, st, G, p)
        e_G, e_p = trial_bounds(F, tau, sr, st, G, p)
        if turns:
            note("trial", np.abs(G_new - Gw).ravel(), np.full(9, e_G))
        if moves:
            note("trial", np.abs(p_new - pw), e_p)
        if not turns and not moves:
            bad.append(f"row {k}: a trial without a force or a torque to follow")
        if not trial_passes(G_new, p_new, F, tau, sr, st, G, p):
            bad.append(f"row {k}: the trial pose is not the formula's (G' off by {np.abs(G_new - Gw).max():.3g} of "
                       f"{e_G:.3g}, p' by {np.abs(p_new - pw).max():.3g} of {e_p.max() if moves else 0:.3g})")
        if not (np.abs(G_new.astype(np.float64) @ G_new.astype(np.float64).T - np.eye(3)) <= ORTHO).all():
            bad.append(f"row {k}: G' is not orthonormal")
        if evaluated != (not shift_rejects(p_new, c, max_shift)):
            bad.append(f"row {k}: the shift test")
        if evaluated:
            xn, ln = pose_coords(x, c, G_new, p_new)
            wn = evaluate(xn, ln, ri, ti, y, rj, tj)
            bWn = weighted_bound(xn, ri, ti, y, rj, tj)
            note("weighted", abs(float(w_new) - wn["weighted"]), bWn / IR.FACTOR)
            if not abs(float(w_new) - wn["weighted"]) <= bWn:
                bad.append(f"row {k}: W' {w_new} vs {wn['weighted']} (bound {bWn})")
        elif w_new != 0:
            bad.append(f"row {k}: W' of a trial that was not evaluated")
        if take != (evaluated and bool(w_new < w_cur)):
            bad.append(f"row {k}: kept {take} with evaluated {evaluated}, W' {w_new}, W {w_cur}")
        if take:
            G, p, xp, lever = G_new.copy(), p_new.copy(), xn, ln
            w_cur_bits = np.asarray(w_new).view(np.int32)
            sr, st = F32(sr * GROW), F32(st * GROW)
            kept += 1
        else:
            w_cur_bits = np.asarray(w_cur).view(np.int32)
            sr, st = F32(sr * SHRINK), F32(st * SHRINK)
    if trials < steps and not (st < MIN_TRANS):            # ended early: nothing left to follow at the pose that holds
        want = evaluate(xp, lever, ri, ti, y, rj, tj)
        bF, bT = force_bounds(xp, lever, ri, ti, y, rj, tj, factor=fac)
        if not ((np.abs(want["force"]) <= bF).all() and (np.abs(want["torque"]) <= bT).all()):
            bad.append(f"the walk ended after {trials} of {steps} trials with s_t {st} and a force left")
    if stats is not None:
        stats = np.asarray(stats, dtype=F32)
        if stats[2] != trials or stats[3] != kept or stats[5] != st or stats[6] != 0 or stats[7] != 0:
            bad.append(f"stats {stats} vs {trials} trials, {kept} kept, s_t {st}")
        if w_cur_bits is not None and np.asarray(stats[1]).view(np.int32) != w_cur_bits:
            bad.append("stats[1] is not the W that held at the end")
        if trials and np.asarray(stats[0]).view(np.int32) != np.asarray(tr[0, 23]).view(np.int32):
            bad.append("stats[0] is not the first row's W")
        if kept == 0 and np.asarray(stats[0]).view(np.int32) != np.asarray(stats[1]).view(np.int32):
            bad.append("W changed though nothing was kept")
    if coords is not None:
        got = np.asarray(coords, dtype=F32).reshape(-1, 3)[: len(x)]
        if not np.array_equal(got.view(np.int32), np.asarray(xp, dtype=F32).view(np.int32)):
            bad.append(f"coords are not the bits of the last kept pose (off by {np.abs(got - xp).max():.3g})")
    return bad, dict(trials=trials, kept=kept, G=G, p=p, coords=xp, st=st)


# ----------------------------------------------------------------------------------------------- the seeded cases
def displaced(case, seed, shift=1.0, angle_deg=15.0):
    """`case` (an `interactions_ref.Case`) with its ligand moved as a rigid body by up to `shift` A and `angle_deg`
    degrees out of where the pocket was carved round it: a copy."""
    import copy
    g = np.random.default_rng(seed)
    out = copy.copy(case)
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = math.radians(angle_deg) * g.uniform(0.3, 1.0)
    Km = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm = np.eye(3) + math.sin(ang) * Km + (1 - math.cos(ang)) * (Km @ Km)
    t = g.normal(size=3)
    t *= shift * g.uniform(0.3, 1.0) / np.linalg.norm(t)
    x = case.x.astype(np.float64)
    centre = x.mean(axis=0) if len(x) else np.zeros(3)
    out.x = ((x - centre) @ Rm.T + centre + t).astype(F32)
    out.name = case.name + "d"
    return out


def cases():
    """The interaction tests' ligands (1, 2, 27, 64 atoms) and receptors (1, 255, 256, 257, 4 097 atoms), each ligand
    displaced by up to 1 A and 15 degrees."""
    return [displaced(c, 900 + k) for k, c in enumerate(IR.cases())]


def smooth_cases():
    """Small seeded cases for the central differences of the host test, which asserts of each that every pair lies at
    least 1e-3 A from each kink of the terms (d = -0.7, 0, 0.5, 1.5) and from the 8 A cut-off."""
    return [displaced(IR.Case(f"s{n}", seed, n, R=R), seed + 1000)
            for n, R, seed in ((1, 40, 302), (2, 60, 302), (5, 60, 303), (8, 48, 300), (12, 32, 307))]
