"""Flexible pose (`interactions.optimise_pose_flexible`, kernels `mcg_torsion_tree` and `mcg_receptor_optimise_flex`;
DESIGN.md section 6 "Flexible pose"): the torsion tree and the walk restated from the DESIGN words, and the rules by which
the kernels' values pass against the restatement.  Importing this module needs no GPU.

The tree is integer work: equality.

The walk is judged TEACHER-FORCED through the trace, as `pose_optimise_ref.check_trace` judges the rigid one: every row
from the state the trace itself says is current.  One thing differs.  The rigid trace carries the whole state (G, p), so
the restatement evaluates the kernel's own coordinates bit for bit.  The flexible state also holds q, which no trace
column carries: the restatement turns its own fp64 copy of q by the KERNEL'S angles (delta_k from the trace's own fp32
tau and s_tau, formed as the kernel forms them) and rounds it to fp32.  Its q therefore lies within the drift bound
`drift_bound` of the kernel's, eps_x, and every rule below carries what eps_x can do to the value it judges.

What is fp32 here: the pose -> coordinates step, r2, the cut-off decision and d, the step lengths, delta_k, the shift test,
the acceptance (W' - W) + 0.840f (C' - C) < 0.  Everything else is fp64.

The pass rules, u = 2^-24.
  F, torque     `pose_optimise_ref.force_bounds` at factor 1, plus per atom eps_x H_i + J_i: H_i = sum over its counted pairs
                of (LIP + |dW/dd| / r), LIP = 8 |w_g1| + |w_g2| / 2 + 2 w_rep the largest |d2W/dd2| of the smooth terms; J_i
                the slope's jump of every pair within 4 eps_x + 1e-6 of a kink of hyd' or hb' or of the cut-off (|w_hyd|,
                |w_hb| / 0.7, |dW/dd|).  The torque adds eps_x sum |F_i| for the lever.
  CLASH         per counted pair 6 u e^2 (the square, the sum, the root and the differences) + 2 e (u (s + r) + 2 eps_x),
                plus (pairs + 8) u CLASH for the sums.
  tau_k         (the longest lever of the side) x (the rigid rule's force error of the side's own atoms, all components) and
                sum over the side of |r_i| (3 (eps_x H_i + J_i) + e_clash_i) for the forces' own error, 16 u sum |r_i| |f_i| for the cross
                product, the dot product, the axis and the butterfly, 2 eps_x sum |f_i| for the lever and 2 eps_x / |ab|
                sum |r_i| |f_i| for the axis.  e_clash_i = 0.840 sum over its clash pairs of (8 u 2 e + 4 eps_x).
  W             `pose_optimise_ref.weighted_bound`, plus eps_x sum_i |F_i|_1 and the terms of every pair within reach of
                the cut-off.
                Each of the four carries its own explicit factor, 4 x the worst error / bound measured for THAT quantity
                on the MI355X over the trace rows of tests/test_pose_flex_gpu.py against this fp64 restatement
                (FLEX_MEASURED, FLEX_FACTORS).  FLEX_FORCE_FACTOR, the largest of them, is the one factor the
                definition names; no quantity is judged by a wider one.
  Trial pose    G', p': `pose_optimise_ref.trial_passes`, unchanged.  q' is not in the trace; it is judged through W', C'
                and the returned coordinates.
  Drift         (`drift_bound`) the linear bound ROUNDINGS u lever kept depth: ROUNDINGS = 24 roundings per Rodrigues
                application (the difference to q_b, the axis, sin and cos, the nine entries of D, the row product, the
                sum), lever = 2 (rho0 + 2) the largest distance inside a molecule the walk can hold, kept the kept
                trials, depth the most moving sides one atom lies in (at least 1); plus 8 u (|x| + |p|) for the pose
                step.  The rule is DRIFT_FACTOR = 4 x the worst measured drift / bound (DRIFT_MEASURED_WORST).
"""
import math

import numpy as np

import interactions_ref as IR
import pose_optimise_ref as PR

U = IR.U
F32 = np.float32
MAX_TORSIONS = 16
W_REP = float(F32(0.840))
STEP_TAU = F32(0.1)
MARGIN = F32(2.0)
TRACE_WIDTH = 43
RCOV = {5: 0.84, 6: 0.76, 7: 0.71, 8: 0.66, 9: 0.57, 14: 1.11, 15: 1.07, 16: 1.05, 17: 1.02, 33: 1.19, 34: 1.20, 35: 1.20}
CLASH_PAD = 0.45
ROUNDINGS = 24.0
# worst error / bound at factor 1 on the MI355X ("Flexible pose"): CLASH of the two stacked benzenes; F of the two
# fragments before the one-atom receptor; the torque of benzene there; tau of the folded heptane
FLEX_MEASURED = dict(force=0.0497, torque=0.0201, tau=0.00488, clash=0.0536)
FLEX_FACTORS = {k: 4 * v for k, v in FLEX_MEASURED.items()}
FLEX_MEASURED_WORST = max(FLEX_MEASURED.values())
FLEX_FORCE_FACTOR = 4 * FLEX_MEASURED_WORST        # 0.214
DRIFT_MEASURED_WORST = 0.0604   # worst drift / bound at factor 1 over every case at steps = 1024: the two stacked benzenes
#                                 (no torsion: the pose step alone); with torsions at most 0.0020.  Worst absolute drift of a
#                                 distance the walk must keep: 1.45e-5 A (the C20 alkane, 74 kept trials)
DRIFT_FACTOR = 0.242            # 4 x DRIFT_MEASURED_WORST
LIP = 8 * 0.0356 + 0.5 * 0.00516 + 2 * 0.840


class Rules:
    """The choices of the definition; the planted mistakes change one at a time."""
    def __init__(self, **kw):
        self.tau_sign = 1.0
        self.side = "b"               # tau and the turn run over the moving side, the one that holds b
        self.tie = "higher"           # a tie: the part of the higher-indexed end moves
        self.near_13 = True           # 1-3 pairs are near: left out of CLASH
        self.clash_frame = "q"        # CLASH from the molecule-frame coordinates
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


RULES = Rules()


def clash_radii(z):
    return np.array([RCOV.get(int(v), RCOV[6]) + CLASH_PAD for v in np.atleast_1d(z)], dtype=F32)


# ----------------------------------------------------------------------------------------------- the tree
def _flood(nb, start, blocked, edge=None):
    """The atoms reachable from `start` without entering `blocked` and without walking the bond `edge`."""
    seen, todo = {start}, [start]
    while todo:
        i = todo.pop()
        for j in nb[i]:
            if j not in seen and j != blocked and (edge is None or {i, j} != set(edge)):
                seen.add(j)
                todo.append(j)
    return seen


def tree(z, bonds, n, rules=RULES):
    """dict: torsions [(a, b)] (used, in order), sides [set], near [set per atom], found, used."""
    n = int(n)
    code = lambda i, j: int(bonds[i][j]) if i != j and 1 <= int(bonds[i][j]) <= 4 else 0   # noqa: E731
    nb = [[j for j in range(n) if code(i, j)] for i in range(n)]
    near = []
    for i in range(n):
        s = {i} | set(nb[i])
        if rules.near_13:
            for j in nb[i]:
                s |= set(nb[j])
        near.append(s)
    carbonyl = [int(z[i]) == 6 and any(code(i, j) == 2 and int(z[j]) in (7, 8, 16) for j in nb[i]) for i in range(n)]
    found = []
    for a in range(n):
        for j in nb[a]:
            if j < a or code(a, j) != 1 or len(nb[a]) < 2 or len(nb[j]) < 2:
                continue
            if a in _flood(nb, j, None, edge=(a, j)):        # reachable round the bond left out: a ring bond
                continue
            side_j = _flood(nb, j, a)
            if (carbonyl[a] and int(z[j]) == 7) or (carbonyl[j] and int(z[a]) == 7):
                continue
            side_a = _flood(nb, a, j)
            j_moves = len(side_j) <= len(side_a) if rules.tie == "higher" else len(side_j) < len(side_a)
            found.append(((a, j), side_j) if j_moves else ((j, a), side_a))
    used = found[:MAX_TORSIONS]
    return dict(torsions=[t for t, _ in used], sides=[s for _, s in used], near=near, found=len(found), used=len(used))


def tree_arrays(t, n, width):
    """The tree as the kernel writes it: torsion_atoms [16,2] int32, side_mask [16] uint64, near_mask [width] uint64,
    counts [2]."""
    atoms = np.full((MAX_TORSIONS, 2), -1, dtype=np.int32)
    side = np.zeros(MAX_TORSIONS, dtype=np.uint64)
    near = np.zeros(width, dtype=np.uint64)
    mask = lambda s: np.uint64(sum(1 << i for i in s))                                     # noqa: E731
    for k, (ab, s) in enumerate(zip(t["torsions"], t["sides"])):
        atoms[k] = ab
        side[k] = mask(s)
    for i in range(n):
        near[i] = mask(t["near"][i])
    return atoms, side, near, np.array([t["found"], t["used"]], dtype=np.int32)


# ----------------------------------------------------------------------------------------------- one evaluation
def clash(q, c, near):
    """(CLASH, force [n,3] = -dCLASH/dq, pairs [(i, j, e, r)]) in fp64 from the given coordinates."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    n = len(q)
    total, f, pairs = 0.0, np.zeros((n, 3)), []
    for i in range(n):
        for j in range(i + 1, n):
            if j in near[i]:
                continue
            d = q[i] - q[j]
            r = math.sqrt(float(d @ d))
            e = float(c[i]) + float(c[j]) - r
            if e > 0:
                total += e * e
                pairs.append((i, j, e, r))
                if r > 0:
                    f[i] += 2 * e * d / r
                    f[j] -= 2 * e * d / r
    return total, f, pairs


def evaluate(q, G, x, lever, lig, rec, c, t, rules=RULES):
    """One evaluation of the state (q, G) whose world coordinates are x and levers `lever` (fp32, as the kernel holds
    them): dict with PR.evaluate's entries, clash, clash_pairs, atom_total [n,3] and tau [16]."""
    ri, ti = lig
    y, rj, tj = rec
    out = PR.evaluate(x, lever, ri, ti, y, rj, tj)
    Gd = np.asarray(G, dtype=np.float64).reshape(3, 3)
    src = np.asarray(q, dtype=np.float64) if rules.clash_frame == "q" else np.asarray(x, dtype=F32).astype(np.float64)
    C, fq, pairs = clash(src, c, t["near"])
    fw = fq @ Gd if rules.clash_frame == "q" else fq
    total = out["atom_forces"] + W_REP * fw
    xd = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    tau = np.zeros(MAX_TORSIONS)
    for k, ((a, b), side) in enumerate(zip(t["torsions"], t["sides"])):
        axis = xd[b] - xd[a]
        axis = axis / np.linalg.norm(axis)
        atoms = sorted(side) if rules.side == "b" else sorted(set(_component(t, a, len(xd))) - set(side))
        m = sum(np.cross(xd[i] - xd[b], total[i]) for i in atoms)
        tau[k] = rules.tau_sign * float(axis @ m)
    out.update(clash=C, clash_force=fw, clash_pairs=pairs, atom_total=total, tau=tau)
    return out


def _component(t, a, n):
    """The atoms bonded, through any chain, to a (read off the near sets, which hold every bond)."""
    seen, todo = {a}, [a]
    while todo:
        i = todo.pop()
        for j in t["near"][i]:
            if j not in seen:
                seen.add(j)
                todo.append(j)
    return seen


def deltas(tau32, s_tau, used):
    """(delta [16] fp32, twists) as the kernel forms them: delta_k = s_tau * (tau_k / max_j |tau_j|) in fp32."""
    tau32 = np.asarray(tau32, dtype=F32)
    mt = F32(np.max(np.abs(tau32))) if len(tau32) else F32(0)
    ok = used > 0 and bool(np.all(np.isfinite(tau32))) and mt > 0
    d = np.zeros(MAX_TORSIONS, dtype=F32)
    if ok:
        for k in range(used):
            d[k] = F32(s_tau) * F32(tau32[k] / mt)
    return d, ok


def twist(q, delta, t, rules=RULES):
    """q [n,3] fp64 with the torsions turned in ascending order, torsion k by delta[k] right-handed about the unit vector
    from a to b through q_b; a delta of 0 leaves the atoms as they are."""
    q = np.array(q, dtype=np.float64).reshape(-1, 3)
    for k, ((a, b), side) in enumerate(zip(t["torsions"], t["sides"])):
        th = float(delta[k])
        if th == 0.0:
            continue
        n = q[b] - q[a]
        n = n / np.linalg.norm(n)
        Km = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
        Rm = np.eye(3) + math.sin(th) * Km + (1 - math.cos(th)) * (Km @ Km)
        atoms = sorted(side) if rules.side == "b" else sorted(set(_component(t, a, len(q))) - set(side))
        pivot = q[b].copy()
        for i in atoms:
            q[i] = (q[i] - pivot) @ Rm.T + pivot
    return q


def outside(q32, rho0):
    """The fp32 test any (qx*qx + qy*qy) + qz*qz > (rho0 + 2)^2."""
    q32 = np.asarray(q32, dtype=F32).reshape(-1, 3)
    lim = F32(rho0) + MARGIN
    r2 = (q32[:, 0] * q32[:, 0] + q32[:, 1] * q32[:, 1]) + q32[:, 2] * q32[:, 2]
    return bool((r2 > lim * lim).any())


def rho0_of(x):
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    r = (x - PR.centroid(x)[None, :]).astype(F32)
    r2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    return F32(np.sqrt(F32(r2.max()))) if len(r) else F32(0)


def accepts(w_new, w_cur, c_new, c_cur):
    """(W' - W) + 0.840f (C' - C) < 0 in fp32, in that order."""
    return bool((F32(w_new) - F32(w_cur)) + F32(0.840) * (F32(c_new) - F32(c_cur)) < 0)


def dihedral(x, i, j, k, l):
    x = np.asarray(x, dtype=np.float64)
    b0, b1, b2 = x[i] - x[j], x[k] - x[j], x[l] - x[k]
    b1 = b1 / np.linalg.norm(b1)
    v, w = b0 - (b0 @ b1) * b1, b2 - (b2 @ b1) * b1
    return math.atan2(float(np.cross(b1, v) @ w), float(v @ w))


# ----------------------------------------------------------------------------------------------- the bounds
def depth_of(t, n):
    return max([sum(1 for s in t["sides"] if i in s) for i in range(n)] + [1])


def drift_bound(x, t, kept, factor=None):
    """How far a returned coordinate, or a distance the walk must keep, may lie from the exact one after `kept` kept
    trials - the linear bound of this module's docstring."""
    factor = DRIFT_FACTOR if factor is None else factor
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    if not len(x):
        return 0.0
    rho0 = float(rho0_of(x))
    lever = 2.0 * (rho0 + 2.0)
    twist_part = ROUNDINGS * U * lever * max(kept, 0) * depth_of(t, len(x)) if t["used"] else 0.0
    return factor * (twist_part + 8 * U * (float(np.abs(x).max()) + rho0 + 4.0))


def value_bounds(want, x, lever, lig, rec, c, t, eps_x):
    """dict of bounds at factor 1 for `want` = evaluate(...): force [3], torque [3], tau [16], clash, weighted."""
    ri, ti = lig
    y, rj, tj = rec
    n = len(np.asarray(x).reshape(-1, 3))
    xd = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    lev = np.abs(np.asarray(lever, dtype=np.float64).reshape(-1, 3))
    bF0, bT0 = PR.force_bounds(xd.astype(F32), lev, ri, ti, y, rj, tj, factor=1.0)      # the rigid rule, all atoms
    counted, d = want["counted"], want["d"]
    defn = IR.DEFINITION
    both = ((np.asarray(ti)[:, None] & IR.HYDROPHOBIC) != 0) & ((np.asarray(tj)[None, :] & IR.HYDROPHOBIC) != 0)
    w = np.array([defn.w[k] for k in IR.TERMS])
    sl = PR._slopes(d, counted, both, np.ones_like(both), defn, PR.WALK)
    dw = np.abs(np.tensordot(np.abs(w), np.abs(sl), axes=1))
    diff = xd[:, None, :] - np.asarray(y, dtype=np.float64)[None, :, :]
    r = np.sqrt((diff ** 2).sum(axis=2))
    tol = 4 * eps_x + 1e-6
    H = (counted * (LIP + np.divide(dw, r, out=np.zeros_like(dw), where=r > 0))).sum(axis=1)
    J = np.zeros(n)
    if eps_x > 0:
        for kink, jump in ((0.5, abs(w[3])), (1.5, abs(w[3])), (-0.7, abs(w[4]) / 0.7), (0.0, abs(w[4]) / 0.7)):
            J += (counted & (np.abs(d - kink) < tol)).sum(axis=1) * jump
        edge = np.abs(r - 8.0) < tol
        J += (edge * (LIP * 8.0)).sum(axis=1)
        w_edge = float((edge * 0.02).sum())           # a pair at the cut-off carries at most |w_g2| g2 + ... < 0.02 of W
    else:
        w_edge = 0.0
    extra = eps_x * H + J
    f_abs = np.abs(want["atom_forces"])
    bF = bF0 + extra.sum()
    bT = np.zeros(3)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        bT[k] = bT0[k] + ((lev[:, a] + lev[:, b]) * extra).sum() + eps_x * f_abs.sum()
    pairs = want["clash_pairs"]
    bC = sum(6 * U * e * e + 2 * e * (U * (e + 2 * rr) + 2 * eps_x) for _, _, e, rr in pairs) + (len(pairs) + 8) * U * want["clash"]
    near_zero = 0
    if eps_x > 0:                                  # a pair about to touch: e within the reach of eps_x
        src = xd
        for i in range(n):
            for j in range(i + 1, n):
                if j not in t["near"][i]:
                    e = float(c[i]) + float(c[j]) - float(np.linalg.norm(src[i] - src[j]))
                    if -tol < e <= 0:
                        near_zero += 1
    bC += near_zero * tol * tol
    e_cl = np.zeros(n)
    for i, j, e, rr in pairs:
        e_cl[i] += W_REP * (8 * U * 2 * e + 4 * eps_x)
        e_cl[j] += W_REP * (8 * U * 2 * e + 4 * eps_x)
    e_cl += near_zero * W_REP * 2 * tol
    bTau = np.zeros(MAX_TORSIONS)
    tot_abs = np.abs(want["atom_total"]).sum(axis=1)
    for k, ((a, b), side) in enumerate(zip(t["torsions"], t["sides"])):
        ab = float(np.linalg.norm(xd[b] - xd[a]))
        for i in side:
            ri_ = float(np.linalg.norm(xd[i] - xd[b]))
            bTau[k] += ri_ * (3 * extra[i] + e_cl[i]) + 16 * U * ri_ * tot_abs[i] + 2 * eps_x * tot_abs[i] \
                + 2 * eps_x / ab * ri_ * tot_abs[i]
        reach = max([float(np.linalg.norm(xd[i] - xd[b])) for i in side] + [0.0])
        own = sorted(side)                           # the rigid rule's force error of the side's own atoms, at the longest lever
        bTau[k] += reach * float(PR.force_bounds(xd[own].astype(F32), lev[own], np.asarray(ri)[own], np.asarray(ti)[own],
                                                 y, rj, tj, factor=1.0)[0].sum())
    bW = PR.weighted_bound(x, ri, ti, y, rj, tj) + eps_x * f_abs.sum() + w_edge
    return dict(force=bF, torque=bT, tau=bTau, clash=bC, weighted=bW)


# ----------------------------------------------------------------------------------------------- the walk
def run_walk(x, lig, rec, z, bonds, steps, max_shift, rules=RULES, t=None):
    """The restatement's own walk, its state held in fp32 between trials (the trace is the restatement rounded to fp32).
    Returns dict: coords, q, G, p, trace [steps,43], w_before, w_after, c_before, c_after, trials, kept, angles, tree."""
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    n = len(x)
    t = tree(z, bonds, n, rules) if t is None else t
    cr = clash_radii(z[:n])
    ctr = PR.centroid(x)
    rho0 = rho0_of(x)
    G, p = np.eye(3, dtype=F32), ctr.copy()
    coords, lever = PR.start_pose(x)
    q = lever.astype(F32)
    q0 = q.copy()
    cur = evaluate(q, G, coords, lever, lig, rec, cr, t, rules)
    state = lambda e: (F32(e["weighted"]), e["force"].astype(F32), e["torque"].astype(F32), e["tau"].astype(F32),   # noqa: E731
                       F32(e["clash"]))
    w_cur, F, T, tau, c_cur = state(cur)
    w0, c0 = w_cur, c_cur
    sr, st, stau = PR.STEP_ROT, PR.STEP_TRANS, STEP_TAU
    trace = np.zeros((steps, TRACE_WIDTH))
    angles = np.zeros(MAX_TORSIONS)
    trials = kept = 0
    while trials < steps and not (st < PR.MIN_TRANS):
        Gn, pn, turns, moves = PR.trial(F, T, sr, st, G, p)
        d, twists = deltas(tau, stau, t["used"])
        if not turns and not moves and not twists:
            break
        Gn, pn = Gn.astype(F32), pn.astype(F32)
        qn = twist(q, d, t, rules).astype(F32) if twists else q
        evaluated = not PR.shift_rejects(pn, ctr, max_shift) and not outside(qn, rho0)
        w_new, c_new, take = F32(0), F32(0), False
        if evaluated:
            xp, lv = PR.pose_coords(qn, np.zeros(3, dtype=F32), Gn, pn)
            nxt = evaluate(qn, Gn, xp, lv, lig, rec, cr, t, rules)
            w_new, Fn, Tn, taun, c_new = state(nxt)
            take = accepts(w_new, w_cur, c_new, c_cur)
        trace[trials] = np.concatenate([F, T, [sr, st], Gn.reshape(9), pn, [w_new, float(evaluated), float(take), w_cur],
                                        [stau], tau, [c_cur, c_new]])
        if take:
            G, p, q, coords = Gn, pn, qn, xp
            w_cur, F, T, tau, c_cur = w_new, Fn, Tn, taun, c_new
            angles += d
            sr, st, stau = F32(sr * PR.GROW), F32(st * PR.GROW), F32(stau * PR.GROW)
            kept += 1
        else:
            sr, st, stau = F32(sr * PR.SHRINK), F32(st * PR.SHRINK), F32(stau * PR.SHRINK)
        trials += 1
    return dict(coords=coords, q=q, q0=q0, G=G, p=p, trace=trace, w_before=float(w0), w_after=float(w_cur),
                c_before=float(c0), c_after=float(c_cur), trials=trials, kept=kept, angles=angles, tree=t, st=float(st))


# ----------------------------------------------------------------------------------------------- the rule over a trace
def check_trace(trace, x, lig, rec, z, bonds, steps, max_shift, stats=None, coords=None, angles=None, factor=None,
                ratios=None):
    """Every violation (a list of strings, empty = passes) of a flexible walk's trace [steps,43] against the restatement,
    teacher-forced as this module's docstring says.  `stats` [12], `coords` [n,3], `angles` [16]: the kernel's, checked
    against the trace where given.  `ratios` collects the worst error / bound at factor 1 per value."""
    bad = []
    ratios = ratios if ratios is not None else {}
    facs = dict(FLEX_FACTORS) if factor is None else {k: factor for k in FLEX_FACTORS}

    def judge(key, k, got, want, bound):
        err = np.atleast_1d(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)))
        bound = np.atleast_1d(np.asarray(bound, dtype=np.float64))
        r = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
        ratios[key] = max(ratios.get(key, 0.0), float(r.max()) if r.size else 0.0)
        if not (err <= facs[key] * bound).all():
            bad.append(f"row {k}: {key} {got} vs {want} (bound {facs[key] * bound})")

    tr = np.asarray(trace, dtype=F32).reshape(steps, TRACE_WIDTH)
    x = np.asarray(x, dtype=F32).reshape(-1, 3)
    n = len(x)
    t = tree(z, bonds, n)
    cr = clash_radii(z[:n])
    ctr = PR.centroid(x)
    rho0 = rho0_of(x)
    used_rows = [k for k in range(steps) if tr[k].any()]
    trials = (used_rows[-1] + 1) if used_rows else 0
    if tr[trials:].any():
        bad.append("rows beyond the last trial are not zero")
    G, p = np.eye(3, dtype=F32), ctr.copy()
    xp, lever = PR.start_pose(x)
    q = lever.astype(np.float64)
    q0 = q.copy()
    sr, st, stau = PR.STEP_ROT, PR.STEP_TRANS, STEP_TAU
    kept = twisted = 0
    total = np.zeros(MAX_TORSIONS)
    prev = None                                    # (W, C) bits that must hold in the next row
    bits = lambda v: int(np.asarray(v, dtype=F32).view(np.int32))                         # noqa: E731
    for k in range(trials):
        row = tr[k]
        F, T, G_new, p_new = row[0:3], row[3:6], row[8:17].reshape(3, 3), row[17:20]
        w_new, evaluated, take, w_cur = row[20], row[21] == 1, row[22] == 1, row[23]
        tau, c_cur, c_new = row[25:41], row[41], row[42]
        if row[21] not in (0, 1) or row[22] not in (0, 1):
            bad.append(f"row {k}: flags {row[21]}, {row[22]}")
        eps = drift_bound(x, t, twisted, factor=1.0) if twisted else 0.0
        want = evaluate(q, G, xp, lever, lig, rec, cr, t)
        bnd = value_bounds(want, xp, lever, lig, rec, cr, t, eps)
        judge("force", k, F, want["force"], bnd["force"])
        judge("torque", k, T, want["torque"], bnd["torque"])
        judge("tau", k, tau, want["tau"], bnd["tau"])
        judge("clash", k, c_cur, want["clash"], bnd["clash"])
        if not abs(float(w_cur) - want["weighted"]) <= bnd["weighted"]:
            bad.append(f"row {k}: W_cur {w_cur} vs {want['weighted']} (bound {bnd['weighted']})")
        if prev is not None and (bits(w_cur), bits(c_cur)) != prev:
            bad.append(f"row {k}: W, C are not the ones that held")
        if tau[t["used"]:].any():
            bad.append(f"row {k}: tau beyond the used torsions")
        if (row[6], row[7], row[24]) != (sr, st, stau):
            bad.append(f"row {k}: step lengths {row[6]}, {row[7]}, {row[24]} are not {sr}, {st}, {stau}")
        sr, st, stau = row[6], row[7], row[24]
        Gw, pw, turns, moves = PR.trial(F, T, sr, st, G, p)
        d, twists = deltas(tau, stau, t["used"])
        if not turns and not moves and not twists:
            bad.append(f"row {k}: a trial with nothing to follow")
        if not PR.trial_passes(G_new, p_new, F, T, sr, st, G, p):
            bad.append(f"row {k}: the rigid part of the trial is not the formula's")
        turned = twists and bool(np.any(d != 0))
        qn = twist(q, d, t) if turned else q
        far = outside(qn.astype(F32), rho0)
        edge = abs(float(np.sqrt((qn ** 2).sum(axis=1)).max()) - (float(rho0) + 2.0)) < 1e-4 if n else False
        if not edge and evaluated != (not PR.shift_rejects(p_new, ctr, max_shift) and not far):
            bad.append(f"row {k}: evaluated {evaluated} against the shift and radius tests")
        if evaluated:
            xn, ln = PR.pose_coords(qn.astype(F32), np.zeros(3, dtype=F32), G_new, p_new)
            eps_n = drift_bound(x, t, twisted + (1 if turned else 0), factor=1.0) if (twisted or turned) else 0.0
            wn = evaluate(qn, G_new, xn, ln, lig, rec, cr, t)
            bn = value_bounds(wn, xn, ln, lig, rec, cr, t, eps_n)
            if not abs(float(w_new) - wn["weighted"]) <= bn["weighted"]:
                bad.append(f"row {k}: W' {w_new} vs {wn['weighted']} (bound {bn['weighted']})")
            judge("clash", k, c_new, wn["clash"], bn["clash"])
            if not turned and bits(c_new) != bits(c_cur):
                bad.append(f"row {k}: no torsion turned, yet CLASH changed its bits ({c_cur} -> {c_new})")
        elif w_new != 0 or c_new != 0:
            bad.append(f"row {k}: W' or C' of a trial that was not evaluated")
        if take != (evaluated and accepts(w_new, w_cur, c_new, c_cur)):
            bad.append(f"row {k}: kept {take} with evaluated {evaluated}, W' {w_new}, W {w_cur}, C' {c_new}, C {c_cur}")
        if take:
            if not (float(w_new) + W_REP * float(c_new) < float(w_cur) + W_REP * float(c_cur)):
                bad.append(f"row {k}: a kept trial did not lower W + 0.840 CLASH")
            G, p, q, xp, lever = G_new.copy(), p_new.copy(), qn, xn, ln
            prev = (bits(w_new), bits(c_new))
            total += d if twists else 0
            twisted += 1 if turned else 0
            kept += 1
            sr, st, stau = F32(sr * PR.GROW), F32(st * PR.GROW), F32(stau * PR.GROW)
        else:
            prev = (bits(w_cur), bits(c_cur))
            sr, st, stau = F32(sr * PR.SHRINK), F32(st * PR.SHRINK), F32(stau * PR.SHRINK)
    if stats is not None:
        stats = np.asarray(stats, dtype=F32)
        if (stats[2], stats[3], stats[5], stats[8], stats[10], stats[11]) != (trials, kept, st, t["used"], 0, 0):
            bad.append(f"stats {stats} vs {trials} trials, {kept} kept, s_t {st}, {t['used']} torsions")
        if prev is not None and (bits(stats[1]), bits(stats[7])) != prev:
            bad.append("stats[1], stats[7] are not the W, C that held at the end")
        if trials and (bits(stats[0]), bits(stats[6])) != (bits(tr[0, 23]), bits(tr[0, 41])):
            bad.append("stats[0], stats[6] are not the first row's W, C")
        if kept == 0 and (bits(stats[0]), bits(stats[6])) != (bits(stats[1]), bits(stats[7])):
            bad.append("W or C changed though nothing was kept")
        rms = math.sqrt(float(((q - q0) ** 2).sum() / n)) if n else 0.0
        if abs(float(stats[9]) - rms) > 2 * drift_bound(x, t, twisted) + 4 * U * rms:
            bad.append(f"conformer_rmsd {stats[9]} vs {rms}")
    if coords is not None:
        got = np.asarray(coords, dtype=F32).reshape(-1, 3)[:n]
        if twisted == 0:
            if not np.array_equal(got.view(np.int32), np.asarray(xp, dtype=F32).view(np.int32)):
                bad.append("no torsion turned, yet coords are not the bits of the last kept pose")
        else:
            err = float(np.abs(got.astype(np.float64) - np.asarray(xp, dtype=np.float64)).max())
            ratios["drift_coords"] = max(ratios.get("drift_coords", 0.0), err / drift_bound(x, t, twisted, factor=1.0))
            if err > drift_bound(x, t, twisted):
                bad.append(f"coords lie {err:.3g} from the restatement's state (bound {drift_bound(x, t, twisted):.3g})")
    if angles is not None:
        got = np.asarray(angles, dtype=np.float64)
        if np.abs(got - total).max() > 4 * U * max(kept, 1) * (np.abs(total).max() + 1.0):
            bad.append(f"angles {got} vs the summed kept turns {total}")
    return bad, dict(trials=trials, kept=kept, twisted=twisted, G=G, p=p, q=q, q0=q0, coords=xp, angles=total, tree=t)
