"""numpy fp64 restatement of the electrostatic definition ("Electrostatic similarity";
`ml_conformer_generator_amd/electrostatics.py`), written from that text and not from the kernels: partial charges by
iterative electronegativity equalisation, the charge points of a molecule with its placed hydrogens, the Coulomb overlap of
Gaussian-smeared charges and its Tanimoto - what `tests/test_electrostatics_host.py` and `tests/test_electrostatics_gpu.py`
hold `mcg_charges_peoe` and `mcg_esp_overlap` to.  The hydrogen count, the class rule and the placement it builds on are
`hydrogens_ref`'s.  A molecule is (z, adj, n) as in `pharmacophore_ref`.  This module also holds the pass rules.

THE PASS RULES
Charges  |q_gpu - q_ref| <= Q_TOL on every heavy-atom and hydrogen charge.  Derivation from the fp32 arithmetic (u = 2^-24 =
  6.0e-8): |chi| <= about 25 and chi is three roundings of that size (b q, a + b q, + c q^2), so a chi is off by eps_chi <=
  3 * 25 u = 4.5e-6 from rounding; a flow f = (chi_j - chi_i) / chi+ with chi+ >= 16 is off by 2 eps_chi / 16 = 5.6e-7 (its own
  rounding, |f| u < 1e-8, is below that); an atom adds at most 4 flows' worth (at most 4 neighbours, the nH hydrogens counting
  as nH of them: neighbours + nH <= 4 on C, N, O; P and S have no hydrogens at 4 neighbours), so step k creates at most
  0.5^k * 4 * 5.6e-7 = 0.5^k * 2.2e-6.  An error d already in the charges moves a chi by b d with b <= 13.85, a flow by at most
  2 * 13.85 d / 16 = 1.75 d, the step's sum by 4 * 1.75 d, so d_k <= d_(k-1) (1 + 7 * 0.5^k) + 0.5^k * 2.2e-6:
  1.1e-6, 3.6e-6, 7.0e-6, 10.2e-6, 12.5e-6, 13.9e-6 over the six steps, every error taken with the worst sign.  The iteration
  is a contraction in practice, so a few 1e-6 are expected; Q_TOL = 5e-5 is about 3.6 x the worst-case bound.  There is no
  discrete decision in the charges: f is continuous where chi_i = chi_j, so no case is left out.
Overlaps |E_gpu - E_ref| <= OVERLAP_C * u * S with S = sum |t_ij| over the terms of the double sum, for E(R,M) and E(M,M).
  Per term, relative errors in units of u, every operation rounded once (u each): the difference dx 1; dx*dx 2 * 1 + 1 = 3; the
  two additions of positive squares + 1 + 1 = 5 on r^2; sqrtf 5 / 2 + 1 = 3.5 on r; mu * r + 1 = 4.5; erf(x) moves relatively by
  at most its argument's relative error (x erf'(x) <= erf(x)) = 4.5, plus erff's own error ERFF_ULP ulp = 2 ERFF_ULP u; the
  division by r 3.5 + 1; the product of the two charges 1; times K 1: 4.5 + 2 ERFF_ULP + 4.5 + 2 = 11 + 2 ERFF_ULP.  (The
  series branch below r = 1e-3 has fewer operations.)  The fp64 accumulation adds nothing visible (256 * 256 terms at 2^-53);
  the one rounding of the sum to fp32 adds u |E| <= u S: OVERLAP_C = 12 + 2 ERFF_ULP.  ROCm's erff error is not documented in
  this installation, so ERFF_ULP is a bound MEASURED against fp64 erf on the fixtures' own arguments mu * r (the GPU test
  `test_erff_error_on_the_fixtures_arguments` measures it again and asserts it): 0.90 ulp at the worst of 29 478 arguments in
  [0.97, 43.8] on the MI355X (the kernel's own erff(r) / r of a single pair: 0.87 ulp, its division included), taken as
  ERFF_ULP = 2.  OVERLAP_C = 16 <= 32.
Measured on the MI355X against these rules (DESIGN.md section 6 records them): charges 4.5e-8 e (0.0009 of Q_TOL); overlaps
  at most 0.068 of their bound, the Tanimoto at most 0.027 of its.
Tanimoto |T_gpu - T_ref| <= tanimoto_tolerance(...): the first-order propagation of the three overlap bounds through T = c /
  D, D = rr + m - c: (|D + c| dc + |c| (drr + dm)) / D^2, plus the fp32 arithmetic of T itself on the rounded sums:
  u |T| ((rr + m) / D + 2) for the two additions and the division.  It is computed per case from the restatement.
The rules judge a case only where E(M,M) >= CONDITION * S (the self-overlap of a neutral molecule is what is left of a sum
of cancelling terms); `test_electrostatics_host.py` asserts it for every fixture, no case skipped."""
import math

import numpy as np

import hydrogens_ref as HR

MU = 1.0                                          # 1 / A: Gaussian charges of width 0.5 A
SMALL_R = 1e-3
EMPTY = 1e-12
STEPS = 6
U32 = 2.0 ** -24
Q_TOL = 5e-5
ERFF_ULP = 2.0
OVERLAP_C = 12.0 + 2.0 * ERFF_ULP
CONDITION = 0.02
assert OVERLAP_C <= 32.0

H_ROW = (7.17, 6.24, -0.56)
H_PLUS = 20.02
# element -> {class or "any": (a, b, c)}: the Gasteiger-Marsili values as the literature gives them
ROWS = {6: {HR.TETRAHEDRAL: (7.98, 9.18, 1.88), HR.PLANAR: (8.79, 9.32, 1.51), HR.LINEAR: (10.39, 9.45, 0.73)},
        7: {HR.TETRAHEDRAL: (11.54, 10.82, 1.36), HR.PLANAR: (12.87, 11.15, 0.85), HR.LINEAR: (15.68, 11.70, -0.27)},
        8: {HR.TETRAHEDRAL: (14.18, 12.92, 1.39), HR.PLANAR: (17.07, 13.79, 0.47), HR.LINEAR: (17.07, 13.79, 0.47)},
        9: {"any": (14.66, 13.85, 2.31)}, 17: {"any": (11.00, 9.69, 1.35)}, 35: {"any": (10.08, 8.47, 1.16)},
        15: {"any": (8.90, 8.24, 0.96)},
        16: {HR.TETRAHEDRAL: (10.14, 9.13, 1.38), HR.PLANAR: (10.88, 9.49, 1.33), HR.LINEAR: (10.88, 9.49, 1.33),
             "oxo": (12.00, 10.81, 1.20)},
        1: {"any": H_ROW}}


def swapped_rows():
    """The mutation: tetrahedral and planar carbon exchanged."""
    rows = {z: dict(r) for z, r in ROWS.items()}
    rows[6][HR.TETRAHEDRAL], rows[6][HR.PLANAR] = ROWS[6][HR.PLANAR], ROWS[6][HR.TETRAHEDRAL]
    return rows


def parameters(z, adj, n, rows=ROWS):
    """Per atom (a, b, c), or None for an element without a row."""
    hyb = HR.hybridisation(z, adj, n)
    out = []
    for a in range(n):
        row = rows.get(z[a])
        if row is None:
            out.append(None)
        elif z[a] == 16 and sum(1 for j in range(n) if j != a and adj[a][j] == 2 and z[j] == 8) >= 2:
            out.append(row["oxo"])
        else:
            out.append(row.get("any") or row[hyb[a]])
    return out


def charges(z, adj, n, rows=ROWS):
    """dict: q [n] heavy-atom charges, q_h [n] the charge of EACH hydrogen of that atom (0 where it has none), nh [n],
    status (1: an element without parameters - every charge NaN)."""
    nh = HR.counts(z, adj, n)
    abc = parameters(z, adj, n, rows)
    if any(p is None for p in abc):
        return dict(q=[math.nan] * n, q_h=[math.nan] * n, nh=nh, status=1)
    nb = [[j for j in range(n) if j != a and adj[a][j] in (1, 2, 3, 4)] for a in range(n)]
    plus = [H_PLUS if z[a] == 1 else p[0] + p[1] + p[2] for a, p in enumerate(abc)]

    def chi(p, q):
        return p[0] + p[1] * q + p[2] * q * q

    def flow(ci, pi, cj, pj):
        return (cj - ci) / (pi if cj > ci else pj)

    q, qh = [0.0] * n, [0.0] * n
    for k in range(1, STEPS + 1):
        damp = 0.5 ** k
        c = [chi(abc[a], q[a]) for a in range(n)]
        ch = [chi(H_ROW, qh[a]) for a in range(n)]
        nq, nqh = list(q), list(qh)
        for a in range(n):
            s = 0.0
            for j in nb[a]:
                s += flow(c[a], plus[a], c[j], plus[j])
            if nh[a] > 0:
                f = flow(c[a], plus[a], ch[a], H_PLUS)
                s += nh[a] * f
                nqh[a] = qh[a] - damp * f
            nq[a] = q[a] + damp * s
        q, qh = nq, nqh
    return dict(q=q, q_h=[qh[a] if nh[a] > 0 else 0.0 for a in range(n)], nh=nh, status=0)


def total_charge(ch):
    return sum(ch["q"]) + sum(h * v for h, v in zip(ch["nh"], ch["q_h"]))


def points(n, xyz, ch, placed):
    """(xyz [P,3] fp64, q [P] fp64): the heavy atoms in order with q, then the placed hydrogens in the placement's output
    order, each with its parent's q_h; the hydrogens the count rule gives but the placement has no direction for add their
    charge to their parent's point.  `placed`: a `hydrogens_ref.place` result (or any dict with counts, parents, coords)."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)[:n]
    q = [ch["q"][a] + (ch["nh"][a] - placed["counts"][a]) * ch["q_h"][a] if ch["nh"][a] > placed["counts"][a] else ch["q"][a]
         for a in range(n)]
    hx = np.asarray(placed["coords"], dtype=np.float64).reshape(-1, 3)
    q += [ch["q_h"][p] for p in placed["parents"]]
    return np.vstack([x, hx]) if len(hx) else x, np.array(q, dtype=np.float64)


def kernel(r, mu=MU):
    """K(r) = erf(mu r) / r, the Coulomb energy of two unit Gaussian charges; its series below 1e-3."""
    if r < SMALL_R:
        return mu * (2.0 / math.sqrt(math.pi)) * (1.0 - (mu * r) ** 2 / 3.0)
    return math.erf(mu * r) / r


_ERF = np.vectorize(math.erf, otypes=[np.float64])


def overlap(xa, qa, xb, qb, mu=MU, drop=None):
    """(E, S): E(A,B) = sum_i sum_j qa_i qb_j K(|a_i - b_j|) and S = sum |term|, every term by `kernel`'s two branches.
    `drop`: the (i, j) of one term left out (the mutation)."""
    xa, xb = np.asarray(xa, dtype=np.float64).reshape(-1, 3), np.asarray(xb, dtype=np.float64).reshape(-1, 3)
    qa, qb = np.asarray(qa, dtype=np.float64).reshape(-1), np.asarray(qb, dtype=np.float64).reshape(-1)
    if not len(qa) or not len(qb):
        return 0.0, 0.0
    d = xa[:, None, :] - xb[None, :, :]
    r = np.sqrt((d * d).sum(axis=2))
    near = r < SMALL_R
    k = np.where(near, mu * (2.0 / math.sqrt(math.pi)) * (1.0 - (mu * r) ** 2 / 3.0), _ERF(mu * r) / np.where(near, 1.0, r))
    t = qa[:, None] * qb[None, :] * k
    if drop is not None:
        t[drop] = 0.0
    return float(math.fsum(t.reshape(-1).tolist())), float(math.fsum(np.abs(t).reshape(-1).tolist()))


def tanimoto(e_rm, e_rr, e_mm):
    d = e_rr + e_mm - e_rm
    return 0.0 if d < EMPTY else e_rm / d


def score(ref_pts, mol_pts, mu=MU):
    """dict of the three overlaps, their S, the Tanimoto and the three tolerances of the pass rules."""
    (xr, qr), (xm, qm) = ref_pts, mol_pts
    rm, s_rm = overlap(xm, qm, xr, qr, mu)
    rr, s_rr = overlap(xr, qr, xr, qr, mu)
    mm, s_mm = overlap(xm, qm, xm, qm, mu)
    tol = {k: OVERLAP_C * U32 * s for k, s in (("cross", s_rm), ("ref", s_rr), ("self", s_mm))}
    t = tanimoto(rm, rr, mm)
    return dict(cross=rm, ref=rr, self=mm, s_cross=s_rm, s_ref=s_rr, s_self=s_mm, tanimoto=t, tol=tol,
                tol_tanimoto=tanimoto_tolerance(rm, rr, mm, tol["cross"], tol["ref"], tol["self"]))


def tanimoto_tolerance(c, rr, m, dc, drr, dm):
    d = rr + m - c
    if d < EMPTY:
        return 0.0
    return (abs(d + c) * dc + abs(c) * (drr + dm)) / (d * d) + U32 * abs(c / d) * ((abs(rr) + abs(m)) / d + 2.0)
