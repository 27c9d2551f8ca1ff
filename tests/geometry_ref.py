"""fp64 restatement of the relaxed-geometry force field and minimiser ("Relaxed geometry";
`ml_conformer_generator_amd/geometry.py`, csrc/mcg_geometry.hip), the analytic test molecules and the two pass rules of
tests/test_geometry_host.py and tests/test_geometry_gpu.py.  numpy only: no torch, no GPU.

The force field is the package's OWN (not MMFF94).  Every constant lives in `PARAMS`; every function takes the
parameters as an argument so that the mutation check can change one of them.
"""
import math

import numpy as np

from ml_conformer_generator_amd.config import ELEMENTS

NONE, BOND, ANGLE, NONBONDED = 0, 1, 2, 3
U32 = 2.0 ** -24                                  # unit roundoff of fp32

PARAMS = {
    "k_bond": 600.0, "k_angle": 150.0, "k_nonbonded": 100.0,
    "s_single": 0.0, "s_aromatic": 0.13, "s_double": 0.18, "s_triple": 0.32,
    "nonbonded_margin": 0.9,
    "restraint_flat": 0.2, "restraint_k": 800.0,
    "theta_linear": 180.0, "theta_trigonal": 120.0, "theta_tetrahedral": 109.47,
    "theta_five_ring": 108.0, "theta_four_ring": 90.0,
}
# what the mutation check changes by 1 % (s_single is 0: 1 % of it is no change)
MUTABLE = [k for k in PARAMS if k != "s_single"]
RCOV = {z: r for z, (_, r, _) in ELEMENTS.items()}
STEP0, GROW, SHRINK = 0.02, 1.2, 0.5

# ---- rule (a): energy and gradient at given coordinates -----------------------------------------------------------------
# |E_gpu - E_ref| <= C_A * 2^-24 * S_E and, per atom and component, |g_gpu - g_ref| <= C_A * 2^-24 * S_g[i], with the term
# sums of `evaluate`: an fp32 distance and its d0 each carry a few units of relative error, so (r - d0) is off by about
# 2^-24 (r + d0), a pair energy by k |r - d0| 2^-24 (r + d0) (+ the second-order k (2^-24 (r + d0))^2), a pair force by
# k 2^-24 (r + d0) (+ k |r - d0| 2^-24 from its direction); the sums add |E| for the accumulation.
# C_A = 4 x the worst ratio err / (2^-24 S) measured on the MI355X over `rule_a_cases()`:
#   worst energy ratio 0.649, worst gradient ratio 0.707 (both tri_nitrile); the other cases 0.03 .. 0.63
MEASURED_RATIO_A = 0.707
C_A = 4.0 * MEASURED_RATIO_A

# ---- rule (b): relaxed coordinates and end energy against the fp64 minimiser --------------------------------------------
# max atom |x_gpu - x_ref| <= TOL_B_COORD and |E_gpu - E_ref| <= TOL_B_ENERGY after 200 steps over `recovery_cases()`:
# 5 x the deviation measured on the MI355X.  fp32 and fp64 may take different accept / reject branches, so this is a
# statement about two minimisers ending in the same place, not about rounding.
#   measured worst (fused56 at 0.1 A, restraint active): coordinates 3.053e-4 A, energy 9.095e-4 kcal/mol; the same
#   accepted-step counts as fp64 in all four cases; benzene agrees to 3.9e-6 A and 3.2e-7
MEASURED_COORD_B = 3.053e-4
MEASURED_ENERGY_B = 9.095e-4
TOL_B_COORD = 5.0 * MEASURED_COORD_B
TOL_B_ENERGY = 5.0 * MEASURED_ENERGY_B


def _cos(deg):
    # the kernel's constants: 90, 120 and 180 degrees are exact
    exact = {90.0: 0.0, 120.0: -0.5, 180.0: -1.0}
    return exact.get(float(deg), math.cos(math.radians(deg)))


def _shrink(code, P):
    return {1: P["s_single"], 2: P["s_double"], 3: P["s_triple"], 4: P["s_aromatic"]}[int(code)]


def topology(z, bonds, P=PARAMS):
    """(class [n,n] int, d0 [n,n] fp64) of a molecule: atomic numbers [n], symmetric bond codes [n,n] (0 / 1 / 2 / 3 / 4)."""
    z = [int(v) for v in z]
    n = len(z)
    bonds = np.asarray(bonds).astype(np.int64).reshape(n, n)
    for v in z:
        if v not in RCOV:
            raise ValueError(f"no covalent radius for Z = {v}")
    rc = [RCOV[v] for v in z]
    nbr = [set(int(j) for j in np.nonzero(bonds[i])[0] if j != i) for i in range(n)]

    def bond_d0(i, j):
        return rc[i] + rc[j] - _shrink(bonds[i, j], P)

    def theta0(j):
        codes = [int(bonds[j, m]) for m in nbr[j]]
        if 3 in codes or codes.count(2) >= 2:
            return P["theta_linear"]
        if 2 in codes or 4 in codes:
            return P["theta_trigonal"]
        return P["theta_tetrahedral"]

    cls = np.zeros((n, n), dtype=np.int64)
    d0 = np.zeros((n, n))
    for i in range(n):
        for k in range(n):
            if i == k:
                continue
            if bonds[i, k] != 0:
                cls[i, k], d0[i, k] = BOND, bond_d0(i, k)
                continue
            common = nbr[i] & nbr[k]
            if not common:
                cls[i, k], d0[i, k] = NONBONDED, rc[i] + rc[k] + P["nonbonded_margin"]
                continue
            best = math.inf
            for j in sorted(common):
                theta = theta0(j)
                if len(common) >= 2:
                    theta = P["theta_four_ring"]
                elif any((nbr[a] & (nbr[k] - {j})) for a in nbr[i] - {j}):
                    theta = min(theta, P["theta_five_ring"])
                la, lb = bond_d0(i, j), bond_d0(j, k)
                best = min(best, math.sqrt(la * la + lb * lb - 2.0 * la * lb * _cos(theta)))
            cls[i, k], d0[i, k] = ANGLE, best
    return cls, d0


def evaluate(x, x0, topo, P=PARAMS):
    """dict(E, grad [n,3], S_E, S_g [n]) at the coordinates x [n,3], restrained to x0: the energy, its gradient and the term
    sums of rule (a), all fp64."""
    cls, d0 = topo
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    n = x.shape[0]
    d = x[:, None, :] - x[None, :, :]
    r = np.sqrt((d * d).sum(-1))
    diff = r - d0
    one_sided = (cls == NONBONDED)
    k = np.where(cls == BOND, P["k_bond"], np.where(cls == ANGLE, P["k_angle"],
                 np.where(one_sided & (diff < 0.0), P["k_nonbonded"], 0.0)))
    k_sum = np.where(one_sided & (diff < 1e-5), P["k_nonbonded"], k)       # the side a rounded distance may fall on
    iu = np.triu_indices(n, 1)
    E_pair = float((0.5 * k * diff * diff)[iu].sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(r > 0.0, k * diff / np.where(r > 0.0, r, 1.0), 0.0)
    grad = (f[:, :, None] * d).sum(1)
    span = r + d0
    S_E = float((k_sum * (np.abs(diff) * span + U32 * span * span))[iu].sum())
    S_g = (k_sum * (span + np.abs(diff))).sum(1)
    dx = x - x0
    u = np.sqrt((dx * dx).sum(-1))
    over = np.maximum(u - P["restraint_flat"], 0.0)
    E_res = float((0.5 * P["restraint_k"] * over * over).sum())
    fr = np.where(u > 0.0, P["restraint_k"] * over / np.where(u > 0.0, u, 1.0), 0.0)
    grad = grad + fr[:, None] * dx
    near = (u - P["restraint_flat"]) > -1e-5
    uspan = u + P["restraint_flat"]
    S_E += float((near * P["restraint_k"] * (over * uspan + U32 * uspan * uspan)).sum())
    S_g = S_g + near * P["restraint_k"] * (uspan + over)
    E = E_pair + E_res
    return dict(E=E, grad=grad, S_E=S_E + abs(E), S_g=S_g)


def minimise(x, x0, topo, steps, P=PARAMS):
    """The kernel's minimiser in fp64: dict(x, E_start, E, accepted)."""
    x = np.array(x, dtype=np.float64)
    ev = evaluate(x, x0, topo, P)
    E0 = E = ev["E"]
    g = ev["grad"]
    gmax = float(np.sqrt((g * g).sum(-1)).max()) if len(x) else 0.0
    s, accepted = STEP0, 0
    for _ in range(steps):
        if not gmax > 0.0:
            break
        xt = x - (s / gmax) * g
        et = evaluate(xt, x0, topo, P)
        if et["E"] < E:
            x, E, g = xt, et["E"], et["grad"]
            gmax = float(np.sqrt((g * g).sum(-1)).max())
            accepted += 1
            s *= GROW
        else:
            s *= SHRINK
    return dict(x=x, E_start=E0, E=E, accepted=accepted)


def rule_a(E_got, grad_got, ref, c=C_A):
    """(passes, energy ratio, gradient ratio) of an energy and a gradient [n,3] against `evaluate`'s result `ref`; a ratio
    is err / (2^-24 S), 0 where the error is 0, inf where the error is not 0 and S is."""
    def ratio(err, s):
        if err == 0.0:
            return 0.0
        return err / (U32 * s) if s > 0.0 else math.inf
    e_ratio = ratio(abs(float(E_got) - ref["E"]), ref["S_E"])
    g_err = np.abs(np.asarray(grad_got, dtype=np.float64) - ref["grad"]).max(axis=1) if len(ref["S_g"]) else np.zeros(0)
    g_ratio = max([ratio(float(e), float(s)) for e, s in zip(g_err, ref["S_g"])] + [0.0])
    return (e_ratio <= c and g_ratio <= c), e_ratio, g_ratio


def bonded_rms(x, topo):
    """RMS deviation of the bonded distances from their d0."""
    cls, d0 = topo
    x = np.asarray(x, dtype=np.float64)
    iu = np.triu_indices(len(x), 1)
    r = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    sel = cls[iu] == BOND
    return float(np.sqrt((((r - d0)[iu][sel]) ** 2).mean()))


def min_nonbonded_distance(x, topo):
    cls, _ = topo
    x = np.asarray(x, dtype=np.float64)
    iu = np.triu_indices(len(x), 1)
    r = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    return float(r[iu][cls[iu] == NONBONDED].min())


# ---- molecules -----------------------------------------------------------------------------------------------------------
def _mol(name, z, pairs, x, x0=None):
    """A case: `pairs` = [(i, j, code)]; coordinates rounded to fp32 (what the kernel is given), kept as fp64."""
    n = len(z)
    bonds = np.zeros((n, n), dtype=np.int8)
    for i, j, c in pairs:
        bonds[i, j] = bonds[j, i] = c
    x = np.asarray(x, dtype=np.float64).reshape(n, 3).astype(np.float32).astype(np.float64)
    x0 = x if x0 is None else np.asarray(x0, dtype=np.float64).reshape(n, 3).astype(np.float32).astype(np.float64)
    return dict(name=name, z=list(z), bonds=bonds, x=x, x0=x0)


def noisy(case, sigma, seed):
    """The case with seeded Gaussian noise of `sigma` A on every coordinate (the restraint then holds to the noisy start)."""
    rng = np.random.RandomState(seed)
    x = case["x"] + rng.normal(0.0, sigma, size=case["x"].shape)
    return _mol(f"{case['name']}+{sigma}", case["z"], [(i, j, int(case["bonds"][i, j])) for i in range(len(x))
                                                       for j in range(i)
                                                       if case["bonds"][i, j]], x)


def regular_ring(n, code, name=None, z=6, centre=(0.0, 0.0, 0.0), phase=0.0):
    """A regular planar n-ring of one element at the field's own bond d0."""
    side = 2.0 * RCOV[z] - _shrink(code, PARAMS)
    R = side / (2.0 * math.sin(math.pi / n))
    x = [(centre[0] + R * math.cos(phase + 2 * math.pi * m / n), centre[1] + R * math.sin(phase + 2 * math.pi * m / n),
          centre[2]) for m in range(n)]
    return _mol(name or f"ring{n}", [z] * n, [(m, (m + 1) % n, code) for m in range(n)], x)


def zigzag(n, name=None, z=None, codes=None, origin=(0.0, 0.0, 0.0), angle=109.47):
    """A planar zigzag chain: bond lengths the field's d0 of each bond, one angle at every centre."""
    z = [6] * n if z is None else list(z)
    codes = [1] * (n - 1) if codes is None else list(codes)
    half = math.radians(angle) / 2.0
    x, p = [], np.array(origin, dtype=np.float64)
    for m in range(n):
        x.append(p.copy())
        if m < n - 1:
            L = RCOV[z[m]] + RCOV[z[m + 1]] - _shrink(codes[m], PARAMS)
            p = p + np.array([L * math.sin(half), L * math.cos(half) * (1 if m % 2 == 0 else -1), 0.0])
    return _mol(name or f"chain{n}", z, [(m, m + 1, codes[m]) for m in range(n - 1)], x)


def fused56():
    """An indane-like 5-6 system: a regular aromatic six-ring and a five-ring of single bonds sharing one (aromatic) edge,
    9 atoms, planar.  The five-ring is regular on the shared edge's length, so it is close to, not at, the field's d0's."""
    six = regular_ring(6, 4)
    a, b = six["x"][0], six["x"][1]                   # the shared edge; the five-ring grows away from the six-ring's centre
    mid = (a + b) / 2.0
    out = mid / np.linalg.norm(mid)
    side = np.linalg.norm(b - a)
    R5 = side / (2.0 * math.sin(math.pi / 5))
    c5 = mid + out * (R5 * math.cos(math.pi / 5))
    ang0 = math.atan2(b[1] - c5[1], b[0] - c5[0])
    extra = [c5 + R5 * np.array([math.cos(ang0 + 2 * math.pi * m / 5), math.sin(ang0 + 2 * math.pi * m / 5), 0.0])
             for m in (1, 2, 3)]
    if np.linalg.norm(extra[-1] - a) > 1.5 * side:    # wrong sense of rotation: walk the other way round
        extra = [c5 + R5 * np.array([math.cos(ang0 - 2 * math.pi * m / 5), math.sin(ang0 - 2 * math.pi * m / 5), 0.0])
                 for m in (1, 2, 3)]
    x = np.vstack([six["x"], np.array(extra)])
    pairs = [(m, (m + 1) % 6, 4) for m in range(6)] + [(1, 6, 1), (6, 7, 1), (7, 8, 1), (8, 0, 1)]
    return _mol("fused56", [6] * 9, pairs, x)


def polyphenyl(n_atoms, name):
    """Para-linked benzene rings in one plane (single bonds between the rings) and a zigzag tail of single bonds that
    brings the atom count to `n_atoms`."""
    rings = n_atoms // 6
    R = (2.0 * RCOV[6] - PARAMS["s_aromatic"])
    L = 2.0 * R + 2.0 * RCOV[6]
    x, pairs = [], []
    for k in range(rings):
        for m in range(6):
            x.append((k * L + R * math.cos(math.pi * m / 3), R * math.sin(math.pi * m / 3), 0.0))
            pairs.append((6 * k + m, 6 * k + (m + 1) % 6, 4))
        if k:
            pairs.append((6 * (k - 1), 6 * k + 3, 1))
    tail = n_atoms - 6 * rings
    if tail:
        start = np.array(x[6 * (rings - 1)])
        chain = zigzag(tail + 1, origin=tuple(start))["x"]
        for t in range(1, tail + 1):
            x.append(tuple(chain[t]))
            pairs.append((6 * (rings - 1) if t == 1 else len(x) - 2, len(x) - 1, 1))
    return _mol(name, [6] * n_atoms, pairs, x)


def clash():
    """Two propane chains, one 1.5 A above the other."""
    a = zigzag(3)["x"]
    x = np.vstack([a, a + np.array([0.0, 0.0, 1.5])])
    return _mol("clash", [6] * 6, [(0, 1, 1), (1, 2, 1), (3, 4, 1), (4, 5, 1)], x)


def displaced():
    """Propane restrained to its regular geometry with one end atom 0.5 A away from it: the restraint is active."""
    base = zigzag(3)
    x = base["x"].copy()
    x[2] += np.array([0.3, 0.0, 0.4])
    return _mol("displaced", base["z"], [(0, 1, 1), (1, 2, 1)], x, x0=base["x"])


def hand_cases():
    """The regular molecules, at the field's own d0's (no noise)."""
    return {
        "single": _mol("single", [8], [], [(0.3, -0.2, 0.1)]),
        "ring3": regular_ring(3, 1), "ring4": regular_ring(4, 1), "ring5": regular_ring(5, 1),
        "benzene": regular_ring(6, 4, "benzene"), "cyclohexane": regular_ring(6, 1, "cyclohexane"),
        "fused56": fused56(),
    }


_RULE_A_CASES = None


def rule_a_cases():
    """The molecules of rule (a), built once: name -> case.  All but the first carry seeded noise of 0.05 A, or a
    deliberate strain, so that every term is exercised away from its minimum."""
    global _RULE_A_CASES
    if _RULE_A_CASES is not None:
        return _RULE_A_CASES
    regular = hand_cases()
    base = [regular["ring3"], regular["ring4"], regular["ring5"], regular["benzene"], regular["cyclohexane"],
            regular["fused56"]]
    for code, nm in ((1, "single"), (2, "double"), (3, "triple"), (4, "aromatic")):
        base.append(zigzag(2, f"pair_{nm}", z=[6, 7], codes=[code]))
    base += [zigzag(3, "tri_tetrahedral", z=[6, 8, 6]),
             zigzag(3, "tri_trigonal", codes=[2, 1], angle=120.0),
             zigzag(3, "tri_aromatic", z=[6, 7, 6], codes=[4, 4], angle=120.0),
             zigzag(3, "tri_allene", codes=[2, 2], angle=180.0),
             zigzag(3, "tri_nitrile", z=[6, 6, 7], codes=[1, 3], angle=180.0),
             polyphenyl(63, "polyphenyl63"), polyphenyl(64, "polyphenyl64"), zigzag(64, "chain64",
                                                                                    z=[6, 6, 7, 6, 8, 6, 16, 6] * 8)]
    cases = {"single": regular["single"]}
    for k, c in enumerate(base):
        cases[c["name"]] = dict(noisy(c, 0.05, 100 + k), name=c["name"])
    cases["clash"] = clash()
    cases["displaced"] = displaced()
    _RULE_A_CASES = cases
    return cases


def recovery_cases():
    """(name, sigma, case) of the recovery test: benzene and the 5-6 system under noise of 0.05 and 0.1 A."""
    regular = hand_cases()
    out = []
    for k, nm in enumerate(("benzene", "fused56")):
        for s, sigma in enumerate((0.05, 0.1)):
            out.append((nm, sigma, dict(noisy(regular[nm], sigma, 500 + 10 * k + s), name=f"{nm}@{sigma}")))
    return out


def pad_cases(cases, N=None, W=None):
    """numpy batch of cases: coords [B,N,3] fp32, restraint [B,N,3] fp32, z [B,W] int32, bonds [B,W,W] int8, n [B] int32."""
    n = [len(c["z"]) for c in cases]
    N = max(n + [1]) if N is None else N
    W = max(n + [1]) if W is None else W
    x = np.zeros((len(cases), N, 3), dtype=np.float32)
    x0 = np.zeros((len(cases), N, 3), dtype=np.float32)
    z = np.zeros((len(cases), W), dtype=np.int32)
    bonds = np.zeros((len(cases), W, W), dtype=np.int8)
    for b, c in enumerate(cases):
        x[b, : n[b]], x0[b, : n[b]] = c["x"], c["x0"]
        z[b, : n[b]] = c["z"]
        bonds[b, : n[b], : n[b]] = c["bonds"]
    return x, x0, z, bonds, np.array(n, dtype=np.int32)
