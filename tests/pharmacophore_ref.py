"""Plain-Python restatement of the pharmacophore features and their overlap score ("Pharmacophore
overlap"), written from nothing but that definition: what `tests/test_pharmacophore_host.py` and
`tests/test_pharmacophore_gpu.py` hold the HIP kernels to.  Perception is integer logic on (z, adj, n) - atomic numbers, a
symmetric n x n list of bond codes (1 / 2 / 3 / 4 aromatic; anything else is no bond) and the atom count; the score is
fp64 over the fp32 feature positions.  Every rule is a function of `RULES`, so the mutation check can drop one."""
import math

import numpy as np

D, A, P, N, H = 1, 2, 4, 8, 16                  # per-atom type bits
TYPE_NAMES = ("donor", "acceptor", "cation", "anion", "hydrophobe", "ring")
RING = 5                                        # type index of a ring feature (the atom bits are indices 0..4)
KAPPA = 0.5                                     # 1/A^2: a unit-width Gaussian
MATCH_D2 = 2.25                                 # (1.5 A)^2
MAX_RINGS = 32
MAX_FEATURES = 64 * 5 + MAX_RINGS
V0 = {5: 3, 6: 4, 7: 3, 8: 2, 9: 1, 14: 4, 15: 3, 16: 2, 17: 1, 33: 3, 34: 2, 35: 1, 53: 1}
W2 = {1: 2, 2: 4, 3: 6, 4: 3}
RULES = frozenset(["D_plain", "D_aromatic", "A_oxygen", "A_nitrogen", "A_aromatic", "P", "N", "H_carbon", "H_halogen",
                   "R"])

# ---- pass rules of the GPU score (tests/test_pharmacophore_gpu.py) --------------------------------------------------
# |T - T64| <= SCORE_C * 2^-24, and |O - O64| <= SCORE_C * 2^-24 * O64 for o_rm and o_mm.  SCORE_C = 4 x the worst value
# MEASURED on the MI355X over the score cases of tests/pharmacophore_cases.py (`score_cases`): every term is fp32
# expf(-kappa d2) of an fp32 d2, so a term is off by expf's last place plus kappa * d2 * (the rounding of d2) - the sums
# themselves are fp64 and add nothing that shows at this scale.
# Measured worst |err| / 2^-24: o_rm / O64 11.97 - the one-feature reference against the one-atom candidate 4.6 A away, a
# single term of 2.1e-5 with kappa d2 = 10.8, where the rounding of d2 alone moves the exponent by about 10.8 * 2^-23;
# o_mm / O64 0.134, T 0.133, O(R,R) 0.016.
SCORE_C_MEASURED = 11.98
SCORE_C = 4.0 * SCORE_C_MEASURED                # 47.9: 2.9e-6 on T
# the kappa mutation (kappa * 1.01) moves T of the pinned score case by 3.06e-3 = 1 071 x that bound
# (test_pharmacophore_host.py::test_mutations_are_caught prints the figure and asserts a ratio above 100)
EPS32 = 2.0 ** -24
# one of the six per-type parts may be a single far pair, so it gets a bound by reasoning instead: a term that is not zero
# has kappa * d2 < 88; d2 (three differences, three products, two sums) is off by at most 5 * 2^-24 relative, which moves
# the exponent by 5 * 88 * 2^-24, and expf by its last place (2 * 2^-24 covers it); below 1e-37 fp32 terms are denormal
PART_REL = (2 + 5 * 88) * EPS32


def neighbours(z, adj, n):
    return [[j for j in range(n) if j != a and adj[a][j] in W2] for a in range(n)]


def atom_quantities(z, adj, n):
    """Per atom: (deg, v2, narom, nH)."""
    out = []
    for a, nb in enumerate(neighbours(z, adj, n)):
        v2 = sum(W2[adj[a][j]] for j in nb)
        narom = sum(1 for j in nb if adj[a][j] == 4)
        out.append((len(nb), v2, narom, max(0, (2 * V0.get(z[a], 0) - v2) // 2)))
    return out


def rings(z, adj, n, dedupe=True, stats=None):
    """The aromatic rings as member masks, ascending.  `dedupe=False` (the mutation): every closed path counts, from
    every member and in both directions.  `stats`: a dict that receives the largest number of full-length paths walked
    from one start atom."""
    q = atom_quantities(z, adj, n)
    ok = [2 <= q[a][2] <= 3 and q[a][0] <= 4 for a in range(n)]
    arom = [[j for j in range(n) if j != a and adj[a][j] == 4 and ok[a] and ok[j]] for a in range(n)]
    found, worst = [], 0
    for s in range(n):
        leaves = 0
        stack = [[s]]
        while stack:
            path = stack.pop()
            last = path[-1]
            if len(path) in (5, 6) and s in arom[last]:
                found.append((s, tuple(path)))
            if len(path) == 6:
                leaves += 1
                continue
            for j in arom[last]:
                if j not in path:
                    stack.append(path + [j])
        worst = max(worst, leaves)
    if stats is not None:
        stats["paths"] = worst
    masks = [sum(1 << a for a in path) for s, path in found if not dedupe or s == min(path)]
    return sorted(set(masks)) if dedupe else sorted(masks)


def perceive(z, adj, n, rules=RULES, swap_da=False, dedupe=True):
    """(types [n] bit masks, ring masks ascending, nH [n])."""
    q = atom_quantities(z, adj, n)
    nb = neighbours(z, adj, n)
    ring_list = rings(z, adj, n, dedupe)
    aromatic = [q[a][2] >= 1 for a in range(n)]

    def codes(a):
        return [adj[a][j] for j in nb[a]]

    def arom_n2(a):
        return z[a] == 7 and aromatic[a] and q[a][0] == 2

    def donor_rings(a):
        """The 5-rings that make the aromatic N `a` a donor."""
        out = []
        for m in ring_list:
            members = [k for k in range(n) if m >> k & 1]
            if a in members and len(members) == 5 and not any(z[k] in (8, 16, 34) for k in members) and \
                    not any(z[k] == 7 and aromatic[k] and q[k][0] == 3 for k in members):
                out.append(members)
        return out

    types = []
    for a in range(n):
        deg, v2, narom, nh = q[a]
        t = 0
        if V0.get(z[a], 0) == 0:
            types.append(0)
            continue
        if "D_plain" in rules and z[a] in (7, 8) and not aromatic[a] and nh >= 1:
            t |= D
        dr = donor_rings(a) if arom_n2(a) else []
        if "D_aromatic" in rules and dr:
            t |= D
        if "A_oxygen" in rules and z[a] == 8 and narom == 0 and v2 <= 4:
            t |= A
        if "A_nitrogen" in rules and z[a] == 7 and not aromatic[a] and any(c in (2, 3) for c in codes(a)) and v2 <= 6:
            t |= A
        if "A_aromatic" in rules and arom_n2(a):
            alone = bool(dr) and not any(sum(1 for k in members if arom_n2(k)) >= 2 for members in dr)
            if not alone:
                t |= A
        if "P" in rules and z[a] == 7 and not aromatic[a] and deg >= 1 and all(c == 1 for c in codes(a)) and \
                not any(aromatic[j] for j in nb[a]) and \
                not any(adj[j][k] == 2 and z[k] in (8, 16) for j in nb[a] for k in nb[j]):
            t |= P
        if "N" in rules and z[a] in (6, 16, 15):
            o1 = [j for j in nb[a] if z[j] == 8 and q[j][0] == 1]
            if any(adj[a][j] == 2 for j in o1) and any(adj[a][j] == 1 for j in o1):
                t |= N
        if "H_carbon" in rules and z[a] == 6 and not aromatic[a] and all(z[j] == 6 for j in nb[a]):
            t |= H
        if "H_halogen" in rules and z[a] in (17, 35, 53):
            t |= H
        if swap_da:
            t = (t & ~3) | ((t & D) << 1) | ((t & A) >> 1)
        types.append(t)
    return types, (ring_list if "R" in rules else []), [v[3] for v in q]


def features(coords, types, ring_list):
    """The feature set at fp32 `coords` [n,3]: a list of (type index, fp32 xyz [3]) - per atom in ascending index its types
    in ascending bit order, then the rings in list order, each at the fp32 centroid of its members (summed in ascending
    atom index, one division)."""
    xyz = np.asarray(coords, dtype=np.float32).reshape(-1, 3)
    out = []
    for a, t in enumerate(types):
        for k in range(5):
            if t >> k & 1:
                out.append((k, xyz[a].copy()))
    for m in ring_list:
        members = [k for k in range(64) if m >> k & 1]
        acc = np.zeros(3, dtype=np.float32)
        for k in members:
            acc = (acc + xyz[k]).astype(np.float32)
        out.append((RING, (acc / np.float32(len(members))).astype(np.float32)))
    return out


def overlap(fa, fb, kappa=KAPPA, per_type=False):
    """O(A, B) in fp64 (or its six per-type parts)."""
    parts = [0.0] * 6
    for t in range(6):
        a = np.array([p for k, p in fa if k == t], dtype=np.float64).reshape(-1, 1, 3)
        b = np.array([p for k, p in fb if k == t], dtype=np.float64).reshape(1, -1, 3)
        if a.size and b.size:
            parts[t] = float(np.exp(-kappa * ((a - b) ** 2).sum(-1)).sum())
    return parts if per_type else math.fsum(parts)


def tanimoto(fr, fm, kappa=KAPPA):
    o_rm, o_rr, o_mm = overlap(fr, fm, kappa), overlap(fr, fr, kappa), overlap(fm, fm, kappa)
    return o_rm / (o_rr + o_mm - o_rm)


def d2_fp32(pa, pb):
    """dx*dx + dy*dy + dz*dz in fp32, every operation rounded (no contraction)."""
    d = (np.asarray(pa, dtype=np.float32) - np.asarray(pb, dtype=np.float32)).astype(np.float32)
    sq = (d * d).astype(np.float32)
    return np.float32(np.float32(sq[0] + sq[1]) + sq[2])


def matches(fr, fm):
    """Reference features with a candidate feature of the same type within 1.5 A."""
    return sum(1 for tr, pr in fr if any(tm == tr and d2_fp32(pr, pm) <= np.float32(MATCH_D2) for tm, pm in fm))


def score(fr, coords, z, adj, n):
    """What the score kernel reports of one candidate against the reference features `fr`: dict of `o_rm`, `o_mm`,
    `tanimoto`, `matches`, `per_type` - NaN / -1 for a non-finite coordinate on a real atom or more than 32 rings."""
    xyz = np.asarray(coords, dtype=np.float32).reshape(-1, 3)[:n]
    types, ring_list, _ = perceive(z, adj, n)
    if not np.isfinite(xyz).all() or len(ring_list) > MAX_RINGS:
        nan = float("nan")
        return dict(o_rm=nan, o_mm=nan, tanimoto=nan, matches=-1, per_type=[nan] * 6)
    fm = features(xyz, types, ring_list)
    parts = overlap(fr, fm, per_type=True)
    o_rm, o_mm, o_rr = math.fsum(parts), overlap(fm, fm), overlap(fr, fr)
    return dict(o_rm=o_rm, o_mm=o_mm, tanimoto=o_rm / (o_rr + o_mm - o_rm), matches=matches(fr, fm), per_type=parts)


def mol(zs, bonds):
    """(z, adj, n) from atomic numbers and (i, j, code) bonds."""
    n = len(zs)
    adj = [[0] * n for _ in range(n)]
    for i, j, c in bonds:
        adj[i][j] = adj[j][i] = c
    return list(zs), adj, n


def permute(z, adj, n, p):
    """The same molecule with new atom i = old atom p[i]."""
    return [z[p[i]] for i in range(n)], [[adj[p[i]][p[j]] for j in range(n)] for i in range(n)], n


def permute_mask(m, p):
    """A ring mask of the molecule before `permute(..., p)` as a mask of the molecule after it."""
    inv = {old: new for new, old in enumerate(p)}
    return sum(1 << inv[k] for k in range(len(p)) if m >> k & 1)
