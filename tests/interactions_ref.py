"""Receptor interactions (`interactions.interaction_scores`, DESIGN.md section 6 "Receptor interactions"): the definition
restated - r2, the cut-off decision and d in numpy fp32 in the stated order, everything else in fp64 -, the typing rules
in plain Python, and the rule by which the kernel's fp32 sums pass against the restatement.

The pass rule (`bounds`), with u = 2^-24 the unit roundoff, in three parts.
  1. The per-pair error of d.  The restatement forms r2 and d by the same fp32 operations, each correctly rounded (the
     three products, the two sums, the square root, the radius sum, the difference), so the two d agree bit for bit and
     so do the cut-off decisions; the rule does not lean on that and grants d one rounding of its size, delta = u (8 +
     S), S the largest radius sum: |d| <= 8 + S for a counted pair.
  2. That error through each term by the term's largest slope, plus the fp32 evaluation of the term itself:
       g1 = exp(-(2d)^2)          slope sqrt(2/e) / 0.5 = 1.716; the square is one rounding of the argument a^2, which
                                  moves g by u a^2 g <= u / e; expf's own error EXPF_ULP ulp <= 2 EXPF_ULP u g;
       g2 = exp(-((d-3)/2)^2)     slope sqrt(2/e) / 2 = 0.429; the difference and the square are three roundings of the
                                  argument: 3 u / e; expf as above;
       rep = d^2 (d < 0)          slope 2 |d|; one rounding: u d^2;
       hyd = 1.5 - d              slope 1; one rounding: u;
       hb = d / -0.7              slope 1 / 0.7; one rounding: u.
     ROCm's installation documents no accuracy for expf, so EXPF_ULP = 1 is nominal and the whole bound carries the
     explicit factor FACTOR = 4 x the worst ratio error / bound measured on the MI355X over the cases of
     tests/test_interactions_gpu.py: 0.0534 (a per-atom term of the one-atom receptor), so FACTOR = 0.214.
  3. The summation error K u sum |term|: a term goes through at most K = (the counted pairs of one atom) + 8 rounded
     additions - a lane's own chain (at most every counted pair of its atom), the two levels of the waves' tree and the six
     of the butterfly.
The weighted sum adds the weights' products and four sums: 6 u sum |w_k T_k|; E adds the three roundings of its divisor and
the division: 4 u |E|.  The weights are the fp32 constants the kernel is handed, read in fp64.
"""
import math

import numpy as np
import torch

from ml_conformer_generator_amd import receptor as RC

U = 2.0 ** -24
EXPF_ULP = 1.0
FACTOR = 0.214                # 4 x 0.0534, the worst measured error / bound ("Receptor interactions")
DONOR, ACCEPTOR, HYDROPHOBIC = 1, 2, 4
METALS = (12, 20, 25, 26, 27, 28, 29, 30)
HALOGENS = (9, 17, 35, 53)
RADII = {6: 1.9, 7: 1.8, 8: 1.7, 9: 1.5, 15: 2.1, 16: 2.0, 17: 1.8, 35: 2.0, 53: 2.2, 14: 2.2, **{z: 1.2 for z in METALS}}
_F = lambda v: float(np.float32(v))                     # what the kernel is handed


class Definition:
    """The constants of the definition; the mutation checks change one at a time."""
    def __init__(self, **kw):
        self.w = dict(g1=_F(-0.0356), g2=_F(-0.00516), rep=_F(0.840), hyd=_F(-0.0351), hb=_F(-0.587))
        self.rotor = _F(0.0585)
        self.width1, self.width2, self.offset2 = 0.5, 2.0, 3.0
        self.hyd_full, self.hyd_zero = 0.5, 1.5
        self.hb_full, self.hb_zero = _F(-0.7), 0.0
        self.cutoff2 = 64.0
        self.divide = True
        for k, v in kw.items():
            if k in self.w:
                self.w[k] = v
            else:
                assert hasattr(self, k), k
                setattr(self, k, v)


DEFINITION = Definition()
TERMS = ("g1", "g2", "rep", "hyd", "hb")


def radius(z):
    return RADII.get(int(z), RC.VDW_RADII.get(int(z), RC.DEFAULT_RADIUS))


def radii(zs):
    return np.array([radius(z) for z in zs], dtype=np.float32)


# ----------------------------------------------------------------------------------------------- typing, plain Python
def neighbours(adj, n):
    return [[j for j in range(n) if j != a and 1 <= adj[a][j] <= 4] for a in range(n)]


def ligand_types(z, adj, n, pharm_types):
    """Per atom the bits: donor and acceptor from `pharm_types` (the pharmacophore restatement's), hydrophobic for a C
    without an N or O neighbour and for F, Cl, Br, I."""
    nb = neighbours(adj, n)
    out = []
    for a in range(n):
        t = pharm_types[a] & (DONOR | ACCEPTOR)
        if (z[a] == 6 and not any(z[j] in (7, 8) for j in nb[a])) or z[a] in HALOGENS:
            t |= HYDROPHOBIC
        out.append(t)
    return out


def _connected_without(nb, a, b):
    seen, todo = {a}, [a]
    while todo:
        u = todo.pop()
        for v in nb[u]:
            if (u, v) in ((a, b), (b, a)) or v in seen:
                continue
            seen.add(v)
            todo.append(v)
    return b in seen


def rotatable_bonds(z, adj, n):
    """The code-1 bonds outside every ring whose two ends both have two or more bonded atoms."""
    nb = neighbours(adj, n)
    return sum(1 for a in range(n) for b in range(a + 1, n) if adj[a][b] == 1 and len(nb[a]) >= 2 and len(nb[b]) >= 2
               and not _connected_without(nb, a, b))


_AMINO = set("ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split())
_DONORS = {("ARG", "NE"), ("ARG", "NH1"), ("ARG", "NH2"), ("ASN", "ND2"), ("GLN", "NE2"), ("LYS", "NZ"), ("TRP", "NE1"),
           ("HIS", "ND1"), ("HIS", "NE2"), ("SER", "OG"), ("THR", "OG1"), ("TYR", "OH")}
_ACCEPTORS = {("ASP", "OD1"), ("ASP", "OD2"), ("GLU", "OE1"), ("GLU", "OE2"), ("ASN", "OD1"), ("GLN", "OE1"),
              ("HIS", "ND1"), ("HIS", "NE2"), ("SER", "OG"), ("THR", "OG1"), ("TYR", "OH")}


def receptor_types(xyz, zs, names=None):
    """(types, untemplated) of receptor heavy atoms: `names` [(residue, atom)] from a PDB string, or None."""
    xyz = np.asarray(xyz, dtype=np.float64)
    types, untemplated = [], 0
    polar = [k for k, z in enumerate(zs) if z in (7, 8)]
    for k, z in enumerate(zs):
        t = 0
        if z in (7, 8):
            t = DONOR | ACCEPTOR
            if names is not None:
                res, atom = names[k]
                if res in ("HOH", "WAT", "H2O", "DOD") and z == 8:
                    pass
                elif res in _AMINO and atom == "N" and z == 7:
                    t = 0 if res == "PRO" else DONOR
                elif res in _AMINO and atom in ("O", "OXT") and z == 8:
                    t = ACCEPTOR
                elif res in _AMINO and ((res, atom) in _DONORS or (res, atom) in _ACCEPTORS):
                    t = (DONOR if (res, atom) in _DONORS else 0) | (ACCEPTOR if (res, atom) in _ACCEPTORS else 0)
                else:
                    untemplated += 1
        elif z in METALS:
            t = DONOR
            untemplated += names is not None
        elif z == 6:
            if not any(np.linalg.norm(xyz[k] - xyz[p]) <= 1.75 for p in polar):
                t = HYDROPHOBIC
        elif z in HALOGENS:
            t = HYDROPHOBIC
        types.append(t)
    return types, untemplated


# ----------------------------------------------------------------------------------------------- the restatement
def surface_distances(x, ri, y, rj, cutoff2=64.0):
    """(counted [n,R] bool, d [n,R] fp64 holding the fp32 values) - r2 = dx*dx + dy*dy + dz*dz, the decision r2 < cutoff2
    and d = sqrt(r2) - (R_i + R_j), all in numpy fp32 in exactly this order."""
    x, y = np.asarray(x, dtype=np.float32).reshape(-1, 3), np.asarray(y, dtype=np.float32).reshape(-1, 3)
    dx = x[:, None, 0] - y[None, :, 0]
    dy = x[:, None, 1] - y[None, :, 1]
    dz = x[:, None, 2] - y[None, :, 2]
    r2 = (dx * dx + dy * dy) + dz * dz
    assert r2.dtype == np.float32
    s = np.asarray(ri, dtype=np.float32)[:, None] + np.asarray(rj, dtype=np.float32)[None, :]
    d = np.sqrt(r2) - s
    assert d.dtype == np.float32
    return r2 < np.float32(cutoff2), d.astype(np.float64)


def pair_terms(x, ri, ti, y, rj, tj, defn=DEFINITION):
    """(terms [5,n,R] fp64 - g1, g2, rep, hyd, hb, zero where the pair does not count -, hbond pairs [n,R] bool, d)."""
    counted, d = surface_distances(x, ri, y, rj, defn.cutoff2)
    ti, tj = np.asarray(ti, dtype=np.int64)[:, None], np.asarray(tj, dtype=np.int64)[None, :]
    g1 = np.exp(-(d / defn.width1) ** 2)
    g2 = np.exp(-((d - defn.offset2) / defn.width2) ** 2)
    rep = np.where(d < 0, d * d, 0.0)
    both = ((ti & HYDROPHOBIC) != 0) & ((tj & HYDROPHOBIC) != 0)
    hyd = np.where(d <= defn.hyd_full, 1.0, np.where(d >= defn.hyd_zero, 0.0,
                                                     (defn.hyd_zero - d) / (defn.hyd_zero - defn.hyd_full)))
    facing = (((ti & DONOR) != 0) & ((tj & ACCEPTOR) != 0)) | (((ti & ACCEPTOR) != 0) & ((tj & DONOR) != 0))
    hb = np.where(d <= defn.hb_full, 1.0, np.where(d >= defn.hb_zero, 0.0,
                                                   (defn.hb_zero - d) / (defn.hb_zero - defn.hb_full)))
    terms = np.stack([g1, g2, rep, np.where(both, hyd, 0.0), np.where(facing, hb, 0.0)]) * counted[None]
    return terms, counted & facing & (d <= defn.hb_full), d


def score(x, ri, ti, y, rj, tj, n_rot, defn=DEFINITION):
    """dict of one molecule: atom_terms [n,5], atom_scores [n], terms [5], weighted, score, hbonds."""
    n = np.asarray(x).reshape(-1, 3).shape[0]
    if n == 0:
        return dict(atom_terms=np.zeros((0, 5)), atom_scores=np.zeros(0), terms=np.zeros(5), weighted=0.0, score=0.0,
                    hbonds=0)
    t, hbond, _ = pair_terms(x, ri, ti, y, rj, tj, defn)
    w = np.array([defn.w[k] for k in TERMS])
    atom_terms = t.sum(axis=2).T
    terms = atom_terms.sum(axis=0)
    weighted = float(w @ terms)
    return dict(atom_terms=atom_terms, atom_scores=atom_terms @ w, terms=terms, weighted=weighted,
                score=weighted / (1.0 + defn.rotor * n_rot) if defn.divide else weighted, hbonds=int(hbond.sum()))


# ----------------------------------------------------------------------------------------------- the pass rule
_SLOPE = (math.sqrt(2 / math.e) / 0.5, math.sqrt(2 / math.e) / 2.0, None, 1.0, 1.0 / 0.7)


def bounds(x, ri, ti, y, rj, tj, n_rot, defn=DEFINITION, factor=None):
    """dict of how far the kernel's fp32 values may lie from `score(...)`: atom_terms [n,5], atom_scores [n], terms [5],
    weighted, score - by the derivation of this module's docstring."""
    factor = FACTOR if factor is None else factor
    t, _, d = pair_terms(x, ri, ti, y, rj, tj, defn)
    on = t[0] > 0                                                       # the counted pairs: g1 > 0 on every one of them
    S = float(np.max(ri) + np.max(rj))
    delta = U * (8.0 + S)
    g1, g2, rep, hyd, hb = t
    per_pair = np.stack([
        _SLOPE[0] * delta + U / math.e + 2 * EXPF_ULP * U * g1,
        _SLOPE[1] * delta + 3 * U / math.e + 2 * EXPF_ULP * U * g2,
        np.where(d < 0, 2 * np.abs(d) * delta + delta * delta + U * d * d, 0.0),
        np.where(hyd > 0, _SLOPE[3] * delta + U, 0.0),
        np.where(hb > 0, _SLOPE[4] * delta + U, 0.0)]) * on[None]
    K = int(on.sum(axis=1).max()) + 8 if on.size else 8
    atom_terms = (per_pair.sum(axis=2) + K * U * np.abs(t).sum(axis=2)).T
    terms = per_pair.sum(axis=(1, 2)) + K * U * np.abs(t).sum(axis=(1, 2))
    w = np.abs(np.array([defn.w[k] for k in TERMS]))
    atom_abs = np.abs(t).sum(axis=2).T
    atom_scores = atom_terms @ w + 6 * U * (atom_abs @ w)
    weighted = float(terms @ w + 6 * U * (np.abs(t).sum(axis=(1, 2)) @ w))
    den = 1.0 + defn.rotor * n_rot
    ref = score(x, ri, ti, y, rj, tj, n_rot, defn)
    e = weighted / den + 4 * U * abs(ref["score"])
    return {k: factor * v for k, v in dict(atom_terms=atom_terms, atom_scores=atom_scores, terms=terms, weighted=weighted,
                                           score=e).items()}


def ratios(got, x, ri, ti, y, rj, tj, n_rot, defn=DEFINITION, factor=1.0):
    """The largest error / bound of each of `got`'s values (a dict like `score`'s) at `factor`; 0 where both are 0."""
    want, bound = score(x, ri, ti, y, rj, tj, n_rot, defn), bounds(x, ri, ti, y, rj, tj, n_rot, defn, factor)
    out = {}
    for k, b in bound.items():
        if k not in got:
            continue
        err = np.abs(np.asarray(got[k], dtype=np.float64) - want[k])
        b = np.asarray(b, dtype=np.float64)
        r = np.divide(err, b, out=np.where(err > 0, np.inf, 0.0), where=b > 0)
        out[k] = float(np.max(r)) if r.size else 0.0
    return out


def passes(got, x, ri, ti, y, rj, tj, n_rot, defn=DEFINITION):
    """Whether every value of `got` lies inside the rule and its `hbonds`, where given, is exact."""
    if "hbonds" in got and int(got["hbonds"]) != score(x, ri, ti, y, rj, tj, n_rot, defn)["hbonds"]:
        return False
    return all(r <= 1.0 for r in ratios(got, x, ri, ti, y, rj, tj, n_rot, defn, FACTOR).values())


def check(got, x, ri, ti, y, rj, tj, n_rot, what=""):
    """Assert `got` inside the rule; prints the figures first.  Returns the ratios at factor 1."""
    want = score(x, ri, ti, y, rj, tj, n_rot)
    r = ratios(got, x, ri, ti, y, rj, tj, n_rot, factor=1.0)
    print(f"INTERACTIONS {what}: E={want['score']:.6g} terms={np.round(want['terms'], 4).tolist()} hbonds={want['hbonds']} "
          f"err/bound(factor 1) {({k: round(v, 4) for k, v in r.items()})} FACTOR {FACTOR}")
    if "hbonds" in got:
        assert int(got["hbonds"]) == want["hbonds"], (what, int(got["hbonds"]), want["hbonds"])
    assert all(v <= FACTOR for v in r.values()), (what, r, FACTOR)
    return r


# ----------------------------------------------------------------------------------------------- the seeded cases
def walk(n, g):
    """n points of a self-avoiding random walk with 1.5 A steps (`relief_ref.ligand`), centred."""
    import relief_ref
    return relief_ref.ligand(n, g)


class Case:
    """One ligand in one typed pocket: x [n,3] fp32, z [n], t [n] types, n_rot; rec [R,3] fp32, rec_z [R], rec_t [R]."""
    def __init__(self, name, seed, n, R=None, far=False):
        g = np.random.default_rng(seed)
        lig = walk(n, g) if n else np.zeros((0, 3))
        k = int(math.ceil(14.0 / 2.6)) + 1
        axis = np.arange(-k, k + 1) * 2.6
        pts = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
        pts = pts + g.normal(size=pts.shape) * 0.3
        pts = pts[np.linalg.norm(pts, axis=1) <= 14.0]
        if n:                                      # the pocket: nothing within 3.2 A of a ligand atom
            pts = pts[np.linalg.norm(pts[:, None, :] - lig[None, :, :], axis=2).min(axis=1) > 3.2]
        if R is not None:
            if R > len(pts):                       # a second, finer shell outside the first
                extra = g.uniform(-30, 30, size=(4 * R, 3))
                extra = extra[np.linalg.norm(extra, axis=1) > 15.0][: R - len(pts)]
                pts = np.concatenate([pts, extra])
            else:
                centre = lig.mean(0) if n else np.zeros(3)
                pts = pts[np.argsort(np.linalg.norm(pts - centre, axis=1), kind="stable")[:R]]
            assert len(pts) == R, (name, len(pts))
        if far:
            pts = pts + np.array([60.0, 0.0, 0.0])
        self.name, self.n = name, n
        self.x = lig.astype(np.float32)
        self.z = g.choice([6, 6, 6, 7, 8, 16, 17], size=n).astype(np.int64)
        self.t = g.integers(0, 8, size=n).astype(np.uint8)
        self.n_rot = int(g.integers(0, 9))
        self.rec = pts.astype(np.float32)
        self.rec_z = g.choice([6, 6, 6, 7, 8, 16, 30], size=len(pts)).astype(np.int64)
        self.rec_t = g.integers(0, 8, size=len(pts)).astype(np.uint8)

    @property
    def receptor(self):
        return torch.from_numpy(self.rec), torch.from_numpy(self.rec_z), torch.from_numpy(self.rec_t)

    def args(self):
        """What `score` and `bounds` take."""
        return self.x, radii(self.z), self.t, self.rec, radii(self.rec_z), self.rec_t, self.n_rot

    def __repr__(self):
        return f"Case({self.name}: n={self.n}, R={len(self.rec)})"


def cases():
    """Ligand sizes 1, 2, 27, 64 in a pocket of a few hundred atoms; receptor sizes 1, 255, 256, 257 and 4 097."""
    return [Case("n1", 11, 1), Case("n2", 12, 2), Case("n27", 13, 27), Case("n64", 14, 64),
            Case("R1", 21, 27, R=1), Case("R255", 22, 27, R=255), Case("R256", 23, 27, R=256), Case("R257", 24, 27, R=257),
            Case("R4097", 25, 27, R=4097)]
