"""Electrostatic similarity on the MI355X (`mcg_charges_peoe`, `mcg_esp_overlap`; DESIGN.md section 6 "Electrostatic
similarity"): the two kernels against the fp64 restatement `electrostatics_ref` under its pass rules (charges within the
derived Q_TOL, overlaps within OVERLAP_C * 2^-24 * sum |t|, the Tanimoto within the propagated bound), integers exact,
sentinels round every output, the status-1 and the NaN row, bit identity whatever the batch, the row and the padded width,
the Python layer, and `electrostatic_scores` / `partial_charges` through `generate_conformers`.  The worst error / bound
ratios are printed (`ESP ...` lines) and recorded in DESIGN.md."""
import functools
import math

import numpy as np
import pytest
import torch

import electrostatics_cases as K
import electrostatics_ref as ER
import hydrogens_cases as HC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 256
SIZES = (1, 63, 64, 65, 256)
NAN_BITS = torch.full((1,), float("nan")).view(torch.int32).item()


def _guarded(size, dtype, fill):
    return torch.full((GUARD + size + GUARD,), fill, dtype=dtype, device=DEV)


def _check_guards(buf, sizes):
    for k, s in sizes.items():
        t = buf[k].view(torch.int32)
        fill = NAN_BITS if buf[k].dtype == torch.float32 else 0x5A5A5A5A
        assert bool((t[:GUARD] == fill).all()) and bool((t[GUARD + s:] == fill).all()), k


# ----------------------------------------------------------------------------------------------- the charge kernel
def _charges(z, bonds, n):
    """`mcg_pharm_perceive` + `mcg_charges_peoe` through the C entry points, every output between sentinels.  Host
    tensors q [B,W], q_h [B,W], nh [B,W], status [B]."""
    from ml_conformer_generator_amd import _lib
    zz, bb, nn = (torch.as_tensor(t).to(DEV).contiguous() for t in (z, bonds, n))
    B, W = int(bb.shape[0]), int(bb.shape[1])
    types = torch.zeros(B, W, dtype=torch.uint8, device=DEV)
    rings = torch.zeros(B, 32, dtype=torch.int64, device=DEV)
    count = torch.zeros(B, dtype=torch.int32, device=DEV)
    L, stream = _lib.lib(), _lib.current_stream_ptr(DEV)
    _lib.check(L.mcg_pharm_perceive(_lib.dptr(zz), _lib.dptr(bb), _lib.dptr(nn), B, W, _lib.dptr(types), _lib.dptr(count),
                                    _lib.dptr(rings), stream), "mcg_pharm_perceive")
    sizes = dict(q=B * W, q_h=B * W, nh=B * W, status=B)
    buf = {k: _guarded(s, torch.float32 if k in ("q", "q_h") else torch.int32, float("nan") if k in ("q", "q_h") else 0x5A5A5A5A)
           for k, s in sizes.items()}
    ptr = {k: v[GUARD:].data_ptr() for k, v in buf.items()}
    _lib.check(L.mcg_charges_peoe(_lib.dptr(zz), _lib.dptr(bb), _lib.dptr(nn), _lib.dptr(types), _lib.dptr(rings),
                                  _lib.dptr(count), B, W, ptr["q"], ptr["q_h"], ptr["nh"], ptr["status"], stream),
               "mcg_charges_peoe")
    torch.cuda.synchronize()
    _check_guards(buf, sizes)
    shape = dict(q=(B, W), q_h=(B, W), nh=(B, W), status=(B,))
    return {k: buf[k][GUARD: GUARD + s].cpu().reshape(shape[k]) for k, s in sizes.items()}


def _graph_batch(items, W, garbage_seed=None):
    _, z, bonds, n = HC.pad_batch(items, W, W, garbage_seed=garbage_seed)
    return z, bonds, n


def test_charges_match_the_restatement():
    f, ref = K.fixtures(), K.references()
    names = list(f)
    assert set(K.REQUIRED) <= set(names)
    out = _charges(*_graph_batch([f[k] for k in names], 64, garbage_seed=7))      # W = 64, junk at and beyond each row's atoms
    worst = 0.0
    for b, name in enumerate(names):
        c, n = ref[name]["charges"], f[name]["mol"][2]
        assert out["nh"][b, :n].tolist() == c["nh"] and not out["nh"][b, n:].any(), name
        assert int(out["status"][b]) == c["status"], name
        for key in ("q", "q_h"):
            assert not out[key][b, n:].view(torch.int32).any(), (name, key)         # +0 at and beyond the row's atoms
            if c["status"]:
                assert bool(torch.isnan(out[key][b, :n]).all()), (name, key)
            elif n:
                err = float(np.abs(out[key][b, :n].double().numpy() - np.array(c[key])).max())
                worst = max(worst, err)
                assert err <= ER.Q_TOL, (name, key, err)
        if not c["status"]:
            total = float(out["q"][b, :n].double().sum() + (out["nh"][b, :n].double() * out["q_h"][b, :n].double()).sum())
            assert abs(total) <= 64 * ER.Q_TOL, (name, total)
    print(f"ESP charges vs fp64 restatement: max |dq| = {worst:.3e} e over {len(names)} molecules, "
          f"{worst / ER.Q_TOL:.4f} of the tolerance {ER.Q_TOL:.1e}")
    # the row without parameters leaves its neighbours alone: the same batch with ethanol in its place
    b = names.index(K.UNCHARGED)
    healthy = _charges(*_graph_batch([f[k] if k != K.UNCHARGED else f["ethanol"] for k in names], 64, garbage_seed=7))
    for key in out:
        keep = [r for r in range(len(names)) if r != b]
        assert torch.equal(out[key][keep].view(torch.int32), healthy[key][keep].view(torch.int32)), key
    assert int(healthy["status"][b]) == 0 and bool(torch.isfinite(healthy["q"][b]).all())


def test_charges_have_the_same_bits_whatever_batch_row_and_width():
    f = K.fixtures()
    mol = HC.grown(5, 20)
    others = [f[k] for k in ("phenol", "acetamide", "dimethyl sulfone", "imidazole", "phosphoric acid", K.UNCHARGED, "benzene")]
    alone = _charges(*_graph_batch([mol], 20))
    assert int(alone["status"][0]) == 0 and int(alone["nh"][0].sum()) >= 20 and float(alone["q"][0].abs().max()) > 0.1
    for row in (0, 1, 4, 5, 7):                       # every wave of a workgroup, a second workgroup, a ragged last one
        items = others[:row] + [mol] + others[row:]
        crowd = _charges(*_graph_batch(items, 20))
        for key in ("q", "q_h", "nh"):
            assert torch.equal(crowd[key][row].view(torch.int32), alone[key][0].view(torch.int32)), (row, key)
    wide = _charges(*_graph_batch([others[0], mol], 64, garbage_seed=3))
    for key in ("q", "q_h", "nh"):
        assert torch.equal(wide[key][1, :20].view(torch.int32), alone[key][0].view(torch.int32)), key
        assert not wide[key][1, 20:].view(torch.int32).any(), key
    full = f["grown 64"]                              # W = n = 64: every lane real, no padding at all
    a = _charges(*_graph_batch([full], 64))
    b = _charges(*_graph_batch([others[1], others[2], full], 64, garbage_seed=5))
    for key in ("q", "q_h", "nh"):
        assert torch.equal(a[key][0].view(torch.int32), b[key][2].view(torch.int32)), key


# ----------------------------------------------------------------------------------------------- the overlap kernel
def _overlap(ref, xyz, q, n, e_rr=None):
    """`mcg_esp_overlap` through the C entry point, every output between sentinels: host cross, self, tanimoto [B]."""
    from ml_conformer_generator_amd import _lib
    rx, rq = (torch.as_tensor(t).to(DEV).contiguous() for t in ref)
    x, c, nn = (torch.as_tensor(t).to(DEV).contiguous() for t in (xyz, q, n))
    B, PW = int(x.shape[0]), int(x.shape[1])
    sizes = dict(cross=B, self=B, tanimoto=B)
    buf = {k: _guarded(s, torch.float32, float("nan")) for k, s in sizes.items()}
    ptr = {k: v[GUARD:].data_ptr() for k, v in buf.items()}
    rr = None if e_rr is None else torch.as_tensor(e_rr, dtype=torch.float32).reshape(1).to(DEV)
    _lib.check(_lib.lib().mcg_esp_overlap(_lib.dptr(rx), _lib.dptr(rq), int(rq.numel()), _lib.dptr(x), _lib.dptr(c),
                                          _lib.dptr(nn), B, PW, ER.MU, _lib.dptr(rr), ptr["cross"], ptr["self"],
                                          ptr["tanimoto"], _lib.current_stream_ptr(DEV)), "mcg_esp_overlap")
    torch.cuda.synchronize()
    _check_guards(buf, sizes)
    return {k: buf[k][GUARD: GUARD + s].cpu() for k, s in sizes.items()}


def _self_overlap(pts):
    x, q = pts
    return _overlap(pts, x[None], q[None], np.array([len(q)], np.int32))["self"][0]


@functools.lru_cache(maxsize=None)
def _restated(ref_key, mol_key):
    """`electrostatics_ref.score` of two named point sets, computed once: a fixture's name, or ("cloud", k, shift)."""
    return ER.score(_points(ref_key), _points(mol_key))


def _points(key):
    return K.fp32_points(key) if isinstance(key, str) else K.cloud(*key[1:])


class _Worst:
    def __init__(self):
        self.ratio = dict(cross=0.0, self=0.0, tanimoto=0.0)

    def check(self, got, b, want, what):
        for key, tol in (("cross", want["tol"]["cross"]), ("self", want["tol"]["self"]), ("tanimoto", want["tol_tanimoto"])):
            err = abs(float(got[key][b]) - want[key])
            if tol > 0:
                self.ratio[key] = max(self.ratio[key], err / tol)
            assert err <= tol, (what, key, err, tol)

    def report(self, title):
        print(f"ESP {title}: worst error / bound: E(R,M) {self.ratio['cross']:.4f}, E(M,M) {self.ratio['self']:.4f}, "
              f"T {self.ratio['tanimoto']:.4f} (bound: {ER.OVERLAP_C:g} * 2^-24 * sum |t|, propagated to T)")


def test_overlap_at_every_size_of_both_sides():
    worst = _Worst()
    counts = (0,) + SIZES
    for P in SIZES:
        ref_key = ("cloud", P, 0.0)
        ref = _points(ref_key)
        e_rr = _self_overlap(ref)
        want_rr = _restated(ref_key, ref_key)
        assert abs(float(e_rr) - want_rr["self"]) <= want_rr["tol"]["self"], P
        # PW = 256: point counts 0, 1, ... 256 in one batch, junk (NaN included) beyond each row's points
        items = [(np.zeros((0, 3), np.float32), np.zeros(0, np.float32))] + [K.cloud(k, 1.3) for k in SIZES]
        wide = _overlap(ref, *K.pad_points(items, 256, garbage_seed=9), e_rr=e_rr)
        assert [float(wide[k][0]) for k in ("cross", "self", "tanimoto")] == [0.0, 0.0, 0.0]      # no point: T = 0
        for b, k in enumerate(counts):
            if k:
                worst.check(wide, b, _restated(ref_key, ("cloud", k, 1.3)), (P, 256, k))
        # the same rows alone at their own width PW = k: the same bits
        for b, k in enumerate(counts):
            if k and k != 256:
                tight = _overlap(ref, *K.pad_points([K.cloud(k, 1.3)], k), e_rr=e_rr)
                for key in tight:
                    assert torch.equal(tight[key].view(torch.int32), wide[key][b: b + 1].view(torch.int32)), (P, k, key)
    worst.report("overlap at P, PW in {1, 63, 64, 65, 256}")


def test_overlap_of_the_molecules():
    ref = K.references()
    names = [k for k in K.fixtures() if k != K.UNCHARGED]
    worst = _Worst()
    for ref_name in ("acetamide", "grown 64"):
        e_rr = _self_overlap(K.fp32_points(ref_name))
        items = [K.fp32_points(k) for k in names]
        got = _overlap(K.fp32_points(ref_name), *K.pad_points(items, 160, garbage_seed=4), e_rr=e_rr)
        for b, name in enumerate(names):
            if len(ref[name]["points"][1]):
                worst.check(got, b, _restated(ref_name, name), (ref_name, name))
        b = names.index(ref_name)                     # T(A,A): the same kernel gives E(R,R), E(M,M) and E(R,M)
        assert abs(float(got["tanimoto"][b]) - 1.0) <= 2.0 ** -22, ref_name
        assert got["cross"][b].view(torch.int32) == got["self"][b].view(torch.int32) == e_rr.view(torch.int32)
    worst.report("overlap of the fixtures against acetamide and grown 64")
    # A against A with every charge negated: -1/3
    for name in ("acetamide", "phenol", "grown 64"):
        x, q = K.fp32_points(name)
        got = _overlap((x, q), x[None], -q[None], np.array([len(q)], np.int32), e_rr=_self_overlap((x, q)))
        want = ER.score((x, q), (x, -q))
        assert abs(want["tanimoto"] + 1.0 / 3.0) <= 1e-12
        assert abs(float(got["tanimoto"][0]) + 1.0 / 3.0) <= want["tol_tanimoto"], name
    # without e_rr the row's own self-overlap stands in: a row against itself scores 1 exactly
    x, q = K.fp32_points("phenol")
    assert float(_overlap((x, q), x[None], q[None], np.array([len(q)], np.int32))["tanimoto"][0]) == 1.0


def test_a_row_with_a_non_finite_point_scores_nan_and_leaves_the_others_alone():
    ref = K.fp32_points("acetamide")
    e_rr = _self_overlap(ref)
    items = [K.fp32_points(k) for k in ("ethanol", "phenol", "grown 64", "acetic acid", "water")]
    xyz, q, n = K.pad_points(items, 140)
    healthy = _overlap(ref, xyz, q, n, e_rr=e_rr)
    for what in ("coordinate", "charge"):
        bad_xyz, bad_q = xyz.copy(), q.copy()
        if what == "coordinate":
            bad_xyz[1, 5, 1] = np.nan
            bad_xyz[3, 0, 2] = np.inf
        else:
            bad_q[1, 2] = np.nan                      # what a status-1 molecule's points carry
            bad_q[3, 7] = np.nan
        got = _overlap(ref, bad_xyz, bad_q, n, e_rr=e_rr)
        for key in got:
            assert bool(torch.isnan(got[key][[1, 3]]).all()), (what, key)
            assert torch.equal(got[key][[0, 2, 4]].view(torch.int32), healthy[key][[0, 2, 4]].view(torch.int32)), (what, key)


def test_overlap_has_the_same_bits_whatever_batch_and_row():
    ref = K.fp32_points("phenol")
    e_rr = _self_overlap(ref)
    mol = K.fp32_points("grown 64")
    others = [K.fp32_points(k) for k in ("ethanol", "acetamide", "water", "dimethyl sulfone")]
    alone = _overlap(ref, *K.pad_points([mol], len(mol[1])), e_rr=e_rr)
    for row in (0, 2, 4):
        crowd = _overlap(ref, *K.pad_points(others[:row] + [mol] + others[row:], 256, garbage_seed=row + 1), e_rr=e_rr)
        for key in alone:
            assert torch.equal(crowd[key][row].view(torch.int32), alone[key][0].view(torch.int32)), (row, key)


def test_erff_error_on_the_fixtures_arguments():
    """The one measured ingredient of OVERLAP_C: the device's fp32 erf (torch's elementwise kernel calls the same `erff`)
    against fp64 erf on the arguments mu * r the fixtures and clouds present, r >= 1e-3."""
    args = []
    for key in [k for k in K.fixtures() if k != K.UNCHARGED] + [("cloud", 256, 0.0)]:
        x, _ = _points(key)
        if len(x) > 1:
            d = x[:, None, :] - x[None, :, :]
            r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)
            args.append(r[r >= ER.SMALL_R])
    a = np.unique(np.concatenate(args) * np.float32(ER.MU))
    got = torch.erf(torch.from_numpy(a).to(DEV)).cpu().double().numpy()
    want = np.array([math.erf(float(v)) for v in a])
    ulp = np.abs(got - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    print(f"ESP erff: worst error {ulp.max():.3f} ulp over {len(a)} arguments in [{a.min():.3f}, {a.max():.3f}] "
          f"(ERFF_ULP = {ER.ERFF_ULP:g})")
    assert ulp.max() <= ER.ERFF_ULP
    # the overlap kernel's own erff: one unit charge at the origin against one at (r, 0, 0) gives K(r) = erff(r) / r, whose
    # one division adds at most one more ulp of the quotient
    sub = a[:: len(a) // 16000 + 1]
    xyz = np.zeros((len(sub), 1, 3), np.float32)
    xyz[:, 0, 0] = sub / np.float32(ER.MU)
    one = (np.zeros((1, 3), np.float32), np.ones(1, np.float32))
    k = _overlap(one, xyz, np.ones((len(sub), 1), np.float32), np.ones(len(sub), np.int32))["cross"].double().numpy()
    want = np.array([ER.kernel(float(v)) for v in xyz[:, 0, 0]])
    k_ulp = np.abs(k - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    print(f"ESP erff: the kernel's K(r) = erff(r) / r is within {k_ulp.max():.3f} ulp over {len(sub)} of those arguments")
    assert k_ulp.max() <= ER.ERFF_ULP + 1.0


# ----------------------------------------------------------------------------------------------- the Python layer
def test_python_layer():
    from ml_conformer_generator_amd import electrostatics as ES
    from ml_conformer_generator_amd import hydrogens as HY
    f, ref = K.fixtures(), K.references()
    names = [k for k in f if f[k]["mol"][2] <= 7]
    xyz, z, bonds, n = (torch.from_numpy(t) for t in HC.pad_batch([f[k] for k in names], 7, 9))
    raw = _charges(z, bonds, n)
    out = ES.partial_charges(z, bonds, n, DEV)
    assert out["q"].is_cuda and out["nh"].dtype == torch.int32 and out["n_nodes"].cpu().tolist() == n.tolist()
    for key in ("q", "q_h", "nh", "status"):
        assert torch.equal(out[key].cpu().view(torch.int32), raw[key].view(torch.int32)), key
    assert torch.equal(out["nh"].cpu(), HY.implicit_counts(z, bonds, n))
    placed = HY.add_hydrogens(xyz, z, bonds, n, DEV)
    pts, q, count = ES.charge_points(xyz.to(DEV), out, placed)
    assert pts.is_cuda and count.cpu().tolist() == [len(ref[k]["points"][1]) for k in names]
    for b, name in enumerate(names):
        k = int(count[b])
        if k and name != K.UNCHARGED:
            assert np.abs(pts[b, :k].cpu().double().numpy() - ref[name]["points"][0]).max() <= 1e-4, name
            assert np.abs(q[b, :k].cpu().double().numpy() - ref[name]["points"][1]).max() <= 2 * ER.Q_TOL, name
    ref_pts = [(float(c), tuple(float(v) for v in p)) for p, c in zip(*K.fp32_points("acetamide"))]
    got = ES.electrostatic_tanimoto(ref_pts, pts, q, count)
    same = _overlap(K.fp32_points("acetamide"), pts.cpu(), q.cpu(), count.cpu(), e_rr=_self_overlap(K.fp32_points("acetamide")))
    for key in ("cross", "self", "tanimoto"):
        assert got[key].is_cuda and torch.equal(got[key].cpu().view(torch.int32), same[key].view(torch.int32)), key
    assert math.isnan(float(got["tanimoto"][names.index(K.UNCHARGED)]))            # status 1: NaN, the others finite
    assert int(torch.isnan(got["tanimoto"]).sum()) == 1 and float(got["tanimoto"][names.index("no atoms")]) == 0.0
    empty = ES.partial_charges(z[:0], bonds[:0], n[:0], DEV)
    assert tuple(empty["q"].shape) == (0, 7) and tuple(ES.electrostatic_tanimoto(ref_pts, pts[:0], q[:0], count[:0])["tanimoto"].shape) == (0,)
    with pytest.raises(ValueError, match="no charge to score against"):            # E(R,R) < 1e-12
        ES.electrostatic_tanimoto([(0.0, (0, 0, 0)), (0.0, (1, 0, 0))], pts, q, count)
    bad = bonds.clone()
    bad[1, 0, 1] = bad[1, 1, 0] = 5
    with pytest.raises(ValueError, match="codes"):
        ES.partial_charges(z, bad, n, DEV)
    # more rows than one launch takes: the rows behind the first 16384 are computed too
    many = ES.MAX_BATCH + 6
    e = f["ethanol"]
    zz, bb, nn = (torch.from_numpy(t) for t in _graph_batch([e], 3))
    big = ES.partial_charges(zz.expand(many, 3), bb.expand(many, 3, 3), nn.expand(many), DEV)
    assert bool((big["q"].view(torch.int32) == big["q"][0].view(torch.int32)).all()) and float(big["q"][-1, 2]) < -0.39
    ex, eq = K.fp32_points("ethanol")
    rows = ES.electrostatic_tanimoto(ref_pts, torch.from_numpy(ex).expand(many, 9, 3), torch.from_numpy(eq).expand(many, 9),
                                     torch.full((many,), 9, dtype=torch.int32))["tanimoto"]
    assert bool((rows.view(torch.int32) == rows[0].view(torch.int32)).all()) and float(rows[-1]) != 0.0


# ----------------------------------------------------------------------------------------------- generation entries
def _reference_charges(ref):
    """Charges on the reference conformer's first atoms, in its coordinates: neutral overall."""
    values = [0.35, -0.35, 0.2, -0.3, 0.1, -0.25, 0.4, -0.15]
    return [(v, tuple(float(c) for c in ref[k])) for k, v in enumerate(values)]


def _own_values(mols, ref_pts):
    """The module-level functions applied to each record's own returned coordinates and graph, one molecule per call."""
    from ml_conformer_generator_amd import electrostatics as ES
    from ml_conformer_generator_amd import hydrogens as HY
    out = []
    for m in mols:
        n = len(m.atomic_numbers)
        z, nn = torch.tensor([m.atomic_numbers], dtype=torch.int32), torch.tensor([n], dtype=torch.int32)
        ch = ES.partial_charges(z, m.bond_orders[None], nn, DEV)
        placed = HY.add_hydrogens(m.coords[None], z, m.bond_orders[None], nn, DEV)
        pts, q, count = ES.charge_points(m.coords[None].to(DEV), ch, placed)
        t = ES.electrostatic_tanimoto(ref_pts, pts, q, count)["tanimoto"]
        out.append((float(t[0]), ch["q"][0, :n].cpu(), ch["q_h"][0, :n].cpu()))
    return out


def _same(a, b):
    return (a != a and b != b) or a == b


def test_generation_with_electrostatic_scores(monkeypatch):
    from test_hydrogens_gpu import _heavy, _setup
    gen, ref, kw = _setup(monkeypatch)                # grown molecules; sample 3 has a non-finite coordinate
    kw = dict(kw, overlay=True)
    ref_pts = _reference_charges(ref)
    launched = dict(charges=0, score=0)
    real_charges, real_score = gen._peoe_charges, gen._esp_score

    def charges(*a, **k):
        launched["charges"] += 1
        return real_charges(*a, **k)

    def score(*a, **k):
        launched["score"] += 1
        return real_score(*a, **k)
    monkeypatch.setattr(gen, "_peoe_charges", charges)
    monkeypatch.setattr(gen, "_esp_score", score)

    plain = gen.generate_conformers(**kw)
    assert launched == dict(charges=0, score=0)       # neither kernel without the keywords
    assert all(m.electrostatic_tanimoto is None and m.partial_charges is None and m.hydrogen_charges is None for m in plain)
    full = gen.generate_conformers(electrostatic_scores=True, reference_charges=ref_pts, partial_charges=True, **kw)
    assert launched == dict(charges=1, score=1)
    assert [m.sample_id for m in full] == list(range(8))
    assert [_heavy(m) for m in full] == [_heavy(m) for m in plain]                # the heavy-atom fields: bit for bit
    scored = 0
    for m, (t, q, qh) in zip(full, _own_values(full, ref_pts)):
        assert m.hydrogen_coords is None                                          # the hydrogens were not asked for
        assert torch.equal(m.partial_charges.view(torch.int32), q.view(torch.int32)), m.sample_id
        assert torch.equal(m.hydrogen_charges.view(torch.int32), qh.view(torch.int32)), m.sample_id
        if m.sample_id == 3 or m.pose is None:
            assert math.isnan(m.electrostatic_tanimoto), m.sample_id
            continue
        assert np.float32(m.electrostatic_tanimoto).view(np.uint32) == np.float32(t).view(np.uint32), m.sample_id
        assert -1.0 / 3.0 - 1e-6 <= m.electrostatic_tanimoto <= 1.0
        scored += 1
    assert scored >= 5 and len({m.electrostatic_tanimoto for m in full if m.electrostatic_tanimoto == m.electrostatic_tanimoto}) >= 5

    # add_hydrogens on and off changes no bit of the scores, and the hydrogens are those of the call with it alone
    both = gen.generate_conformers(electrostatic_scores=True, reference_charges=ref_pts, add_hydrogens=True, **kw)
    only_h = gen.generate_conformers(add_hydrogens=True, **kw)
    for a, b, h in zip(full, both, only_h):
        assert _same(a.electrostatic_tanimoto, b.electrostatic_tanimoto) and b.partial_charges is None
        assert (b.hydrogen_coords is None) == (h.hydrogen_coords is None) and b.hydrogen_parents == h.hydrogen_parents
        if h.hydrogen_coords is not None:
            assert torch.equal(b.hydrogen_coords.view(torch.int32), h.hydrogen_coords.view(torch.int32))
    alone = gen.generate_conformers(partial_charges=True, **{k: v for k, v in kw.items() if k != "overlay"})
    assert all(m.electrostatic_tanimoto is None and m.pose is None for m in alone)
    assert all(torch.equal(a.partial_charges.view(torch.int32), b.partial_charges.view(torch.int32)) for a, b in zip(alone, full))

    # the threshold and rank_by="electrostatic" select what the host walk selects from the records' own values
    values = sorted(m.electrostatic_tanimoto for m in full if m.electrostatic_tanimoto == m.electrostatic_tanimoto)
    t = (values[1] + values[2]) / 2
    kept = gen.generate_conformers(min_electrostatic_tanimoto=t, reference_charges=ref_pts, **kw)
    assert [m.sample_id for m in kept] == [m.sample_id for m in full if m.electrostatic_tanimoto >= t]
    assert 0 < len(kept) < len(full) and all(_same(m.electrostatic_tanimoto, full[m.sample_id].electrostatic_tanimoto) for m in kept)
    shaped = gen.generate_conformers(electrostatic_scores=True, reference_charges=ref_pts, shape_scores=True, **kw)

    def rank(m):
        s = m.shape_tanimoto + m.electrostatic_tanimoto
        return (-s if s == s else math.inf, m.sample_id)
    want = [m.sample_id for m in sorted(shaped, key=rank)][:3]
    top = gen.generate_conformers(electrostatic_scores=True, reference_charges=ref_pts, rank_by="electrostatic", top_k=3, **kw)
    assert [m.sample_id for m in top] == want
    by_shape = gen.generate_conformers(electrostatic_scores=True, reference_charges=ref_pts, top_k=3, **kw)
    assert [m.sample_id for m in by_shape] == [m.sample_id for m in sorted(
        shaped, key=lambda m: (-m.shape_tanimoto if m.shape_tanimoto == m.shape_tanimoto else math.inf, m.sample_id))][:3]
    for entry in ("generate_conformers_sharded", "forward"):
        again = getattr(gen, entry)(electrostatic_scores=True, reference_charges=ref_pts, partial_charges=True, **kw)
        assert all(_same(a.electrostatic_tanimoto, b.electrostatic_tanimoto) and
                   torch.equal(a.partial_charges.view(torch.int32), b.partial_charges.view(torch.int32))
                   for a, b in zip(again, full)), entry
    print(f"ESP generation: {scored} of 8 records scored, T in [{values[0]:.4f}, {values[-1]:.4f}]; threshold {t:.4f} keeps "
          f"{len(kept)}; rank_by='electrostatic' top 3 {want}")


def test_generation_with_the_references_own_graph(monkeypatch):
    """The reference's charges computed from its graph on the reference conformer's coordinates - hydrogens placed by the
    same kernel - equal the module-level functions applied to that graph and those coordinates."""
    from test_hydrogens_gpu import _setup
    from ml_conformer_generator_amd import electrostatics as ES
    from ml_conformer_generator_amd import hydrogens as HY
    gen, _, kw = _setup(monkeypatch)
    fx = HC.grown(77, 17)
    z, adj, n = fx["mol"]
    ref = torch.from_numpy(fx["xyz"]) + torch.tensor([12.0, -5.0, 3.0])
    kw = dict(kw, reference_conformer=ref, overlay=True)
    graph = (z, torch.tensor(adj, dtype=torch.int8))
    got = gen.generate_conformers(electrostatic_scores=True, reference_graph=graph, **kw)
    zz, nn = torch.tensor([z], dtype=torch.int32), torch.tensor([n], dtype=torch.int32)
    ch = ES.partial_charges(zz, graph[1][None], nn, DEV)
    pts, q, count = ES.charge_points(ref[None].to(DEV), ch, HY.add_hydrogens(ref[None], zz, graph[1][None], nn, DEV))
    k = int(count[0])
    assert k > n
    given = gen.generate_conformers(electrostatic_scores=True, reference_charges=(pts[0, :k].cpu(), q[0, :k].cpu()), **kw)
    assert [m.sample_id for m in got] == [m.sample_id for m in given] and len(got) == 8
    assert all(_same(a.electrostatic_tanimoto, b.electrostatic_tanimoto) for a, b in zip(got, given))
    assert sum(1 for m in got if m.electrostatic_tanimoto == m.electrostatic_tanimoto) >= 5
