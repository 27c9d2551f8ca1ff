"""The electrostatic definition and its plumbing without a GPU: the restatement (`electrostatics_ref`) against the three
molecules checked by hand, charge neutrality, the hydrogen counts, the properties of the score, the condition of the pass
rules on every fixture, mutations of the definition that the pass rules must catch, the point assembly in torch, the
refusals of `parse_request`, `select` on fake rows, the record path with the device seams replaced by the restatement, the
argument checks of the two C entries and the header."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import electrostatics_cases as K
import electrostatics_ref as ER
import hydrogens_cases as HC
import hydrogens_ref as HR
from conftest import REPO
from ml_conformer_generator_amd import electrostatics as ES
from ml_conformer_generator_amd import hydrogens as HY
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd.handoff import GeneratedMolecule, Measured, measured_from_tensors
from test_pharmacophore_host import _seam_perceive
from test_shape_overlay_host import _no_device, _ref, _shell_generator, _stub_overlay

CHARGED = [k for k in K.fixtures() if k != K.UNCHARGED]


# ----------------------------------------------------------------------------------------------- the restatement
def test_fixtures_cover_the_table():
    f, ref = K.fixtures(), K.references()
    assert set(K.REQUIRED) <= set(f)
    assert f["grown 64"]["mol"][2] == 64 and f["methane"]["mol"][2] == 1 and f["no atoms"]["mol"][2] == 0
    assert ref[K.UNCHARGED]["charges"]["status"] == 1 and all(math.isnan(v) for v in ref[K.UNCHARGED]["charges"]["q"])
    assert ref[K.UNPLACED]["placed"]["unplaced"] == 2
    assert all(ref[k]["charges"]["status"] == 0 for k in CHARGED)
    assert max(len(ref[k]["points"][1]) for k in CHARGED) <= ES.MAX_POINTS
    seen = {z for k in CHARGED for z in f[k]["mol"][0]}
    assert {6, 7, 8, 9, 15, 16, 17, 35} <= seen
    # every class of C, N, O and S, and the sulfone row, is read by some fixture
    rows = {(z, tuple(p)) for k in CHARGED for z, p in zip(f[k]["mol"][0], ER.parameters(*f[k]["mol"]))}
    for z in (6, 7):
        assert {(z, ER.ROWS[z][c]) for c in (HR.TETRAHEDRAL, HR.PLANAR, HR.LINEAR)} <= rows, z
    assert {(8, ER.ROWS[8][HR.TETRAHEDRAL]), (8, ER.ROWS[8][HR.PLANAR]), (16, ER.ROWS[16][HR.TETRAHEDRAL]),
            (16, ER.ROWS[16]["oxo"])} <= rows


def test_the_three_checked_molecules():
    ref = K.references()
    c = ref["methane"]["charges"]
    assert abs(c["q"][0] + 0.0776) <= 5e-4 and abs(c["q_h"][0] - 0.0194) <= 5e-4 and c["nh"] == [4]
    c = ref["water"]["charges"]
    assert abs(c["q"][0] + 0.4105) <= 5e-4 and abs(c["q_h"][0] - 0.2052) <= 5e-4 and c["nh"] == [2]
    c = ref["ethanol"]["charges"]
    assert abs(c["q"][2] + 0.3953) <= 5e-4 and abs(c["q_h"][2] - 0.2094) <= 5e-4 and c["nh"] == [3, 2, 1]


def test_every_molecule_is_neutral_and_counts_its_hydrogens_like_the_placement():
    f, ref = K.fixtures(), K.references()
    for name in CHARGED:
        c = ref[name]["charges"]
        assert abs(ER.total_charge(c)) <= 1e-12, name
        assert abs(float(ref[name]["points"][1].sum())) <= 1e-12, name           # the unplaced ones fold into their parent
        assert all(v == 0.0 for v, h in zip(c["q_h"], c["nh"]) if h == 0), name
    names = list(f)
    _, z, bonds, n = HC.pad_batch([f[k] for k in names], 64, 64, garbage_seed=11)
    nh = HY.implicit_counts(torch.from_numpy(z), torch.from_numpy(bonds), torch.from_numpy(n))
    for b, name in enumerate(names):
        k = f[name]["mol"][2]
        assert nh[b, :k].tolist() == ref[name]["charges"]["nh"] and not nh[b, k:].any(), name


def test_score_properties():
    ref = K.references()
    rot, shift = HC.MOTION
    for name in ("ethanol", "acetamide", "phenol", "dimethyl sulfone", "grown 64"):
        x, q = ref[name]["points"]
        own = ER.score((x, q), (x, q))
        assert abs(own["tanimoto"] - 1.0) <= 1e-12, name
        assert abs(ER.score((x, q), (x, -q))["tanimoto"] + 1.0 / 3.0) <= 1e-12, name
    a, b = ref["acetamide"]["points"], ref["acetic acid"]["points"]
    ab, ba = ER.score(a, b), ER.score(b, a)
    assert abs(ab["tanimoto"] - ba["tanimoto"]) <= 1e-12 and -1.0 / 3.0 <= ab["tanimoto"] < 1.0
    moved = lambda p: (p[0] @ rot.T + shift, p[1])                                # noqa: E731
    assert abs(ER.score(moved(a), moved(b))["tanimoto"] - ab["tanimoto"]) <= 1e-12
    assert ER.score(a, ref["no atoms"]["points"])["tanimoto"] == 0.0              # nothing is charged: T = 0
    series = ER.MU * (2.0 / math.sqrt(math.pi)) * (1.0 - (ER.MU * 1e-3) ** 2 / 3.0)  # at the switch the series meets erf(r) / r:
    assert abs(series - math.erf(ER.MU * 1e-3) / 1e-3) <= 1e-12                   # its next term is (mu r)^4 / 10 = 1e-13
    assert ER.kernel(0.0) == ER.MU * 2.0 / math.sqrt(math.pi) and ER.kernel(ER.SMALL_R) == math.erf(ER.MU * 1e-3) / 1e-3


def test_every_fixture_meets_the_condition_of_the_pass_rules():
    ref = K.references()
    lowest = (math.inf, None)
    for name in CHARGED:
        x, q = ref[name]["points"]
        e, s = ER.overlap(x, q, x, q)
        assert e >= ER.CONDITION * s, (name, e, s)
        if s > 0:
            lowest = min(lowest, (e / s, name))
    print(f"ESP condition: the smallest E(M,M) / sum |t| is {lowest[0]:.3f} at {lowest[1]!r}")
    assert lowest[0] >= 0.03
    for k in (1, 63, 64, 65, 256):
        x, q = K.cloud(k)
        e, s = ER.overlap(x, q, x, q)
        assert e >= ER.CONDITION * s, k


def test_mutations_fail_the_pass_rules():
    ref = K.references()
    a, b = ref["acetamide"]["points"], ref["acetic acid"]["points"]
    true = ER.score(a, b)
    # one dropped term (the largest of the cross sum)
    terms = [(abs(a[1][i] * b[1][j] * ER.kernel(float(np.linalg.norm(a[0][i] - b[0][j])))), i, j)
             for i in range(len(a[1])) for j in range(len(b[1]))]
    _, i, j = max(terms)
    dropped = ER.overlap(b[0], b[1], a[0], a[1], drop=(j, i))[0]
    assert abs(dropped - true["cross"]) > 100 * true["tol"]["cross"]
    flipped = np.array(b[1])
    flipped[int(np.argmax(np.abs(flipped)))] *= -1.0                               # one sign-flipped charge
    wrong = ER.score(a, (b[0], flipped))
    assert abs(wrong["cross"] - true["cross"]) > 100 * true["tol"]["cross"]
    assert abs(wrong["tanimoto"] - true["tanimoto"]) > 100 * true["tol_tanimoto"]
    off = ER.score(a, b, mu=1.01 * ER.MU)                                          # MU off by 1 %
    assert abs(off["self"] - true["self"]) > 100 * true["tol"]["self"]
    assert abs(off["cross"] - true["cross"]) > 10 * true["tol"]["cross"]
    z, adj, n = K.fixtures()["acetamide"]["mol"]                                   # one parameter row swapped
    swapped = ER.charges(z, adj, n, rows=ER.swapped_rows())
    worst = max(abs(u - v) for u, v in zip(swapped["q"], ref["acetamide"]["charges"]["q"]))
    assert worst > 100 * ER.Q_TOL
    print(f"ESP mutations: dropped term {abs(dropped - true['cross']) / true['tol']['cross']:.0f} x, flipped charge "
          f"{abs(wrong['tanimoto'] - true['tanimoto']) / true['tol_tanimoto']:.0f} x, MU + 1 % "
          f"{abs(off['self'] - true['self']) / true['tol']['self']:.0f} x their tolerances; swapped row {worst / ER.Q_TOL:.0f} x Q_TOL")


# ----------------------------------------------------------------------------------------------- the restatement as seams
def _seam_hydrogens(calls):
    def run(x, z, bonds, n, perceived=None):
        x, z, bonds = torch.as_tensor(x), torch.as_tensor(z), torch.as_tensor(bonds)
        counts = torch.as_tensor(n).reshape(-1).tolist()
        calls.append(("hydrogens", len(counts), perceived is not None))
        W = int(bonds.shape[1])
        placed = [HR.place(z[b, :k].tolist(), bonds[b, :k, :k].tolist(), k, x[b, :k].numpy()) for b, k in enumerate(counts)]
        hmax = max([max(p["n_hydrogens"], 0) for p in placed] + [0])
        out = dict(coords=torch.zeros(len(counts), hmax, 3), parents=torch.full((len(counts), hmax), -1, dtype=torch.int32),
                   counts=torch.zeros(len(counts), W, dtype=torch.int32),
                   n_hydrogens=torch.tensor([p["n_hydrogens"] for p in placed], dtype=torch.int32),
                   unplaced=torch.tensor([p["unplaced"] for p in placed], dtype=torch.int32))
        for b, p in enumerate(placed):
            h = max(p["n_hydrogens"], 0)
            out["coords"][b, :h] = torch.from_numpy(p["coords"].astype(np.float32)).reshape(-1, 3)
            out["parents"][b, :h] = torch.tensor(p["parents"], dtype=torch.int32)
            out["counts"][b, : counts[b]] = torch.tensor(p["counts"], dtype=torch.int32)
        return out
    return run


def _seam_charges(calls):
    def run(z, bonds, n, perceived=None):
        z, bonds = torch.as_tensor(z), torch.as_tensor(bonds)
        counts = torch.as_tensor(n).reshape(-1).tolist()
        calls.append(("charges", len(counts), perceived is not None))
        W = int(bonds.shape[1])
        out = dict(q=torch.zeros(len(counts), W), q_h=torch.zeros(len(counts), W),
                   nh=torch.zeros(len(counts), W, dtype=torch.int32), status=torch.zeros(len(counts), dtype=torch.int32),
                   n_nodes=torch.tensor(counts, dtype=torch.int32))
        for b, k in enumerate(counts):
            c = ER.charges(z[b, :k].tolist(), bonds[b, :k, :k].tolist(), k)
            out["q"][b, :k] = torch.tensor(c["q"], dtype=torch.float32)
            out["q_h"][b, :k] = torch.tensor(c["q_h"], dtype=torch.float32)
            out["nh"][b, :k] = torch.tensor(c["nh"], dtype=torch.int32)
            out["status"][b] = c["status"]
        return out
    return run


def _seam_score(calls):
    def run(reference_points, pts, q, count):
        xr, qr = ES.load_reference_charges(reference_points)
        calls.append(("score", int(qr.numel()), int(pts.shape[0])))
        sim = []
        for b, k in enumerate(torch.as_tensor(count).reshape(-1).tolist()):
            x, c = pts[b, :k].double().numpy(), q[b, :k].double().numpy()
            ok = np.isfinite(x).all() and np.isfinite(c).all()
            sim.append(ER.score((xr.double().numpy(), qr.double().numpy()), (x, c))["tanimoto"] if ok else math.nan)
        return torch.tensor(sim, dtype=torch.float32)
    return run


def test_charge_points_in_torch_match_the_restatement():
    f, ref = K.fixtures(), K.references()
    names = [k for k in f if f[k]["mol"][2] <= 7]
    assert K.UNPLACED in names and K.UNCHARGED in names and "no atoms" in names and "methane" in names
    xyz, z, bonds, n = (torch.from_numpy(t) for t in HC.pad_batch([f[k] for k in names], 7, 9))
    placed = _seam_hydrogens([])(xyz, z, bonds, n)
    charges = _seam_charges([])(z, bonds, n)
    pts, q, count = ES.charge_points(xyz, charges, placed)
    assert pts.dtype == torch.float32 and q.dtype == torch.float32 and count.dtype == torch.int32
    assert int(pts.shape[1]) == int(count.max()) == max(len(ref[k]["points"][1]) for k in names)
    for b, name in enumerate(names):
        x_ref, q_ref = ref[name]["points"]
        k = len(q_ref)
        assert int(count[b]) == k, name
        assert not pts[b, k:].any() and not q[b, k:].any(), name
        if k:
            assert np.abs(pts[b, :k].double().numpy() - x_ref).max() <= 1e-6, name
        if name == K.UNCHARGED:
            assert bool(torch.isnan(q[b, :k]).all())
        else:
            assert np.abs(q[b, :k].double().numpy() - q_ref).max(initial=0.0) <= 2e-7, name
    b = names.index(K.UNPLACED)                                 # the stray oxygen carries its two hydrogens' charge: zero net
    assert abs(float(q[b, 3])) <= 1e-7 and abs(float(charges["q"][b, 3])) > 0.3
    with pytest.raises(ValueError, match="at most 256"):
        ES.charge_points(torch.zeros(1, 64, 3), dict(q=torch.zeros(1, 64), q_h=torch.zeros(1, 64), nh=torch.zeros(1, 64, dtype=torch.int32),
                                                     n_nodes=torch.tensor([64])),
                         dict(coords=torch.zeros(1, 193, 3), parents=torch.zeros(1, 193, dtype=torch.int32),
                              counts=torch.zeros(1, 64, dtype=torch.int32), n_hydrogens=torch.tensor([193])))


# ----------------------------------------------------------------------------------------------- host-side checks
def test_reference_charges_thresholds_and_flags():
    nan = float("nan")
    xyz, q = ES.load_reference_charges([(0.5, (0, 0, 0)), (-0.5, (1.5, 0, 0))])
    assert xyz.dtype == torch.float32 and tuple(xyz.shape) == (2, 3) and q.tolist() == [0.5, -0.5]
    again = ES.load_reference_charges((xyz, q))
    assert torch.equal(again[0], xyz) and torch.equal(again[1], q)
    assert len(ES.load_reference_charges([(0.1, (0, 0, 0))] * ES.MAX_POINTS)[1]) == ES.MAX_POINTS
    for bad in ([], 3.5, [(0.1, (0, 0))], [(nan, (0, 0, 0))], [(0.1, (0, nan, 0))], [("donor", (0, 0, 0))], [0.5],
                [(0.1, (0, 0, 0))] * (ES.MAX_POINTS + 1), [(True, (0, 0, 0))], (torch.zeros(2, 3), torch.zeros(3))):
        with pytest.raises(ValueError):
            ES.load_reference_charges(bad)
    assert ES.check_threshold("t", -1) == -1.0 and ES.check_threshold("t", 1) == 1.0 and ES.check_threshold("t", -0.2) == -0.2
    for bad in (-1.0001, 1.0001, True, nan, "0.5", None, [0.5]):
        with pytest.raises(ValueError, match=r"\[-1, 1\]"):
            ES.check_threshold("t", bad)
    assert [ES.check_rank_by(v) for v in ("shape", "combo", "electrostatic")] == ["shape", "combo", "electrostatic"]
    for bad in ("esp", None, 1):
        with pytest.raises(ValueError):
            ES.check_rank_by(bad)
    assert ES.select_score(0.5, -0.25) == 0.25 and math.isnan(ES.select_score(0.5, None)) and \
        math.isnan(ES.select_score(None, 0.5)) and math.isnan(ES.select_score(nan, 0.5))
    # shapes and widths are refused before any device work
    with pytest.raises(ValueError, match="at most 64 atoms"):
        ES.partial_charges(torch.zeros(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8), torch.tensor([3]))
    with pytest.raises(ValueError, match="bond_orders"):
        ES.partial_charges(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, 5, dtype=torch.int8), torch.tensor([3]))
    with pytest.raises(ValueError, match="n_nodes"):
        ES.partial_charges(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, 4, dtype=torch.int8), torch.tensor([5]))
    ref = [(0.5, (0, 0, 0)), (-0.5, (1.5, 0, 0))]
    with pytest.raises(ValueError, match="at most 256"):
        ES.electrostatic_tanimoto(ref, torch.zeros(1, 257, 3), torch.zeros(1, 257), torch.tensor([4]))
    with pytest.raises(ValueError, match="charges"):
        ES.electrostatic_tanimoto(ref, torch.zeros(1, 8, 3), torch.zeros(1, 7), torch.tensor([4]))
    with pytest.raises(ValueError, match="points"):
        ES.electrostatic_tanimoto(ref, torch.zeros(1, 8, 2), torch.zeros(1, 8), torch.tensor([4]))
    with pytest.raises(ValueError, match="n_nodes"):
        ES.electrostatic_tanimoto(ref, torch.zeros(1, 8, 3), torch.zeros(1, 8), torch.tensor([9]))


POINTS = [(0.4, (0.2, 0.1, 0.0)), (-0.4, (1.5, -0.4, 0.3)), (0.1, (0.0, 1.6, -0.2)), (-0.1, (-0.8, 0.0, 1.4))]


def test_parse_request_implications_and_defaults():
    gen = _shell_generator()
    parse = postprocess.parse_request
    assert parse(gen, _ref()) == postprocess.Request()
    assert parse(gen, _ref(), electrostatic_scores=False, reference_charges=None, min_electrostatic_tanimoto=None,
                 partial_charges=False) == postprocess.Request()
    req = parse(gen, _ref(), overlay=True, electrostatic_scores=True, reference_charges=POINTS)
    assert req.scores_electrostatics and req.overlay and not req.scores_shape and req.rank_by == "shape"
    assert req.ref_charge_points[1].tolist() == pytest.approx([0.4, -0.4, 0.1, -0.1]) and req.ref_charge_graph is None
    assert not req.removes and not req.partial_charges and req.needs_charges
    req = parse(gen, _ref(), overlay=True, min_electrostatic_tanimoto=-0.2, reference_charges=POINTS)
    assert req.scores_electrostatics and req.min_electrostatic_tanimoto == -0.2 and req.removes
    graph = K.fixtures()["phenol"]["mol"][:2]
    req = parse(gen, _ref(7), overlay=True, electrostatic_scores=True, reference_graph=graph)
    assert req.ref_charge_points is None and req.ref_charge_graph[0] == graph[0] and not req.scores_chemistry
    assert torch.equal(req.ref_charge_graph[2], _ref(7)) and req.ref_graph is None and req.ref_pharm_graph is None
    req = parse(gen, _ref(), overlay=True, top_k=3, electrostatic_scores=True, reference_charges=POINTS,
                rank_by="electrostatic")
    assert req.rank_by == "electrostatic" and req.scores_shape and req.top_k == 3
    req = parse(gen, None, partial_charges=True)                                  # no reference, no pose
    assert req.partial_charges and req.needs_charges and not req.scores_electrostatics and not req.overlay
    assert req == postprocess.Request(partial_charges=True)
    tri = (torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32) * 4,
           torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))
    req = parse(gen, None, overlay=True, electrostatic_scores=True, reference_charges=POINTS, reference_shape=tri)
    assert req.scores_electrostatics and req.ref_charge_points is not None


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_electrostatic_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._pharm_perceive = gen._add_hydrogens = gen._peoe_charges = gen._esp_score = gen._score = gen._pose = _no_device
    call = getattr(gen, entry)
    graph = K.fixtures()["phenol"]["mol"][:2]
    nan = float("nan")
    cases = [dict(electrostatic_scores=True, reference_charges=POINTS),                       # no overlay
             dict(min_electrostatic_tanimoto=0.5, reference_charges=POINTS),
             dict(overlay=True, electrostatic_scores=True),                                   # coordinates carry no graph
             dict(overlay=True, min_electrostatic_tanimoto=0.5),
             dict(overlay=True, reference_charges=POINTS),                                    # charges nobody reads
             dict(overlay=True, electrostatic_scores=True, reference_graph=graph),            # 7 atoms on a 17-atom conformer
             dict(overlay=True, electrostatic_scores=True, reference_graph=3.5),
             dict(overlay=True, electrostatic_scores=True, reference_charges=[]),
             dict(overlay=True, electrostatic_scores=True, reference_charges=[(0.1, (0, nan, 0))]),
             dict(overlay=True, electrostatic_scores=True, reference_charges=[(0.1, (0, 0, 0))] * 257),
             dict(overlay=True, electrostatic_scores=1, reference_charges=POINTS),
             dict(overlay=True, electrostatic_scores="yes", reference_charges=POINTS),
             dict(overlay=True, electrostatic_scores=None, reference_charges=POINTS),
             dict(partial_charges=1), dict(partial_charges="yes"), dict(partial_charges=None),
             dict(rank_by="electrostatic"), dict(rank_by="esp"),
             dict(overlay=True, shape_scores=True, rank_by="electrostatic"),                   # no electrostatic score
             dict(overlay=True, electrostatic_scores=True, reference_charges=POINTS, rank_by="electrostatic")]   # no shape
    for bad in (-1.0001, 1.0001, 2, True, False, nan, "0.5", [0.5]):
        cases.append(dict(overlay=True, min_electrostatic_tanimoto=bad, reference_charges=POINTS))
    for kw in cases:
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    with pytest.raises(ValueError, match="reference_charges"):                # a mesh has no graph
        tri = (torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32) * 4,
               torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))
        call(reference_shape=tri, n_atoms=17, n_samples=4, overlay=True, electrostatic_scores=True, reference_graph=graph)
    for finisher in ("rdkit", HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                                         "finish_tag_chunk")):
        gen.finisher = finisher
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, overlay=True, electrostatic_scores=True, reference_charges=POINTS)
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, partial_charges=True)


# ----------------------------------------------------------------------------------------------- select
def _rows(shape, pharm, esp, keys=None):
    n = len(shape)
    measured = [Measured(shape_tanimoto=s, pharmacophore_tanimoto=p, electrostatic_tanimoto=e,
                         graph_key=None if keys is None else keys[i], chemical_tanimoto=0.1)
                for i, (s, p, e) in enumerate(zip(shape, pharm, esp))]
    return postprocess.Rows(list(range(n)), list(range(n)), measured, list(range(n)))


def test_select_filters_behind_the_pharmacophore_filter_and_ranks_by_the_sum():
    nan = float("nan")
    Req = postprocess.Request
    shape = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4]
    pharm = [0.1, 0.5, 0.6, 0.7, 0.9, 0.3]
    esp = [-0.1, 0.5, nan, None, 0.9, 0.3]
    none = lambda rows: (_ for _ in ()).throw(AssertionError("no pair matrix was asked for"))        # noqa: E731
    # NaN and None do not pass, not even the lowest threshold; the input's order stays
    assert postprocess.select(_rows(shape, pharm, esp), Req(scores_electrostatics=True, min_electrostatic_tanimoto=0.3),
                              none, none) == [1, 4, 5]
    assert postprocess.select(_rows(shape, pharm, esp), Req(scores_electrostatics=True, min_electrostatic_tanimoto=-1.0),
                              none, none) == [0, 1, 4, 5]
    both = Req(scores_pharmacophore=True, min_pharmacophore_tanimoto=0.4, scores_electrostatics=True,
               min_electrostatic_tanimoto=0.0)
    assert postprocess.select(_rows(shape, pharm, esp), both, none, none) == [1, 4]
    # before `unique`: the best-ranked copy of a graph is chosen among the rows that passed
    keys = [7, 7, 8, 8, 9, 9]
    req = Req(scores_shape=True, scores_electrostatics=True, min_electrostatic_tanimoto=0.0, unique=True)
    assert postprocess.select(_rows(shape, pharm, esp, keys), req, none, none) == [1, 4]
    assert postprocess.select(_rows(shape, pharm, esp, keys), Req(scores_shape=True, unique=True), none, none) == [0, 2, 4]
    # rank_by: shape alone and "combo" as before, or shape + electrostatic (NaN / None rank last)
    assert postprocess.select(_rows(shape, pharm, esp), Req(scores_shape=True, top_k=3), none, none) == [0, 1, 2]
    combo = Req(scores_shape=True, scores_pharmacophore=True, rank_by="combo", top_k=3)
    assert postprocess.select(_rows(shape, pharm, esp), combo, none, none) == [4, 1, 2]               # 1.4, 1.3, 1.3
    by_esp = Req(scores_shape=True, scores_electrostatics=True, rank_by="electrostatic", top_k=6)
    assert postprocess.select(_rows(shape, pharm, esp), by_esp, none, none) == [4, 1, 0, 5, 2, 3]    # 1.4 1.3 0.8 0.7, NaN
    by_esp = Req(scores_shape=True, scores_electrostatics=True, rank_by="electrostatic", unique=True)
    assert postprocess.select(_rows(shape, pharm, esp, keys), by_esp, none, none) == [1, 2, 4]
    by_esp = Req(scores_shape=True, scores_electrostatics=True, rank_by="electrostatic", min_shape_tanimoto=0.55)
    assert postprocess.select(_rows(shape, pharm, esp), by_esp, none, none) == [1, 0, 2, 3]          # shape alone thresholds


# ----------------------------------------------------------------------------------------------- the record path
SHARD = ["ethanol", "acetic acid", "phenol", "pyridine", "acetamide", "imidazole", "dimethyl sulfone", K.UNCHARGED]


def _graph_shard(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
    ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
    f = K.fixtures()
    el = torch.full((n_samples, 42), 9, dtype=torch.int8)                         # junk beyond the atoms
    bond = torch.full((n_samples, 42, 42), 3, dtype=torch.int8)
    x = torch.zeros(n_samples, 12, 3)
    n = torch.zeros(n_samples, dtype=torch.int32)
    for b, sid in enumerate(ids):
        z, adj, k = f[SHARD[sid]]["mol"]
        el[b, :k] = torch.tensor(z, dtype=torch.int8)
        bond[b, :k, :k] = torch.tensor(adj, dtype=torch.int8)
        n[b] = k
        x[b, :k] = torch.from_numpy(f[SHARD[sid]]["xyz"])
        if sid == 6:
            x[b, 0, 0] = float("nan")                                             # its pose fails
    valid = torch.tensor([0 if sid == 4 else 1 for sid in ids], dtype=torch.uint8)
    return dict(x=x, elements=el, bond=bond, n_nodes=n, valid=valid)


def _own(m, name):
    """The restatement's charges and score of a record's own coordinates and graph."""
    z, adj, n = K.fixtures()[name]["mol"]
    assert m.atomic_numbers == z and m.bond_orders.tolist() == adj
    ch = ER.charges(z, adj, n)
    placed = HR.place(z, adj, n, m.coords.numpy())
    xr, qr = ES.load_reference_charges(POINTS)
    x, q = ER.points(n, m.coords.numpy(), dict(ch, q=[float(np.float32(v)) for v in ch["q"]],
                                               q_h=[float(np.float32(v)) for v in ch["q_h"]]), placed)
    x = np.vstack([x[:n], placed["coords"].astype(np.float32).astype(np.float64).reshape(-1, 3)])
    return ch, np.float32(ER.score((xr.double().numpy(), qr.double().numpy()), (x, q))["tanimoto"])


def test_record_path_carries_the_values_and_launches_nothing_unasked():
    calls = []
    gen = _shell_generator()
    gen._pharm_perceive, gen._add_hydrogens = _seam_perceive(calls), _seam_hydrogens(calls)
    gen._peoe_charges, gen._esp_score = _seam_charges(calls), _seam_score(calls)
    gen._generate_shard = _graph_shard
    gen._pose = _stub_overlay(lambda k: k * 0.0 + 0.5)
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    kw = dict(reference_conformer=_ref(), n_samples=8, overlay=True)

    plain = gen.generate_conformers(**kw)
    assert calls == [] and [m.sample_id for m in plain] == [0, 1, 2, 3, 5, 6, 7]             # 4: invalid
    assert all(m.electrostatic_tanimoto is None and m.partial_charges is None and m.hydrogen_charges is None for m in plain)
    got = gen.generate_conformers(electrostatic_scores=True, reference_charges=POINTS, **kw)
    # perceived once, placed once, one charge launch, one score call over the rows
    assert calls == [("perceive", 8), ("hydrogens", 8, True), ("charges", 8, True), ("score", 4, 8)]
    assert [m.sample_id for m in got] == [0, 1, 2, 3, 5, 6, 7]
    for a, m in zip(plain, got):
        assert m.partial_charges is None and m.hydrogen_charges is None and m.hydrogen_coords is None
        if m.sample_id in (6, 7):                               # a failed pose; an element without parameters
            assert math.isnan(m.electrostatic_tanimoto)
            continue
        assert a == m
        assert np.float32(m.electrostatic_tanimoto) == _own(m, SHARD[m.sample_id])[1], m.sample_id
    assert len({m.electrostatic_tanimoto for m in got if m.sample_id < 6}) == 5

    # with add_hydrogens the placement is made once and serves both; the scores keep their bits
    del calls[:]
    both = gen.generate_conformers(electrostatic_scores=True, reference_charges=POINTS, add_hydrogens=True,
                                   partial_charges=True, **kw)
    assert calls == [("perceive", 8), ("hydrogens", 8, True), ("charges", 8, True), ("score", 4, 8)]
    for m, e in zip(both, got):
        assert repr(m.electrostatic_tanimoto) == repr(e.electrostatic_tanimoto)
        name = SHARD[m.sample_id]
        n = len(m.atomic_numbers)
        assert tuple(m.partial_charges.shape) == (n,) == tuple(m.hydrogen_charges.shape)
        assert m.partial_charges.dtype == torch.float32
        if m.sample_id == 7:
            assert bool(torch.isnan(m.partial_charges).all()) and bool(torch.isnan(m.hydrogen_charges).all())
            continue
        ch = _own(m, name)[0] if m.sample_id != 6 else ER.charges(*K.fixtures()[name]["mol"])
        assert m.partial_charges.tolist() == [float(np.float32(v)) for v in ch["q"]]
        assert m.hydrogen_charges.tolist() == [float(np.float32(v)) for v in ch["q_h"]]
        if m.sample_id != 6:
            lines = m.to_xyz_block(hydrogens=True, charges=True).split("\n")[2:-1]
            assert len(lines) == n + len(m.hydrogen_parents) and all(len(ln.split()) == 5 for ln in lines)
            assert abs(sum(float(ln.split()[4]) for ln in lines)) <= 1e-5
            assert m.to_xyz_block(charges=True).split("\n")[2].split()[4] == "%.6f" % float(m.partial_charges[0])
            assert m.to_xyz_block(hydrogens=True) == "\n".join(" ".join(ln.split()[:4]) for ln in
                                                              m.to_xyz_block(hydrogens=True, charges=True).split("\n")[:-1]) + "\n"
    with pytest.raises(ValueError, match="partial_charges=True"):
        got[0].to_xyz_block(charges=True)

    # partial_charges alone: no reference, no pose, no placement
    del calls[:]
    alone = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, partial_charges=True)
    assert calls == [("perceive", 8), ("charges", 8, True)]
    assert all(m.electrostatic_tanimoto is None and m.pose is None and m.partial_charges is not None for m in alone)

    # the reference's own charges from its graph on the conformer's coordinates: perceived, placed and charged first
    del calls[:]
    fx = K.fixtures()["phenol"]
    ref_xyz = torch.from_numpy(fx["xyz"])
    own = gen.generate_conformers(electrostatic_scores=True, reference_graph=fx["mol"][:2],
                                  **dict(kw, reference_conformer=ref_xyz))
    n_ref = len(K.references()["phenol"]["points"][1])
    assert calls == [("perceive", 8), ("hydrogens", 8, True), ("charges", 8, True), ("perceive", 1), ("hydrogens", 1, True),
                     ("charges", 1, True), ("score", n_ref, 8)]
    assert all((m.electrostatic_tanimoto is not None) for m in own)
    with pytest.raises(ValueError, match="without charge parameters"):
        gen.generate_conformers(electrostatic_scores=True, reference_graph=([6, 14, 6], [[0, 1, 0], [1, 0, 1], [0, 1, 0]]),
                                **dict(kw, reference_conformer=_ref(3)))

    def ids(entry="generate_conformers", **more):
        return [m.sample_id for m in getattr(gen, entry)(**dict(kw, reference_charges=POINTS, **more))]
    by_id = {m.sample_id: m for m in got}
    scores = sorted(m.electrostatic_tanimoto for m in got if m.sample_id < 6)
    t = float(scores[2])
    assert ids(min_electrostatic_tanimoto=t) == [i for i in (0, 1, 2, 3, 5) if by_id[i].electrostatic_tanimoto >= t]
    assert ids(min_electrostatic_tanimoto=-1.0) == [0, 1, 2, 3, 5]                # NaN never passes
    shaped = {m.sample_id: m.shape_tanimoto for m in gen.generate_conformers(shape_scores=True, **kw)}
    order = sorted((i for i in by_id if i < 6), key=lambda i: (-(shaped[i] + by_id[i].electrostatic_tanimoto), i))
    assert ids(electrostatic_scores=True, rank_by="electrostatic", top_k=3) == order[:3]
    assert ids("generate_conformers_sharded", electrostatic_scores=True, rank_by="electrostatic", top_k=3) == order[:3]
    assert [repr(m.electrostatic_tanimoto) for m in gen.forward(electrostatic_scores=True, reference_charges=POINTS, **kw)] \
        == [repr(m.electrostatic_tanimoto) for m in got]
    assert isinstance(got[0], GeneratedMolecule)


def test_measured_from_tensors_slices_the_charges_on_first_read():
    inf = float("inf")
    q = torch.tensor([[0.1, -0.1, inf], [float("nan"), inf, inf], [inf, inf, inf]])
    qh = torch.tensor([[0.05, 0.0, inf], [float("nan"), inf, inf], [inf, inf, inf]])
    rec = measured_from_tensors(dict(partial_charges=q, hydrogen_charges=qh, electrostatic_tanimoto=torch.tensor([0.5, float("nan"), 0.0])), 3)
    assert [r.partial_charges[2] for r in rec] == [2, 1, 0] and rec[0].partial_charges[0] is rec[1].partial_charges[0]
    assert rec[0].electrostatic_tanimoto == 0.5 and math.isnan(rec[1].electrostatic_tanimoto)
    assert all(getattr(Measured(), k) is None for k in ("electrostatic_tanimoto", "partial_charges", "hydrogen_charges"))


# ----------------------------------------------------------------------------------------------- the C entries
def test_c_entries_refuse_bad_arguments_without_a_device():
    from ml_conformer_generator_amd import _lib
    assert "mcg_charges_peoe" in _lib.SIGNATURES and "mcg_esp_overlap" in _lib.SIGNATURES
    h = _lib.lib()
    assert h.mcg_abi_version() == 4
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    good = [p, p, p, p, p, p, 1, 8, p, p, p, p, None]
    assert h.mcg_charges_peoe(*good[:6], 0, 8, *good[8:]) == 0                    # B = 0 launches nothing
    for k in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11):                                    # each required buffer
        bad = list(good)
        bad[k] = None
        assert h.mcg_charges_peoe(*bad) != 0 and b"mcg_charges_peoe" in h.mcg_last_error(), k
    for B, W in ((-1, 8), (16385, 8), (1, 0), (1, 65)):
        assert h.mcg_charges_peoe(*good[:6], B, W, *good[8:]) != 0, (B, W)
    good = [p, p, 4, p, p, p, 1, 8, 1.0, None, p, p, p, None]
    assert h.mcg_esp_overlap(*good[:6], 0, *good[7:]) == 0                        # B = 0 launches nothing
    for k in (0, 1, 3, 4, 5, 10, 11, 12):
        bad = list(good)
        bad[k] = None
        assert h.mcg_esp_overlap(*bad) != 0 and b"mcg_esp_overlap" in h.mcg_last_error(), k
    for P, B, PW, mu in ((0, 1, 8, 1.0), (257, 1, 8, 1.0), (4, -1, 8, 1.0), (4, 16385, 8, 1.0), (4, 1, 0, 1.0),
                         (4, 1, 257, 1.0), (4, 1, 8, 0.0), (4, 1, 8, -1.0), (4, 1, 8, float("nan")), (4, 1, 8, float("inf"))):
        assert h.mcg_esp_overlap(p, p, P, p, p, p, B, PW, mu, None, p, p, p, None) != 0, (P, B, PW, mu)


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_esp`: both entries' argument checks in a stand-alone program under host-side ASan + UBSan, on the CPU."""
    exe = str(tmp_path / "esp_arg_check")
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_esp", f"ESP_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 wrong" in ran.stdout, ran.stdout + ran.stderr


def test_header_compiles_with_the_new_declarations(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mlconfgen_hip.h"\n'
                   "int main(void) {\n"
                   "  int (*a)(const int32_t*, const int8_t*, const int32_t*, const uint8_t*, const uint64_t*, const int32_t*, int, int,\n"
                   "           float*, float*, int32_t*, int32_t*, void*) = mcg_charges_peoe;\n"
                   "  int (*b)(const float*, const float*, int, const float*, const float*, const int32_t*, int, int, float,\n"
                   "           const float*, float*, float*, float*, void*) = mcg_esp_overlap;\n"
                   "  return (a == 0) + (b == 0) + MCG_CHARGES_MAX_ATOMS - 64 + MCG_ESP_MAX_POINTS - 256 + MCG_CHARGES_MAX_B\n"
                   "         - MCG_ESP_MAX_B;\n}\n")
    inc = os.path.join(REPO, "include")
    assert shutil.which("gcc") or shutil.which("g++") or shutil.which("cc")
    for cc, flags in (("gcc", ["-std=c99", "-Wall", "-Wextra", "-Werror"]), ("g++", ["-std=c++11", "-Wall", "-Werror", "-x", "c++"]),
                      ("cc", ["-std=c99", "-Wall", "-Werror"])):
        if shutil.which(cc):
            r = subprocess.run([cc, *flags, "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
