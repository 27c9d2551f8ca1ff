"""The pharmacophore definition and its plumbing without a GPU: the restatement (`pharmacophore_ref`) against pins written
out by hand, its invariances and score properties, mutations of the definition that the pass rules must catch, the
argument checks of the two entry points and of `parse_request`, `select` on fake rows, and the measuring / returning
paths with the device seams replaced by the restatement."""
import ctypes
import math
import os
import random

import numpy as np
import pytest
import torch

import pharmacophore_cases as C
import pharmacophore_ref as R
from ml_conformer_generator_amd import pharmacophore as PH
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd.handoff import GeneratedMolecule, Measured
from test_fingerprint_host import BondedMol, _as_mol
from test_shape_overlay_host import _no_device, _ref, _shell_generator, _Stage, _stub_overlay


# ----------------------------------------------------------------------------------------------- the restatement
def test_restatement_reproduces_its_pins():
    assert {"ethanol", "dimethyl ether", "acetic acid", "methanesulfonic acid", "acetamide", "N,N-dimethylacetamide",
            "trimethylamine", "aniline", "acetamidine", "acetonitrile", "benzene", "chlorobenzene", "pyridine", "pyrrole",
            "N-methylpyrrole", "imidazole", "oxazole", "indole", "naphthalene", "cyclohexane", "methane",
            "no atoms"} <= set(C.PINNED)
    for name, (mol, types, rings, nh) in C.PINNED.items():
        assert R.perceive(*mol) == (types, rings, nh), name
    # each ring of a fused system is found once; a Kekule ring is no ring
    assert R.rings(*C.PINNED["naphthalene"][0]) == [63, 1008] and R.rings(*C.PINNED["indole"][0]) == [271, 504]
    kekule = R.mol([6] * 6, [(i, (i + 1) % 6, 1 + i % 2) for i in range(6)])
    assert R.perceive(*kekule)[1] == []
    assert R.perceive([26, 6], [[0, 1], [1, 0]], 2)[0] == [0, 0]          # an element outside the table carries nothing
    assert R.rings(*C.k33()) == [63] and len(R.rings(*C.petersen_field())) == 132


def test_perception_is_covariant_under_renumbering():
    rng = random.Random(3)
    mols = [m for m, _, _, _ in C.PINNED.values()] + C.molecule_like_set()[:150] + [C.k33(), C.petersen_field()]
    for mol in mols:
        types, rings, nh = R.perceive(*mol)
        for _ in range(2):
            p, moved = C.random_permutation(rng, mol)
            t2, r2, h2 = R.perceive(*moved)
            assert t2 == [types[p[i]] for i in range(mol[2])] and h2 == [nh[p[i]] for i in range(mol[2])]
            assert r2 == sorted(R.permute_mask(m, p) for m in rings)


def test_junk_graphs_terminate_within_the_bounds():
    rng = random.Random(64)
    for k in range(12):
        mol = C.junk_graph(rng, 64) if k < 6 else C.sparse_aromatic_junk(rng, 64)
        stats = {}
        found = R.rings(*mol, stats=stats)
        assert stats["paths"] <= 48 and len(found) <= R.MAX_RINGS, k
        assert len(R.perceive(*mol)[0]) == 64
    stats = {}
    R.rings(*C.petersen_field(), stats=stats)                 # every atom with three aromatic bonds: the most there can be
    assert 24 <= stats["paths"] <= 48


def _feats(name, xyz=None, seed=0):
    mol = C.PINNED[name][0] if isinstance(name, str) else name
    types, rings, _ = R.perceive(*mol)
    if xyz is None:
        g = np.random.default_rng(seed)
        xyz = g.normal(0, 1.5, (mol[2], 3)).astype(np.float32)
    return R.features(xyz, types, rings)


def test_score_properties():
    a, b = _feats(C.REFERENCE_MOLECULE, seed=1), _feats("indole", seed=2)
    assert R.tanimoto(a, a) == 1.0 and R.tanimoto(b, b) == 1.0
    assert R.tanimoto(a, b) == pytest.approx(R.tanimoto(b, a), rel=1e-15)
    for k in range(30):
        x = _feats(C.molecule_like_set()[40 + k], seed=10 + k)
        if x:
            assert 0.0 <= R.tanimoto(a, x) <= 1.0
    # a type mismatch contributes nothing
    p = np.zeros(3, dtype=np.float32)
    assert R.overlap([(0, p)], [(1, p)]) == 0.0 and R.overlap([(0, p)], [(0, p)]) == 1.0
    assert R.tanimoto([(0, p), (5, p)], [(1, p), (5, p)]) == pytest.approx(1 / 3)
    # T falls as one matched feature is pulled away; matches flips at 1.5 A
    base = [(0, p), (2, np.array([3, 0, 0], dtype=np.float32))]
    last = 2.0
    for d in np.linspace(0.0, 6.0, 25):
        moved = [(0, np.array([0, d, 0], dtype=np.float32)), base[1]]
        t = R.tanimoto(base, moved)
        assert t < last
        last = t
        assert R.matches(base, moved) == (2 if d <= 1.5 else 1)
    assert R.overlap(base, base) == pytest.approx(2.0) and R.KAPPA == 0.5
    assert R.overlap([(0, p)], [(0, np.array([1, 1, 0], dtype=np.float32))]) == pytest.approx(math.exp(-1.0))


def test_score_cases_keep_clear_of_the_match_boundary():
    refs, cases = C.score_cases()
    assert {len(v) for v in refs.values()} == {1, 10, R.MAX_FEATURES}
    assert {c["mol"][2] for c in cases} >= set(C.CANDIDATE_SIZES)
    worst = math.inf
    for c in cases:
        types, rings, _ = R.perceive(*c["mol"])
        for tr, pr in refs[c["ref"]]:
            for tm, pm in R.features(c["coords"], types, rings):
                if tr == tm:
                    d = math.sqrt(float(((np.float64(pr) - np.float64(pm)) ** 2).sum()))
                    worst = min(worst, abs(d - 1.5))
    assert worst >= C.MARGIN


# ----------------------------------------------------------------------------------------------- mutations
def test_mutations_are_caught():
    """Each change of the definition fails a stated pass rule on a pinned case: perception is compared bit for bit, the
    score within SCORE_C * 2^-24."""
    pins = list(C.PINNED.items())

    def caught(**change):
        return [name for name, (mol, types, rings, _) in pins if R.perceive(*mol, **change)[:2] != (types, rings)]
    for rule in R.RULES:
        assert caught(rules=R.RULES - {rule}), rule
    assert "dimethyl ether" in caught(swap_da=True) and "pyrrole" in caught(swap_da=True)
    assert set(caught(dedupe=False)) >= {"benzene", "naphthalene", "indole"}
    # kappa off by 1 %: far outside the score's pass rule
    ref = _feats(C.REFERENCE_MOLECULE, seed=1)
    types, rings, _ = R.perceive(*C.REFERENCE_MOLECULE)
    g = np.random.default_rng(1)
    xyz = g.normal(0, 1.5, (14, 3)).astype(np.float32)
    shifted = R.features(xyz + np.float32(0.7), types, rings)
    moved = abs(R.tanimoto(ref, shifted, R.KAPPA * 1.01) - R.tanimoto(ref, shifted))
    print(f"kappa * 1.01 moves T by {moved:.3e} = {moved / (R.SCORE_C * R.EPS32):.0f} x the pass value")
    assert moved > 100 * R.SCORE_C * R.EPS32                # measured: 1 071 x
    assert R.SCORE_C == 4.0 * R.SCORE_C_MEASURED


# ----------------------------------------------------------------------------------------------- entry points
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check

    def perceive(z=p, bonds=p, n=p, B=3, W=42, types=p, count=p, rings=p):
        return h.mcg_pharm_perceive(z, bonds, n, B, W, types, count, rings, None)

    for bad in (dict(z=None), dict(bonds=None), dict(n=None), dict(types=None), dict(count=None), dict(rings=None),
                dict(B=-1), dict(W=0), dict(W=65), dict(W=-3)):
        assert perceive(**bad) == 1, bad
        assert b"mcg_pharm_perceive" in h.mcg_last_error(), bad

    def score(coords=p, n=p, types=p, rings=p, count=p, B=3, N=42, W=42, xyz=p, typ=p, F=10, o_rr=p, o_rm=p, o_mm=p,
              t=p, hits=p, parts=None):
        return h.mcg_pharm_score(coords, n, types, rings, count, B, N, W, xyz, typ, F, o_rr, o_rm, o_mm, t, hits, parts,
                                 None)

    for bad in (dict(n=None), dict(types=None), dict(rings=None), dict(count=None), dict(xyz=None), dict(typ=None),
                dict(o_rm=None), dict(o_mm=None), dict(t=None), dict(hits=None), dict(B=-1), dict(N=0), dict(N=65),
                dict(W=0), dict(W=65), dict(F=0), dict(F=PH.MAX_FEATURES + 1), dict(coords=None, B=2)):
        assert score(**bad) == 1, bad
        assert b"mcg_pharm_score" in h.mcg_last_error(), bad
    assert perceive(B=0) == 0 and score(B=0) == 0 and score(coords=None, B=0) == 0       # nothing to do, nothing launched
    assert h.mcg_abi_version() == 4 and PH.MAX_FEATURES == R.MAX_FEATURES >= 352 and PH.MAX_RINGS == R.MAX_RINGS
    assert "mcg_pharm_perceive" in _lib.SIGNATURES and "mcg_pharm_score" in _lib.SIGNATURES
    with pytest.raises(ValueError):
        PH.perceive_features(torch.zeros(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8),
                             torch.tensor([3]))
    with pytest.raises(ValueError):
        PH.perceive_features(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8),
                             torch.tensor([3, 6]))


def test_load_reference_features_and_checkers():
    xyz, typ = PH.load_reference_features([("donor", (0, 1, 2)), ("ring", [0.5, 0.25, -1]), ("hydrophobe", (3, 3, 3))])
    assert typ.tolist() == [0, 5, 4] and typ.dtype == torch.uint8 and xyz.dtype == torch.float32
    assert xyz.tolist() == [[0, 1, 2], [0.5, 0.25, -1], [3, 3, 3]]
    again = PH.load_reference_features((xyz, typ))
    assert torch.equal(again[0], xyz) and torch.equal(again[1], typ)
    assert PH.TYPE_NAMES == R.TYPE_NAMES and PH.KAPPA == R.KAPPA and PH.MATCH_DISTANCE ** 2 == R.MATCH_D2
    nan = float("nan")
    for bad in ([], [("doner", (0, 0, 0))], [("donor", (0, 0))], [("donor", (0, 0, nan))], [("donor", (0, 0, math.inf))],
                [("donor", "abc")], [("donor",)], 3.5, None, [("ring", (0, 0, 0))] * (PH.MAX_FEATURES + 1),
                (torch.zeros(2, 3), torch.tensor([0, 6], dtype=torch.uint8))):
        with pytest.raises(ValueError):
            PH.load_reference_features(bad)
    assert len(PH.load_reference_features([("ring", (0, 0, 0))] * PH.MAX_FEATURES)[1]) == PH.MAX_FEATURES
    assert PH.check_threshold("t", 0) == 0.0 and PH.check_threshold("t", 1) == 1.0 and PH.check_threshold("t", 0.3) == 0.3
    for bad in (-0.1, 1.0001, True, nan, "0.5", None, [0.5]):
        with pytest.raises(ValueError):
            PH.check_threshold("t", bad)
    assert PH.check_flag("f", True) is True and PH.check_rank_by("combo") == "combo"
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            PH.check_flag("f", bad)
    for bad in ("pharmacophore", None, 1):
        with pytest.raises(ValueError):
            PH.check_rank_by(bad)
    # the host-side list of the reference: the order and the fp32 centroid of the definition
    mol = C.PINNED["indole"][0]
    types, rings, _ = R.perceive(*mol)
    xyz = torch.randn(1, 12, 3, generator=torch.Generator().manual_seed(5))
    masks = torch.zeros(1, 32, dtype=torch.int64)
    masks[0, :2] = torch.tensor(rings)
    points = PH.feature_points(xyz, torch.tensor([types + [31] * 0], dtype=torch.uint8), masks, torch.tensor([2]))[0]
    want = R.features(xyz[0, :9].numpy(), types, rings)
    assert [k for k, _ in points] == [R.TYPE_NAMES[t] for t, _ in want]
    assert np.array_equal(np.array([p for _, p in points], np.float32), np.array([p for _, p in want], np.float32))


# ----------------------------------------------------------------------------------------------- parse_request
FEATS = [("donor", (0.0, 0.0, 0.0)), ("ring", (1.5, 0.0, 0.0))]


def test_parse_request_implications_and_defaults():
    gen = _shell_generator()
    parse = postprocess.parse_request
    assert parse(gen, _ref()) == postprocess.Request()
    assert parse(gen, _ref(), pharmacophore_scores=False, reference_pharmacophore=None, min_pharmacophore_tanimoto=None,
                 rank_by="shape") == postprocess.Request()
    req = parse(gen, _ref(), overlay=True, pharmacophore_scores=True, reference_pharmacophore=FEATS)
    assert req.scores_pharmacophore and req.overlay and not req.scores_shape and req.rank_by == "shape"
    assert req.ref_features[1].tolist() == [0, 5] and req.ref_pharm_graph is None and not req.removes and req.measures
    req = parse(gen, _ref(), overlay=True, min_pharmacophore_tanimoto=0.25, reference_pharmacophore=FEATS)
    assert req.scores_pharmacophore and req.min_pharmacophore_tanimoto == 0.25 and req.removes
    graph = C.PINNED["aniline"][0][:2]
    req = parse(gen, _ref(7), overlay=True, pharmacophore_scores=True, reference_graph=graph)
    assert req.ref_features is None and req.ref_pharm_graph[0] == graph[0] and not req.scores_chemistry
    assert torch.equal(req.ref_pharm_graph[2], _ref(7)) and req.ref_graph is None
    req = parse(gen, _ref(7), overlay=True, pharmacophore_scores=True, chemical_scores=True, reference_graph=graph)
    assert req.scores_chemistry and req.ref_graph[0] == graph[0] and req.ref_pharm_graph[0] == graph[0]
    req = parse(gen, _ref(), overlay=True, top_k=3, pharmacophore_scores=True, reference_pharmacophore=FEATS,
                rank_by="combo")
    assert req.rank_by == "combo" and req.scores_shape and req.top_k == 3
    tri = (torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32) * 4,
           torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))
    req = parse(gen, None, overlay=True, pharmacophore_scores=True, reference_pharmacophore=FEATS, reference_shape=tri)
    assert req.scores_pharmacophore and req.ref_features is not None


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_pharmacophore_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._pharm_perceive = gen._pharm_score = gen._score = gen._pose = _no_device
    call = getattr(gen, entry)
    graph = C.PINNED["aniline"][0][:2]
    nan = float("nan")
    cases = [dict(pharmacophore_scores=True, reference_pharmacophore=FEATS),                  # no overlay
             dict(min_pharmacophore_tanimoto=0.5, reference_pharmacophore=FEATS),
             dict(overlay=True, pharmacophore_scores=True),                                   # coordinates carry no graph
             dict(overlay=True, min_pharmacophore_tanimoto=0.5),
             dict(overlay=True, reference_pharmacophore=FEATS),                               # features nobody reads
             dict(overlay=True, pharmacophore_scores=True, reference_graph=graph),            # 7 atoms on a 17-atom conformer
             dict(overlay=True, pharmacophore_scores=True, reference_graph=3.5),
             dict(overlay=True, pharmacophore_scores=True, reference_pharmacophore=[]),
             dict(overlay=True, pharmacophore_scores=True, reference_pharmacophore=[("doner", (0, 0, 0))]),
             dict(overlay=True, pharmacophore_scores=True, reference_pharmacophore=[("donor", (0, nan, 0))]),
             dict(overlay=True, pharmacophore_scores=True, reference_pharmacophore=[("ring", (0, 0, 0))] * 353),
             dict(overlay=True, pharmacophore_scores=1, reference_pharmacophore=FEATS),
             dict(overlay=True, pharmacophore_scores="yes", reference_pharmacophore=FEATS),
             dict(overlay=True, pharmacophore_scores=None, reference_pharmacophore=FEATS),
             dict(rank_by="combo"), dict(rank_by="pharmacophore"), dict(rank_by=None),
             dict(overlay=True, shape_scores=True, rank_by="combo"),                          # no pharmacophore score
             dict(overlay=True, pharmacophore_scores=True, reference_pharmacophore=FEATS, rank_by="combo")]  # no shape score
    for bad in (-0.1, 1.0001, 2, True, False, nan, "0.5", [0.5]):
        cases.append(dict(overlay=True, min_pharmacophore_tanimoto=bad, reference_pharmacophore=FEATS))
    for kw in cases:
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    with pytest.raises(ValueError, match="reference_pharmacophore"):          # a mesh has no graph
        tri = (torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32) * 4,
               torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]))
        call(reference_shape=tri, n_atoms=17, n_samples=4, overlay=True, pharmacophore_scores=True, reference_graph=graph)
    gen.finisher = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                              "finish_tag_chunk")
    with pytest.raises(ValueError, match="custom finisher"):
        call(reference_conformer=_ref(), n_samples=4, overlay=True, pharmacophore_scores=True, reference_pharmacophore=FEATS)


# ----------------------------------------------------------------------------------------------- select
def _rows(shape, pharm, keys=None):
    n = len(shape)
    measured = [Measured(shape_tanimoto=s, pharmacophore_tanimoto=p, graph_key=None if keys is None else keys[i],
                         chemical_tanimoto=0.1)
                for i, (s, p) in enumerate(zip(shape, pharm))]
    return postprocess.Rows(list(range(n)), list(range(n)), measured, list(range(n)))


def test_select_filters_and_ranks_by_the_combined_score():
    nan = float("nan")
    Req = postprocess.Request
    shape = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4]
    pharm = [0.1, 0.5, nan, None, 0.9, 0.3]
    none = lambda rows: (_ for _ in ()).throw(AssertionError("no pair matrix was asked for"))        # noqa: E731
    # the filter: NaN and None do not pass, not even a threshold of 0; the input's order stays
    assert postprocess.select(_rows(shape, pharm), Req(scores_pharmacophore=True, min_pharmacophore_tanimoto=0.3),
                              none, none) == [1, 4, 5]
    assert postprocess.select(_rows(shape, pharm), Req(scores_pharmacophore=True, min_pharmacophore_tanimoto=0.0),
                              none, none) == [0, 1, 4, 5]
    # behind max_chemical_tanimoto, before unique: the best-ranked copy of a graph is chosen among the rows that passed
    keys = [7, 7, 8, 8, 9, 9]
    req = Req(scores_shape=True, scores_pharmacophore=True, min_pharmacophore_tanimoto=0.3, unique=True)
    assert postprocess.select(_rows(shape, pharm, keys), req, none, none) == [1, 4]
    assert postprocess.select(_rows(shape, pharm, keys), Req(scores_shape=True, unique=True), none, none) == [0, 2, 4]
    req = Req(scores_chemistry=True, max_chemical_tanimoto=0.05, min_pharmacophore_tanimoto=0.0)
    assert postprocess.select(_rows(shape, pharm), req, none, none) == []
    # rank_by: shape alone, or the sum (NaN / None rank last)
    assert postprocess.select(_rows(shape, pharm), Req(scores_shape=True, top_k=3), none, none) == [0, 1, 2]
    combo = Req(scores_shape=True, scores_pharmacophore=True, rank_by="combo", top_k=3)
    assert postprocess.select(_rows(shape, pharm), combo, none, none) == [4, 1, 0]                # 1.4, 1.3, 1.0
    combo = Req(scores_shape=True, scores_pharmacophore=True, rank_by="combo", top_k=6)
    assert postprocess.select(_rows(shape, pharm), combo, none, none) == [4, 1, 0, 5, 2, 3]
    # unique under combo keeps the copy with the better sum: 1 (1.3) over 0 (1.0), 5 (0.7) over 4? no - 4 (1.4)
    combo = Req(scores_shape=True, scores_pharmacophore=True, rank_by="combo", unique=True)
    assert postprocess.select(_rows(shape, pharm, keys), combo, none, none) == [1, 2, 4]
    # min_shape_tanimoto thresholds the shape score alone, whatever the ranking
    combo = Req(scores_shape=True, scores_pharmacophore=True, rank_by="combo", min_shape_tanimoto=0.55)
    assert postprocess.select(_rows(shape, pharm), combo, none, none) == [1, 0, 2, 3]
    plain = Req(scores_shape=True, scores_pharmacophore=True, min_shape_tanimoto=0.55)
    assert postprocess.select(_rows(shape, pharm), plain, none, none) == [0, 1, 2, 3]
    combo = Req(scores_shape=True, scores_pharmacophore=True, rank_by="combo", min_shape_tanimoto=0.45, top_k=2)
    assert postprocess.select(_rows([0.9, nan, 0.7, 0.6, 0.5, 0.4], pharm), combo, none, none) == [4, 0]
    # the diversity walk runs in the combined order
    pair = [[1, .9, 0, 0, 0, 0], [.9, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, .9],
            [0, 0, 0, 0, .9, 1]]
    combo = Req(scores_shape=True, scores_pharmacophore=True, rank_by="combo", max_pairwise_tanimoto=0.5, overlay=True)
    assert postprocess.select(_rows(shape, pharm), combo, lambda rows: pair, none) == [4, 1, 2, 3]
    shape_first = Req(scores_shape=True, scores_pharmacophore=True, max_pairwise_tanimoto=0.5, overlay=True)
    assert postprocess.select(_rows(shape, pharm), shape_first, lambda rows: pair, none) == [0, 2, 3, 4]
    assert PH.select_score(0.5, 0.25) == 0.75 and math.isnan(PH.select_score(0.5, None)) and \
        math.isnan(PH.select_score(None, 0.5)) and math.isnan(PH.select_score(nan, 0.5))


# ----------------------------------------------------------------------------------------------- seams = restatement
def _seam_perceive(calls):
    def run(z, bonds, n):
        z, bonds, n = torch.as_tensor(z), torch.as_tensor(bonds), torch.as_tensor(n).reshape(-1).tolist()
        calls.append(("perceive", len(n)))
        types = torch.zeros(len(n), bonds.shape[1], dtype=torch.uint8)
        masks = torch.zeros(len(n), 32, dtype=torch.int64)
        for b, k in enumerate(n):
            t, rings, _ = R.perceive(z[b, :k].tolist(), bonds[b, :k, :k].tolist(), k)
            types[b, :k] = torch.tensor(t, dtype=torch.uint8)
            masks[b, : len(rings)] = torch.tensor(rings, dtype=torch.int64)
        return types, masks, torch.tensor([int((m != 0).sum()) for m in masks], dtype=torch.int32)
    return run


def _seam_score(calls):
    def run(feats, coords, n, types, masks, count):
        xyz, typ = PH.load_reference_features(feats)
        fr = [(int(t), p.numpy()) for t, p in zip(typ, xyz)]
        calls.append(("score", len(fr), int(coords.shape[0])))
        sim, hits = [], []
        for b, k in enumerate(torch.as_tensor(n).reshape(-1).tolist()):
            fm = R.features(coords[b, :k].numpy(), types[b, :k].tolist(), masks[b, : int(count[b])].tolist())
            sim.append(R.tanimoto(fr, fm) if fm else 0.0)
            hits.append(R.matches(fr, fm))
        return torch.tensor(sim, dtype=torch.float32), torch.tensor(hits, dtype=torch.int32)
    return run


SHARD = ["ethanol", "acetic acid", "aniline", "pyridine", "trimethylamine", "indole", "imidazole", "chlorobenzene"]


def _shard_coords(sid, k):
    g = torch.Generator().manual_seed(40 + sid)
    return torch.randn(k, 3, generator=g) * 1.2


def _graph_shard(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
    ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
    el = torch.full((n_samples, 42), 9, dtype=torch.int8)                         # junk beyond the atoms
    bond = torch.full((n_samples, 42, 42), 3, dtype=torch.int8)
    x = torch.zeros(n_samples, 12, 3)
    n = torch.zeros(n_samples, dtype=torch.int32)
    for b, sid in enumerate(ids):
        z, adj, k = C.PINNED[SHARD[sid]][0]
        el[b, :k] = torch.tensor(z, dtype=torch.int8)
        bond[b, :k, :k] = torch.tensor(adj, dtype=torch.int8)
        n[b] = k
        x[b, :k] = _shard_coords(sid, k)
        if sid == 6:
            x[b, 0, 0] = float("nan")                                             # its pose fails
    valid = torch.tensor([0 if sid == 4 else 1 for sid in ids], dtype=torch.uint8)
    return dict(x=x, elements=el, bond=bond, n_nodes=n, valid=valid)


def _want(feats, coords, name):
    types, rings, _ = R.perceive(*C.PINNED[name][0])
    fm = R.features(np.asarray(coords, dtype=np.float32), types, rings)
    fr = [(R.TYPE_NAMES.index(k), np.array(p, dtype=np.float32)) for k, p in feats]
    return np.float32(R.tanimoto(fr, fm)), R.matches(fr, fm)


REF_FEATS = [("donor", (0.2, 0.1, 0.0)), ("acceptor", (0.5, -0.4, 0.3)), ("ring", (0.0, 0.6, -0.2)),
             ("hydrophobe", (-0.8, 0.0, 0.4)), ("cation", (0.1, 0.1, 0.9)), ("anion", (0.9, 0.2, -0.5))]


def test_record_path_carries_the_scores_and_passes_the_filter():
    calls = []
    gen = _shell_generator()
    gen._pharm_perceive, gen._pharm_score = _seam_perceive(calls), _seam_score(calls)
    gen._generate_shard = _graph_shard
    gen._pose = _stub_overlay(lambda k: k * 0.0 + 0.5)
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    kw = dict(reference_conformer=_ref(), n_samples=8, overlay=True)

    plain = gen.generate_conformers(**kw)
    assert calls == [] and [m.sample_id for m in plain] == [0, 1, 2, 3, 5, 6, 7]             # 4: invalid
    assert all(m.pharmacophore_tanimoto is None and m.pharmacophore_matches is None for m in plain)
    got = gen.generate_conformers(pharmacophore_scores=True, reference_pharmacophore=REF_FEATS, **kw)
    assert calls == [("perceive", 8), ("score", 6, 8)]          # one launch each over the rows: the reference is given
    assert [m.sample_id for m in got] == [0, 1, 2, 3, 5, 6, 7]
    for a, m in zip(plain, got):
        if m.sample_id == 6:                                     # its pose failed: not in the reference's frame
            assert m.pose is None and m.pharmacophore_tanimoto is None and m.pharmacophore_matches is None
            continue
        assert a == m
        t, hits = _want(REF_FEATS, m.coords, SHARD[m.sample_id])
        assert np.float32(m.pharmacophore_tanimoto) == t and m.pharmacophore_matches == hits
    assert len({m.pharmacophore_tanimoto for m in got}) > 4

    # the reference's features perceived from its graph at the conformer's atoms: one more perceive launch, first
    del calls[:]
    graph = C.PINNED["aniline"][0][:2]
    own = gen.generate_conformers(pharmacophore_scores=True, reference_graph=graph, **dict(kw, reference_conformer=_ref(7)))
    assert calls == [("perceive", 1), ("perceive", 8), ("score", 2, 8)]                      # aniline: D and R
    types, rings, _ = R.perceive(*C.PINNED["aniline"][0])
    fr = [(R.TYPE_NAMES[t], tuple(p.tolist())) for t, p in R.features(_ref(7).numpy(), types, rings)]
    for m in own:
        if m.sample_id != 6:
            assert np.float32(m.pharmacophore_tanimoto) == _want(fr, m.coords, SHARD[m.sample_id])[0]
    with pytest.raises(ValueError, match="no pharmacophore features"):       # a reference in which nothing is perceived
        gen.generate_conformers(pharmacophore_scores=True, reference_graph=([9, 9, 9], [[0, 1, 0], [1, 0, 1], [0, 1, 0]]),
                                reference_conformer=_ref(3), n_samples=8, overlay=True)

    def ids(**more):
        return [m.sample_id for m in gen.generate_conformers(**dict(kw, reference_pharmacophore=REF_FEATS, **more))]
    by_id = {m.sample_id: m for m in got}
    scores = sorted(m.pharmacophore_tanimoto for m in got if m.pharmacophore_tanimoto is not None)
    t = float(scores[3])
    assert ids(min_pharmacophore_tanimoto=t) == [i for i in (0, 1, 2, 3, 5, 7) if by_id[i].pharmacophore_tanimoto >= t]
    assert ids(min_pharmacophore_tanimoto=0.0) == [0, 1, 2, 3, 5, 7]                          # the failed pose never passes
    shaped = {m.sample_id: m.shape_tanimoto for m in gen.generate_conformers(shape_scores=True, **kw)}
    combo = sorted((i for i in by_id if i != 6), key=lambda i: (-(shaped[i] + by_id[i].pharmacophore_tanimoto), i))
    assert ids(pharmacophore_scores=True, rank_by="combo", top_k=3) == combo[:3]
    assert [m.sample_id for m in gen.generate_conformers_sharded(
        pharmacophore_scores=True, reference_pharmacophore=REF_FEATS, rank_by="combo", top_k=3, **kw)] == combo[:3]
    assert [m.pharmacophore_matches for m in gen.forward(pharmacophore_scores=True, reference_pharmacophore=REF_FEATS,
                                                         **kw)] == [m.pharmacophore_matches for m in got]
    assert isinstance(got[0], GeneratedMolecule)


class _MolStage:
    """`_generate_shard` for the object path: finished stand-in Mols (with hydrogens) of the shard molecules at the shard
    coordinates; sample 4 is dropped by the finish, sample 6's pose fails."""
    def __init__(self, gen):
        self.gen = gen

    def __call__(self, ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
        mols = []
        for sid in ids:
            z, adj, k = C.PINNED[SHARD[sid]][0]
            h = sid % 3
            m = _as_mol((z, adj, k), hydrogens=h)
            pos = np.concatenate([_shard_coords(sid, k).double().numpy(), np.full((h, 3), 7.0)])
            if sid == 6:
                pos[0, 0] = np.nan
            m.conf.pos = pos
            mols.append(None if sid == 4 else m)
        self.gen._finish_stage = _Stage(mols)
        return dict(x=torch.zeros(n_samples, 5, 3))


def test_object_path_mols_carry_the_properties_and_pass_the_filter():
    calls = []
    gen = _shell_generator(finisher="rdkit")
    gen._pharm_perceive, gen._pharm_score = _seam_perceive(calls), _seam_score(calls)
    gen._generate_shard = _MolStage(gen)
    gen._pose = _stub_overlay(lambda k: k * 0.0 + 0.5)
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    kw = dict(reference_conformer=_ref(), n_samples=8, sample_seed=5, overlay=True)
    plain = gen.generate_conformers(**kw)
    assert calls == [] and [m.props["sample_id"] for m in plain] == [0, 1, 2, 3, 5, 6, 7]
    assert all("pharmacophore_tanimoto" not in m.props and "pharmacophore_matches" not in m.props for m in plain)
    got = gen.generate_conformers(pharmacophore_scores=True, reference_pharmacophore=REF_FEATS, **kw)
    assert calls == [("perceive", 6), ("score", 6, 6)]           # the live, posed Mols in ONE batched call each
    assert [m.props["sample_id"] for m in got] == [0, 1, 2, 3, 5, 6, 7]
    for m in got:
        sid = m.props["sample_id"]
        if sid == 6:
            assert "pharmacophore_tanimoto" not in m.props and "pharmacophore_matches" not in m.props
            continue
        heavy = np.array([p for p, z in zip(m.conf.pos, m.z) if z != 1], dtype=np.float32)
        t, hits = _want(REF_FEATS, heavy, SHARD[sid])
        assert np.float32(m.props["pharmacophore_tanimoto"]) == t and m.props["pharmacophore_matches"] == hits
        assert isinstance(m.props["pharmacophore_matches"], int)
    by_id = {m.props["sample_id"]: m.props.get("pharmacophore_tanimoto") for m in got}
    t = sorted(v for v in by_id.values() if v is not None)[3]
    kept = gen.generate_conformers(min_pharmacophore_tanimoto=t, reference_pharmacophore=REF_FEATS, **kw)
    assert [m.props["sample_id"] for m in kept] == [i for i in (0, 1, 2, 3, 5, 7) if by_id[i] >= t]
    combo = gen.generate_conformers_sharded(pharmacophore_scores=True, reference_pharmacophore=REF_FEATS, shape_scores=True,
                                            rank_by="combo", top_k=2, **kw)
    want = sorted((m for m in combo), key=lambda m: -(m.props["shape_tanimoto"] + m.props["pharmacophore_tanimoto"]))
    assert len(combo) == 2 and [m.props["sample_id"] for m in combo] == [m.props["sample_id"] for m in want]
    graph = BondedMol(*_aniline_with_bonds())
    own = gen.generate_conformers(pharmacophore_scores=True, reference_graph=graph, **dict(kw, reference_conformer=_ref(7)))
    assert all(("pharmacophore_tanimoto" in m.props) == (m.props["sample_id"] != 6) for m in own)


def _aniline_with_bonds():
    z, adj, n = C.PINNED["aniline"][0]
    order = {1: 1.0, 2: 2.0, 3: 3.0, 4: 1.5}
    return list(z), [(i, j, order[adj[i][j]]) for i in range(n) for j in range(i) if adj[i][j]]
