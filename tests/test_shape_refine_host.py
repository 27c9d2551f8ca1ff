"""Refined poses, host side (no GPU): every refusal of `refine_overlay` / `refine_steps` before any device work, the C
entry's argument checks, the refined seam taken only when asked on the proxy and the object path, and the fp64 CPU
restatement of the ascent reproducing the gain table of DESIGN.md section 6 ("Refined pose")."""
import ctypes

import numpy as np
import pytest
import torch

import overlay_refine_ref as RR
from conftest import load_golden
from ml_conformer_generator_amd import postprocess
from test_shape_overlay_host import PosedMol, _no_device, _ref, _rot_z, _shell_generator, _stub_overlay, _stub_shard

BAD_BUDGETS = (0, -3, 2.5, 64.0, "64", None, 1025)


# ----------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_refine_refusals_happen_before_any_device_work(entry):
    gen = _shell_generator()
    gen._generate_shard = gen._score = gen._pose = gen._pair = _no_device
    call = getattr(gen, entry)
    with pytest.raises(ValueError, match="overlay=True"):
        call(reference_conformer=_ref(), n_samples=4, refine_overlay=True)
    with pytest.raises(ValueError, match="overlay=True"):
        call(reference_conformer=_ref(), n_samples=4, shape_scores=True, refine_overlay=8)
    for bad in BAD_BUDGETS:
        with pytest.raises(ValueError, match="refine_overlay"):
            call(reference_conformer=_ref(), n_samples=4, overlay=True, refine_overlay=bad)


def test_shape_overlay_refuses_bad_step_counts_before_any_device_work(monkeypatch):
    from ml_conformer_generator_amd import cheminformatics as CH
    monkeypatch.setattr(CH, "_shape_inputs", _no_device)
    x, n = torch.zeros(2, 5, 3), torch.tensor([5, 5])
    for bad in (True, False, -1, 1025, 2.0, "8", None):
        with pytest.raises(ValueError, match="refine_steps"):
            CH.shape_overlay(_ref(), x, n, refine_steps=bad)
    assert CH.check_refine_steps(0) == 0 and CH.check_refine_steps(np.int64(1024)) == 1024


def test_an_empty_batch_returns_every_key_of_the_call():
    from ml_conformer_generator_amd import cheminformatics as CH
    per_row = dict(coords=((20, 3), torch.float32), rotation=((3, 3), torch.float32), translation=((3,), torch.float32),
                   tanimoto=((), torch.float32), orientation=((), torch.long), flipped=((), torch.bool),
                   scores=((4,), torch.float32), start_tanimoto=((), torch.float32), refined=((), torch.bool),
                   refined_scores=((4,), torch.float32), objective=((4, 2), torch.float32))
    plain = ["coords", "rotation", "translation", "tanimoto", "orientation", "flipped"]
    for with_scores in (False, True):
        for refined_entry in (False, True):
            want = plain + (["scores"] if with_scores else []) + (["start_tanimoto", "refined"] if refined_entry else []) \
                + (["refined_scores", "objective"] if with_scores and refined_entry else [])
            out = CH._overlay(_ref(), torch.zeros(0, 20, 3), torch.zeros(0, dtype=torch.int32), "cpu", with_scores, 5,
                              refined_entry)
            assert list(out) == want
            for key, t in out.items():
                assert t.shape == (0,) + per_row[key][0] and t.dtype == per_row[key][1], key


def test_the_request_carries_the_step_budget():
    gen = _shell_generator()
    gen._reference_coord = lambda r: torch.as_tensor(r, dtype=torch.float32)
    req = postprocess.parse_request(gen, _ref(), shape_scores=False, top_k=None, min_shape_tanimoto=None, overlay=True)
    assert req.refine_steps == 0
    assert postprocess.parse_request(gen, _ref(), shape_scores=False, top_k=None, min_shape_tanimoto=None, overlay=True,
                                     max_pairwise_tanimoto=None, refine_overlay=True).refine_steps == 64
    assert postprocess.parse_request(gen, _ref(), shape_scores=False, top_k=None, min_shape_tanimoto=None, overlay=True,
                                     max_pairwise_tanimoto=None, refine_overlay=np.int32(5)).refine_steps == 5
    assert postprocess.parse_request(gen, _ref(), shape_scores=False, top_k=None, min_shape_tanimoto=None, overlay=True,
                                     max_pairwise_tanimoto=None, refine_overlay=1024).refine_steps == 1024


# ----------------------------------------------------------------------------------------------- C entry
def test_refined_entry_refuses_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check
    ok = dict(ref=p, n_ref=17, ref_xf=p, frames=p, xf=p, nn=p, B=3, N=27, rot=p, axes=p, n=40, alpha=0.8, f=p, score=None,
              best=p, which=p, flipped=p, pose=p, posed=p, steps=64, ws=p, obj=None, start=p, refined=p, rscore=None)

    def refined(**kw):
        a = dict(ok, **kw)
        return h.mcg_shape_overlay_refined(a["ref"], a["n_ref"], a["ref_xf"], a["frames"], a["xf"], a["nn"], a["B"],
                                           a["N"], a["rot"], a["axes"], a["n"], a["alpha"], 2.7, a["f"], a["score"],
                                           a["best"], a["which"], a["flipped"], a["pose"], a["posed"], a["steps"], a["ws"],
                                           a["obj"], a["start"], a["refined"], a["rscore"], None)

    for bad in (dict(ref=None), dict(ref_xf=None), dict(frames=None), dict(xf=None), dict(nn=None), dict(rot=None),
                dict(axes=None), dict(f=None), dict(best=None), dict(which=None), dict(flipped=None), dict(pose=None),
                dict(posed=None), dict(ws=None), dict(start=None), dict(refined=None), dict(B=0), dict(N=0), dict(N=65),
                dict(n_ref=2), dict(n_ref=65), dict(n=1), dict(steps=-1), dict(steps=1025), dict(alpha=0.0)):
        assert refined(**bad) == 1, bad
        assert b"mcg_shape_overlay_refined" in h.mcg_last_error(), bad
    assert "mcg_shape_overlay_refined" in _lib.SIGNATURES


# ----------------------------------------------------------------------------------------------- seams
def _pose_stub(calls):
    """A device-free `_pose` that records the step budget it received: the overlay stub, and where the budget is not 0 - a
    refined pose - one with a different translation (k + 2) and score."""
    plain, refined = _stub_overlay(lambda k: k + 1.0), _stub_overlay(lambda k: k + 2.0)

    def run(ref, coords, n, refine_steps=0):
        calls.append(int(refine_steps))
        return (refined if refine_steps else plain)(ref, coords, n)
    return run


def test_proxy_path_takes_the_refined_seam_only_when_asked():
    gen = _shell_generator()
    gen._generate_shard = _stub_shard()
    calls = []
    gen._pose = _pose_stub(calls)
    plain = gen.generate_conformers(reference_conformer=_ref(), n_samples=8)
    posed = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True)
    assert calls == [0]
    calls.clear()
    refined = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True, refine_overlay=True)
    assert calls == [64]
    calls.clear()
    gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True, refine_overlay=7)
    assert calls == [7]
    assert [m.sample_id for m in refined] == [m.sample_id for m in posed] == [m.sample_id for m in plain]
    for a, b in zip(plain, refined):
        if b.sample_id == 5:                          # failed: generated coordinates, no pose, NaN score
            assert b.pose is None and b.overlay_tanimoto != b.overlay_tanimoto
            continue
        R, t = b.pose
        assert torch.allclose(b.coords, a.coords @ R + t, atol=1e-6)
        assert float(t[0]) == pytest.approx(float(a.coords[0, 0]) + 2.0)        # the refined seam's pose
        assert b.overlay_tanimoto == pytest.approx(float(a.coords[0, 0]) + 2.0)


def test_object_path_takes_the_refined_seam_only_when_asked():
    gen = _shell_generator(finisher="rdkit")
    gen._reference_coord = lambda r: torch.as_tensor(r, dtype=torch.float32)
    calls = []
    gen._pose = _pose_stub(calls)
    gen._score = _no_device

    def mols():
        return [PosedMol([[0.5, 0, 0]] * 4 + [[0, 0, 1.0]], z=[6] * 4 + [1]), None]
    for refine, want_call, shift in ((False, 0, 1.5), (True, 64, 2.5), (3, 3, 2.5)):
        calls.clear()
        req = postprocess.parse_request(gen, _ref(), shape_scores=False, top_k=None, min_shape_tanimoto=None, overlay=True,
                                        max_pairwise_tanimoto=None, refine_overlay=refine)
        done = mols()
        samples = postprocess.measure_finished(gen, req, done)
        scores = [s.measured.shape_tanimoto for s in samples]
        assert calls == [want_call] and scores == [None, None]
        assert samples[1].measured.overlay_tanimoto is None and samples[1].measured.pose is None
        score, pose = samples[0].measured.overlay_tanimoto, samples[0].measured.pose
        rot, trans = pose[:9].reshape(3, 3), pose[9:]
        assert score == pytest.approx(shift) and torch.allclose(rot, _rot_z(90.0)) and trans.tolist() == [shift, 0, 0]
        np.testing.assert_allclose(done[0].conf.pos, [[shift, 0.5, 0.0]] * 4 + [[shift, 0.0, 1.0]], atol=1e-6)


# ----------------------------------------------------------------------------------------------- CPU restatement
def test_the_cpu_restatement_reproduces_the_gain_table():
    g = load_golden("shape_quadrupole.npz")
    rows = {(p[0], p[1]): RR.refined_pose_scores(p[2], p[3]) for p in RR.table_pairs(g)}
    assert len(rows) == 15
    start = sum(v[0] for v in rows.values()) / len(rows)
    refined = sum(v[1] for v in rows.values()) / len(rows)
    assert start == pytest.approx(0.401, abs=2e-3) and refined == pytest.approx(0.478, abs=2e-3)
    assert rows[("ceyyag", "walk27")] == pytest.approx((0.365, 0.670), abs=2e-3)
    assert rows[("ceyyag", "yibfeu")] == pytest.approx((0.422, 0.518), abs=2e-3)
    assert all(v[1] >= v[0] for v in rows.values())


def test_the_restated_ascent_never_lowers_the_objective_and_stays_rigid():
    g = load_golden("shape_quadrupole.npz")
    y, zs = RR.starts(g["xyz_ceyyag"], g["xyz_walk27"])
    for z in zs:
        G, t, before, after = RR.refine(y, z, 32)
        assert after >= before
        assert before == pytest.approx(RR.overlap(y, z), rel=1e-12)
        assert float((G @ G.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
        assert float(torch.det(G)) == pytest.approx(1.0, abs=1e-12)
        assert RR.overlap(y, z.double() @ G + t) == pytest.approx(after, rel=1e-9)
