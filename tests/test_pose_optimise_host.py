"""Optimised pose, host side (DESIGN.md section 6 "Optimised pose"): the restatement's forces against central differences
of its own W, hand pairs, the pass rules against the restatement rounded to fp32 and against planted mistakes, the option's
refusals and its place in the stage order against stub seams, and the C entry's argument checks.  No GPU."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import interactions_ref as IR
import pose_optimise_ref as P
from conftest import REPO
from ml_conformer_generator_amd import interactions as IX
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd.handoff import Measured, measured_from_tensors
from test_interactions_host import _graph_shard, _receptor, _record_receptor, _seam_interactions
from test_shape_overlay_host import _no_device, _ref, _shell_generator, _stub_overlay

F32 = np.float32
CASES = P.cases()
SMOOTH = P.smooth_cases()


def _args(c):
    return IR.radii(c.z), c.t, c.rec, IR.radii(c.rec_z), c.rec_t


# ----------------------------------------------------------------------------------------------- forces = -grad W
def _clear_of_kinks(c, h):
    """Every pair of the case, at the pose and at every pose a central difference of step h reaches, at least 1e-3 A
    from each kink of the terms and from the cut-off."""
    x = c.x.astype(np.float64)
    diff = x[:, None, :] - c.rec.astype(np.float64)[None, :, :]
    r = np.sqrt((diff ** 2).sum(axis=2))
    d = r - (IR.radii(c.z).astype(np.float64)[:, None] + IR.radii(c.rec_z).astype(np.float64)[None, :])
    gap = min(float(np.abs(d - k).min()) for k in P.KINKS)
    return min(gap, float(np.abs(r - 8.0).min())) - h >= 1e-3


@pytest.mark.parametrize("case", SMOOTH, ids=lambda c: c.name)
def test_forces_are_minus_the_gradient_of_the_restatements_own_w(case):
    c, h = case, 1e-5
    assert _clear_of_kinks(c, h), "the seeded case must keep every pair 1e-3 A from each kink and from the cut-off"
    ri, ti, y, rj, tj = _args(c)
    x = c.x.astype(np.float64)
    lever = x - x.mean(axis=0)
    got = P.evaluate(x, lever, ri, ti, y, rj, tj, smooth=True)
    W = lambda xx: P.evaluate(xx, lever, ri, ti, y, rj, tj, smooth=True)["weighted"]      # noqa: E731
    scale = max(1e-3, float(np.abs(got["atom_forces"]).max()))
    for i in range(c.n):
        for k in range(3):
            e = np.zeros_like(x)
            e[i, k] = h
            numeric = -(W(x + e) - W(x - e)) / (2 * h)
            assert abs(numeric - got["atom_forces"][i, k]) <= 1e-6 * scale + 1e-9, (c.name, i, k)
    # the torque is the derivative along a rotation about the point the levers are seen from
    centre = x.mean(axis=0)
    for k in range(3):
        n = np.zeros(3)
        n[k] = 1.0
        turn = lambda a: centre + lever + a * np.cross(n, lever)                           # noqa: E731 (first order)
        numeric = -(W(turn(h)) - W(turn(-h))) / (2 * h)
        assert abs(numeric - got["torque"][k]) <= 1e-5 * max(1e-3, float(np.abs(got["torque"]).max())) + 1e-8, (c.name, k)
    assert np.allclose(got["force"], got["atom_forces"].sum(axis=0))


def _pair(z_i, t_i, z_j, t_j, d):
    """One ligand atom at the origin and one receptor atom on +x at surface distance d."""
    r = IR.radius(z_i) + IR.radius(z_j) + d
    out = P.evaluate(np.zeros((1, 3), F32), np.zeros((1, 3)), IR.radii([z_i]), [t_i], np.array([[r, 0, 0]], F32),
                     IR.radii([z_j]), [t_j])
    return out, float(out["d"][0, 0])


def test_hand_pairs():
    w = IR.DEFINITION.w
    # C...C at surface distance 0: g1' = 0 there and g2 alone acts: g2 grows towards d = 3 and its weight is negative, so
    # W falls as d grows - attractive towards the g2 optimum at d = 3, i.e. the ligand atom is drawn away from contact
    out, d = _pair(6, 0, 6, 0, 0.0)
    assert abs(d) < 1e-6
    g2_slope = -((d - 3) / 2) * math.exp(-((d - 3) / 2) ** 2)
    assert out["force"][0] == pytest.approx(w["g2"] * g2_slope + w["g1"] * (-8 * d * math.exp(-4 * d * d)), abs=1e-9)
    assert out["force"][0] == pytest.approx(w["g2"] * 1.5 * math.exp(-2.25), rel=1e-4)    # g1 adds nothing at d = 0
    assert out["force"][0] < 0 and out["force"][1] == out["force"][2] == 0                # away from the partner: d grows
    assert not out["torque"].any()
    # donor facing acceptor at d = -0.35: the hb slope -1 / 0.7 joins, and pulls the atoms together against the repulsion
    both, d = _pair(7, IR.DONOR, 8, IR.ACCEPTOR, -0.35)
    bare, _ = _pair(7, 0, 8, 0, -0.35)
    assert both["force"][0] - bare["force"][0] == pytest.approx(w["hb"] * (-1 / float(F32(0.7))), rel=1e-6)
    assert both["force"][0] - bare["force"][0] > 0                                        # towards the partner
    assert both["terms"][4] == pytest.approx(0.5, abs=1e-5)
    # at d < 0 without a hydrogen bond the repulsion wins: the force pushes the ligand atom away, -x
    out, d = _pair(6, 0, 6, 0, -0.5)
    assert out["force"][0] < 0 and abs(w["rep"] * 2 * d) > abs(w["g1"] * -8 * d * math.exp(-4 * d * d))
    # both hydrophobic on the ramp: slope -1
    hyd, _ = _pair(6, IR.HYDROPHOBIC, 6, IR.HYDROPHOBIC, 1.0)
    bare, _ = _pair(6, 0, 6, 0, 1.0)
    assert hyd["force"][0] - bare["force"][0] == pytest.approx(w["hyd"] * -1.0, rel=1e-9)
    # coincident centres: direction 0
    r0 = P.evaluate(np.zeros((1, 3), F32), np.zeros((1, 3)), IR.radii([6]), [0], np.zeros((1, 3), F32), IR.radii([6]), [0])
    assert not r0["force"].any() and r0["terms"][2] > 0


# ----------------------------------------------------------------------------------------------- the rules
def _walked(c, walk=P.WALK, steps=24, max_shift=2.0):
    return P.run_walk(c.x, *_args(c), steps, max_shift, walk=walk)


def _violations(c, run, steps=24, max_shift=2.0):
    stats = np.array([run["w_before"], run["w_after"], run["trials"], run["kept"], run["rmsd"], run["st"], 0, 0], F32)
    return P.check_trace(run["trace"].astype(F32), c.x, *_args(c), steps, max_shift, stats=stats, coords=run["coords"])[0]


@pytest.mark.parametrize("case", [c for c in CASES if c.name in ("n2d", "n27d", "R257d")], ids=lambda c: c.name)
def test_rule_passes_the_restatement_rounded_to_fp32(case):
    run = _walked(case)
    assert run["kept"] > 0 and run["w_after"] < run["w_before"]
    assert _violations(case, run) == []
    # the fp64 walk descends too; the two may stop in different places
    slow = P.run_walk(case.x, *_args(case), 24, 2.0, state=np.float64)
    assert slow["w_after"] < slow["w_before"]
    # the shift rejection at work: with no room to move every translating trial is rejected unevaluated
    tight = _walked(case, max_shift=0.0)
    assert tight["kept"] == 0 and not tight["trace"][: tight["trials"], 21].any() and tight["trials"] > 0
    assert _violations(case, tight, max_shift=0.0) == []
    assert np.array_equal(tight["coords"], case.x)


MISTAKES = [("the sign of the torque", dict(torque_sign=-1.0)),
            ("a growth factor of 1.1", dict(grow=F32(1.1))),
            ("the torque taken about c instead of p", dict(torque_about="c")),
            ("g2' with the factor 2 missing", dict(g2_factor=1.0))]


@pytest.mark.parametrize("what, change", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_rule_fails_a_planted_mistake(what, change):
    c = next(c for c in CASES if c.name == "n27d")
    run = _walked(c, walk=P.Walk(**change))
    assert _violations(c, run) != [], what


def test_rule_fails_a_trial_without_orthonormalisation():
    g = np.random.default_rng(5)
    G = P.gram_schmidt(g.normal(size=(3, 3)))
    G[0] *= 1 + 1e-4                                  # what drift looks like once it is visible
    G[1] += 2e-4 * G[0]
    G = G.astype(F32)
    F, tau, p = g.normal(size=3).astype(F32), g.normal(size=3).astype(F32), (g.normal(size=3) * 5).astype(F32)
    sr, st = F32(0.05), F32(0.25)
    right = P.trial(F, tau, sr, st, G, p)
    wrong = P.trial(F, tau, sr, st, G, p, P.Walk(orthonormalise=False))
    assert P.trial_passes(right[0].astype(F32), right[1].astype(F32), F, tau, sr, st, G, p)
    assert not P.trial_passes(wrong[0].astype(F32), wrong[1].astype(F32), F, tau, sr, st, G, p)
    assert np.abs(right[0] @ right[0].T - np.eye(3)).max() < 1e-12 and np.linalg.det(right[0]) > 0
    # a skipped part of the move is exact: no torque leaves G as it is, no force leaves p
    still = P.trial(F, np.zeros(3, F32), sr, st, G, p)
    assert np.array_equal(still[0], G.astype(np.float64)) and not still[2] and still[3]
    nowhere = P.trial(np.array([np.nan, 0, 0], F32), tau, sr, st, G, p)
    assert np.array_equal(nowhere[1], p.astype(np.float64)) and nowhere[2] and not nowhere[3]


def test_rule_fails_a_non_strict_keep():
    c = next(c for c in CASES if c.name == "n27d")
    run = _walked(c)
    trace = run["trace"].astype(F32)
    rows = [k for k in range(run["trials"]) if trace[k, 21] == 1 and trace[k, 22] == 0]
    assert rows, "the walk has an evaluated trial that was rejected"
    k = rows[0]
    trace[k, 20], trace[k, 22] = trace[k, 23], 1.0    # W' == W kept: what `<=` in place of `<` does on a plateau
    bad = P.check_trace(trace, c.x, *_args(c), 24, 2.0)[0]
    assert any(f"row {k}: kept" in v for v in bad)
    # and the mutant itself keeps an equal W where the definition does not
    flat = IR.Case("flat", 77, 3, far=True)           # no counted pair: W = 0 everywhere, no force - the walk ends at once
    assert P.run_walk(flat.x, *_args(flat), 8, 2.0, walk=P.Walk(strict=False))["trials"] == 0


def test_step_lengths_and_the_end_of_the_walk():
    c = next(c for c in CASES if c.name == "n27d")
    run = P.run_walk(c.x, *_args(c), 200, 2.0)
    tr = run["trace"]
    assert run["trials"] < 200 and run["st"] < 2.0 ** -8          # ended by the step length, not by the budget
    assert tr[0, 6] == float(F32(0.05)) and tr[0, 7] == float(F32(0.25))
    for k in range(1, run["trials"]):
        f = F32(1.2) if tr[k - 1, 22] else F32(0.5)
        assert F32(tr[k, 7]) == F32(F32(tr[k - 1, 7]) * f) and F32(tr[k, 6]) == F32(F32(tr[k - 1, 6]) * f)
    assert not tr[run["trials"]:].any()
    shifts = np.linalg.norm(tr[: run["trials"], 17:20][tr[: run["trials"], 22] == 1] - run["c"], axis=1)
    assert (shifts <= 2.0 + 1e-5).all()
    assert P.run_walk(c.x, *_args(c), 0, 2.0)["trials"] == 0


# ----------------------------------------------------------------------------------------------- the option
def test_parse_request_implications_and_defaults():
    gen = _shell_generator()
    parse = postprocess.parse_request
    assert parse(gen, _ref(), optimise_pose=False) == postprocess.Request()
    rec = _receptor()
    assert parse(gen, _ref(), overlay=True, receptor=rec, interaction_scores=True).optimise_steps == 0
    req = parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose=True)
    assert req.optimise_steps == IX.OPTIMISE_STEPS == 64 and req.scores_interactions and not req.removes
    assert isinstance(req.typed_receptor, IX.PreparedReceptor)
    assert parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose=1).optimise_steps == 1
    assert parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose=1024, rank_by="interaction",
                 top_k=2).optimise_steps == 1024
    assert IX.check_max_shift(0) == 0.0 and IX.check_max_shift(2.5) == 2.5
    for bad in (-1.0, float("nan"), float("inf"), True, "2"):
        with pytest.raises(ValueError):
            IX.check_max_shift(bad)


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_option_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._optimise_pose = gen._interaction_scores = gen._receptor_coords = gen._score = gen._pose = _no_device
    gen._score_placed = gen._relieve = _no_device
    call = getattr(gen, entry)
    rec = _receptor()
    cases = [dict(optimise_pose=True),                                                        # no receptor
             dict(overlay=True, optimise_pose=True),
             dict(optimise_pose=True, receptor=rec)]                                          # no overlay
    for bad in (0, -1, 1025, 2.0, "yes", None, [8]):
        cases.append(dict(overlay=True, receptor=rec, optimise_pose=bad))
    for kw in cases:
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    with pytest.raises(ValueError, match=r"optimise_pose must be True or an integer step budget in 1\.\.1024"):
        call(reference_conformer=_ref(), n_samples=4, overlay=True, receptor=rec, optimise_pose=0)
    with pytest.raises(ValueError, match="optimise_pose needs a receptor"):
        call(reference_conformer=_ref(), n_samples=4, overlay=True, optimise_pose=True)
    for finisher in ("rdkit", HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                                         "finish_tag_chunk")):
        gen.finisher = finisher
        with pytest.raises(ValueError, match="optimise_pose cannot be combined with a finisher"):
            call(reference_conformer=_ref(), n_samples=4, overlay=True, receptor=rec, optimise_pose=True)


MOVE = torch.tensor([0.25, 0.0, 0.0])


def _seam_optimise(calls):
    """A device-free stand-in for `interactions.optimise_pose`: rows at an even batch row move by (0.25, 0, 0) and keep 3
    trials; a row with a non-finite coordinate gets what the kernel gives it."""
    def run(prepared, coords, n_nodes, atomic_numbers, bond_orders, steps):
        assert isinstance(prepared, IX.PreparedReceptor)
        B, N = int(coords.shape[0]), int(coords.shape[1])
        calls.append(("optimise", B, steps))
        real = (torch.arange(N).view(1, N) < torch.as_tensor(n_nodes).view(B, 1)).unsqueeze(2)
        good = torch.tensor([bool(torch.isfinite(coords[b, : int(n_nodes[b])]).all()) for b in range(B)])
        moved = good & (torch.arange(B) % 2 == 0)
        out = torch.where(real, torch.where(moved.view(B, 1, 1), coords + MOVE, coords), torch.zeros(()))
        t = torch.zeros(B, 3)
        t[moved] = MOVE
        nan = torch.full((B,), float("nan"))
        before = -1.0 - 0.125 * torch.arange(B, dtype=torch.float32)
        return dict(coords=out, rotation=torch.eye(3).expand(B, 3, 3).clone(), translation=t, moved=moved,
                    weighted_before=torch.where(good, before, nan), weighted_after=torch.where(good, before - moved.float(), nan),
                    trials=torch.where(good, torch.full((B,), steps), torch.full((B,), -1)).int(),
                    kept=torch.where(good, 3 * moved.int(), torch.full((B,), -1, dtype=torch.int32)).int(),
                    rmsd=torch.where(good, 0.25 * moved.float(), nan), gradient=torch.zeros(B, 6))
    return run


def test_record_path_carries_the_values_in_its_place_and_launches_nothing_unasked():
    calls = []
    gen = _shell_generator()
    gen._generate_shard = _graph_shard
    pose = _stub_overlay(lambda k: k * 0.0 + 0.5)

    def named(name, fn):
        def run(*a, **k):
            calls.append((name,))
            return fn(*a, **k)
        return run
    gen._pose = named("pose", pose)
    gen._score = named("score", lambda ref, coords, n: coords[:, 0, 1].clone())
    gen._receptor_coords = named("contacts", lambda rec, coords, n, z: torch.full(tuple(coords.shape[:2]), -1.0))
    gen._interaction_scores = named("interactions", _seam_interactions([]))
    gen._score_placed = named("placed", lambda ref, coords, n: torch.full((coords.shape[0],), 0.75))
    gen._optimise_pose = _no_device
    rec = _record_receptor()
    kw = dict(reference_conformer=_ref(), n_samples=8, overlay=True, receptor=rec, optimise_geometry=False,
              interaction_scores=True, shape_scores=True)
    new = ("interaction_score_before", "pose_optimisation_rmsd", "pose_trials_kept")

    plain = gen.generate_conformers(**kw)                                          # the option off: the seam is not touched
    assert all(getattr(m, f) is None for m in plain for f in new)
    off = gen.generate_conformers(optimise_pose=False, **kw)
    plainly = lambda v: (v.tolist() if torch.is_tensor(v) else                     # noqa: E731
                         [plainly(x) for x in v] if isinstance(v, (list, tuple)) else v)
    flat = lambda m: {k: plainly(getattr(m, k)) for k in vars(m._measured)}       # noqa: E731 (every value as it is read)
    keep = lambda mols: [m for m in mols if m.sample_id != 6]                     # noqa: E731 (6 holds a NaN: never equal)
    assert [flat(m) for m in keep(off)] == [flat(m) for m in keep(plain)]
    assert all(torch.equal(a.coords, b.coords) for a, b in zip(keep(off), keep(plain)))

    gen._optimise_pose = _seam_optimise(calls)
    del calls[:]
    got = gen.generate_conformers(optimise_pose=5, **{k: v for k, v in kw.items() if k != "interaction_scores"})
    # directly behind the pose, in front of everything that reads coordinates; the option implies the score
    assert calls == [("pose",), ("optimise", 8, 5), ("placed",), ("score",), ("contacts",), ("interactions",)]
    assert [m.sample_id for m in got] == [m.sample_id for m in plain] == [0, 1, 2, 3, 5, 6, 7]
    for a, b in zip(plain, got):
        row = b.sample_id
        if row == 6:                                                               # pose failed: left alone, no values
            assert all(getattr(b, f) is None for f in new) and b.pose is None and b.interaction_score is None
            continue
        n_rot = b.interaction_terms["n_rot"]
        if row % 2 == 0:
            assert torch.equal(b.coords, a.coords + MOVE) and b.pose_trials_kept == 3
            assert b.pose_optimisation_rmsd == 0.25 and b.overlay_tanimoto == pytest.approx(0.75)
            assert torch.equal(b.pose[0], a.pose[0]) and torch.equal(b.pose[1], a.pose[1] + MOVE)
            want = F32(-1.0 - 0.125 * row) / (F32(1.0) + F32(0.0585) * F32(n_rot))
            assert F32(b.interaction_score_before) == want
            assert b.interaction_score != a.interaction_score                      # scored where it now is
        else:                                                                      # unmoved: every bit it had
            assert torch.equal(b.coords, a.coords) and b.pose_trials_kept == 0 and b.pose_optimisation_rmsd == 0.0
            assert torch.equal(b.pose[0], a.pose[0]) and torch.equal(b.pose[1], a.pose[1])
            assert b.overlay_tanimoto == a.overlay_tanimoto
            assert b.interaction_score_before == b.interaction_score == a.interaction_score
    sharded = gen.generate_conformers_sharded(optimise_pose=5, **kw)              # no process group: one rank
    assert [m.pose_trials_kept for m in sharded] == [m.pose_trials_kept for m in got]
    assert [repr(m.interaction_score_before) for m in gen.forward(optimise_pose=5, **kw)] == \
        [repr(m.interaction_score_before) for m in got]
    # with the relief in front of it
    order = []
    gen._relieve = lambda rec, coords, n, z, steps: (order.append("relieve"), dict(
        coords=coords, rotation=torch.eye(3).expand(len(coords), 3, 3).clone(), translation=torch.zeros(len(coords), 3),
        rmsd=torch.zeros(len(coords)), moved=torch.zeros(len(coords), dtype=torch.bool)))[1]
    opt = gen._optimise_pose
    gen._optimise_pose = lambda *a: (order.append("optimise"), opt(*a))[1]
    gen.generate_conformers(optimise_pose=True, relieve_clashes=True, **kw)
    assert order == ["relieve", "optimise"]


def test_measured_from_tensors_reads_the_new_spellings():
    nan = float("nan")
    rec = measured_from_tensors(dict(interaction_score_before=torch.tensor([-1.5, nan, -0.25]),
                                     pose_optimisation_rmsd=torch.tensor([0.5, nan, 0.0]),
                                     pose_trials_kept=torch.tensor([4, -1, 0], dtype=torch.int32)), 3)
    assert (rec[0].interaction_score_before, rec[0].pose_optimisation_rmsd, rec[0].pose_trials_kept) == (-1.5, 0.5, 4)
    assert (rec[1].interaction_score_before, rec[1].pose_optimisation_rmsd, rec[1].pose_trials_kept) == (None, None, None)
    assert (rec[2].interaction_score_before, rec[2].pose_optimisation_rmsd, rec[2].pose_trials_kept) == (-0.25, 0.0, 0)
    assert all(getattr(Measured(), k) is None for k in ("interaction_score_before", "pose_optimisation_rmsd",
                                                        "pose_trials_kept"))


# ----------------------------------------------------------------------------------------------- the C entry
def test_c_entry_refuses_bad_arguments_without_a_device():
    from ml_conformer_generator_amd import _lib
    assert "mcg_receptor_optimise" in _lib.SIGNATURES
    h = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    #       x  r  t  n  B  N   y  yt R    sph   steps shift out xf st grad  trace stream
    good = [p, p, p, p, 2, 27, p, p, 100, None, 64, 2.0, p, p, p, None, None, None]
    for k in (0, 1, 2, 3, 6, 7, 12, 13, 14):                                      # each required buffer
        bad = list(good)
        bad[k] = None
        assert h.mcg_receptor_optimise(*bad) == 1 and b"mcg_receptor_optimise" in h.mcg_last_error(), k
    for B, N, Rn in ((0, 27, 100), (-1, 27, 100), (16385, 27, 100), (2, 0, 100), (2, 65, 100), (2, 27, 0), (2, 27, -5),
                     (2, 27, (1 << 17) + 1)):
        bad = list(good)
        bad[4], bad[5], bad[8] = B, N, Rn
        assert h.mcg_receptor_optimise(*bad) == 1, (B, N, Rn)
    for steps, shift in ((-1, 2.0), (1025, 2.0), (64, -0.5), (64, float("nan")), (64, float("inf")), (64, -float("inf"))):
        bad = list(good)
        bad[10], bad[11] = steps, shift
        assert h.mcg_receptor_optimise(*bad) == 1, (steps, shift)


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_pose`: the entry's argument checks in a stand-alone program under host-side ASan + UBSan, on the CPU."""
    exe = str(tmp_path / "pose_arg_check")
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_pose", f"POSE_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 not refused" in ran.stdout, ran.stdout + ran.stderr


def test_header_compiles_with_the_new_declaration(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mlconfgen_hip.h"\n'
                   "int main(void) {\n"
                   "  int (*a)(const float*, const float*, const uint8_t*, const int32_t*, int, int, const float*,\n"
                   "           const uint8_t*, int, const float*, int, float, float*, float*, float*, float*, float*, void*)\n"
                   "      = mcg_receptor_optimise;\n"
                   "  return a == 0;\n}\n")
    inc = os.path.join(REPO, "include")
    assert shutil.which("gcc") or shutil.which("g++") or shutil.which("cc")
    for cc, flags in (("gcc", ["-std=c99", "-Wall", "-Wextra", "-Werror"]), ("g++", ["-std=c++11", "-Wall", "-Werror", "-x", "c++"]),
                      ("cc", ["-std=c99", "-Wall", "-Werror"])):
        if shutil.which(cc):
            r = subprocess.run([cc, *flags, "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr


def test_the_shared_text_lives_in_one_place():
    """The rigid-body helpers and the pair arithmetic are written once and included by every kernel that runs them."""
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()                     # noqa: E731
    for name in ("mcg_shape_refine.hip", "mcg_receptor_relief.hip", "mcg_pose_optimise.hip"):
        text = read(name)
        assert '#include "mcg_rigid_step.h"' in text
        assert all(f"void {fn}(" not in text for fn in ("mat3_mul", "rodrigues_row", "orthonormalise")), name
    for name in ("mcg_interactions.hip", "mcg_pose_optimise.hip"):
        text = read(name)
        assert '#include "mcg_interaction_pair.h"' in text and "pair_terms(" in text and "expf(" not in text, name
    assert "mcg_pose_optimise.hip" in read("Makefile")
    # the tile list and the trial step: written in the two headers, in no kernel file
    import re
    sources = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp")))
    for name in (f for f in sources if f.endswith(".hip")):
        text = read(name)
        assert "__ballot(keep)" not in text and "rodrigues_row(" not in text, name
    assert "__ballot(keep)" in read("mcg_receptor_tiles.h") and "rodrigues_row(" in read("mcg_rigid_step.h")
    for name in ("mcg_interactions.hip", "mcg_pose_optimise.hip", "mcg_receptor_relief.hip"):
        text = read(name)
        assert '#include "mcg_receptor_tiles.h"' in text and "build_tile_list(" in text, name
    assert "mcg_receptor_tiles.h" in read("Makefile")
    # the two receptor pose walks: their step constants and their entries' argument check stand in mcg_receptor_walk.h
    for name in ("mcg_pose_optimise.hip", "mcg_pose_flex.hip"):
        text = read(name)
        assert '#include "mcg_receptor_walk.h"' in text and "walk_args_ok(" in text and "max_shift finite" not in text, name
    assert "bad arguments (non-null buffers" in read("mcg_receptor_walk.h")
    assert "mcg_receptor_walk.h" in re.search(r"^HDRS = (.*(?:\\\n.*)*)", read("Makefile"), re.M).group(1)
    # the walks' factors, the tile test's slack and each walk's first and last step lengths are defined once (GR_*: the
    # geometry relaxation's own descent; RF_*, RL_*: the refined overlay's and the relief walk's own lengths)
    once = re.compile(r"\b(\w*(?:GROW|SHRINK|SLACK|STEP_ROT|STEP_TRANS|MIN_TRANS)\w*)\s*=[^=]")
    defined = sorted((const, name) for name in sources for const in once.findall(read(name)) if not const.startswith("GR_"))
    assert defined == [("RF_STEP_ROT", "mcg_shape_refine.hip"), ("RF_STEP_TRANS", "mcg_shape_refine.hip"),
                       ("RL_STEP_ROT", "mcg_receptor_relief.hip"), ("RL_STEP_TRANS", "mcg_receptor_relief.hip"),
                       ("RW_MIN_TRANS", "mcg_receptor_walk.h"), ("RW_STEP_ROT", "mcg_receptor_walk.h"),
                       ("RW_STEP_TRANS", "mcg_receptor_walk.h"), ("TILE_SLACK_ABS", "mcg_receptor_tiles.h"),
                       ("TILE_SLACK_REL", "mcg_receptor_tiles.h"), ("WALK_GROW", "mcg_rigid_step.h"),
                       ("WALK_SHRINK", "mcg_rigid_step.h")], defined
