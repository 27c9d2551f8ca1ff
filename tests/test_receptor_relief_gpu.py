"""Clash relief on the MI355X (`mcg_receptor_relieve`, DESIGN.md section 6 "Clash relief"): penalty, force and torque
against the fp64 restatement inside the derived rule (`relief_ref.py`), before and after the walk; rigid, proper moves;
clashes gone by the independent contact kernel; clean and bad rows; bit identity whatever the batch, row, padded width,
tile skipping and receptor order; and `relieve_clashes` through `generate_conformers` in a carved pocket around the
posed molecules of the same seeded call."""
import math

import numpy as np
import pytest
import torch

import relief_ref as RR
from composed_cases import carved_pocket as _carved_pocket
from conftest import load_golden
from ml_conformer_generator_amd import receptor as RC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x5EED_0000_2026_1016
CASES = RR.cases()
CLASHING = [c for c in CASES if c.name != "clean"]
KEYS = ("coords", "rotation", "translation", "penalty_before", "penalty_after", "accepted_steps", "rmsd", "moved")
_DONE = {}


def _relieve(case, steps, width=None, **kw):
    """One molecule alone (computed once per argument set), at padded width `width` (default: its own n)."""
    key = (case.name, steps, width, tuple(sorted(kw.items())))
    if key not in _DONE:
        x, n, z = RR.pad([case], width or case.n)
        out = RC.relieve_clashes(case.receptor, x, n, z, steps=steps, device=DEV, return_gradient=True, **kw)
        _DONE[key] = {k: v.cpu() for k, v in out.items()}
    return _DONE[key]


def _same(a, b, n, what):
    """Every output of one molecule `torch.equal` (NaN-free rows), its coordinates over the real rows."""
    for k in KEYS + ("gradient",):
        u, v = (a[k][:, :n], b[k][:, :n]) if k == "coords" else (a[k], b[k])
        assert torch.equal(u, v), (what, k)


# ----------------------------------------------------------------------------------------------- against fp64
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_start_values_match_the_restatement(case):
    ri, rj = case.radii()
    for width in sorted({case.n, max(case.n, 41), 64}):
        out = _relieve(case, 0, width)
        got = np.concatenate([out["penalty_before"].numpy(), out["gradient"][0].numpy()])
        RR.check(got, case.x, ri, case.rec, rj, f"{case} start, width {width}")
        assert torch.equal(out["coords"][0, : case.n], torch.from_numpy(case.x))               # bit for bit
        assert not out["coords"][0, case.n:].any()
        assert torch.equal(out["rotation"][0], torch.eye(3)) and not out["translation"].any()
        assert int(out["accepted_steps"]) == 0 and not bool(out["moved"]) and float(out["rmsd"]) == 0.0
        assert torch.equal(out["penalty_after"], out["penalty_before"])
    assert (float(out["penalty_before"]) > 0) == (case.name != "clean")


@pytest.mark.parametrize("case", CLASHING, ids=lambda c: c.name)
def test_penalty_after_the_walk_matches_the_restatement_at_the_returned_pose(case):
    ri, rj = case.radii()
    out = _relieve(case, 32)
    moved = out["coords"][0, : case.n].numpy()
    RR.check(out["penalty_after"].numpy(), moved, ri, case.rec, rj, f"{case} after 32 trials")
    assert float(out["penalty_after"]) <= float(out["penalty_before"])
    assert bool(out["moved"]) and 1 <= int(out["accepted_steps"]) <= 32
    rmsd = math.sqrt(((moved.astype(np.float64) - case.x) ** 2).sum(1).mean())
    assert float(out["rmsd"]) == pytest.approx(rmsd, rel=1e-4, abs=1e-6)
    print(f"RELIEF gpu {case}: P {float(out['penalty_before']):.4g} -> {float(out['penalty_after']):.4g}, "
          f"{int(out['accepted_steps'])} kept, rmsd {rmsd:.2f}")
    one = _relieve(case, 1)                                           # a walk cut short: a penalty that is not zero yet
    RR.check(one["penalty_after"].numpy(), one["coords"][0, : case.n].numpy(), ri, case.rec, rj, f"{case} after 1 trial")
    assert float(one["penalty_after"]) <= float(one["penalty_before"]) and int(one["accepted_steps"]) <= 1
    if case.name in ("n26", "n39", "n64"):
        assert float(one["penalty_after"]) > 0.0


def test_moves_are_rigid_and_proper():
    """The tolerances of `test_refined_poses_are_rigid_and_proper`, which states them for the same algebra - an fp32
    rotation built from up to 1 024 Rodrigues factors, re-orthonormalised, applied to coordinates of 10-20 A."""
    eye = torch.eye(3, dtype=torch.float64)
    for c in CLASHING:
        out = _relieve(c, 32, 64)
        R, t = out["rotation"][0].double(), out["translation"][0].double()
        x, moved = torch.from_numpy(c.x).double(), out["coords"][0, : c.n].double()
        assert abs(float(torch.det(R)) - 1.0) < 1e-5
        assert float((R @ R.T - eye).abs().max()) < 1e-5
        assert float((moved - (x @ R + t)).abs().max()) < 1e-4
        assert float((torch.cdist(x, x) - torch.cdist(moved, moved)).abs().max()) < 1e-4
        assert not out["coords"][0, c.n:].any()
        shift = float((moved.mean(0) - x.mean(0)).norm())
        assert shift <= RC.RELIEF_MAX_SHIFT + 1e-4, (c, shift)
    tight = _relieve(CLASHING[3], 32, max_shift=0.3)                  # a leash shorter than the way out
    x, moved = torch.from_numpy(CLASHING[3].x).double(), tight["coords"][0, : CLASHING[3].n].double()
    assert float((moved.mean(0) - x.mean(0)).norm()) <= 0.3 + 1e-4
    assert float(tight["penalty_after"]) <= float(tight["penalty_before"])


def test_clashes_are_gone_by_the_contact_kernel():
    cleared = 0
    for c in CLASHING:
        ri, rj = c.radii()
        if RR.walk(c.x, ri, c.rec, rj, 16)["penalty"][-1] != 0.0:     # (the host test: this never happens)
            continue
        cleared += 1
        out = _relieve(c, 32)
        x, n, z = RR.pad([c], c.n)
        before = RC.clash_summary(RC.receptor_overlap(c.receptor, x, n, z, DEV))
        after = RC.clash_summary(RC.receptor_overlap(c.receptor, out["coords"], n, z, DEV))
        assert int(after[0]) == 0 and float(after[1]) < RC.CLASH_OVERLAP, (c, after)
        assert float(out["penalty_after"]) == 0.0
        print(f"RELIEF gpu {c}: clashes {int(before[0])} -> 0, worst overlap {float(before[1]):.2f} -> {float(after[1]):.2f}")
    assert cleared == len(CLASHING)


# ----------------------------------------------------------------------------------------------- clean and bad rows
def test_a_clean_row_comes_back_bit_identical():
    clean = next(c for c in CASES if c.name == "clean")
    out = _relieve(clean, 32, 41)
    assert float(out["penalty_before"]) == 0.0 and float(out["penalty_after"]) == 0.0 and not bool(out["moved"])
    assert torch.equal(out["coords"][0, : clean.n], torch.from_numpy(clean.x)) and not out["coords"][0, clean.n:].any()
    assert torch.equal(out["rotation"][0], torch.eye(3)) and not out["translation"].any() and not out["gradient"].any()


def test_bad_rows_are_left_alone_and_spare_their_neighbours():
    c = next(c for c in CASES if c.name == "n26")
    x, n, z = RR.pad([c] * 5, 41)
    base = {k: v.cpu() for k, v in RC.relieve_clashes(c.receptor, x, n, z, device=DEV, return_gradient=True).items()}
    for bad in (float("nan"), float("inf")):
        xb, nb = x.clone(), n.clone()
        xb[1, 7, 2] = bad
        nb[3] = 0
        out = {k: v.cpu() for k, v in RC.relieve_clashes(c.receptor, xb, nb, z, device=DEV, return_gradient=True).items()}
        torch.testing.assert_close(out["coords"][1, : c.n], xb[1, : c.n], rtol=0, atol=0, equal_nan=True)
        assert not out["coords"][1, c.n:].any() and not out["coords"][3].any()
        for b in (1, 3):
            for k in ("rotation", "translation", "penalty_before", "penalty_after", "rmsd", "gradient"):
                assert bool(out[k][b].isnan().all()), (b, k)
            assert int(out["accepted_steps"][b]) == 0 and not bool(out["moved"][b])
        for b in (0, 2, 4):
            for k in KEYS + ("gradient",):
                assert torch.equal(out[k][b], base[k][b]), (b, k)


# ----------------------------------------------------------------------------------------------- determinism
def test_bits_do_not_depend_on_batch_row_width_tiles_or_receptor_order():
    for c in (next(c for c in CASES if c.name == "multi"), next(c for c in CASES if c.name == "R257")):
        alone = _relieve(c, 32)
        for width in (41, 64):
            _same(alone, _relieve(c, 32, width), c.n, (c, width))
        _same(alone, _relieve(c, 32, skip_tiles=False), c.n, (c, "walk every tile"))
        perm = torch.randperm(len(c.rec), generator=torch.Generator().manual_seed(9))
        x, n, z = RR.pad([c], c.n)
        rec = (torch.from_numpy(c.rec)[perm], torch.from_numpy(c.rec_z)[perm])
        shuffled = {k: v.cpu() for k, v in RC.relieve_clashes(rec, x, n, z, device=DEV, return_gradient=True).items()}
        _same(alone, shuffled, c.n, (c, "shuffled receptor"))
        # inside a batch of 70, at two rows, among molecules of other sizes (the same receptor: other ligands in it)
        others = [RR.Case(f"o{k}", 5000 + k, 5 + k % 36) for k in range(70)]
        for o in others:
            o.rec, o.rec_z = c.rec, c.rec_z
        for row in (0, 37, 69):
            batch = list(others)
            batch[row] = c
            x, n, z = RR.pad(batch, 41)
            out = {k: v.cpu() for k, v in RC.relieve_clashes(c.receptor, x, n, z, device=DEV,
                                                             return_gradient=True).items()}
            _same(alone, {k: v[row: row + 1] for k, v in out.items()}, c.n, (c, "row", row))


# ----------------------------------------------------------------------------------------------- generation entries
def _posed_setup(monkeypatch):
    """The monkeypatched posed setup of test_receptor_gpu.py."""
    from ml_conformer_generator_amd import conformer_generator as CG
    from test_shape_frames_gpu import _gen, _molecule_like_shards
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen))
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"]) + torch.tensor([12.0, -5.0, 3.0])
    kw = dict(reference_conformer=ref, variance=2, optimise_geometry=False, sample_seed=SEED, n_samples=12, overlay=True)
    base = gen.generate_conformers(**kw)
    assert base and all(m.receptor_clashes is None for m in base)
    return gen, ref, kw, base


def _measured(m):
    return {k: (None if v is None else v.tolist() if torch.is_tensor(v) else v) for k, v in vars(m._measured).items()}


def test_generation_relieves_the_posed_molecules(monkeypatch):
    """(The generated coordinates are those of the un-posed call of the same seed: the patched shard swaps the
    coordinates behind `last_batch`.)"""
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto
    gen, ref, kw, base = _posed_setup(monkeypatch)
    rec = _carved_pocket(ref, base)
    generated = {m.sample_id: m for m in gen.generate_conformers(**dict(kw, overlay=False))}
    plain = gen.generate_conformers(receptor=rec, **kw)
    got = gen.generate_conformers(receptor=rec, relieve_clashes=True, **kw)
    assert [m.sample_id for m in got] == [m.sample_id for m in plain]
    n_moved = 0
    for a, b in zip(plain, got):
        if b.pose is None:
            assert b.relief_rmsd is None and b.receptor_clashes_before is None and torch.equal(a.coords, b.coords)
            continue
        assert b.receptor_clashes_before == a.receptor_clashes and b.receptor_clashes <= b.receptor_clashes_before
        moved = not torch.equal(a.coords, b.coords)
        assert (b.relief_rmsd > 0) == moved
        R, t = b.pose
        x0 = generated[b.sample_id].coords.double()
        assert float((b.coords.double() - (x0 @ R.double() + t.double())).abs().max()) < 2e-4
        assert abs(float(torch.det(R.double())) - 1.0) < 1e-5
        if not moved:                                             # every bit it had
            assert _measured(b) == dict(_measured(a), relief_rmsd=0.0, receptor_clashes_before=a.receptor_clashes)
            continue
        n_moved += 1
        k, n_ref = len(b.atomic_numbers), int(ref.shape[0])
        pair = torch.zeros(2, max(k, n_ref), 3)
        pair[0, :n_ref], pair[1, :k] = ref, b.coords
        want = pairwise_shape_tanimoto(ref, pair, torch.tensor([n_ref, k], dtype=torch.int32), DEV)[0, 1]
        # the tolerance test_shape_diversity_gpu.py states for this pair of kernels (REF_ROW_ATOL)
        assert abs(b.overlay_tanimoto - float(want)) < 2e-4
        rmsd = float(((b.coords.double() - a.coords.double()) ** 2).sum(1).mean().sqrt())
        assert b.relief_rmsd == pytest.approx(rmsd, rel=1e-3, abs=1e-5)
    print(f"RELIEF e2e: {n_moved} of {len(got)} moved; clashes "
          f"{[m.receptor_clashes_before for m in got]} -> {[m.receptor_clashes for m in got]}; rmsd "
          f"{[None if m.relief_rmsd is None else round(m.relief_rmsd, 2) for m in got]}")
    assert n_moved >= 1

    def no_relief(*a, **k):
        raise AssertionError("the relief ran in a call that did not ask for it")
    monkeypatch.setattr(gen, "_relieve", no_relief)
    monkeypatch.setattr(gen, "_score_placed", no_relief)
    off = gen.generate_conformers(receptor=rec, relieve_clashes=False, **kw)
    assert off == plain and [_measured(m) for m in off] == [_measured(m) for m in plain]
    assert all(m.relief_rmsd is None and m.receptor_clashes_before is None for m in off)


def test_relief_keeps_molecules_the_clash_filter_would_drop(monkeypatch):
    gen, ref, kw, base = _posed_setup(monkeypatch)
    rec = _carved_pocket(ref, base)
    dropped = gen.generate_conformers(receptor=rec, max_receptor_clashes=0, **kw)
    kept = gen.generate_conformers(receptor=rec, max_receptor_clashes=0, relieve_clashes=True, **kw)
    before, after = {m.sample_id for m in dropped}, {m.sample_id for m in kept}
    print(f"RELIEF filter: {sorted(before)} without, {sorted(after)} with relief")
    assert before <= after and len(after) > len(before)
    assert all(m.receptor_clashes == 0 for m in kept)
    assert any(m.receptor_clashes_before > 0 for m in kept)
