"""Optimised pose on the MI355X (`mcg_receptor_optimise`, DESIGN.md section 6 "Optimised pose"): every trial of the
kernel's walk against the restatement, TEACHER-FORCED through the trace (`pose_optimise_ref.check_trace`: no comparison
depends on two walks taking the same branch); the returned coordinates as the bits of the last kept pose; W before and
after as the bits `mcg_receptor_interactions` gives; junk beyond every row and sentinels round every output; bit identity
whatever the batch, row, padded width, tile skipping and receptor order; empty, non-finite and out-of-reach rows; and the
option through `generate_conformers`, `generate_conformers_sharded` and `forward` in a carved pocket."""
import numpy as np
import pytest
import torch

import interactions_ref as IR
import pose_optimise_ref as P
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import interactions as IX

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = P.cases()
GUARD = 96                                        # sentinel elements on either side of every output
STEPS = 64
SHIFT = 2.0
F32 = np.float32
_DONE = {}
NAMES = ("coords", "xform", "stats", "gradient", "trace")


def _pad(case_list, width):
    """The kernel's ligand inputs of cases at padded width `width`, junk beyond every row's atoms."""
    B = len(case_list)
    x = np.full((B, width, 3), 7.5, dtype=np.float32)
    r = np.full((B, width), 1.9, dtype=np.float32)
    t = np.full((B, width), 7, dtype=np.uint8)
    for b, c in enumerate(case_list):
        x[b, : c.n], r[b, : c.n], t[b, : c.n] = c.x, IR.radii(c.z), c.t
    return (torch.from_numpy(x), torch.tensor([c.n for c in case_list], dtype=torch.int32), torch.from_numpy(r),
            torch.from_numpy(t))


def _launch(case_list, width, receptor, steps=STEPS, max_shift=SHIFT, skip_tiles=True):
    """The C entry itself on cases against one receptor, every output inside a buffer of sentinels; host tensors."""
    prepared = IX.prepare_receptor(receptor)
    x, n, r, t = (v.to(DEV).contiguous() for v in _pad(case_list, width))
    B = len(case_list)
    rec, rec_t = prepared.xyzr.to(DEV), prepared.types.to(DEV)
    spheres = prepared.spheres.to(DEV) if skip_tiles else None
    sizes = (B * width * 3, B * 12, B * 8, B * 6, B * steps * 24)
    bufs = [torch.full((k + 2 * GUARD,), -777.0, device=DEV) for k in sizes]
    views = [buf[GUARD: GUARD + k] for buf, k in zip(bufs, sizes)]
    _lib.check(_lib.lib().mcg_receptor_optimise(
        _lib.dptr(x), _lib.dptr(r), _lib.dptr(t), _lib.dptr(n), B, width, _lib.dptr(rec), _lib.dptr(rec_t),
        int(rec.shape[0]), _lib.dptr(spheres), steps, float(max_shift), *(v.data_ptr() for v in views),
        _lib.current_stream_ptr(DEV)), "mcg_receptor_optimise")
    torch.cuda.synchronize()
    for buf, k in zip(bufs, sizes):
        host = buf.cpu()
        assert bool((host[:GUARD] == -777).all()) and bool((host[GUARD + k:] == -777).all()), "a write outside the output"
    shapes = ((B, width, 3), (B, 12), (B, 8), (B, 6), (B, steps, 24))
    out = {name: v.cpu().reshape(shape) for name, v, shape in zip(NAMES, views, shapes)}
    out["input"] = x.cpu()
    return out


def _one(case, width=None, steps=STEPS, skip_tiles=True):
    key = (case.name, width, steps, skip_tiles)
    if key not in _DONE:
        _DONE[key] = _launch([case], width or max(case.n, 1), case.receptor, steps, skip_tiles=skip_tiles)
    return _DONE[key]


def _args(c):
    """What the restatement takes of a case: the receptor as the kernel walks it (sorted; the order changes no value of
    the restatement, only which rows its arrays hold)."""
    return IR.radii(c.z), c.t, c.rec, IR.radii(c.rec_z), c.rec_t


def _same(a, b, n, what, row_a=0, row_b=0, steps=STEPS):
    """The outputs of one molecule bit for bit (NaN-free rows)."""
    bits = lambda t: t.contiguous().view(torch.int32)                             # noqa: E731
    assert torch.equal(bits(a["coords"][row_a, :n]), bits(b["coords"][row_b, :n])), what
    for k in ("xform", "stats", "gradient"):
        assert torch.equal(bits(a[k][row_a]), bits(b[k][row_b])), (what, k)
    assert torch.equal(bits(a["trace"][row_a, :steps]), bits(b["trace"][row_b, :steps])), (what, "trace")


def _score(case, coords, receptor=None):
    """`mcg_receptor_interactions`' mol_terms of one molecule at `coords` [n,3]."""
    n = case.n
    out = IX.score_typed(receptor or case.receptor, coords.reshape(1, n, 3), torch.tensor([n], dtype=torch.int32),
                         torch.from_numpy(IR.radii(case.z)).reshape(1, n), torch.from_numpy(case.t).reshape(1, n),
                         torch.zeros(1, dtype=torch.int32), device=DEV)
    return out["mol_terms"].cpu()[0]


# ----------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_trial_matches_the_restatement_teacher_forced(case):
    c = case
    out = _one(c)
    ratios = {}
    bad, end = P.check_trace(out["trace"][0].numpy(), c.x, *_args(c), STEPS, SHIFT, stats=out["stats"][0].numpy(),
                             coords=out["coords"][0].numpy(), ratios=ratios)
    stats = out["stats"][0]
    mine = P.run_walk(c.x, *_args(c), STEPS, SHIFT, state=np.float64)
    print(f"POSE {c}: W {float(stats[0]):.6f} -> {float(stats[1]):.6f} in {int(stats[2])} trials, {int(stats[3])} kept, rmsd "
          f"{float(stats[4]):.4f}, s_t {float(stats[5]):.5f}; restatement's own walk {mine['w_before']:.6f} -> "
          f"{mine['w_after']:.6f} in {mine['trials']} trials, {mine['kept']} kept, rmsd {mine['rmsd']:.4f}; "
          f"err/bound(factor 1) {({k: round(v, 4) for k, v in ratios.items()})} FORCE_FACTOR {P.FORCE_FACTOR}")
    assert bad == [], bad[:5]
    # the returned rows, the transform and the statistics
    n = c.n
    assert not out["coords"][0, n:].any()                                         # padded rows zero
    xf = out["xform"][0].double().numpy()
    Rm, t = xf[:9].reshape(3, 3), xf[9:]
    assert (np.abs(Rm @ Rm.T - np.eye(3)) <= P.ORTHO).all() and np.linalg.det(Rm) > 0
    got = out["coords"][0, :n].double().numpy()
    x = c.x.astype(np.float64)
    centre = P.centroid(c.x).astype(np.float64)
    # x @ R + t against (x - c) @ G + p: three products and sums on either side, the rounding of t and of the row
    bound = 8 * P.U * (np.abs(x).sum(axis=1, keepdims=True) + np.abs(centre).sum() + np.abs(end["p"]).sum() + 1.0)
    assert (np.abs(x @ Rm + t - got) <= bound).all()
    assert not P.shift_rejects(end["p"], P.centroid(c.x), SHIFT)                  # |p - c| <= max_shift, as the kernel tests it
    assert np.linalg.norm(end["p"].astype(np.float64) - centre) <= SHIFT * (1 + 4 * P.U) + 4 * P.U * np.abs(centre).max()
    kept = int(stats[3])
    assert float(stats[1]) <= float(stats[0]) and (kept == 0 or float(stats[1]) < float(stats[0]))
    rmsd = float(np.sqrt(((got - x) ** 2).sum() / n))
    assert abs(float(stats[4]) - rmsd) <= 1e-5 * max(rmsd, 1.0)
    if kept == 0:
        assert torch.equal(out["coords"][0, :n].view(torch.int32), out["input"][0, :n].view(torch.int32))
        assert xf.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and float(stats[4]) == 0.0
    # the net force and torque at the input pose are the first trial's
    if end["trials"]:
        assert torch.equal(out["gradient"][0].view(torch.int32), out["trace"][0, 0, :6].contiguous().view(torch.int32))
    # W before and after are the scoring kernel's bits
    assert torch.equal(stats[0].view(torch.int32), _score(c, out["input"][0, :n])[5].view(torch.int32))
    assert torch.equal(stats[1].view(torch.int32), _score(c, out["coords"][0, :n])[5].view(torch.int32))


def test_the_displaced_cases_move_downhill():
    moved = [c.name for c in CASES if int(_one(c)["stats"][0, 3]) > 0]
    assert len(moved) >= 6, moved                                                 # the walk has something to do in most


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[7]], ids=lambda c: c.name)
@pytest.mark.parametrize("steps", [0, 1, 8])
def test_a_smaller_budget_is_a_prefix_of_the_walk(case, steps):
    c = case
    full, out = _one(c), _one(c, steps=steps)
    n = c.n
    if steps == 0:                                                                # nothing tried: the input's bits
        assert torch.equal(out["coords"][0, :n].view(torch.int32), out["input"][0, :n].view(torch.int32))
        assert out["xform"][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
        assert out["stats"][0, 2:].tolist() == [0, 0, 0, 0.25, 0, 0]
        assert torch.equal(out["stats"][0, 0].view(torch.int32), out["stats"][0, 1].view(torch.int32))
        assert torch.equal(out["stats"][0, 0].view(torch.int32), full["stats"][0, 0].view(torch.int32))
        assert torch.equal(out["gradient"][0].view(torch.int32), full["gradient"][0].view(torch.int32))
        return
    assert torch.equal(out["trace"][0].view(torch.int32), full["trace"][0, :steps].contiguous().view(torch.int32))
    bad, _ = P.check_trace(out["trace"][0].numpy(), c.x, *_args(c), steps, SHIFT, stats=out["stats"][0].numpy(),
                           coords=out["coords"][0].numpy())
    assert bad == [], bad[:5]


def test_the_shift_limit_rejects_unevaluated():
    c = CASES[2]
    for max_shift in (0.0, 0.3):
        out = _launch([c], c.n, c.receptor, 16, max_shift)
        bad, end = P.check_trace(out["trace"][0].numpy(), c.x, *_args(c), 16, max_shift, stats=out["stats"][0].numpy(),
                                 coords=out["coords"][0].numpy())
        assert bad == [], bad[:5]
        flags = out["trace"][0, : end["trials"], 21]
        assert end["trials"] > 0 and bool((flags == 0).any())
        if max_shift == 0.0:
            assert end["kept"] == 0 and not flags.any()
            assert torch.equal(out["coords"][0, : c.n].view(torch.int32), out["input"][0, : c.n].view(torch.int32))


# ----------------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3], CASES[7], CASES[8]], ids=lambda c: c.name)
def test_bits_do_not_depend_on_batch_row_width_skipping_or_receptor_order(case):
    c = case
    alone = _one(c)
    for width in (41, 64):
        if width >= c.n:
            _same(alone, _one(c, width), c.n, (c, width))
    _same(alone, _one(c, skip_tiles=False), c.n, (c, "walk every tile"))
    xyz, z, t = c.receptor
    for seed in range(4):
        p = torch.randperm(len(z), generator=torch.Generator().manual_seed(seed))
        _same(alone, _launch([c], max(c.n, 1), (xyz[p], z[p], t[p])), c.n, (c, "shuffled receptor", seed))
    # inside a batch of 70, at three rows, among molecules of other sizes (the same receptor: other ligands in it)
    others = [IR.Case(f"o{k}", 5000 + k, 1 + k % 40) for k in range(70)]
    width = 64 if c.n > 41 else 41
    for row in (0, 37, 69):
        batch = list(others)
        batch[row] = c
        _same(alone, _launch(batch, width, c.receptor), c.n, (c, "row", row), 0, row)


def test_tiles_are_skipped_without_a_changed_bit():
    c = CASES[2]
    g = np.random.default_rng(3)
    far = g.uniform(-6, 6, size=(3000, 3)) + np.array([0.0, 0.0, 70.0])           # whole tiles out of reach
    rec = (torch.from_numpy(np.concatenate([c.rec[:300], far, c.rec[300:]]).astype(np.float32)),
           torch.cat([torch.from_numpy(c.rec_z[:300]), torch.full((3000,), 6), torch.from_numpy(c.rec_z[300:])]),
           torch.cat([torch.from_numpy(c.rec_t[:300]), torch.full((3000,), 4, dtype=torch.uint8),
                      torch.from_numpy(c.rec_t[300:])]))
    on, off = _launch([c], 27, rec, skip_tiles=True), _launch([c], 27, rec, skip_tiles=False)
    _same(on, off, c.n, "far slab")
    _same(on, _one(c), c.n, "the slab adds nothing")                              # pairs that do not count add exactly +0


# ----------------------------------------------------------------------------------------------- special rows
def test_empty_and_non_finite_rows_beside_good_rows():
    good = [CASES[2], CASES[1], CASES[3]]
    rec = CASES[2].receptor
    empty = IR.Case("empty", 51, 0)
    bad = IR.Case("bad", 52, 9)
    bad.x = bad.x.copy()
    bad.x[4, 1] = np.float32("nan")
    inf = IR.Case("inf", 53, 5)
    inf.x = inf.x.copy()
    inf.x[0, 0] = np.float32("inf")
    batch = [good[0], empty, good[1], bad, inf, good[2]]
    out = _launch(batch, 64, rec)
    for row, c in ((1, empty), (3, bad), (4, inf)):                               # as they came, NaN everywhere else
        assert torch.equal(out["coords"][row, : c.n].view(torch.int32), torch.from_numpy(c.x).view(torch.int32))
        assert not out["coords"][row, c.n:].any() and not out["trace"][row].any()
        assert all(bool(torch.isnan(out[k][row]).all()) for k in ("xform", "stats", "gradient"))
    for row, c in ((0, good[0]), (2, good[1]), (5, good[2])):                     # the other rows are unaffected
        alone = _launch([c], 64, rec)
        _same(alone, out, c.n, ("beside bad rows", row), 0, row)
        assert bool(torch.isfinite(out["stats"][row]).all())


def test_receptor_beyond_the_cut_off_leaves_the_molecule_where_it_is():
    far = IR.Case("far", 31, 27, far=True)
    for skip in (True, False):
        out = _launch([far], 41, far.receptor, skip_tiles=skip)
        assert torch.equal(out["coords"][0, :27].view(torch.int32), out["input"][0, :27].view(torch.int32))
        assert out["xform"][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
        assert out["stats"][0].tolist() == [0, 0, 0, 0, 0, 0.25, 0, 0]            # no counted pair: no trial at all
        assert not out["gradient"].any() and not out["trace"].any()


# ----------------------------------------------------------------------------------------------- the module's own path
def test_optimise_pose_on_graphs_equals_the_typed_launch():
    import interactions_cases as K
    from test_interactions_gpu import _padded
    mols = [K.MOLECULES[name][0] for name in ("toluene", "acetamide", "biphenyl", "pyridine", "ethanol", "butane")]
    z, bonds, n = _padded(mols, 41)
    g = np.random.default_rng(8)
    x = torch.zeros(len(mols), 41, 3)
    for b, (_, _, k) in enumerate(mols):
        x[b, :k] = torch.from_numpy(IR.walk(k, g).astype(np.float32)) + torch.tensor([0.6, -0.3, 0.2])
    rec = IR.cases()[2].receptor
    out = {k: v.cpu() for k, v in IX.optimise_pose(rec, x, n, z, bonds, steps=16, device=DEV, trace=True).items()}
    types = IX.ligand_types(z, bonds, n, DEV)
    typed = IX.optimise_typed(rec, x, n, IX.interaction_radii(z[:, :41].to(DEV)), types, 16, 2.0, False, DEV)
    assert torch.equal(out["coords"].view(torch.int32), typed["coords"].cpu().view(torch.int32))
    assert torch.equal(out["weighted_after"].view(torch.int32), typed["stats"][:, 1].cpu().view(torch.int32))
    assert out["moved"].tolist() == (out["kept"] > 0).tolist() and bool(out["moved"].any())
    assert tuple(out["rotation"].shape) == (6, 3, 3) and tuple(out["trace"].shape) == (6, 16, 24)
    posed = (x.double() @ out["rotation"].double() + out["translation"].double()[:, None, :])
    real = torch.arange(41).view(1, -1, 1) < n.view(-1, 1, 1)
    assert float(((posed - out["coords"].double()) * real).abs().max()) < 1e-4
    scores = IX.interaction_scores(rec, out["coords"], n, z, bonds, device=DEV)
    assert torch.equal(scores["terms"][:, 5].cpu().view(torch.int32), out["weighted_after"].view(torch.int32))
    empty = IX.optimise_pose(rec, x[:0], n[:0], z[:0], bonds[:0], device=DEV)
    assert tuple(empty["coords"].shape) == (0, 41, 3) and tuple(empty["kept"].shape) == (0,)


# ----------------------------------------------------------------------------------------------- generation entries
NEW = ("interaction_score_before", "pose_optimisation_rmsd", "pose_trials_kept")


def _flat(m, skip=()):
    return {k: (None if v is None else v.tolist() if torch.is_tensor(v) else v) for k, v in vars(m._measured).items()
            if k not in skip and k != "interaction_atom_scores"}


def test_generation_with_optimise_pose(monkeypatch):
    from composed_cases import carved_pocket
    from test_receptor_relief_gpu import _posed_setup
    gen, ref, kw, base = _posed_setup(monkeypatch)
    pts, z = carved_pocket(ref, base)
    g = torch.Generator().manual_seed(12)
    z = torch.tensor([6, 6, 7, 8])[torch.randint(0, 4, (len(z),), generator=g)]
    rec = (pts, z, torch.randint(0, 8, (len(z),), generator=g))
    launched = []
    real = gen._optimise_pose
    monkeypatch.setattr(gen, "_optimise_pose", lambda *a, **k: launched.append(1) or real(*a, **k))
    generated = {m.sample_id: m for m in gen.generate_conformers(**dict(kw, overlay=False))}

    plain = gen.generate_conformers(receptor=rec, interaction_scores=True, **kw)
    off = gen.generate_conformers(receptor=rec, interaction_scores=True, optimise_pose=False, **kw)
    assert launched == [] and off == plain and [_flat(m) for m in off] == [_flat(m) for m in plain]
    assert all(a.interaction_atom_scores is None if b.interaction_atom_scores is None else
               torch.equal(a.interaction_atom_scores.view(torch.int32), b.interaction_atom_scores.view(torch.int32))
               for a, b in zip(off, plain))
    assert all(getattr(m, f) is None for m in plain for f in NEW)
    got = gen.generate_conformers(receptor=rec, optimise_pose=True, **kw)         # implies the score
    assert launched == [1] and [m.sample_id for m in got] == [m.sample_id for m in plain]
    n_moved = 0
    for a, b in zip(plain, got):
        if b.pose is None:
            assert all(getattr(b, f) is None for f in NEW) and torch.equal(a.coords, b.coords)
            continue
        assert b.interaction_score <= b.interaction_score_before
        assert np.float32(b.interaction_score_before) == np.float32(a.interaction_score)      # E where the walk started
        Rm, t = b.pose
        x0 = generated[b.sample_id].coords.double()
        assert float((b.coords.double() - (x0 @ Rm.double() + t.double())).abs().max()) < 2e-4
        assert abs(float(torch.det(Rm.double())) - 1.0) < 1e-5
        if b.pose_trials_kept == 0:                                               # every bit it had
            assert torch.equal(a.coords, b.coords) and b.pose_optimisation_rmsd == 0.0
            assert _flat(b, NEW) == _flat(a, NEW) and b.interaction_score == b.interaction_score_before
            continue
        n_moved += 1
        assert b.interaction_score < b.interaction_score_before
        rmsd = float(((b.coords.double() - a.coords.double()) ** 2).sum(1).mean().sqrt())
        assert b.pose_optimisation_rmsd == pytest.approx(rmsd, rel=1e-3, abs=1e-5) and rmsd > 0
        shift = float((b.coords.double().mean(0) - a.coords.double().mean(0)).norm())
        assert shift <= IX.OPTIMISE_MAX_SHIFT + 1e-4
    assert n_moved >= 1
    print(f"POSE e2e: {n_moved} of {len(got)} moved; E "
          f"{[None if m.interaction_score_before is None else round(m.interaction_score_before, 3) for m in got]} -> "
          f"{[None if m.interaction_score is None else round(m.interaction_score, 3) for m in got]}; kept "
          f"{[m.pose_trials_kept for m in got]}")
    public = lambda m: (_flat(m), None if m.interaction_atom_scores is None else                # noqa: E731
                        m.interaction_atom_scores.view(torch.int32).tolist(), m.coords.view(torch.int32).tolist())
    for entry in ("generate_conformers_sharded", "forward"):
        again = getattr(gen, entry)(receptor=rec, optimise_pose=True, **kw)
        assert [public(m) for m in again] == [public(m) for m in got], entry
    fewer = gen.generate_conformers(receptor=rec, optimise_pose=2, relieve_clashes=True, **kw)
    assert all(m.pose_trials_kept is None or m.pose_trials_kept <= 2 for m in fewer)
    assert all(m.relief_rmsd is not None for m in fewer if m.pose is not None)
