"""The cases of tests/large_receptor_cases.py, without a GPU: that every place has the property it was chosen for - which
rounds of `build_tile_list`'s compaction keep tiles there - with the stated margin; that a lost round would show (the SIGNAL
condition: leaving out the atoms of one round moves an asserted output by more than 100 times what the stage's check
allows, and the stage's own `passes` / `check_trace` / `compare` rejects the result); that the receptor subsets the
restatements read are sufficient; and the host preparation - the sorts and the tile spheres - at the limit of 131 072 atoms."""
import numpy as np
import pytest
import torch

import flex_pose_ref as FR
import interactions_ref as IR
import large_receptor_cases as LC
import pocket_ref as PR
import pose_optimise_ref as PO
import relief_ref as RR
from ml_conformer_generator_amd import pocket as PK
from ml_conformer_generator_amd import receptor as RC
from test_pocket_gpu import MAX_LEFT_OUT, eps_for

SIGNAL = 100.0
BOTH_ROUNDS = LC.cases(("BOTH", "SEAM"))


def _ids(cases):
    return [f"{R}-{kind}" for R, kind in cases]


def _real_rows(name):
    return [r for r, row in enumerate(LC.entries()[name].rows) if row.n]


# ----------------------------------------------------------------------------------------------- the cases
def test_the_receptors_have_the_sizes_at_which_each_branch_runs():
    assert [LC.receptor(R).T for R in LC.SIZES] == [256, 257, 270, 512]
    assert LC.SIZES[-1] == RC.MAX_RECEPTOR_ATOMS and LC.SIZES[2] - 269 * 256 == 36          # a partial last tile
    for R in LC.SIZES:
        rec = LC.receptor(R)
        assert tuple(rec.xyz.shape) == (R, 3) and len(torch.unique(rec.xyz, dim=0)) == R     # no two atoms coincide
        assert torch.equal(rec.vdw[:, :3], rec.ix[:, :3])                                   # one order, two sets of radii
        assert set(rec.z.tolist()) == {6, 7, 8, 16} and set(rec.types.tolist()) <= {0, 3, 4}
        for kind, site in rec.sites.items():                                                # the cavities
            d = np.linalg.norm(rec.xyz.double().numpy() - site[None, :], axis=1)
            assert int((d <= LC.CAVITY).sum()) == (1 if kind == "SEAM" else 0), (R, kind)
    seam = LC.receptor(65537)
    assert np.array_equal(seam.sites["SEAM"], seam.vdw[-1, :3].double().numpy())            # the one atom of tile 256
    assert np.array_equal(seam.vdw_spheres[256, :3].double().numpy(), seam.sites["SEAM"])


def test_the_tile_test_is_the_pocket_modules_restatement():
    """`kept` against `pocket.kept_tiles`, which restates the same device text for the pocket's bricks."""
    for R, kind in LC.GRIDS:
        _, spheres = LC.receptor(R).recentred(LC.grid_place(R, kind))
        keep, _ = LC.grid_lists(R, kind)
        want = PK.kept_tiles(spheres, LC.GRID_N, LC.GRID_SPACING, LC.GRID_PROBE, LC.GRID_REACH)
        assert keep.sum(axis=1).tolist() == want.tolist()


@pytest.mark.parametrize("R, kind", LC.cases(), ids=_ids(LC.cases()))
def test_every_tile_list_has_its_property_with_half_an_angstrom_to_spare(R, kind):
    T = LC.receptor(R).T
    names = ("interactions",) if kind in ("LO_ONLY", "LAST") else tuple(LC.entries())
    for name in names:
        for r in _real_rows(name):
            keep, margin = LC.row_list(R, kind, name, r)
            lo, hi = LC.rounds(keep)
            print(f"LARGE {R} {kind} {name} row {r}: {int(lo)} + {int(hi)} of {T} tiles kept in rounds one + two, nearest "
                  f"tile {float(np.abs(margin).min()):.2f} A from its limit, place "
                  f"{np.round(LC.place(R, kind, name, r) - LC.receptor(R).sites[kind], 2).tolist()} from the site")
            assert LC.has_property(kind, T, keep), (name, r, int(lo), int(hi))
            assert float(np.abs(margin).min()) >= LC.MARGIN
            assert float(np.linalg.norm(LC.place(R, kind, name, r) - LC.receptor(R).sites[kind])) <= 2.0
            if kind == "SEAM":
                assert bool(keep[256]) and R - 256 * 256 == 1
            if kind == "BOTH":
                assert int(np.flatnonzero(keep).max()) >= 256                           # an index that needs the ninth bit


@pytest.mark.parametrize("R, kind", LC.GRIDS, ids=_ids(LC.GRIDS))
def test_the_grids_tile_lists(R, kind):
    keep, margin = LC.grid_lists(R, kind)
    lo, hi = LC.rounds(keep)
    near = np.abs(margin) < LC.MARGIN
    print(f"LARGE {R} {kind} grid: tiles kept per brick, rounds one + two: {list(zip(lo.tolist(), hi.tolist()))}; "
          f"{int(near.sum())} (brick, tile) pairs lie within {LC.MARGIN} A of their limit and may flip")
    assert keep.shape == (12, LC.receptor(R).T)
    assert LC.grid_decided(kind, keep, margin)
    if kind == "HI_ONLY":
        assert not lo.any() and hi.all() and not near[:, :256].any()
    else:
        assert (lo > 0).all() and (hi > 0).all()                                        # as it stands: every brick both


# ----------------------------------------------------------------------------------------------- the signal
def _moved(a, b, bound):
    """The largest |a - b| / bound over the values; inf where the bound is 0 and the values differ."""
    err = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    r = np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0)
    return float(r.max()) if r.size else 0.0


def _flex_start(R, kind, r, idx):
    """(`flex_pose_ref.evaluate`, `value_bounds`) of the flexible walk's row at its input pose against the atoms `idx`."""
    row, x, _ = LC.launch(R, kind, "flex")["rows"][r]
    g = row.graph
    xp, lever = PO.start_pose(x)
    tree, cr = FR.tree(g.z, g.bonds, g.n), FR.clash_radii(g.z)
    lig, rec = (IR.radii(row.z), row.t), LC.receptor_args(R, "flex", idx)
    want = FR.evaluate(lever.astype(np.float64), np.eye(3, dtype=np.float32), xp, lever, lig, rec, cr, tree)
    return want, FR.value_bounds(want, xp, lever, lig, rec, cr, tree, 0.0)


@pytest.mark.parametrize("R, kind", BOTH_ROUNDS, ids=_ids(BOTH_ROUNDS))
def test_a_lost_round_moves_an_asserted_output_a_hundred_bounds(R, kind):
    """Per scoring entry and row, for round two lost and for round one lost: the worst (change / what the stage's check
    allows) over the outputs the GPU test asserts."""
    for lost, seen in (("two", "first"), ("one", "second")):
        for r in _real_rows("interactions"):
            full = LC.score_args(R, kind, r)
            part = LC.score_args(R, kind, r, LC.subset(R, kind, "interactions", r, rounds_kept=seen))
            a, b, bound = IR.score(*full), IR.score(*part), IR.bounds(*full)
            moved = max(_moved(a[k], b[k], bound[k]) for k in bound)
            print(f"SIGNAL {R} {kind} interactions row {r}, round {lost} lost: {moved:.3g} bounds")
            assert moved > SIGNAL
            assert not IR.passes(b, *full)                                               # the negative control
            # the rigid walk reads the same pairs: W and the net force at its input pose
            row, x, _ = LC.launch(R, kind, "optimise")["rows"][r]
            full = LC.score_args(R, kind, r, name="optimise")[:6]
            part = LC.score_args(R, kind, r, LC.subset(R, kind, "optimise", r, rounds_kept=seen), "optimise")[:6]
            xp, lever = PO.start_pose(x)
            a, b = PO.evaluate(xp, lever, *full[1:]), PO.evaluate(xp, lever, *part[1:])
            bF, bT = PO.force_bounds(xp, lever, *full[1:])
            moved = max(_moved(a["weighted"], b["weighted"], PO.weighted_bound(xp, *full[1:])),
                        _moved(a["force"], b["force"], bF), _moved(a["torque"], b["torque"], bT))
            print(f"SIGNAL {R} {kind} optimise row {r}, round {lost} lost: {moved:.3g} bounds")
            assert moved > SIGNAL
        for r in _real_rows("flex"):
            a, bound = _flex_start(R, kind, r, LC.subset(R, kind, "flex", r))
            b, _ = _flex_start(R, kind, r, LC.subset(R, kind, "flex", r, rounds_kept=seen))
            moved = max(_moved(a["weighted"], b["weighted"], bound["weighted"]),
                        *(_moved(a[k], b[k], FR.FLEX_FACTORS[k] * np.asarray(bound[k])) for k in ("force", "torque")))
            print(f"SIGNAL {R} {kind} flex row {r}, round {lost} lost: {moved:.3g} bounds")
            assert moved > SIGNAL
        for r in _real_rows("relief"):
            row, x, _ = LC.launch(R, kind, "relief")["rows"][r]
            ri = LC.ligand_radii("relief", row)
            y, rj, _ = LC.receptor_args(R, "relief", LC.subset(R, kind, "relief", r))
            ys, rs, _ = LC.receptor_args(R, "relief", LC.subset(R, kind, "relief", r, rounds_kept=seen))
            a, b, bound = RR.seven(x, ri, y, rj), RR.seven(x, ri, ys, rs), RR.bounds(x, ri, y, rj)
            moved = _moved(a, b, bound)
            print(f"SIGNAL {R} {kind} relief row {r}, round {lost} lost: {moved:.3g} bounds (P {a[0]:.4g} -> {b[0]:.4g})")
            assert moved > SIGNAL
            assert not RR.passes(b, x, ri, y, rj)


@pytest.mark.parametrize("R, kind", BOTH_ROUNDS, ids=_ids(BOTH_ROUNDS))
def test_the_walks_restatements_reject_a_walk_that_lost_round_two(R, kind):
    """The negative control of the two teacher-forced rules: the restatement's own walk against the receptor without the
    atoms of round two, judged against the whole subset."""
    r = 0
    row, x, _ = LC.launch(R, kind, "optimise")["rows"][r]
    full = LC.score_args(R, kind, r, name="optimise")[1:6]
    part = LC.score_args(R, kind, r, LC.subset(R, kind, "optimise", r, rounds_kept="first"), "optimise")[1:6]
    lost = PO.run_walk(x, *part, LC.STEPS, LC.MAX_SHIFT, state=np.float32)
    bad, _ = PO.check_trace(lost["trace"].astype(np.float32), x, *full, LC.STEPS, LC.MAX_SHIFT)
    assert bad != []
    whole = PO.run_walk(x, *full, LC.STEPS, LC.MAX_SHIFT, state=np.float32)
    bad, _ = PO.check_trace(whole["trace"].astype(np.float32), x, *full, LC.STEPS, LC.MAX_SHIFT)
    assert bad == [], bad[:3]
    row, x, _ = LC.launch(R, kind, "flex")["rows"][r]
    g, lig = row.graph, (IR.radii(row.z), row.t)
    rec_full = LC.receptor_args(R, "flex", LC.subset(R, kind, "flex", r))
    rec_part = LC.receptor_args(R, "flex", LC.subset(R, kind, "flex", r, rounds_kept="first"))
    lost = FR.run_walk(x, lig, rec_part, g.z, g.bonds, LC.STEPS, LC.MAX_SHIFT)
    bad, _ = FR.check_trace(np.asarray(lost["trace"], dtype=np.float32), x, lig, rec_full, g.z, g.bonds, LC.STEPS, LC.MAX_SHIFT)
    assert bad != []


# ----------------------------------------------------------------------------------------------- the subsets
@pytest.mark.parametrize("R, kind", LC.cases(), ids=_ids(LC.cases()))
def test_the_subsets_hold_every_atom_that_can_contribute(R, kind):
    """No atom outside a row's subset comes within the cut-off (the relief: within contact) of where an atom of the row can
    be during the launch - over the WHOLE receptor, which is more than the subset of twice the margin; and the restatement
    on the atoms that the doubled margin adds gives exact zeros, so the two subsets restate the same sums."""
    rec = LC.receptor(R)
    names = ("interactions",) if kind in ("LO_ONLY", "LAST") else tuple(LC.entries())
    for name in names:
        e = LC.entries()[name]
        for r in _real_rows(name):
            row, x, point = LC.launch(R, kind, name)["rows"][r]
            idx, wide = LC.subset(R, kind, name, r), LC.subset(R, kind, name, r, margin=2.0)
            assert set(idx.tolist()) <= set(wide.tolist()) and 20 <= len(idx) <= 4000
            xyzr = rec.sorted(e.radii).double().numpy()
            outside = np.ones(R, dtype=bool)
            outside[idx] = False
            d = np.linalg.norm(xyzr[outside, :3] - point[None, :], axis=1) - e.extent(row, point)
            reach = LC.CUTOFF if e.cutoff is not None else RR.CARBON + xyzr[outside, 3]
            assert float((d - reach).min()) >= 1.0                      # the margin, with the largest radius still unused
            assert float(np.linalg.norm(x.astype(np.float64) - point[None, :], axis=1).max()) <= e.extent(row, point)
            ring = np.setdiff1d(wide, idx)
            if name == "relief":
                y, rj, _ = LC.receptor_args(R, name, ring)
                assert not RR.seven(x, LC.ligand_radii(name, row), y, rj).any()
            elif len(ring):
                out = IR.score(*LC.score_args(R, kind, r, ring, name))
                assert not out["atom_terms"].any() and out["hbonds"] == 0 and out["weighted"] == 0.0


@pytest.mark.parametrize("R, kind", LC.GRIDS, ids=_ids(LC.GRIDS))
def test_the_pocket_restatement_on_its_subset(R, kind):
    """The subset of twice the margin gives the same masks and margins, exactly; the restatement alone leaves out less
    than MAX_LEFT_OUT of the pairs at `eps_for`; a lost round is rejected by `compare`; and the centre holds a pocket."""
    args = (LC.GRID_N, LC.GRID_SPACING, LC.GRID_PROBE, LC.GRID_REACH)
    want, margin = PR.masks(*LC.grid_subset(R, kind), *args)
    wide, wide_margin = PR.masks(*LC.grid_subset(R, kind, margin=2.0), *args)
    assert np.array_equal(want, wide) and np.array_equal(margin, wide_margin)
    eps = eps_for(max(LC.GRID_SPACING * (LC.GRID_N // 2), 1.0), LC.GRID_REACH)
    wrong, left_out = PR.compare(want, want, margin, eps)
    below = margin < eps
    print(f"LARGE {R} {kind} grid: eps {eps:.2e} A^2, the restatement leaves out {100 * left_out:.4f} % of the pairs "
          f"({int(below[:, :26].sum())} rays, {int(below[:, 26].sum())} occupancies); occupied "
          f"{int((want >> 31).sum())} of {len(want)} points, mean buriedness {PK.buriedness(want).mean():.1f}")
    assert wrong == 0 and left_out <= MAX_LEFT_OUT
    for seen in ("first", "second"):
        lost, _ = PR.masks(*LC.grid_subset(R, kind, rounds_kept=seen), *args)
        wrong, _ = PR.compare(lost, want, margin, eps)
        print(f"LARGE {R} {kind} grid: with round {'two' if seen == 'first' else 'one'} lost {wrong} pairs are wrong")
        assert wrong > (0 if kind == "SEAM" else 100) or (kind == "HI_ONLY" and seen == "second")
    if (R, kind) == LC.GRIDS[0]:                                        # where the GPU test calls `find_pocket`
        found = PK.pocket_from_masks(want, None, LC.grid_place(R, kind), radius=4.0, reach=LC.GRID_REACH)
        assert found.n_centres >= 1 and PK.grid_size(4.0, 1.0) == LC.GRID_N


# ----------------------------------------------------------------------------------------------- the host preparation
def test_the_sorts_at_the_limit_do_not_depend_on_the_input_order():
    rec = LC.receptor(131072)
    perm = torch.randperm(rec.R, generator=torch.Generator().manual_seed(17))
    radii = RC.vdw_radii(rec.z)
    again = RC.sort_receptor(rec.xyz[perm], radii[perm])
    assert torch.equal(again.view(torch.int32), rec.vdw.view(torch.int32))
    given = torch.cat([rec.xyz, radii[:, None]], dim=1)
    assert torch.equal(torch.unique(again, dim=0), torch.unique(given, dim=0)) and len(torch.unique(again, dim=0)) == rec.R
    ix_radii = rec.ix[:, 3]
    prepared = RC.sort_typed_receptor(rec.ix[perm, :3], ix_radii[perm], rec.ix_types[perm])
    assert torch.equal(prepared[0].view(torch.int32), rec.ix.view(torch.int32)) and torch.equal(prepared[1], rec.ix_types)
    five = lambda xyzr, t: torch.unique(torch.cat([xyzr.double(), t.double()[:, None]], dim=1), dim=0)      # noqa: E731
    from ml_conformer_generator_amd import interactions as IX
    assert torch.equal(five(*prepared), five(torch.cat([rec.xyz, IX.interaction_radii(rec.z)[:, None]], dim=1), rec.types))
    assert len(five(*prepared)) == rec.R


@pytest.mark.parametrize("R", [65537, 68900])
def test_every_atom_lies_inside_its_tiles_sphere(R):
    """In fp64, the last tile - padded with the last atom again - included."""
    rec = LC.receptor(R)
    for xyzr, spheres in ((rec.vdw, rec.vdw_spheres), (rec.ix, rec.ix_spheres)):
        assert tuple(spheres.shape) == (rec.T, 4)
        q = spheres.double().numpy()[np.arange(R) // 256]
        a = xyzr.double().numpy()
        assert (np.linalg.norm(a[:, :3] - q[:, :3], axis=1) + a[:, 3] <= q[:, 3]).all()
    last = rec.vdw_spheres[-1].double().numpy()
    tail = rec.vdw[256 * (rec.T - 1):].double().numpy()
    assert len(tail) == R - 256 * (rec.T - 1) and last[3] <= np.linalg.norm(tail[:, :3] - last[:3], axis=1).max() + 1.81
