"""The six receptor entries on the MI355X above 65 536 receptor atoms, where `mcg_tiles::build_tile_list`
(csrc/mcg_receptor_tiles.h) compacts its tile list in a second round of 256 tiles ("Shared device
text"): `mcg_receptor_interactions`, `mcg_receptor_optimise`, `mcg_receptor_optimise_flex`, `mcg_receptor_relieve` and
`mcg_pocket_masks` at the places of tests/large_receptor_cases.py - chosen so that both rounds keep tiles, round two alone,
round one alone, or the one-atom tile 256 -, and `mcg_receptor_overlap`, which walks every tile by split.  Each entry is
called raw between sentinels, gives the same bits with tile skipping off (every one of 257 / 270 / 512 tiles kept: the full
list) and is judged by its stage's own restatement and rule, unchanged, on the receptor subset the host test shows
sufficient; the host test also shows that a lost round would move an asserted output by more than a hundred bounds.  The
wrappers run once at 131 072 atoms from a shuffled receptor against the raw calls."""
import time

import numpy as np
import pytest
import torch

import flex_cases as FC
import flex_pose_ref as FR
import interactions_ref as IR
import large_receptor_cases as LC
import pocket_ref as PR
import pose_optimise_ref as PO
import relief_ref as RR
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import interactions as IX
from ml_conformer_generator_amd import pocket as PK
from ml_conformer_generator_amd import receptor as RC
from test_pocket_gpu import MAX_LEFT_OUT, eps_for
from test_receptor_gpu import _restate

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 96
WALKED = LC.cases(LC.WALKED)
WORST = {}                                        # (entry, R) -> the worst error / bound at factor 1, printed as it grows
_DEVICE = {}
_STARTED = time.time()


def _ids(cases):
    return [f"{R}-{kind}" for R, kind in cases]


def _on_device(R):
    """The receptor's arrays on the device, uploaded once."""
    if R not in _DEVICE:
        rec = LC.receptor(R)
        _DEVICE[R] = {k: getattr(rec, k).to(DEV).contiguous() for k in ("ix", "ix_types", "ix_spheres", "vdw", "vdw_spheres")}
    return _DEVICE[R]


def _guarded(sizes, dtype=torch.float32, fill=-777.0):
    bufs = [torch.full((k + 2 * GUARD,), fill, dtype=dtype, device=DEV) for k in sizes]
    return bufs, [b[GUARD: GUARD + k] for b, k in zip(bufs, sizes)]


def _check_guards(bufs, sizes, fill=-777.0):
    torch.cuda.synchronize()
    for buf, k in zip(bufs, sizes):
        host = buf.cpu()
        assert bool((host[:GUARD] == fill).all()) and bool((host[GUARD + k:] == fill).all()), "a write outside the output"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    for k in a:
        if k != "input":
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _note(entry, R, ratio, factor):
    WORST[(entry, R)] = max(WORST.get((entry, R), 0.0), float(ratio))
    print(f"LARGE-GPU {entry} R={R}: worst error / bound at factor 1 so far {WORST[(entry, R)]:.4g} (the stage's factor "
          f"{factor}); {time.time() - _STARTED:.1f} s into the file")


def _ligand(L):
    return tuple(torch.from_numpy(L[k]).to(DEV).contiguous() for k in ("x", "r", "t", "n"))


# ----------------------------------------------------------------------------------------------- the raw calls
def _interactions(R, L, skip_tiles, rot=LC.N_ROT):
    d = _on_device(R)
    x, r, t, n = _ligand(L)
    B, W = x.shape[:2]
    rot = torch.tensor(rot, dtype=torch.int32, device=DEV)
    fsz, isz = (B * W * 6, B * 8), (B,)
    fb, fv = _guarded(fsz)
    ib, iv = _guarded(isz, torch.int32, -777)
    _lib.check(_lib.lib().mcg_receptor_interactions(
        _lib.dptr(x), _lib.dptr(r), _lib.dptr(t), _lib.dptr(n), _lib.dptr(rot), B, W, _lib.dptr(d["ix"]), _lib.dptr(d["ix_types"]),
        R, _lib.dptr(d["ix_spheres"] if skip_tiles else None), fv[0].data_ptr(), fv[1].data_ptr(), iv[0].data_ptr(),
        _lib.current_stream_ptr(DEV)), "mcg_receptor_interactions")
    _check_guards(fb, fsz)
    _check_guards(ib, isz, -777)
    return dict(atom_terms=fv[0].cpu().reshape(B, W, 6), mol_terms=fv[1].cpu().reshape(B, 8), hbonds=iv[0].cpu())


def _optimise(R, L, skip_tiles, steps=LC.STEPS):
    d = _on_device(R)
    x, r, t, n = _ligand(L)
    B, W = x.shape[:2]
    sizes = (B * W * 3, B * 12, B * 8, B * 6, B * steps * 24)
    bufs, v = _guarded(sizes)
    _lib.check(_lib.lib().mcg_receptor_optimise(
        _lib.dptr(x), _lib.dptr(r), _lib.dptr(t), _lib.dptr(n), B, W, _lib.dptr(d["ix"]), _lib.dptr(d["ix_types"]), R,
        _lib.dptr(d["ix_spheres"] if skip_tiles else None), steps, float(LC.MAX_SHIFT), *(u.data_ptr() for u in v),
        _lib.current_stream_ptr(DEV)), "mcg_receptor_optimise")
    _check_guards(bufs, sizes)
    shapes = ((B, W, 3), (B, 12), (B, 8), (B, 6), (B, steps, 24))
    return {k: u.cpu().reshape(s) for k, u, s in zip(("coords", "xform", "stats", "gradient", "trace"), v, shapes)}


def _flex(R, L, skip_tiles, steps=LC.STEPS):
    d = _on_device(R)
    x, r, t, n = _ligand(L)
    B, W = x.shape[:2]
    graphs = [row.graph for row, _, _ in L["rows"]]
    z, bonds, nn, _ = FC.padded(graphs, W)
    cl = np.full((B, W), 1.3, dtype=np.float32)
    for b, g in enumerate(graphs):
        cl[b, : g.n] = FR.clash_radii(g.z)
    cl = L.get("clash", cl)
    tree = IX.torsion_tree(torch.from_numpy(z), torch.from_numpy(bonds), torch.from_numpy(nn), DEV)
    used = tree["counts"][:, 1].contiguous()
    cd = torch.from_numpy(cl).to(DEV)
    T = FR.MAX_TORSIONS
    sizes = (B * W * 3, B * 12, B * 12, B * T, B * 22, B * steps * 43)
    bufs, v = _guarded(sizes)
    _lib.check(_lib.lib().mcg_receptor_optimise_flex(
        _lib.dptr(x), _lib.dptr(r), _lib.dptr(t), _lib.dptr(n), B, W, _lib.dptr(d["ix"]), _lib.dptr(d["ix_types"]), R,
        _lib.dptr(d["ix_spheres"] if skip_tiles else None), steps, float(LC.MAX_SHIFT), _lib.dptr(cd),
        _lib.dptr(tree["torsion_atoms"]), _lib.dptr(tree["side_mask"]), _lib.dptr(tree["near_mask"]), _lib.dptr(used),
        *(u.data_ptr() for u in v), _lib.current_stream_ptr(DEV)), "mcg_receptor_optimise_flex")
    _check_guards(bufs, sizes)
    shapes = ((B, W, 3), (B, 12), (B, 12), (B, T), (B, 22), (B, steps, 43))
    return {k: u.cpu().reshape(s) for k, u, s in zip(("coords", "xform", "stats", "angles", "gradient", "trace"), v, shapes)}


def _relieve(R, L, skip_tiles, steps=LC.STEPS):
    d = _on_device(R)
    x, r, _, n = _ligand(L)
    B, W = x.shape[:2]
    sizes = (B * W * 3, B * 12, B * 4, B * 6)
    bufs, v = _guarded(sizes)
    _lib.check(_lib.lib().mcg_receptor_relieve(
        _lib.dptr(x), _lib.dptr(r), _lib.dptr(n), B, W, _lib.dptr(d["vdw"]), R, _lib.dptr(d["vdw_spheres"] if skip_tiles else None),
        steps, RC.RELIEF_MARGIN, float(LC.MAX_SHIFT), *(u.data_ptr() for u in v), _lib.current_stream_ptr(DEV)),
        "mcg_receptor_relieve")
    _check_guards(bufs, sizes)
    shapes = ((B, W, 3), (B, 12), (B, 4), (B, 6))
    return {k: u.cpu().reshape(s) for k, u, s in zip(("coords", "xform", "stats", "gradient"), v, shapes)}


def _overlap(rec_xyz, rec_r, x, r, n, splits):
    B, W = x.shape[:2]
    R = int(rec_xyz.shape[0])
    sizes = (B * W, splits * B * W if splits > 1 else 1)
    bufs, v = _guarded(sizes)
    _lib.check(_lib.lib().mcg_receptor_overlap(_lib.dptr(x), _lib.dptr(r), _lib.dptr(n), B, W, _lib.dptr(rec_xyz), _lib.dptr(rec_r),
                                               R, splits, v[1].data_ptr() if splits > 1 else None, v[0].data_ptr(),
                                               _lib.current_stream_ptr(DEV)), "mcg_receptor_overlap")
    _check_guards(bufs, sizes)
    return v[0].cpu().reshape(B, W)


def _masks(xyzr, spheres, splits):
    P = LC.GRID_N ** 3
    bufs, v = _guarded((P,), torch.int32, 0x5B5B5B5B)
    rec = xyzr.to(DEV).contiguous()
    _lib.check(_lib.lib().mcg_pocket_masks(_lib.dptr(rec), int(rec.shape[0]), _lib.dptr(None if spheres is None else spheres.to(DEV)),
                                           LC.GRID_N, float(LC.GRID_SPACING), LC.GRID_PROBE, float(LC.GRID_REACH), splits,
                                           v[0].data_ptr(), _lib.current_stream_ptr(DEV)), "mcg_pocket_masks")
    _check_guards(bufs, (P,), 0x5B5B5B5B)
    return v[0].cpu().numpy().view(np.uint32).copy()


def _real(L):
    return [b for b, (row, _, _) in enumerate(L["rows"]) if row.n]


# ----------------------------------------------------------------------------------------------- the scoring entry
@pytest.mark.parametrize("R, kind", LC.cases(), ids=_ids(LC.cases()))
def test_interactions(R, kind):
    L = LC.launch(R, kind, "interactions")
    on, off = _interactions(R, L, True), _interactions(R, L, False)
    _same(on, off, "every tile walked")
    for b in _real(L):
        n = L["rows"][b][0].n
        a, m = on["atom_terms"][b].double().numpy(), on["mol_terms"][b].double().numpy()
        got = dict(atom_terms=a[:n, :5], atom_scores=a[:n, 5], terms=m[:5], weighted=m[5], score=m[6], hbonds=int(on["hbonds"][b]))
        keep, _ = LC.row_list(R, kind, "interactions", b)
        ratios = IR.check(got, *LC.score_args(R, kind, b), what=f"{R} {kind} row {b}, tiles kept {LC.rounds(keep)}")
        _note("interactions", R, max(ratios.values()), IR.FACTOR)
        assert not on["atom_terms"][b, n:].any() and float(on["mol_terms"][b, 7]) == 0.0
        assert got["terms"][1] > 0                                                       # pairs were counted at all
    assert not on["atom_terms"][1].any() and not on["mol_terms"][1].any() and int(on["hbonds"][1]) == 0    # the empty row


# ----------------------------------------------------------------------------------------------- the three walks
def _empty_row_is_left_alone(out, b=1):
    for k in ("xform", "stats", "gradient"):
        assert bool(torch.isnan(out[k][b]).all()), k
    assert not out["coords"][b].any() and ("trace" not in out or not out["trace"][b].any())


@pytest.mark.parametrize("R, kind", WALKED, ids=_ids(WALKED))
def test_optimise(R, kind):
    L = LC.launch(R, kind, "optimise")
    on, off = _optimise(R, L, True), _optimise(R, L, False)
    _same(on, off, "every tile walked")
    for b in _real(L):
        row, x, _ = L["rows"][b]
        ratios = {}
        bad, end = PO.check_trace(on["trace"][b].numpy(), x, *LC.score_args(R, kind, b, name="optimise")[1:6], LC.STEPS,
                                  LC.MAX_SHIFT, stats=on["stats"][b].numpy(), coords=on["coords"][b].numpy(), ratios=ratios)
        print(f"LARGE-GPU optimise {R} {kind} row {b}: W {float(on['stats'][b, 0]):.6f} -> {float(on['stats'][b, 1]):.6f}, "
              f"{end['trials']} trials, {end['kept']} kept; err/bound(factor 1) {({k: round(v, 4) for k, v in ratios.items()})}")
        assert bad == [], bad[:5]
        assert end["trials"] == LC.STEPS and not on["coords"][b, row.n:].any()
        assert torch.equal(_bits(on["gradient"][b]), _bits(on["trace"][b, 0, :6]))
        _note("optimise", R, max(ratios["force"], ratios["torque"]), PO.FORCE_FACTOR)
        _note("optimise W", R, ratios["weighted"], IR.FACTOR)
    _empty_row_is_left_alone(on)


@pytest.mark.parametrize("R, kind", WALKED, ids=_ids(WALKED))
def test_optimise_flex(R, kind):
    L = LC.launch(R, kind, "flex")
    on, off = _flex(R, L, True), _flex(R, L, False)
    _same(on, off, "every tile walked")
    for b in _real(L):
        row, x, _ = L["rows"][b]
        g = row.graph
        ratios = {}
        rec = LC.receptor_args(R, "flex", LC.subset(R, kind, "flex", b))
        bad, end = FR.check_trace(on["trace"][b].numpy(), x, (IR.radii(row.z), row.t), rec, g.z, g.bonds, LC.STEPS, LC.MAX_SHIFT,
                                  stats=on["stats"][b].numpy(), coords=on["coords"][b].numpy(), angles=on["angles"][b].numpy(),
                                  ratios=ratios)
        print(f"LARGE-GPU flex {R} {kind} row {b} ({g.name}): W {float(on['stats'][b, 0]):.6f} -> {float(on['stats'][b, 1]):.6f}, "
              f"{end['trials']} trials, {end['kept']} kept, {end['twisted']} with a turn; err/bound(factor 1) "
              f"{({k: round(v, 5) for k, v in ratios.items()})} FLEX_FACTORS {FR.FLEX_FACTORS}")
        assert bad == [], bad[:5]
        assert end["trials"] == LC.STEPS and int(on["stats"][b, 8]) == len(g.torsions)
        for k in ("force", "torque", "tau", "clash"):
            _note(f"flex {k}", R, ratios[k], FR.FLEX_FACTORS[k])
    _empty_row_is_left_alone(on)
    assert not on["angles"][1].isfinite().any()


@pytest.mark.parametrize("R, kind", WALKED, ids=_ids(WALKED))
def test_relieve(R, kind):
    L = LC.launch(R, kind, "relief")
    on, off = _relieve(R, L, True), _relieve(R, L, False)
    _same(on, off, "every tile walked")
    for b in _real(L):
        row, x, _ = L["rows"][b]
        ri = LC.ligand_radii("relief", row)
        y, rj, _ = LC.receptor_args(R, "relief", LC.subset(R, kind, "relief", b))
        start = np.concatenate([on["stats"][b, :1].numpy(), on["gradient"][b].numpy()])
        err, bound = RR.check(start, x, ri, y, rj, f"{R} {kind} row {b} start")
        moved = on["coords"][b, : row.n].numpy()
        err2, bound2 = RR.check(on["stats"][b, 1:2].numpy(), moved, ri, y, rj, f"{R} {kind} row {b} after {LC.STEPS} trials")
        ratio = max(float(np.max(err / np.where(bound > 0, bound, np.inf))), float(err2[0] / bound2[0]) if bound2[0] > 0 else 0.0)
        _note("relieve", R, ratio, 1.0)
        assert float(on["stats"][b, 1]) <= float(on["stats"][b, 0])
        assert not on["coords"][b, row.n:].any()
        if int(on["stats"][b, 2]) == 0:
            assert torch.equal(_bits(on["coords"][b, : row.n]), _bits(torch.from_numpy(x)))
    assert any(int(on["stats"][b, 2]) > 0 for b in _real(L))                            # a trial was kept: the walk walked
    _empty_row_is_left_alone(on)


# ----------------------------------------------------------------------------------------------- the pocket grid
@pytest.mark.parametrize("R, kind", LC.GRIDS, ids=_ids(LC.GRIDS))
def test_pocket_masks(R, kind):
    xyzr, spheres = LC.receptor(R).recentred(LC.grid_place(R, kind))
    want, margin = PR.masks(*LC.grid_subset(R, kind), LC.GRID_N, LC.GRID_SPACING, LC.GRID_PROBE, LC.GRID_REACH)
    eps = eps_for(max(LC.GRID_SPACING * (LC.GRID_N // 2), 1.0), LC.GRID_REACH)
    keep, _ = LC.grid_lists(R, kind)
    first = None
    for splits in (1, 2, PK.default_splits(LC.GRID_N, R), PK.MAX_SPLITS):
        got = _masks(xyzr, spheres, splits)
        wrong, left_out = PR.compare(got, want, margin, eps)
        print(f"LARGE-GPU pocket {R} {kind} splits={splits}: eps {eps:.2e}, left out {100 * left_out:.4f} % of pairs, "
              f"{int(PR.differing_pairs(got, want).sum())} pairs differ at all, {wrong} beyond eps; tiles kept per brick "
              f"{list(zip(*(v.tolist() for v in LC.rounds(keep))))}; {time.time() - _STARTED:.1f} s into the file")
        assert left_out <= MAX_LEFT_OUT and wrong == 0
        assert int((got & ~(PK.RAY_BITS | PK.OCCUPIED)).sum()) == 0
        first = got if first is None else first
        assert np.array_equal(got, first), "the split count changed a bit"
    assert np.array_equal(_masks(xyzr, None, 2), first), "tile skipping changed a bit"


# ----------------------------------------------------------------------------------------------- the split walk
def _spread_rows(R):
    """The relief's rows at two sites far apart, so that the maxima come from different ends of the receptor."""
    kinds = ("LO_ONLY", "HI_ONLY") if R == 131072 else ("LO_ONLY", "SEAM")
    rows = LC.entries()["relief"].rows
    x = np.full((3, LC.WIDTH, 3), 7.5, dtype=np.float32)
    z = np.full((3, LC.WIDTH), 8, dtype=np.int64)
    for b, kind in ((0, kinds[0]), (2, kinds[1])):
        x[b, : rows[b].n], z[b, : rows[b].n] = rows[b].at(LC.receptor(R).sites[kind]), rows[b].z
    return x, z, np.array([row.n for row in rows], dtype=np.int32)


@pytest.mark.parametrize("R", [131072, 65537])
def test_overlap_by_split(R):
    rec = LC.receptor(R)
    x, z, n = _spread_rows(R)
    want = _restate(x, z, n, rec.xyz.numpy(), rec.z.numpy())                             # the stage's criterion: fp32, bit for bit
    assert np.isfinite(want[0, : n[0]]).all() and np.isneginf(want[1]).all() and want[2, : n[2]].max() > 0
    xd, nd = torch.from_numpy(x).to(DEV), torch.from_numpy(n).to(DEV)
    ri = RC.vdw_radii(torch.from_numpy(z))
    rd = ri.to(DEV).contiguous()
    rec_xyz, rec_r = rec.xyz.to(DEV), RC.vdw_radii(rec.z).to(DEV)
    default = RC.default_splits(3, LC.WIDTH, R)
    assert default == 256 and rec.T > 256
    for splits in (1, 7, 256, default):
        got = _overlap(rec_xyz, rec_r, xd, rd, nd, splits).numpy()
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg=f"R={R} splits={splits}")
    # fp64 brute force: the fp32 value errs by the roundings of its own pair alone - d (3 differences, 3 products, 2 sums,
    # the root: 4 u relative), the radius sum and the difference - at magnitudes of at most 8 A
    exact = np.full(want.shape, -np.inf)
    y, ry = rec.xyz.double().numpy(), RC.vdw_radii(rec.z).double().numpy()
    for b in (0, 2):
        for i in range(int(n[b])):
            exact[b, i] = (float(ri[b, i]) + ry - np.linalg.norm(x[b, i].astype(np.float64) - y, axis=1)).max()
    real = np.isfinite(exact)
    assert (np.abs(want[real] - exact[real]) <= 8 * 2.0 ** -24 * 8.0).all()


# ----------------------------------------------------------------------------------------------- the wrappers, once
def test_wrappers_at_the_limit_from_a_shuffled_receptor():
    R, kind = 131072, "BOTH"
    rec = LC.receptor(R)
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(23))
    pair = (rec.xyz[perm], rec.z[perm])
    # receptor_overlap
    x, z, n = _spread_rows(R)
    args = (torch.from_numpy(x), torch.from_numpy(n), torch.from_numpy(z))
    raw = _overlap(rec.xyz.to(DEV), RC.vdw_radii(rec.z).to(DEV), args[0].to(DEV),
                   RC.vdw_radii(args[2]).to(DEV).contiguous(), args[1].to(DEV), 256)
    assert torch.equal(_bits(RC.receptor_overlap(pair, *args, DEV).cpu()), _bits(raw))
    # relieve_clashes
    L = LC.launch(R, kind, "relief")
    raw = _relieve(R, L, True)
    z = torch.full((3, LC.WIDTH), 6)
    got = RC.relieve_clashes(pair, torch.from_numpy(L["x"]), torch.from_numpy(L["n"]), z, steps=LC.STEPS,
                             max_shift=LC.MAX_SHIFT, device=DEV, return_gradient=True)
    for b in _real(L):
        k = L["rows"][b][0].n
        assert torch.equal(_bits(got["coords"][b, :k].cpu()), _bits(raw["coords"][b, :k]))
        assert torch.equal(_bits(got["rotation"][b].cpu().reshape(9)), _bits(raw["xform"][b, :9]))
        assert torch.equal(_bits(got["penalty_before"][b].cpu()), _bits(raw["stats"][b, 0]))
        assert torch.equal(_bits(got["penalty_after"][b].cpu()), _bits(raw["stats"][b, 1]))
        assert torch.equal(_bits(got["gradient"][b].cpu()), _bits(raw["gradient"][b]))
    # the graph-taking entries: interaction_scores, optimise_pose, optimise_pose_flexible
    L = LC.launch(R, kind, "flex")
    graphs = [row.graph for row, _, _ in L["rows"]]
    zz, bonds, nn, _ = (torch.from_numpy(v) for v in FC.padded(graphs, LC.WIDTH))
    xx = torch.from_numpy(L["x"])
    prepared = IX.prepare_receptor(pair)
    assert torch.equal(_bits(prepared.xyzr), _bits(rec.ix)) and torch.equal(prepared.types, rec.ix_types)
    assert torch.equal(_bits(prepared.spheres), _bits(rec.ix_spheres))
    scores = {k: v.cpu() for k, v in IX.interaction_scores(pair, xx, nn, zz, bonds, device=DEV).items()}
    typed = dict(L, t=scores["types"].numpy(), r=IX.interaction_radii(zz).numpy())
    raw = _interactions(R, typed, True, rot=tuple(scores["n_rot"].tolist()))
    assert torch.equal(_bits(scores["atom_terms"]), _bits(raw["atom_terms"][:, :, :5]))
    assert torch.equal(_bits(scores["terms"]), _bits(raw["mol_terms"][:, :6]))
    assert torch.equal(_bits(scores["score"]), _bits(raw["mol_terms"][:, 6])) and torch.equal(scores["hbonds"], raw["hbonds"])
    assert scores["types"][0, : graphs[0].n].tolist() == [4] * graphs[0].n              # all carbon: as the cases type them
    rigid = IX.optimise_pose(pair, xx, nn, zz, bonds, steps=LC.STEPS, max_shift=LC.MAX_SHIFT, device=DEV, trace=True)
    raw = _optimise(R, typed, True)
    flexible = IX.optimise_pose_flexible(pair, xx, nn, zz, bonds, steps=LC.STEPS, max_shift=LC.MAX_SHIFT, device=DEV, trace=True)
    raw_flex = _flex(R, dict(typed, clash=IX.clash_radii(zz).numpy()), True)
    for got, want in ((rigid, raw), (flexible, raw_flex)):
        for b in _real(L):
            k = graphs[b].n
            assert torch.equal(_bits(got["coords"][b, :k].cpu()), _bits(want["coords"][b, :k]))
            assert torch.equal(_bits(got["trace"][b].cpu()), _bits(want["trace"][b]))
            assert torch.equal(_bits(got["weighted_after"][b].cpu()), _bits(want["stats"][b, 1]))
    assert flexible["torsions"].cpu().tolist() == [3, -1, 3]
    # ray_masks with the prefilter on and off, and find_pocket
    centre = LC.grid_place(R, kind)
    xyzr, spheres = rec.recentred(centre)
    raw = _masks(xyzr, spheres, PK.default_splits(LC.GRID_N, R))
    for prefilter in (True, False):
        got = PK.ray_masks(pair, centre, radius=4.0, reach=LC.GRID_REACH, device=DEV, prefilter=prefilter)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), raw), prefilter
    found = PK.find_pocket(pair, centre, radius=4.0, reach=LC.GRID_REACH, device=DEV)
    assert np.array_equal(found.masks, raw) and found.n_centres >= 1
    print(f"LARGE-GPU wrappers: done {time.time() - _STARTED:.1f} s into the file; worst ratios {WORST}")
