"""Flexible pose on the MI355X (`mcg_torsion_tree`, `mcg_receptor_optimise_flex`; DESIGN.md section 6 "Flexible pose"): the
tree against the restatement, exactly; every trial of the walk against the restatement, TEACHER-FORCED through the trace
(`flex_pose_ref.check_trace`); the invariants a torsional walk must keep; and bit identity - with `mcg_receptor_optimise`
for molecules without a torsion, and whatever the batch, row, padded width, tile skipping, receptor order and budget."""
import math

import numpy as np
import pytest
import torch

import flex_cases as FC
import flex_pose_ref as FR
import interactions_ref as IR
import pose_optimise_ref as PR
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import interactions as IX

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GRAPHS = FC.cases()
BY_NAME = FC.by_name()
RECEPTORS = IR.cases()                            # a few hundred to a few thousand atoms
GUARD = 96
SHIFT = 2.0
F32 = np.float32
T = FR.MAX_TORSIONS
_DONE = {}
NAMES = ("coords", "xform", "stats", "angles", "gradient", "trace")
OFFSET = np.array([0.6, -0.3, 0.2])               # out of the middle of the pocket, so that there is a force to follow


def _steps(g):
    return 24 if g.n <= 20 else 8                 # the restatement's rule costs n^2 per row


def _receptor_of(g):
    """Each graph in its own receptor of `interactions_ref.cases()`: 1, 255, 256, 257, 4 097 atoms and the pockets."""
    return RECEPTORS[(2, 4, 5, 6, 7, 8, 3)[sum(map(ord, g.name)) % 7]]


def _typed(g):
    """(coords centred in the pocket [n,3] fp32, radii, types) of a graph: C hydrophobic, N and O donor + acceptor."""
    x = (g.x.astype(np.float64) - (g.x.astype(np.float64).mean(axis=0) if g.n else 0) + OFFSET).astype(F32)
    return x, IR.radii(g.z), np.where(g.z == 6, 4, 3).astype(np.uint8)


def _lig(g):
    x, r, t = _typed(g)
    return r, t


def _rec(c):
    return c.rec, IR.radii(c.rec_z), c.rec_t


def _guarded(sizes, dtype, fill):
    bufs = [torch.full((k + 2 * GUARD,), fill, dtype=dtype, device=DEV) for k in sizes]
    return bufs, [b[GUARD: GUARD + k] for b, k in zip(bufs, sizes)]


def _check_guards(bufs, sizes, fill):
    for buf, k in zip(bufs, sizes):
        host = buf.cpu()
        assert bool((host[:GUARD] == fill).all()) and bool((host[GUARD + k:] == fill).all()), "a write outside the output"


def _tree_launch(graphs, width, junk_seed=5):
    """The C entry on graphs padded to `width` with junk beyond every row, every output inside sentinels; host arrays."""
    z, bonds, n, _ = FC.padded(graphs, width, junk_seed)
    B = len(graphs)
    zd, bd, nd = (torch.from_numpy(v).to(DEV).contiguous() for v in (z, bonds, n))
    isz, lsz = (B * T * 2, B * 2), (B * T, B * width)
    ib, iv = _guarded(isz, torch.int32, -777)
    lb, lv = _guarded(lsz, torch.int64, -777)
    _lib.check(_lib.lib().mcg_torsion_tree(_lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nd), B, width, iv[0].data_ptr(),
                                           lv[0].data_ptr(), lv[1].data_ptr(), iv[1].data_ptr(),
                                           _lib.current_stream_ptr(DEV)), "mcg_torsion_tree")
    torch.cuda.synchronize()
    _check_guards(ib, isz, -777)
    _check_guards(lb, lsz, -777)
    return dict(torsion_atoms=iv[0].cpu().reshape(B, T, 2), side_mask=lv[0].cpu().reshape(B, T),
                near_mask=lv[1].cpu().reshape(B, width), counts=iv[1].cpu().reshape(B, 2))


def _want_tree(g, width):
    atoms, side, near, counts = FR.tree_arrays(FR.tree(g.z, g.bonds, g.n), g.n, width)
    return atoms, side.view(np.int64), near.view(np.int64), counts


def _launch(graphs, width, case, steps, max_shift=SHIFT, skip_tiles=True, coords=None, receptor=None, edit_tree=None):
    """`mcg_receptor_optimise_flex` itself on graphs against one receptor, every output inside sentinels; host tensors.
    The tree is `interactions.torsion_tree`'s (held to the restatement by the tree tests), after `edit_tree(tree)`."""
    prepared = IX.prepare_receptor(receptor if receptor is not None else case.receptor)
    B = len(graphs)
    z, bonds, n, _ = FC.padded(graphs, width)
    x = np.full((B, width, 3), 7.5, dtype=F32)
    r = np.full((B, width), 1.9, dtype=F32)
    t = np.full((B, width), 7, dtype=np.uint8)
    cl = np.full((B, width), 1.3, dtype=F32)
    for b, g in enumerate(graphs):
        x[b, : g.n], r[b, : g.n], t[b, : g.n] = _typed(g)
        cl[b, : g.n] = FR.clash_radii(g.z)
        if coords is not None and coords[b] is not None:
            x[b, : g.n] = coords[b]
    tree = IX.torsion_tree(torch.from_numpy(z), torch.from_numpy(bonds), torch.from_numpy(n), DEV)
    if edit_tree is not None:
        edit_tree(tree)
    xd, rd, td, cd, nd = (torch.from_numpy(v).to(DEV).contiguous() for v in (x, r, t, cl, n))
    rec, rec_t = prepared.xyzr.to(DEV), prepared.types.to(DEV)
    spheres = prepared.spheres.to(DEV) if skip_tiles else None
    sizes = (B * width * 3, B * 12, B * 12, B * T, B * 22, B * steps * 43)
    bufs, views = _guarded(sizes, torch.float32, -777.0)
    used = tree["counts"][:, 1].contiguous()
    _lib.check(_lib.lib().mcg_receptor_optimise_flex(
        _lib.dptr(xd), _lib.dptr(rd), _lib.dptr(td), _lib.dptr(nd), B, width, _lib.dptr(rec), _lib.dptr(rec_t),
        int(rec.shape[0]), _lib.dptr(spheres), steps, float(max_shift), _lib.dptr(cd), _lib.dptr(tree["torsion_atoms"]),
        _lib.dptr(tree["side_mask"]), _lib.dptr(tree["near_mask"]), _lib.dptr(used), *(v.data_ptr() for v in views),
        _lib.current_stream_ptr(DEV)), "mcg_receptor_optimise_flex")
    torch.cuda.synchronize()
    _check_guards(bufs, sizes, -777.0)
    shapes = ((B, width, 3), (B, 12), (B, 12), (B, T), (B, 22), (B, steps, 43))
    out = {name: v.cpu().reshape(shape) for name, v, shape in zip(NAMES, views, shapes)}
    out["input"] = torch.from_numpy(x)
    return out


def _rigid(graphs, width, case, steps, skip_tiles=True, receptor=None):
    """`mcg_receptor_optimise` on the same rows: host tensors coords, xform, stats, gradient, trace."""
    B = len(graphs)
    x = np.full((B, width, 3), 7.5, dtype=F32)
    r = np.full((B, width), 1.9, dtype=F32)
    t = np.full((B, width), 7, dtype=np.uint8)
    for b, g in enumerate(graphs):
        x[b, : g.n], r[b, : g.n], t[b, : g.n] = _typed(g)
    n = torch.tensor([g.n for g in graphs], dtype=torch.int32)
    out = IX.optimise_typed(receptor if receptor is not None else case.receptor, torch.from_numpy(x), n, torch.from_numpy(r),
                            torch.from_numpy(t), steps, SHIFT, skip_tiles, DEV, trace=True)
    return {k: v.cpu() for k, v in out.items()}


def _one(g, steps=None, width=None, skip_tiles=True):
    steps = _steps(g) if steps is None else steps
    key = (g.name, steps, width, skip_tiles)
    if key not in _DONE:
        _DONE[key] = _launch([g], width or max(g.n, 1), _receptor_of(g), steps, skip_tiles=skip_tiles)
    return _DONE[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, n, what, row_a=0, row_b=0, steps=None):
    assert torch.equal(_bits(a["coords"][row_a, :n]), _bits(b["coords"][row_b, :n])), what
    for k in ("xform", "stats", "angles", "gradient"):
        assert torch.equal(_bits(a[k][row_a]), _bits(b[k][row_b])), (what, k)
    assert torch.equal(_bits(a["trace"][row_a, :steps]), _bits(b["trace"][row_b, :steps])), (what, "trace")


def _score(g, coords, case):
    """`mcg_receptor_interactions`' mol_terms of one molecule at `coords` [n,3]."""
    x, r, t = _typed(g)
    out = IX.score_typed(case.receptor, coords.reshape(1, g.n, 3), torch.tensor([g.n], dtype=torch.int32),
                         torch.from_numpy(r).reshape(1, g.n), torch.from_numpy(t).reshape(1, g.n),
                         torch.zeros(1, dtype=torch.int32), device=DEV)
    return out["mol_terms"].cpu()[0]


# ----------------------------------------------------------------------------------------------- the tree
@pytest.mark.parametrize("width", ["n", 41, 64])
def test_tree_equals_the_restatement(width):
    for g in GRAPHS + FC.stereo_cases():
        W = max(g.n, 1) if width == "n" else width
        if g.n > W:
            continue
        got = _tree_launch([g], W)
        atoms, side, near, counts = _want_tree(g, W)
        assert got["counts"][0].tolist() == counts.tolist() == [g.found, len(g.torsions)], g.name
        assert np.array_equal(got["torsion_atoms"][0].numpy(), atoms), g.name
        assert got["torsion_atoms"][0, : len(g.torsions)].tolist() == [list(t) for t in g.torsions], g.name
        assert np.array_equal(got["side_mask"][0].numpy(), side), g.name
        assert np.array_equal(got["near_mask"][0].numpy(), near), g.name


def test_tree_at_rows_0_37_69_of_a_batch_of_70():
    pool = [g for g in GRAPHS if g.n <= 41]
    batch = [pool[(3 * k) % len(pool)] for k in range(70)]
    got = _tree_launch(batch, 41, junk_seed=9)
    for row in (0, 37, 69):
        alone = _tree_launch([batch[row]], 41, junk_seed=10)
        for k in ("torsion_atoms", "side_mask", "near_mask", "counts"):
            assert torch.equal(got[k][row], alone[k][0]), (row, k)
    for row, g in enumerate(batch):
        atoms, side, near, counts = _want_tree(g, 41)
        assert np.array_equal(got["torsion_atoms"][row].numpy(), atoms) and np.array_equal(got["side_mask"][row].numpy(), side)
        assert np.array_equal(got["near_mask"][row].numpy(), near) and got["counts"][row].tolist() == counts.tolist()


def test_torsion_tree_through_the_module():
    z, bonds, n, _ = FC.padded(GRAPHS, 64)
    out = IX.torsion_tree(torch.from_numpy(z), torch.from_numpy(bonds), torch.from_numpy(n), DEV)
    assert out["counts"].cpu().tolist() == [[g.found, len(g.torsions)] for g in GRAPHS]
    empty = IX.torsion_tree(torch.from_numpy(z[:0]), torch.from_numpy(bonds[:0]), torch.from_numpy(n[:0]), DEV)
    assert tuple(empty["torsion_atoms"].shape) == (0, 16, 2)


# ----------------------------------------------------------------------------------------------- the walk
WALKED = [g for g in GRAPHS if g.n >= 1]
RATIOS = {}


@pytest.mark.parametrize("g", WALKED, ids=lambda g: g.name)
def test_every_trial_matches_the_restatement_teacher_forced(g):
    case, steps = _receptor_of(g), _steps(g)
    out = _one(g)
    x, r, t = _typed(g)
    ratios = {}
    bad, end = FR.check_trace(out["trace"][0].numpy(), x, (r, t), _rec(case), g.z, g.bonds, steps, SHIFT,
                              stats=out["stats"][0].numpy(), coords=out["coords"][0].numpy(),
                              angles=out["angles"][0].numpy(), ratios=ratios)
    stats = out["stats"][0]
    for k, v in ratios.items():
        RATIOS[k] = max(RATIOS.get(k, 0.0), v)
    print(f"FLEX {g.name} in {case}: W {float(stats[0]):.6f} -> {float(stats[1]):.6f}, CLASH {float(stats[6]):.6f} -> "
          f"{float(stats[7]):.6f} in {int(stats[2])} trials, {int(stats[3])} kept ({end['twisted']} with a turn), rmsd "
          f"{float(stats[4]):.4f}, conformer {float(stats[9]):.4f}, angles {out['angles'][0, : end['tree']['used']].tolist()}; "
          f"err/bound(factor 1) {({k: round(v, 5) for k, v in ratios.items()})} so far {({k: round(v, 5) for k, v in RATIOS.items()})} "
          f"FLEX_FACTORS {FR.FLEX_FACTORS}")
    assert bad == [], bad[:5]
    n = g.n
    assert not out["coords"][0, n:].any()
    # W before / after: the bits of mcg_receptor_interactions at the input / returned coordinates
    assert _bits(_score(g, out["input"][0, :n], case)[5:6]).tolist() == _bits(stats[0:1]).tolist()
    assert _bits(_score(g, out["coords"][0, :n], case)[5:6]).tolist() == _bits(stats[1:2]).tolist()
    # CLASH before / after against the restatement, from the coordinates themselves
    tree = end["tree"]
    cr = FR.clash_radii(g.z)
    for col, pts in ((6, out["input"][0, :n]), (7, out["coords"][0, :n])):
        want, _, pairs = FR.clash(pts.double().numpy(), cr, tree["near"])
        eps = 8 * FR.U * (float(pts.abs().max()) + 1.0)                            # the coordinates' own rounding
        bound = sum(6 * FR.U * e * e + 2 * e * (FR.U * (e + 2 * rr) + 2 * eps) for _, _, e, rr in pairs) + \
            (len(pairs) + 8) * FR.U * want + 64 * eps * eps
        assert abs(float(stats[col]) - want) <= bound + FR.drift_bound(x, tree, end["twisted"]) * 4 * math.sqrt(max(want, 0)), \
            (col, float(stats[col]), want)
    # the total never rises, and falls strictly when a trial was kept
    before, after = float(stats[0]) + FR.W_REP * float(stats[6]), float(stats[1]) + FR.W_REP * float(stats[7])
    assert after < before if stats[3] > 0 else after == before
    # the summed angles against the dihedral change of the coordinates (mod 2 pi): an end atom at least 1 A off the axis,
    # four atoms, each off by the drift rule and its own rounding
    nb = [[j for j in range(n) if g.bonds[i, j]] for i in range(n)]
    tol = 4 * (FR.drift_bound(x, tree, end["kept"]) + 8 * FR.U * (np.abs(x).max() + 1)) / 1.0 + end["kept"] * FR.U * math.pi
    for k, (a, b) in enumerate(tree["torsions"]):
        i, l = [v for v in nb[a] if v != b][0], [v for v in nb[b] if v != a][0]
        turn = FR.dihedral(out["coords"][0].double().numpy(), i, a, b, l) - FR.dihedral(x, i, a, b, l)
        diff = (turn - float(out["angles"][0, k]) + math.pi) % (2 * math.pi) - math.pi
        assert abs(diff) <= tol, (k, turn, float(out["angles"][0, k]), tol)


def _pieces(tree, n):
    sig = [tuple(i in s for s in tree["sides"]) for i in range(n)]
    return sig


@pytest.mark.parametrize("g", WALKED + FC.stereo_cases(), ids=lambda g: g.name)
def test_the_walk_keeps_what_a_torsional_walk_must_keep(g):
    out = _one(g, steps=1024)                                                   # the largest budget: the most kept trials
    x, _, _ = _typed(g)
    n = g.n
    tree = FR.tree(g.z, g.bonds, n)
    kept = int(out["stats"][0, 3])
    got = out["coords"][0, :n].double().numpy()
    d0 = np.linalg.norm(x.astype(np.float64)[:, None] - x.astype(np.float64)[None], axis=2)
    d1 = np.linalg.norm(got[:, None] - got[None], axis=2)
    sig = _pieces(tree, n)
    worst = 0.0
    bound1 = 2 * FR.drift_bound(x, tree, kept, factor=1.0)
    for i in range(n):
        for j in range(i + 1, n):
            if j in tree["near"][i] or sig[i] == sig[j]:                        # bonded, 1-3, or one rigid piece
                worst = max(worst, abs(d1[i, j] - d0[i, j]))
    print(f"FLEX-DRIFT {g.name}: worst kept distance moved {worst:.3e} A after {kept} kept trials; bound(factor 1) "
          f"{bound1:.3e}, ratio {worst / bound1 if bound1 else 0:.4f}, DRIFT_FACTOR {FR.DRIFT_FACTOR}")
    assert worst <= 2 * FR.drift_bound(x, tree, kept)
    # atoms outside every moving side: x' = (x - c) @ G + p
    xf = out["xform"][0].double().numpy()
    Rm, t = xf[:9].reshape(3, 3), xf[9:]
    fixed = [i for i in range(n) if not any(sig[i])]
    if fixed:
        want = x.astype(np.float64)[fixed] @ Rm + t
        centre = PR.centroid(x).astype(np.float64)
        bound = 8 * FR.U * (np.abs(x.astype(np.float64)[fixed]).sum(axis=1, keepdims=True) + 2 * np.abs(centre).sum() + SHIFT + 1.0)
        assert (np.abs(got[fixed] - want) <= bound).all(), np.abs(got[fixed] - want).max()
    assert (np.abs(Rm @ Rm.T - np.eye(3)) <= PR.ORTHO).all() and np.linalg.det(Rm) > 0


def test_stereo_identity_survives_the_walk():
    from ml_conformer_generator_amd import stereo
    for g in FC.stereo_cases():
        out = _one(g)
        assert int(out["stats"][0, 3]) > 0 and out["angles"][0].abs().max() > 0, g.name       # it did turn
        z, bonds, n, _ = FC.padded([g])
        args = (torch.from_numpy(z), torch.from_numpy(bonds), torch.from_numpy(n))
        before = stereo.stereo_identity_bytes(out["input"][:, : g.n], *args, device=DEV)
        after = stereo.stereo_identity_bytes(out["coords"][:, : g.n], *args, device=DEV)
        assert before == after and before[0] is not None, g.name


def test_torsions_turn_and_end_lower_than_the_rigid_walk():
    better = []
    for g in WALKED:
        if not g.torsions:
            continue
        case, steps = _receptor_of(g), _steps(g)
        flex = _one(g)
        rigid = _rigid([g], max(g.n, 1), case, steps)
        c0 = float(flex["stats"][0, 6])
        total_flex = float(flex["stats"][0, 1]) + FR.W_REP * float(flex["stats"][0, 7])
        total_rigid = float(rigid["stats"][0, 1]) + FR.W_REP * c0               # a rigid walk leaves CLASH where it was
        if float(flex["angles"][0].abs().max()) > 0 and total_flex < total_rigid:
            better.append(g.name)
        print(f"FLEX-VS-RIGID {g.name}: flexible {total_flex:.5f}, rigid {total_rigid:.5f}")
    assert len(better) >= 3, better


# ----------------------------------------------------------------------------------------------- bit identity
RIGID_NAMES = ("toluene", "benzene", "n_methylacetamide", "ring12", "stacked_benzenes", "one_atom")


@pytest.mark.parametrize("name", RIGID_NAMES)
def test_a_molecule_without_a_torsion_walks_as_the_rigid_entry_walks_it(name):
    g = BY_NAME[name]
    case = _receptor_of(g)
    flex = _one(g, steps=64)
    rigid = _rigid([g], max(g.n, 1), case, 64)
    assert int(flex["stats"][0, 8]) == 0
    assert torch.equal(_bits(flex["coords"]), _bits(rigid["coords"]))
    assert torch.equal(_bits(flex["xform"]), _bits(rigid["xform"]))
    assert torch.equal(_bits(flex["stats"][:, :6]), _bits(rigid["stats"][:, :6]))            # W, W', trials, kept, rmsd, s_t
    assert torch.equal(_bits(flex["gradient"][:, :6]), _bits(rigid["gradient"]))
    assert torch.equal(_bits(flex["trace"][:, :, :24]), _bits(rigid["trace"]))
    assert not flex["angles"].any() and not flex["gradient"][:, 6:].any() and float(flex["stats"][0, 9]) == 0
    assert torch.equal(_bits(flex["stats"][:, 6]), _bits(flex["stats"][:, 7]))               # CLASH kept its bits
    assert int(flex["stats"][0, 3]) > 0 or name == "one_atom"
    assert float(flex["stats"][0, 6]) > 0 or name != "stacked_benzenes"


def _walked_as_rigid(flex, rigid, n, what, row_f=0, row_r=0):
    """The fields `test_a_molecule_without_a_torsion_walks_as_the_rigid_entry_walks_it` compares, trace included."""
    assert int(flex["stats"][row_f, 8]) == 0, what
    assert torch.equal(_bits(flex["coords"][row_f, :n]), _bits(rigid["coords"][row_r, :n])), what
    assert torch.equal(_bits(flex["xform"][row_f]), _bits(rigid["xform"][row_r])), what
    assert torch.equal(_bits(flex["stats"][row_f, :6]), _bits(rigid["stats"][row_r, :6])), what
    assert torch.equal(_bits(flex["gradient"][row_f, :6]), _bits(rigid["gradient"][row_r])), what
    assert torch.equal(_bits(flex["trace"][row_f, :, :24]), _bits(rigid["trace"][row_r])), what
    assert not flex["angles"][row_f].any() and not flex["gradient"][row_f, 6:].any() and float(flex["stats"][row_f, 9]) == 0
    assert torch.equal(_bits(flex["stats"][row_f, 6]), _bits(flex["stats"][row_f, 7])), what      # CLASH kept its bits


@pytest.mark.parametrize("cut", ["n_torsions_0", "slot_0_names_an_atom_beyond_n"])
def test_a_row_cut_to_no_torsion_walks_as_the_rigid_entry_walks_it(cut):
    """The flexible kernel with a torsion count the kernel's own slot check cuts to 0 at run time, against the rigid
    kernel, where the torsion state is compiled out."""
    g = BY_NAME["isopentylbenzene"]
    case = _receptor_of(g)
    assert len(g.torsions) > 0

    def edit(tree):
        if cut == "n_torsions_0":
            tree["counts"][:, 1] = 0
        else:
            tree["torsion_atoms"][:, 0, 1] = g.n

    flex = _launch([g], g.n, case, 64, edit_tree=edit)
    rigid = _rigid([g], g.n, case, 64)
    _walked_as_rigid(flex, rigid, g.n, cut)
    assert int(flex["stats"][0, 3]) > 0


def test_a_batch_of_a_flexible_a_rigid_and_an_empty_row():
    """Nothing of a row's torsion state reaches the next row through the shared LDS struct."""
    case, steps = RECEPTORS[2], 12
    hexane, toluene = BY_NAME["hexane"], BY_NAME["toluene"]
    batch = _launch([hexane, toluene, BY_NAME["empty"]], 41, case, steps)
    for row, g in ((0, hexane), (1, toluene)):
        _same(batch, _launch([g], 41, case, steps), g.n, ("batch of three", g.name), row, 0, steps)
    _walked_as_rigid(batch, _rigid([toluene], 41, case, steps), toluene.n, "toluene beside hexane", 1, 0)
    assert int(batch["stats"][0, 8]) == len(hexane.torsions) > 0 and bool(torch.isnan(batch["stats"][2]).all())


def test_bits_do_not_depend_on_batch_row_width_or_tiles():
    case = RECEPTORS[2]
    pool = [BY_NAME[k] for k in ("hexane", "isopentylbenzene", "biphenyl", "toluene", "folded_heptane", "butane")]
    steps = 12
    alone = {g.name: _launch([g], max(g.n, 1), case, steps) for g in pool}
    batch = _launch(pool, 41, case, steps)
    wide = _launch(pool[::-1], 64, case, steps, skip_tiles=False)
    for row, g in enumerate(pool):
        _same(batch, alone[g.name], g.n, ("batch", g.name), row, 0, steps)
        _same(wide, alone[g.name], g.n, ("wide, no tiles", g.name), len(pool) - 1 - row, 0, steps)
    assert any(int(alone[g.name]["stats"][0, 3]) > 0 and float(alone[g.name]["angles"].abs().max()) > 0 for g in pool)
    # the receptor's atoms listed in another order
    perm = np.random.default_rng(3).permutation(len(case.rec))
    shuffled = (torch.from_numpy(case.rec[perm]), torch.from_numpy(case.rec_z[perm]), torch.from_numpy(case.rec_t[perm]))
    again = _launch(pool, 41, case, steps, receptor=shuffled)
    for row, g in enumerate(pool):
        _same(again, batch, g.n, ("shuffled receptor", g.name), row, row, steps)


def test_a_smaller_budget_is_a_prefix():
    g, case = BY_NAME["isopentylbenzene"], RECEPTORS[2]
    full = _launch([g], g.n, case, 16)
    part = _launch([g], g.n, case, 7)
    assert torch.equal(_bits(part["trace"][0]), _bits(full["trace"][0, :7]))
    assert torch.equal(_bits(part["gradient"]), _bits(full["gradient"]))


def test_empty_and_non_finite_rows_beside_good_ones():
    case = RECEPTORS[2]
    good, other = BY_NAME["hexane"], BY_NAME["butane"]
    graphs = [good, BY_NAME["empty"], other, good, other]
    bad_nan, bad_inf = _typed(good)[0].copy(), _typed(other)[0].copy()
    bad_nan[2, 1] = np.nan
    bad_inf[0, 0] = np.inf
    out = _launch(graphs, 9, case, 10, coords=[None, None, None, bad_nan, bad_inf])
    for row, g in ((0, good), (2, other)):
        _same(out, _launch([g], 9, case, 10), g.n, ("beside bad rows", g.name), row, 0, 10)
    for row in (1, 3, 4):
        for k in ("xform", "stats", "angles", "gradient"):
            assert bool(torch.isnan(out[k][row]).all()), (row, k)
        assert not out["trace"][row].any()
        n = graphs[row].n
        assert torch.equal(_bits(out["coords"][row, :n]), _bits(out["input"][row, :n])) and not out["coords"][row, n:].any()


def test_a_receptor_beyond_the_cut_off():
    g = BY_NAME["hexane"]
    far = IR.Case("far", 31, 27, far=True)
    for skip in (True, False):
        out = _launch([g], g.n, far, 8, skip_tiles=skip)
        assert torch.equal(_bits(out["coords"][0]), _bits(out["input"][0]))
        assert out["xform"][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
        assert out["stats"][0].tolist() == [0, 0, 0, 0, 0, 0.25, 0, 0, 3, 0, 0, 0]          # nothing to follow: no trial
        assert not out["gradient"].any() and not out["trace"].any() and not out["angles"].any()


# ----------------------------------------------------------------------------------------------- the module's own path
def test_optimise_pose_flexible_on_graphs():
    pool = [BY_NAME[k] for k in ("hexane", "isopentylbenzene", "toluene", "folded_heptane")]
    z, bonds, n, _ = FC.padded(pool, 41)
    x = torch.zeros(len(pool), 41, 3)
    for b, g in enumerate(pool):
        x[b, : g.n] = torch.from_numpy(_typed(g)[0])
    rec = RECEPTORS[2].receptor
    args = (rec, x, torch.from_numpy(n), torch.from_numpy(z), torch.from_numpy(bonds))
    out = {k: v.cpu() for k, v in IX.optimise_pose_flexible(*args, steps=16, device=DEV, trace=True).items()}
    assert out["torsions"].tolist() == [len(g.torsions) for g in pool] == out["torsions_found"].tolist()
    assert tuple(out["trace"].shape) == (4, 16, 43) and tuple(out["gradient"].shape) == (4, 22)
    assert tuple(out["torsion_angles"].shape) == (4, 16) and tuple(out["rotation"].shape) == (4, 3, 3)
    scores = IX.interaction_scores(rec, out["coords"], torch.from_numpy(n), torch.from_numpy(z), torch.from_numpy(bonds),
                                   device=DEV)
    assert torch.equal(_bits(scores["terms"][:, 5].cpu()), _bits(out["weighted_after"]))
    rigid = {k: v.cpu() for k, v in IX.optimise_pose(*args, steps=16, device=DEV).items()}
    row = 2                                                                     # toluene: no torsion
    for k in ("coords", "rotation", "translation", "weighted_before", "weighted_after", "rmsd"):
        assert torch.equal(_bits(out[k][row]), _bits(rigid[k][row])), k
    assert out["trials"][row] == rigid["trials"][row] and out["kept"][row] == rigid["kept"][row]
    assert float(out["clash_before"][3]) > 0 and bool(out["moved"].any())
    empty = IX.optimise_pose_flexible(rec, x[:0], torch.from_numpy(n[:0]), torch.from_numpy(z[:0]),
                                      torch.from_numpy(bonds[:0]), device=DEV)
    assert tuple(empty["coords"].shape) == (0, 41, 3) and tuple(empty["torsions"].shape) == (0,)
