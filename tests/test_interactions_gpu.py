"""Receptor interactions on the MI355X (`mcg_receptor_interactions`, DESIGN.md section 6 "Receptor interactions"): the
kernel's sums against the restatement inside the derived rule (`interactions_ref.py`), the hydrogen-bond count exactly;
junk beyond every row and sentinels round every output; bit identity whatever the batch, row, padded width, tile skipping
and receptor order; empty, non-finite and out-of-reach rows; the device typing against the plain-Python rules; and the
options through `generate_conformers` and `generate_conformers_sharded` in a carved pocket."""
import math

import numpy as np
import pytest
import torch

import interactions_cases as K
import interactions_ref as R
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import interactions as IX

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = R.cases()
GUARD = 96                                        # sentinel elements on either side of every output
_DONE = {}


def _pad(case_list, width):
    """The kernel's ligand inputs of cases at padded width `width`, junk beyond every row's atoms."""
    B = len(case_list)
    x = np.full((B, width, 3), 7.5, dtype=np.float32)
    r = np.full((B, width), 1.9, dtype=np.float32)
    t = np.full((B, width), 7, dtype=np.uint8)
    for b, c in enumerate(case_list):
        x[b, : c.n], r[b, : c.n], t[b, : c.n] = c.x, R.radii(c.z), c.t
    return (torch.from_numpy(x), torch.tensor([c.n for c in case_list], dtype=torch.int32), torch.from_numpy(r),
            torch.from_numpy(t), torch.tensor([c.n_rot for c in case_list], dtype=torch.int32))


def _launch(case_list, width, receptor, skip_tiles=True):
    """The C entry itself on cases against one receptor, every output inside a buffer of sentinels; host tensors
    atom_terms [B,width,6], mol_terms [B,8], hbonds [B]."""
    prepared = IX.prepare_receptor(receptor)
    x, n, r, t, rot = (v.to(DEV).contiguous() for v in _pad(case_list, width))
    B = len(case_list)
    rec, rec_t = prepared.xyzr.to(DEV), prepared.types.to(DEV)
    spheres = prepared.spheres.to(DEV) if skip_tiles else None
    sizes = (B * width * 6, B * 8, B)
    atoms = torch.full((sizes[0] + 2 * GUARD,), -777.0, device=DEV)
    mol = torch.full((sizes[1] + 2 * GUARD,), -777.0, device=DEV)
    hb = torch.full((sizes[2] + 2 * GUARD,), -777, dtype=torch.int32, device=DEV)
    views = [buf[GUARD: GUARD + k] for buf, k in zip((atoms, mol, hb), sizes)]
    _lib.check(_lib.lib().mcg_receptor_interactions(
        _lib.dptr(x), _lib.dptr(r), _lib.dptr(t), _lib.dptr(n), _lib.dptr(rot), B, width, _lib.dptr(rec), _lib.dptr(rec_t),
        int(rec.shape[0]), _lib.dptr(spheres), views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(),
        _lib.current_stream_ptr(DEV)), "mcg_receptor_interactions")
    torch.cuda.synchronize()
    for buf, k in zip((atoms, mol, hb), sizes):
        host = buf.cpu()
        assert bool((host[:GUARD] == -777).all()) and bool((host[GUARD + k:] == -777).all()), "a write outside the output"
    return dict(atom_terms=views[0].cpu().reshape(B, width, 6), mol_terms=views[1].cpu().reshape(B, 8), hbonds=views[2].cpu())


def _one(case, width=None, skip_tiles=True):
    key = (case.name, width, skip_tiles)
    if key not in _DONE:
        _DONE[key] = _launch([case], width or max(case.n, 1), case.receptor, skip_tiles)
    return _DONE[key]


def _got(out, b, n):
    """Row b of a launch in the restatement's spelling."""
    a, m = out["atom_terms"][b].double().numpy(), out["mol_terms"][b].double().numpy()
    return dict(atom_terms=a[:n, :5], atom_scores=a[:n, 5], terms=m[:5], weighted=m[5], score=m[6], hbonds=int(out["hbonds"][b]))


def _same(a, b, n, what, row_a=0, row_b=0):
    """The outputs of one molecule bit for bit (NaN-free rows): its atoms' terms, its sums, its count."""
    assert torch.equal(a["atom_terms"][row_a, :n].view(torch.int32), b["atom_terms"][row_b, :n].view(torch.int32)), what
    assert torch.equal(a["mol_terms"][row_a].view(torch.int32), b["mol_terms"][row_b].view(torch.int32)), what
    assert int(a["hbonds"][row_a]) == int(b["hbonds"][row_b]), what


# ----------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("name", list(K.HAND))
def test_hand_pairs(name):
    pair, want = K.HAND[name]
    case = R.Case("hand", 1, 1)
    case.x, case.z, case.t, case.n_rot = pair["x"], np.array(pair["z"]), np.array(pair["t"], dtype=np.uint8), 0
    case.rec, case.rec_z, case.rec_t = pair["y"], np.array(pair["zr"]), np.array(pair["tr"], dtype=np.uint8)
    out = _launch([case], 1, case.receptor)
    got = _got(out, 0, 1)
    R.check(got, *case.args(), what=name)
    terms = dict(zip(R.TERMS, got["terms"]))
    for k, v in want.items():
        if k == "hbonds":
            assert got["hbonds"] == v
        elif k == "counted":
            assert bool(terms["g2"] > 0) is v and (v or not out["mol_terms"][0].any())
        else:
            assert terms[k] == pytest.approx(v, abs=1e-6), (name, k)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases_match_the_restatement(case):
    bound = R.bounds(*case.args())
    for width in sorted({case.n, max(case.n, 41), 64}):
        out = _one(case, width)
        got = _got(out, 0, case.n)
        R.check(got, *case.args(), what=f"{case} width {width}")
        assert not out["atom_terms"][0, case.n:].any()                            # 0 on padded atoms
        assert float(out["mol_terms"][0, 7]) == 0.0
        # the atoms' terms sum to the molecule's, inside the rule
        total = got["atom_terms"].sum(axis=0)
        assert (np.abs(total - got["terms"]) <= bound["atom_terms"].sum(axis=0) + bound["terms"]).all()
        assert abs(got["atom_scores"].sum() - got["weighted"]) <= bound["atom_scores"].sum() + bound["weighted"]


def test_hbond_counts_are_exact_and_present():
    counts = [int(_one(c)["hbonds"][0]) for c in CASES]
    assert counts == [R.score(*c.args())["hbonds"] for c in CASES]
    dense = R.Case("dense", 41, 27)
    dense.rec = (dense.rec * np.float32(0.8)).astype(np.float32)                  # the pocket drawn in: contacts below -0.7 A
    out = _launch([dense], 27, dense.receptor)
    want = R.score(*dense.args())
    assert int(out["hbonds"][0]) == want["hbonds"] and want["hbonds"] >= 3
    R.check(_got(out, 0, 27), *dense.args(), what="dense pocket")


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
    others = [R.Case(f"o{k}", 5000 + k, 1 + k % 40) for k in range(70)]
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
    on, off = _launch([c], 27, rec, True), _launch([c], 27, rec, False)
    _same(on, off, c.n, "far slab")
    _same(on, _one(c), c.n, "the slab adds nothing")                              # pairs that do not count add exactly +0


# ----------------------------------------------------------------------------------------------- special rows
def test_empty_and_non_finite_rows_beside_good_rows():
    good = [CASES[2], CASES[1], CASES[3]]
    rec = CASES[2].receptor
    empty = R.Case("empty", 51, 0)
    bad = R.Case("bad", 52, 9)
    bad.x = bad.x.copy()
    bad.x[4, 1] = np.float32("nan")
    inf = R.Case("inf", 53, 5)
    inf.x = inf.x.copy()
    inf.x[0, 0] = np.float32("inf")
    batch = [good[0], empty, good[1], bad, inf, good[2]]
    out = _launch(batch, 64, rec)
    assert not out["atom_terms"][1].any() and not out["mol_terms"][1].any() and int(out["hbonds"][1]) == 0
    for row, c in ((3, bad), (4, inf)):
        assert bool(torch.isnan(out["atom_terms"][row, : c.n]).all()) and not out["atom_terms"][row, c.n:].any()
        assert bool(torch.isnan(out["mol_terms"][row, :7]).all()) and float(out["mol_terms"][row, 7]) == 0.0
        assert int(out["hbonds"][row]) == -1
    for row, c in ((0, good[0]), (2, good[1]), (5, good[2])):                     # the other rows are unaffected
        alone = _launch([c], 64, rec)
        _same(alone, out, c.n, ("beside bad rows", row), 0, row)
        assert bool(torch.isfinite(out["mol_terms"][row]).all())


def test_receptor_beyond_the_cut_off_scores_exact_zeros():
    far = R.Case("far", 31, 27, far=True)
    for skip in (True, False):
        out = _launch([far], 41, far.receptor, skip)
        assert not out["atom_terms"].any() and not out["mol_terms"].any() and int(out["hbonds"][0]) == 0
        assert float(out["mol_terms"][0, 6]) == 0.0


# ----------------------------------------------------------------------------------------------- the module's own path
def test_device_typing_and_rotatable_bonds_equal_the_plain_python_rules():
    mols = [m for name in K.MOLECULES for m, _ in K.renumberings(K.MOLECULES[name][0])]
    z, bonds, n = _padded(mols)
    types = IX.ligand_types(z, bonds, n, DEV).cpu()
    rot = IX.rotatable_bonds(z, bonds, n, DEV).cpu().tolist()
    for b, (zz, adj, k) in enumerate(mols):
        assert types[b, :k].tolist() == R.ligand_types(zz, adj, k, K.pharm_types((zz, adj, k))), b
        assert not types[b, k:].any()
        assert rot[b] == R.rotatable_bonds(zz, adj, k), b
    assert rot[: 4] == [0] * 4 and set(rot[-4:]) == {61}


def _padded(mols, width=64):
    B = len(mols)
    z = torch.full((B, width), 9, dtype=torch.int32)                              # junk beyond the atoms
    bonds = torch.full((B, width, width), 3, dtype=torch.int8)
    n = torch.zeros(B, dtype=torch.int32)
    for b, (zz, adj, k) in enumerate(mols):
        z[b, :k] = torch.tensor(zz, dtype=torch.int32)
        bonds[b, :k, :k] = torch.tensor(adj, dtype=torch.int8).reshape(k, k)
        n[b] = k
    return z, bonds, n


def test_interaction_scores_on_graphs_equal_the_typed_launch():
    mols = [K.MOLECULES[name][0] for name in ("toluene", "acetamide", "biphenyl", "pyridine", "ethanol", "butane")]
    z, bonds, n = _padded(mols, 41)
    g = np.random.default_rng(8)
    x = torch.zeros(len(mols), 41, 3)
    for b, (_, _, k) in enumerate(mols):
        x[b, :k] = torch.from_numpy(R.walk(k, g).astype(np.float32))
    rec = CASES[2].receptor
    out = {k: v.cpu() for k, v in IX.interaction_scores(rec, x, n, z, bonds, device=DEV).items()}
    prepared = IX.prepare_receptor(rec)
    for b, (zz, adj, k) in enumerate(mols):
        t = R.ligand_types(zz, adj, k, K.pharm_types((zz, adj, k)))
        rot = R.rotatable_bonds(zz, adj, k)
        assert out["types"][b, :k].tolist() == t and int(out["n_rot"][b]) == rot
        args = (x[b, :k].numpy(), R.radii(zz), t, prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(),
                prepared.types.numpy(), rot)
        got = dict(atom_terms=out["atom_terms"][b, :k].double().numpy(), atom_scores=out["atom_scores"][b, :k].double().numpy(),
                   terms=out["terms"][b, :5].double().numpy(), weighted=float(out["terms"][b, 5]), score=float(out["score"][b]),
                   hbonds=int(out["hbonds"][b]))
        R.check(got, *args, what=f"graph {b}")
    again = IX.interaction_scores(prepared, x, n, z, bonds, skip_tiles=False, device=DEV)
    assert all(torch.equal(out[k], again[k].cpu()) for k in out)


# ----------------------------------------------------------------------------------------------- generation entries
def _flat(m, skip=()):
    return {k: (None if v is None else v.tolist() if torch.is_tensor(v) else v) for k, v in vars(m._measured).items()
            if k not in skip}


NEW = ("interaction_score", "interaction_terms", "receptor_hbonds", "interaction_atom_scores")


def _public(m):
    """Every measured value of a record, the new ones through their properties (the per-atom scores are sliced lazily)."""
    atoms = m.interaction_atom_scores
    return (_flat(m, NEW), m.interaction_score, m.interaction_terms, m.receptor_hbonds,
            None if atoms is None else atoms.view(torch.int32).tolist())


def test_generation_with_interaction_scores(monkeypatch):
    from composed_cases import carved_pocket
    from test_receptor_relief_gpu import _posed_setup
    gen, ref, kw, base = _posed_setup(monkeypatch)
    pts, z = carved_pocket(ref, base)
    g = torch.Generator().manual_seed(12)
    z = torch.tensor([6, 6, 7, 8])[torch.randint(0, 4, (len(z),), generator=g)]
    rec = (pts, z, torch.randint(0, 8, (len(z),), generator=g))
    launched = []
    real = gen._interaction_scores
    monkeypatch.setattr(gen, "_interaction_scores", lambda *a, **k: launched.append(1) or real(*a, **k))

    plain = gen.generate_conformers(receptor=rec, **kw)
    defaults = gen.generate_conformers(receptor=rec, interaction_scores=False, max_interaction_score=None, rank_by="shape", **kw)
    assert launched == [] and defaults == plain and [_flat(m) for m in defaults] == [_flat(m) for m in plain]
    assert all(getattr(m, f) is None for m in plain for f in NEW)
    got = gen.generate_conformers(receptor=rec, interaction_scores=True, **kw)
    assert launched == [1]                                                        # one call over the rows
    assert got == plain and [_flat(m, NEW) for m in got] == [_flat(m, NEW) for m in plain]       # every other bit as before
    prepared = IX.prepare_receptor(rec)
    scored = {}
    for m in got:
        if m.pose is None:
            assert all(getattr(m, f) is None for f in NEW)
            continue
        k = len(m.atomic_numbers)
        own = IX.interaction_scores(prepared, m.coords[None], torch.tensor([k], dtype=torch.int32),
                                    torch.tensor([m.atomic_numbers], dtype=torch.int32), m.bond_orders[None], device=DEV)
        assert np.float32(m.interaction_score).view(np.uint32) == own["score"].cpu().numpy().view(np.uint32)[0], m.sample_id
        assert m.receptor_hbonds == int(own["hbonds"][0]) and m.interaction_terms["n_rot"] == int(own["n_rot"][0])
        assert [np.float32(m.interaction_terms[t]) for t in R.TERMS] == own["terms"][0, :5].cpu().numpy().tolist()
        assert torch.equal(m.interaction_atom_scores.view(torch.int32), own["atom_scores"][0].cpu().view(torch.int32))
        scored[m.sample_id] = m.interaction_score
    assert len(scored) >= 8 and len(set(scored.values())) >= 8
    values = sorted(scored.values())
    t = (values[2] + values[3]) / 2
    kept = gen.generate_conformers(receptor=rec, max_interaction_score=t, **kw)
    assert [m.sample_id for m in kept] == [i for i in sorted(scored) if scored[i] <= t] and 0 < len(kept) < len(got)
    order = sorted(scored, key=lambda i: (scored[i], i))
    top = gen.generate_conformers(receptor=rec, interaction_scores=True, rank_by="interaction", top_k=3, **kw)
    assert [m.sample_id for m in top] == order[:3]
    shaped = gen.generate_conformers(receptor=rec, interaction_scores=True, shape_scores=True, **kw)
    by_shape = gen.generate_conformers(receptor=rec, interaction_scores=True, top_k=3, **kw)
    assert [m.sample_id for m in by_shape] == [m.sample_id for m in sorted(
        shaped, key=lambda m: (-m.shape_tanimoto if m.shape_tanimoto == m.shape_tanimoto else math.inf, m.sample_id))][:3]
    for entry in ("generate_conformers_sharded", "forward"):
        again = getattr(gen, entry)(receptor=rec, interaction_scores=True, **kw)
        assert [_public(m) for m in again] == [_public(m) for m in got], entry
    sharded_top = gen.generate_conformers_sharded(receptor=rec, interaction_scores=True, rank_by="interaction", top_k=3, **kw)
    assert [m.sample_id for m in sharded_top] == order[:3]
    print(f"INTERACTIONS e2e: {len(scored)} of {len(got)} scored, E in [{values[0]:.3f}, {values[-1]:.3f}], hbonds "
          f"{[m.receptor_hbonds for m in got]}; E <= {t:.3f} keeps {[m.sample_id for m in kept]}; top 3 {order[:3]}")
