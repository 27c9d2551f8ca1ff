"""Solid references on the MI355X (`csrc/mcg_mesh.hip`, DESIGN.md section 6 "Solid references"): the winding-number kernel
against the fp64 restatement (tests/mesh_ref.py) on closed meshes and on open prefixes at every tile and split boundary,
bit identity of a point's value whatever the batch and the mode, the occupancy, the field entries against the entries they
derive from, poses into a box, `atoms_outside`, and `reference_shape` through `generate_conformers` end to end."""
import functools
import statistics

import numpy as np
import pytest
import torch

import mesh_cases as C
import mesh_ref as R
from conftest import load_golden
from ml_conformer_generator_amd import cheminformatics as CH
from parity_tolerance import close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x5EED_0000_2026_1017


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _pocket_solid():
    return CH.solid_reference(C.pocket())


@functools.lru_cache(maxsize=None)
def _pocket_occupancy64():
    """The fp64 occupancy of the pocket on its own 40^3 grid: computed once, shared, never written to."""
    solid = _pocket_solid()
    return R.occupancy(solid.triangles, solid.axes)


# ----------------------------------------------------------------------------------------------- winding number
@pytest.mark.parametrize("P", C.BATCHES)
@pytest.mark.parametrize("name", ["tetrahedron", "cube", "pocket"])
def test_winding_of_closed_meshes(name, P):
    mesh, pts, owners, p0 = C.test_points(name, P, seed=P)
    tri = C.triangles(mesh)
    w64 = R.winding(tri, pts)
    assert float(((w64.abs() - 0.5).abs()).min()) > 0.25                # every point, none left out
    con = R.probe_contributions(tri, pts[p0:], owners)
    assert R.WINDING_TOL < 0.1 * float(con.abs().min())
    w = CH.mesh_winding(tri, points=pts, device=DEV).cpu()
    err = float((w.double() - w64).abs().max())
    print(f"MESH winding {name} F={tri.shape[0]} P={len(pts)}: max |w - w64| = {err:.3e}")
    assert torch.equal(R.inside(w), R.inside(w64))
    assert err <= R.WINDING_TOL


@pytest.mark.parametrize("F", C.PREFIXES)
def test_winding_of_open_prefixes(F):
    """The first F triangles of the pocket: an open surface (legal), one either side of every tile and split boundary."""
    mesh = C.pocket()
    tri = C.triangles(mesh, F)
    owners = sorted({0, F - 1, F // 2} | {k for k in C.EDGE_TRIANGLES if k < F})
    probes, own = C.probe_points(mesh, owners)
    pts = torch.cat([C.random_points(mesh, 65, seed=F), probes])
    w64 = R.winding(tri, pts)
    w = CH.mesh_winding(tri, points=pts, device=DEV).cpu()
    err = float((w.double() - w64).abs().max())
    print(f"MESH winding prefix F={F} P={len(pts)}: max |w - w64| = {err:.3e}")
    assert err <= R.WINDING_TOL
    con = R.probe_contributions(tri, probes, own)
    assert R.WINDING_TOL < 0.1 * float(con.abs().min())


def test_winding_in_grid_mode_and_bit_identity():
    mesh = C.pocket()
    tri = C.triangles(mesh)
    lo, hi = mesh.vertices.min(0) - 2.0, mesh.vertices.max(0) + 2.0
    axes = torch.stack([torch.linspace(float(lo[k]), float(hi[k]), 8) for k in range(3)])
    pts = R.grid_points(axes).to(torch.float32)
    w64 = R.winding(tri, pts)
    grid = CH.mesh_winding(tri, axes=axes, device=DEV).cpu()
    assert grid.shape == (512,)
    err = float((grid.double() - w64).abs().max())
    print(f"MESH winding pocket grid n=8: max |w - w64| = {err:.3e}")
    assert err <= R.WINDING_TOL
    keep = (w64.abs() - 0.5).abs() > 0.25
    assert torch.equal(R.inside(grid)[keep], R.inside(w64)[keep]) and int(keep.sum()) >= 500
    batch = CH.mesh_winding(tri, points=pts, device=DEV).cpu()
    assert torch.equal(_bits(batch), _bits(grid))                         # array mode = grid mode
    for k in (0, 100, 255, 256, 511):                                     # alone, and inside a batch of 257
        alone = CH.mesh_winding(tri, points=pts[k:k + 1], device=DEV).cpu()
        assert torch.equal(_bits(alone), _bits(grid[k:k + 1])), k
        others = C.random_points(mesh, 257, seed=k)
        others[131] = pts[k]
        assert torch.equal(_bits(CH.mesh_winding(tri, points=others, device=DEV).cpu()[131:132]), _bits(grid[k:k + 1])), k
    for F in (1, 256, 1025):                                              # one part and two
        a = CH.mesh_winding(tri[:F], points=pts, device=DEV).cpu()
        b = CH.mesh_winding(tri[:F], axes=axes, device=DEV).cpu()
        assert torch.equal(_bits(a), _bits(b)), F


def test_non_finite_points_and_points_on_the_mesh():
    mesh = C.pocket()
    tri = C.triangles(mesh)
    pts = C.random_points(mesh, 257, seed=9)
    base = CH.mesh_winding(tri, points=pts, device=DEV).cpu()
    for k, bad in ((0, float("nan")), (100, float("inf")), (256, -float("inf"))):
        p = pts.clone()
        p[k, 1] = bad
        got = CH.mesh_winding(tri, points=p, device=DEV).cpu()
        keep = torch.arange(257) != k
        assert bool(torch.isnan(got[k])) and torch.equal(_bits(got[keep]), _bits(base[keep]))
    on = torch.from_numpy(mesh.vertices[[0, 17, 1245]].copy())            # points ON vertices: finite, not NaN
    assert bool(torch.isfinite(CH.mesh_winding(tri, points=on, device=DEV)).all())
    cube = C.mesh_of("cube")
    corner = torch.from_numpy(cube.vertices[:1].copy())                   # every triangle at the corner contributes 0
    w = CH.mesh_winding(C.triangles(cube), points=corner, device=DEV).cpu()
    assert float((w.double() - R.winding(C.triangles(cube), corner)).abs().max()) <= R.WINDING_TOL


def test_occupancy_equals_the_restatement_on_the_pocket():
    solid = _pocket_solid()
    f = solid.on(DEV)["f"].cpu()
    want = _pocket_occupancy64()
    assert f.shape == (64000,) and set(f.unique().tolist()) == {0.0, 1.0}
    assert torch.equal(f.double(), want)
    cell = float(torch.prod(solid.axes[:, 1] - solid.axes[:, 0]))
    print(f"MESH occupancy: {int(f.sum())} of 64000 grid points inside, {float(f.sum()) * cell:.1f} A^3")
    assert 0.8 < float(f.sum()) * cell / 999.917 < 1.2


# ----------------------------------------------------------------------------------------------- field entries
def test_overlay_field_equals_overlay_bit_for_bit():
    """`mcg_shape_overlay_field` fed the density `mcg_shape_overlay` computed for a 17-atom reference, and
    `mcg_shape_tanimoto_field` that of `mcg_shape_tanimoto`: every output, bit for bit."""
    from ml_conformer_generator_amd import _lib
    from test_shape_frames_gpu import _pad, _ragged_batch
    g = load_golden("shape_quadrupole.npz")
    ref = torch.as_tensor(g["xyz_ceyyag"]).to(torch.float32)
    assert ref.shape[0] == 17
    mols = _ragged_batch()[:9] + [torch.as_tensor(g["xyz_yibfeu"])]
    coords, n = _pad(mols, 64)
    coords[3, 2, 0] = float("nan")                                        # a failing row
    want = CH.shape_overlay(ref, coords, n, DEV, with_scores=True)
    # the same launch again, by hand, to get at its density and the reference's transform
    conformer = CH.ConformerReference(ref)
    x, nn = conformer.rows(coords.to(DEV), n.to(DEV, torch.int32), DEV)
    dev = DEV
    xform = torch.empty(x.shape[0], 12, device=dev)
    _, frames = CH.shape_frames_hip(x, nn, dev, centre_atoms=True, xform_out=xform)
    ref_frame = frames[0, :17].contiguous()
    axes = CH._grid_axes(ref_frame.cpu(), 40).to(dev).contiguous()
    rots = CH._orientations().reshape(4, 9).to(dev).contiguous()
    f = torch.empty(64000, device=dev)
    score = torch.empty(len(mols) * 4, device=dev)
    _lib.check(_lib.lib().mcg_shape_tanimoto(_lib.dptr(ref_frame), 17, _lib.dptr(frames[1:]), _lib.dptr(nn[1:]), len(mols),
                                             64, _lib.dptr(rots), 4, _lib.dptr(axes), 40, float(CH.ALPHA),
                                             float(CH.AMPLITUDE), _lib.dptr(f), _lib.dptr(score),
                                             _lib.current_stream_ptr(dev)), "mcg_shape_tanimoto")

    class Field(CH.SolidReference):
        """That density, transform and grid as the device side of a solid that has no mesh to count atoms against."""
        pose_keys = ()

        def __init__(self):
            self.n, self._on = 40, {dev: dict(f=f, xform=xform[0].contiguous(), axes=axes)}

        def pose_extras(self, out, nn, dev):
            return {}
    got = CH.shape_overlay(Field(), coords, n, DEV, with_scores=True)
    assert list(got) == list(want)
    assert int(got["orientation"][3]) == -1 and int((got["orientation"] >= 0).sum()) == len(mols) - 1
    for key in ("coords", "rotation", "translation", "tanimoto", "scores"):
        assert torch.equal(_bits(got[key]), _bits(want[key])), key
    assert torch.equal(got["orientation"], want["orientation"]) and torch.equal(got["flipped"], want["flipped"])
    score_f = torch.empty_like(score)
    _lib.check(_lib.lib().mcg_shape_tanimoto_field(_lib.dptr(f), _lib.dptr(frames[1:]), _lib.dptr(nn[1:]), len(mols), 64,
                                                   _lib.dptr(rots), 4, _lib.dptr(axes), 40, float(CH.ALPHA),
                                                   float(CH.AMPLITUDE), _lib.dptr(score_f), _lib.current_stream_ptr(dev)),
               "mcg_shape_tanimoto_field")
    assert torch.equal(_bits(score_f), _bits(score))


# ----------------------------------------------------------------------------------------------- overlay onto a solid
@pytest.mark.parametrize("width", [30, 64])
def test_overlay_onto_a_box(width):
    """A 2 x 3 x 5 lattice of points 1.5 A apart, anywhere in space, posed into a 4 x 6 x 10 A box: by the symmetry of both the
    pose centres the lattice in the box with its axes along the box's, every atom more than 1 A inside."""
    v, faces = C.box(4.0, 6.0, 10.0, origin=(3.0, -2.0, 7.0))
    solid = CH.solid_reference((v, faces))
    lat = C.lattice().double()
    B = 5
    coords = torch.zeros(B, width, 3)
    for b in range(B):
        q, t = C.rigid_motion(100 + b)
        coords[b, :30] = (lat @ q + t).to(torch.float32)
    n = torch.full((B,), 30, dtype=torch.int32)
    res = {k: t.cpu() for k, t in CH.shape_overlay_solid(solid, coords, n, DEV, with_scores=True).items()}
    f64 = R.occupancy(solid.triangles, solid.axes)
    assert res["atoms_outside"].tolist() == [0] * B and res["orientation"].min() >= 0
    for b in range(B):
        Q, d = res["rotation"][b].double(), res["translation"][b].double()
        assert abs(float(torch.det(Q)) - 1.0) <= 1e-5
        assert float((Q @ Q.T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-5
        posed = res["coords"][b, :30].double()
        assert float((posed - (coords[b, :30].double() @ Q + d)).abs().max()) < 1e-4
        assert float(res["coords"][b, 30:].abs().max() if width > 30 else 0.0) == 0.0
        assert float(res["tanimoto"][b]) == float(res["scores"][b].max())
        framed = (posed - torch.from_numpy(solid.t_r)) @ torch.from_numpy(solid.M_r)
        want = R.field_tanimoto(f64, solid.axes, framed)
        ok, err, _ = close(res["tanimoto"][b].reshape(1), torch.tensor([want]))
        assert ok, (b, float(res["tanimoto"][b]), want)
        lo, hi = torch.tensor([3.0, -2.0, 7.0]) + 1.0, torch.tensor([7.0, 4.0, 17.0]) - 1.0
        assert bool(((posed > lo) & (posed < hi)).all())
    print(f"MESH box overlay width {width}: tanimoto {res['tanimoto'].tolist()}")
    # an empty batch: the keys, dtypes and trailing shapes of a one-molecule call, whatever the kind of reference
    def layout(out):
        out = dict(enumerate(out)) if isinstance(out, tuple) else out if isinstance(out, dict) else {0: out}
        return {k: (t.dtype, t.device, tuple(t.shape[1:])) for k, t in out.items()}
    for reference in (solid, lat.to(torch.float32)):
        calls = [lambda x, m: CH.shape_scores(reference, x, m, DEV), lambda x, m: CH.shape_overlay(reference, x, m, DEV),
                 lambda x, m: CH.shape_overlay(reference, x, m, DEV, with_scores=True)]
        if reference is not solid:
            calls += [lambda x, m: CH.shape_overlay(reference, x, m, DEV, refine_steps=8),
                      lambda x, m: CH.shape_overlay(reference, x, m, DEV, with_scores=True, refine_steps=8)]
        for call in calls:
            one, none = call(coords[:1], n[:1]), call(coords[:0], n[:0])
            assert layout(none) == layout(one) and list(layout(none)) == list(layout(one))
            assert all(t.shape[0] == 0 for t in (none.values() if isinstance(none, dict) else none))
        pair = CH.pairwise_shape_tanimoto(reference, coords[:0], n[:0], DEV)
        assert pair.shape == (0, 0) and pair.dtype == CH.pairwise_shape_tanimoto(reference, coords[:1], n[:1], DEV).dtype


def test_atoms_outside_matches_the_restatement():
    mesh = C.pocket()
    tri = C.triangles(mesh)
    g = np.random.default_rng(4)
    verts = mesh.vertices
    for width in (1, 39, 64):
        B = 7
        n = g.integers(1, width + 1, B).astype(np.int32) if width > 1 else np.ones(B, dtype=np.int32)
        n[0], n[1] = width, 0                                             # a full row and one with no atoms
        pick = verts[g.integers(0, len(verts), (B, width))]               # molecules straddling the surface: atoms
        x = (pick + g.normal(size=(B, width, 3)) * 1.5).astype(np.float32)      # scattered 1.5 A around surface vertices
        x[2, 0, 2] = np.nan
        n[2] = max(int(n[2]), 1)
        w64 = R.winding(tri, torch.from_numpy(x.reshape(-1, 3))).reshape(B, width)
        real = torch.arange(width)[None, :] < torch.from_numpy(n)[:, None].long()
        margin = ((w64.abs() - 0.5).abs())[real & torch.isfinite(w64)]
        assert float(margin.min()) > 0.25
        want = R.atoms_outside(tri, x, n)
        got, w = CH.mesh_atoms_outside(tri, torch.from_numpy(x), torch.from_numpy(n), DEV, with_winding=True)
        assert got.cpu().tolist() == want and want[1] == 0 and want[2] == -1
        assert got.dtype == torch.int32
        assert CH.mesh_atoms_outside(tri, torch.from_numpy(x), torch.from_numpy(n), DEV).cpu().tolist() == want
        flat = CH.mesh_winding(tri, points=torch.from_numpy(x.reshape(-1, 3)), device=DEV).cpu().reshape(B, width)
        w = w.cpu()
        assert torch.equal(_bits(w[real]), _bits(flat[real]))              # the same bits as the winding entry
        assert float(w[~real].abs().max() if bool((~real).any()) else 0.0) == 0.0
        print(f"MESH atoms_outside width {width}: {want}")
    with pytest.raises(ValueError):
        CH.mesh_atoms_outside(tri, torch.zeros(2, 65, 3), torch.tensor([65, 1]), DEV)
    with pytest.raises(ValueError):
        CH.mesh_atoms_outside(tri, torch.zeros(2, 10, 3), torch.tensor([11, 1]), DEV)


# ----------------------------------------------------------------------------------------------- generation entries
def _restated_score(solid, coords):
    """`shape_scores_solid` restated: the molecule's principal frame (the frames kernel, pinned elsewhere) in the four
    orientations against the fp64 occupancy, each as the fp64 grid sum; the best."""
    x = coords.unsqueeze(0)
    _, frames = CH.shape_frames_hip(x, torch.tensor([coords.shape[0]]), DEV, centre_atoms=True)
    fr = frames[0].cpu().double()
    f64 = _pocket_occupancy64()
    return max(R.field_tanimoto(f64, solid.axes, fr @ rot.double()) for rot in CH._orientations())


def test_generation_into_the_pocket_end_to_end(monkeypatch):
    from ml_conformer_generator_amd import conformer_generator as CG
    from test_shape_frames_gpu import _gen, _molecule_like_shards
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen))
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    pocket = C.pocket()
    solid = _pocket_solid()
    kw = dict(reference_shape=pocket, n_atoms=38, variance=1, n_samples=8, sample_seed=SEED, optimise_geometry=False)
    plain = gen.generate_conformers(**kw)
    assert len(plain) == 8 and all(m.atoms_outside is None and m.pose is None and m.shape_tanimoto is None for m in plain)
    assert all(37 <= m.GetNumAtoms() <= 39 for m in plain)
    got = gen.generate_conformers(overlay=True, shape_scores=True, **kw)
    assert [m.sample_id for m in got] == list(range(8))
    tri = C.triangles(pocket)
    for a, m in zip(plain, got):
        Q, d = m.pose
        assert abs(float(torch.det(Q.double())) - 1.0) <= 1e-5
        assert float((m.coords.double() - (a.coords.double() @ Q.double() + d.double())).abs().max()) < 1e-4
        w64 = R.winding(tri, m.coords)
        assert m.atoms_outside == int((~R.inside(w64)).sum())
        want = _restated_score(solid, m.coords)
        ok, err, _ = close(torch.tensor([m.shape_tanimoto]), torch.tensor([want]))
        assert ok, (m.sample_id, m.shape_tanimoto, want)
        assert m.overlay_tanimoto == m.overlay_tanimoto and 0.0 < m.shape_tanimoto <= 1.0
    counts = [m.atoms_outside for m in got]
    print(f"MESH e2e: atoms_outside {counts}  shape_tanimoto {[round(m.shape_tanimoto, 4) for m in got]}")
    k = int(statistics.median(counts))
    kept = gen.generate_conformers(overlay=True, shape_scores=True, max_atoms_outside=k, **kw)
    expect = [m for m in got if m.atoms_outside <= k]
    assert 0 < len(expect) and [m.sample_id for m in kept] == [m.sample_id for m in expect]
    for a, b in zip(kept, expect):
        assert torch.equal(a.coords, b.coords) and a.atoms_outside == b.atoms_outside
        assert a.shape_tanimoto == b.shape_tanimoto
    # selection from the recorded values, as `select_diverse` would
    x, n = CH.padded_coords([m.coords for m in got])
    pair = CH.pairwise_shape_tanimoto_solid(solid, x, n, DEV).cpu()
    assert torch.equal(pair, pair.T) and bool((torch.diagonal(pair) == 1).all())
    off = pair[~torch.eye(8, dtype=torch.bool)]
    thr = float(off.sort().values[len(off) // 2])                          # the median pair similarity: excludes some
    scores = [m.shape_tanimoto for m in got]
    want = CH.select_diverse(scores, list(range(8)), pair, thr, top_k=3)
    picked = gen.generate_conformers(overlay=True, top_k=3, max_pairwise_tanimoto=thr, **kw)
    assert [m.sample_id for m in picked] == want and 1 <= len(want) <= 3
    top = gen.generate_conformers_sharded(overlay=True, top_k=4, **kw)
    assert [m.sample_id for m in top] == CH.select_diverse(scores, list(range(8)), None, None, top_k=4)


def test_the_notebook_call(tmp_path, monkeypatch):
    """Section 3 of the reference's notebook, with no `trimesh` and no reference conformer: an STL path in, molecules out
    (the synthetic weights' molecules are no drug-like shapes, hundreds of angstroms wide, and every record is kept: this
    pins the call, its keys and its filter, not chemistry)."""
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd import mesh as M
    from test_shape_frames_gpu import _gen
    path = tmp_path / "pocket.stl"
    path.write_bytes(M.write_stl(C.pocket()))
    gen = _gen()
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))
    mols = gen.generate_conformers(reference_shape=str(path), n_atoms=38, n_samples=10, variance=1, overlay=True,
                                   shape_scores=True, max_atoms_outside=39, optimise_geometry=False, sample_seed=SEED)
    assert len(mols) == 10
    print(f"MESH notebook call: atoms_outside {[m.atoms_outside for m in mols]}")
    for m in mols:
        assert m.shape_tanimoto is not None and m.pose is not None and 0 <= m.atoms_outside <= 39
    strict = gen.generate_conformers(reference_shape=str(path), n_atoms=38, n_samples=10, variance=1, overlay=True,
                                     shape_scores=True, max_atoms_outside=2, optimise_geometry=False, sample_seed=SEED)
    assert [m.sample_id for m in strict] == [m.sample_id for m in mols if m.atoms_outside <= 2]
