"""Solid references, host side (no GPU): `mesh.py` - mass properties against closed forms and the demo pocket's figures,
the solid's frame, STL loading and the watertight check -, every refusal of `reference_shape` / `max_atoms_outside` before
any device work, the seams a `reference_shape` call takes, and the mutation check of the fp64 restatement
(tests/mesh_ref.py) that the GPU tests compare against."""
import io

import numpy as np
import pytest
import torch

import mesh_cases as C
import mesh_ref as R
from ml_conformer_generator_amd import cheminformatics as CH
from ml_conformer_generator_amd import mesh as M
from ml_conformer_generator_amd import postprocess
from test_shape_overlay_host import _no_device, _ref, _shell_generator, _stub_overlay, _stub_shard


# ----------------------------------------------------------------------------------------------- mass properties
def test_box_mass_properties():
    p = M.mass_properties(M.load_mesh(C.box(2.0, 3.0, 5.0)), density=1.0)
    assert p["volume"] == pytest.approx(30.0, rel=1e-12)
    np.testing.assert_allclose(p["center_mass"], [1.0, 1.5, 2.5], rtol=1e-12)
    np.testing.assert_allclose(np.diag(p["inertia"]), [85.0, 72.5, 32.5], rtol=1e-12)
    np.testing.assert_allclose(p["inertia"] - np.diag(np.diag(p["inertia"])), 0.0, atol=1e-12)
    np.testing.assert_allclose(p["principal_inertia_components"], [32.5, 72.5, 85.0], rtol=1e-12)
    far = M.mass_properties(M.load_mesh(C.box(2.0, 3.0, 5.0, origin=(100.0, -50.0, 25.0))), density=1.0)
    np.testing.assert_allclose(far["principal_inertia_components"], [32.5, 72.5, 85.0], rtol=1e-11)


def test_tetrahedron_against_its_closed_form():
    v, f = C.tetrahedron()
    p = M.mass_properties(M.load_mesh((v, f)), density=1.0)
    vol = abs(np.linalg.det(v[1:] - v[0])) / 6.0
    assert p["volume"] == pytest.approx(vol, rel=1e-12)
    centre = v.mean(axis=0)
    np.testing.assert_allclose(p["center_mass"], centre, rtol=1e-12)
    d = v - centre                                   # covariance of a uniform tetrahedron: V / 20 sum_i d_i d_i^T
    np.testing.assert_allclose(p["covariance"], vol / 20.0 * d.T @ d, rtol=1e-11, atol=1e-14)


def test_invariance_under_rigid_motion_and_face_permutation():
    mesh = C.pocket()
    base = M.mass_properties(mesh)
    q, t = C.rigid_motion(3)
    v = mesh.vertices.astype(np.float64) @ q.numpy() + t.numpy()
    perm = np.random.default_rng(0).permutation(mesh.faces.shape[0])
    moved = M.mass_properties(M.Mesh(v.astype(np.float64), mesh.faces[perm]))          # fp64 vertices: no re-rounding
    assert moved["volume"] == pytest.approx(base["volume"], rel=1e-10)
    np.testing.assert_allclose(moved["principal_inertia_components"], base["principal_inertia_components"], rtol=1e-10)
    np.testing.assert_allclose(moved["center_mass"], base["center_mass"] @ q.numpy() + t.numpy(), rtol=1e-10)


def test_pocket_figures():
    mesh = C.pocket()
    assert mesh.vertices.shape == (1246, 3) and mesh.vertices.dtype == np.float32 and mesh.faces.shape == (2488, 3)
    p = M.mass_properties(mesh)
    assert p["volume"] == pytest.approx(999.917, rel=1e-5)
    np.testing.assert_allclose(p["principal_inertia_components"], [238.721, 724.944, 862.088], rtol=1e-5)
    ctx = M.mesh_context(mesh)
    assert ctx.dtype == torch.float32 and ctx.shape == (3,)
    np.testing.assert_allclose(ctx.numpy(), [238.721, 724.944, 862.088], rtol=1e-5)
    np.testing.assert_allclose(M.mesh_context(mesh, 0.04).numpy(), 2 * ctx.numpy(), rtol=1e-6)


def test_pocket_volume_against_a_winding_number_voxelisation():
    """The occupied volume of a 64^3 voxelisation (cell-centred samples of the bounding box, classified by the fp64
    winding number) against the exact volume.  Every fp64 winding number is an integer to 1e-12; the volume error is that
    of the cells the surface cuts: each misjudges at most its own volume, and with their fractions spread evenly the sum
    behaves like a random walk, so a bound of a tenth of the cut cells' total volume leaves a wide margin (measured:
    0.3 A^3 against a bound of about 17)."""
    mesh = C.pocket()
    n = 64
    lo, hi = mesh.vertices.astype(np.float64).min(0), mesh.vertices.astype(np.float64).max(0)
    h = (hi - lo) / n
    axes = torch.stack([torch.from_numpy(lo[k] + (np.arange(n) + 0.5) * h[k]) for k in range(3)])
    w = R.winding(C.triangles(mesh), R.grid_points(axes))
    assert float((w - w.round()).abs().max()) < 1e-12
    occ = R.inside(w).reshape(n, n, n)
    cut = torch.zeros_like(occ)
    for d in range(3):                               # a cell is cut where a face neighbour is classified differently
        a, b = occ.narrow(d, 0, n - 1), occ.narrow(d, 1, n - 1)
        cut.narrow(d, 0, n - 1).logical_or_(a != b)
        cut.narrow(d, 1, n - 1).logical_or_(a != b)
    cell = float(np.prod(h))
    volume, bound = float(occ.sum()) * cell, 0.1 * float(cut.sum()) * cell
    exact = M.mass_properties(mesh)["volume"]
    print(f"MESH voxel volume {volume:.3f} vs exact {exact:.3f}; {int(cut.sum())} cut cells, bound {bound:.2f}")
    assert abs(volume - exact) < bound < 0.05 * exact


# ----------------------------------------------------------------------------------------------- frame
def test_solid_frame_is_proper_descending_and_aligns_a_box():
    for src in (C.pocket(), M.load_mesh(C.box(4.0, 6.0, 10.0, origin=(3.0, -2.0, 7.0))), M.load_mesh(C.tetrahedron())):
        Mr, t = M.solid_frame(src)
        assert np.linalg.det(Mr) == pytest.approx(1.0, abs=1e-12)
        np.testing.assert_allclose(Mr.T @ Mr, np.eye(3), atol=1e-12)
        cov = M.mass_properties(src)["covariance"]
        d = Mr.T @ cov @ Mr
        assert d[0, 0] > d[1, 1] > d[2, 2] > 0
        np.testing.assert_allclose(d - np.diag(np.diag(d)), 0.0, atol=1e-9 * d[0, 0])
        np.testing.assert_allclose(t, M.mass_properties(src)["center_mass"])
    Mr, t = M.solid_frame(M.load_mesh(C.box(4.0, 6.0, 10.0, origin=(3.0, -2.0, 7.0))))
    np.testing.assert_allclose(t, [5.0, 1.0, 12.0], rtol=1e-12)
    np.testing.assert_allclose(np.abs(Mr), [[0, 0, 1], [0, 1, 0], [1, 0, 0]], atol=1e-12)       # z longest, then y, x
    framed = (np.array(C.box(4.0, 6.0, 10.0, origin=(3.0, -2.0, 7.0))[0]) - t) @ Mr
    np.testing.assert_allclose(np.abs(framed), np.tile([5.0, 3.0, 2.0], (8, 1)), atol=1e-12)


# ----------------------------------------------------------------------------------------------- loading
@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("name", ["pocket", "cube"])
def test_stl_round_trip(name, binary, tmp_path):
    mesh = C.mesh_of(name)
    data = M.write_stl(mesh, binary=binary)
    path = tmp_path / "mesh.stl"
    path.write_bytes(data)
    for src in (data, io.BytesIO(data), str(path), path):
        got = M.load_mesh(src)
        assert np.array_equal(got.vertices[got.faces], mesh.vertices[mesh.faces])       # vertex numbering: file order
        assert got.vertices.shape == mesh.vertices.shape
    if name == "pocket":
        assert M._read_stl(data).shape == (2488, 3, 3)               # 7 464 corner records weld to 1 246 vertices


def test_other_sources_and_orientation():
    v, f = C.box(2.0, 3.0, 5.0)
    tri = np.asarray(v)[f]
    if np.einsum("fi,fi->", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])) > 0:
        f = np.ascontiguousarray(f[:, ::-1])                          # now listed inward
    out = M.load_mesh((v, f))
    assert M.mass_properties(out)["volume"] == pytest.approx(30.0)
    assert np.array_equal(out.faces, f[:, ::-1])
    again = M.load_mesh((v, f[:, ::-1]))                              # listed outward: kept
    assert np.array_equal(again.faces, f[:, ::-1])

    class Holder:
        vertices, faces = torch.as_tensor(v), torch.as_tensor(f)
    held = M.load_mesh(Holder())
    assert np.array_equal(held.faces, out.faces) and M.load_mesh(out) is out
    dup = np.concatenate([v, v[:3]])                                  # unwelded copies of three vertices
    f2 = f.copy()
    f2[f2 == 0] = 8
    welded = M.load_mesh((dup, f2))
    assert welded.vertices.shape == (8, 3) and M.mass_properties(welded)["volume"] == pytest.approx(30.0)


def test_meshes_that_are_not_watertight_are_refused():
    v, f = C.box(2.0, 3.0, 5.0)
    msg = "The mesh needs to be watertight."
    with pytest.raises(ValueError, match=msg):
        M.load_mesh((v, f[1:]))                                       # one face removed
    with pytest.raises(ValueError, match=msg):
        M.load_mesh((v, np.concatenate([f, f[:1]])))                  # a duplicated face
    bad = f.copy()
    bad[0, 2] = bad[0, 1]
    with pytest.raises(ValueError, match=msg):
        M.load_mesh((v, bad))                                         # a degenerate face
    flipped = f.copy()
    flipped[0] = flipped[0, ::-1]
    with pytest.raises(ValueError, match=msg):
        M.load_mesh((v, flipped))                                     # one face against the others
    pocket = C.pocket()
    with pytest.raises(ValueError, match=msg):
        M.load_mesh((pocket.vertices, np.delete(pocket.faces, 1000, axis=0)))
    with pytest.raises(ValueError, match="no faces"):
        M.load_mesh((v, f[:0]))
    with pytest.raises(ValueError, match="more than"):
        M.load_mesh((v, np.tile(f, (M.MAX_FACES // 12 + 1, 1))))
    with pytest.raises(ValueError, match="non-finite"):
        M.load_mesh((np.where(np.arange(24).reshape(8, 3) == 4, np.nan, v), f))
    with pytest.raises(ValueError):
        M.load_mesh(b"not an stl file at all")
    with pytest.raises(ValueError):
        M.load_mesh((v, f + 1))                                       # names a vertex that does not exist


# ----------------------------------------------------------------------------------------------- requests
def _pocket_gen():
    gen = _shell_generator()
    gen._generate_shard = gen._score = gen._pose = gen._pair = _no_device
    return gen


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_reference_shape_refusals_happen_before_any_device_work(entry):
    call = getattr(_pocket_gen(), entry)
    pocket = C.pocket()
    ctx = torch.tensor([50.0, 100.0, 130.0])
    ok = dict(reference_shape=pocket, n_atoms=38, n_samples=4)
    for kw, match in ((dict(reference_conformer=_ref()), "cannot be combined with reference_conformer"),
                      (dict(reference_context=ctx), "cannot be combined with reference_conformer or reference_context"),
                      (dict(overlay=True, refine_overlay=True), "refine_overlay cannot be combined with reference_shape"),
                      (dict(overlay=True, refine_overlay=8), "refine_overlay cannot be combined with reference_shape"),
                      (dict(overlay=True, receptor=(torch.zeros(4, 3), torch.full((4,), 6))),
                       "receptor cannot be combined with reference_shape"),
                      (dict(max_atoms_outside=2), "max_atoms_outside needs overlay=True"),
                      (dict(overlay=True, max_atoms_outside=-1), "max_atoms_outside must be an integer >= 0"),
                      (dict(overlay=True, max_atoms_outside=1.5), "max_atoms_outside must be an integer >= 0"),
                      (dict(overlay=True, max_atoms_outside=True), "max_atoms_outside must be an integer >= 0"),
                      (dict(max_pairwise_tanimoto=0.5), "max_pairwise_tanimoto needs overlay=True"),
                      (dict(top_k=0), "top_k"), (dict(min_shape_tanimoto=1.5), "min_shape_tanimoto"),
                      (dict(shape_density=0.0), "shape_density"), (dict(shape_density="0.02"), "shape_density"),
                      (dict(n_atoms=None), "Reference Number of Atoms should be provided, when generating samples using "
                                           "context.")):
        with pytest.raises(ValueError, match=match):
            call(**dict(ok, **kw))
    v, f = C.box(2.0, 3.0, 5.0)
    with pytest.raises(ValueError, match="The mesh needs to be watertight."):
        call(**dict(ok, reference_shape=(v, f[1:])))
    with pytest.raises(ValueError, match="max_atoms_outside needs a reference_shape"):
        call(reference_conformer=_ref(), n_samples=4, overlay=True, max_atoms_outside=2)
    with pytest.raises(ValueError, match="max_atoms_outside needs a reference_shape"):
        call(reference_context=ctx, n_atoms=20, n_samples=4, max_atoms_outside=2)


def test_a_custom_finisher_is_refused_with_a_mesh_too():
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator(finisher=HP.TaskRef("fake_host_tasks.py", "finish_tag_chunk"))
    with pytest.raises(ValueError, match="custom finisher"):
        postprocess.parse_request(gen, None, shape_scores=True, reference_shape=C.pocket())


def test_a_plain_reference_shape_request_asks_for_nothing():
    import dataclasses
    gen = _pocket_gen()
    req = postprocess.parse_request(gen, None, reference_shape=C.pocket())
    assert isinstance(req.reference, CH.SolidReference) and req.reference.mesh is C.pocket()
    assert not req.measures and not req.removes and not req.selects_by_shape
    assert dataclasses.replace(req, reference=None) == postprocess.Request()
    assert postprocess.parse_request(gen, _ref()) == postprocess.Request()              # and without one: as before
    full = postprocess.parse_request(gen, None, shape_scores=True, top_k=3, min_shape_tanimoto=0.1, overlay=True,
                                     max_pairwise_tanimoto=0.9, reference_shape=C.pocket(), max_atoms_outside=2)
    assert isinstance(full.reference, CH.SolidReference) and full.reference.mesh is C.pocket()
    assert full.overlay and full.scores_shape and full.removes and full.max_atoms_outside == 2
    assert (full.top_k, full.min_shape_tanimoto, full.max_pairwise_tanimoto) == (3, 0.1, 0.9)


def test_solid_reference_host_side():
    v, f = C.box(4.0, 6.0, 10.0, origin=(3.0, -2.0, 7.0))
    solid = CH.solid_reference((v, f), n=12)
    assert CH.solid_reference(solid) is solid and solid.n == 12
    assert solid.triangles.shape == (12, 9) and solid.triangles.dtype == torch.float32
    np.testing.assert_allclose(solid.triangles_own.reshape(-1, 3).numpy().min(0), [3.0, -2.0, 7.0])
    np.testing.assert_allclose(np.abs(solid.triangles.reshape(-1, 3).numpy()), np.tile([5.0, 3.0, 2.0], (36, 1)), atol=1e-6)
    np.testing.assert_allclose(solid.xform[9:].numpy(), [5.0, 1.0, 12.0], rtol=1e-6)
    pad = 6.0 * CH.ATOM_RADIUS
    np.testing.assert_allclose(solid.axes[:, 0].numpy(), [-5.0 - pad, -3.0 - pad, -2.0 - pad], rtol=1e-6)
    np.testing.assert_allclose(solid.axes[:, -1].numpy(), [5.0 + pad, 3.0 + pad, 2.0 + pad], rtol=1e-6)
    with pytest.raises(ValueError, match="2 to 256"):
        CH.solid_reference((v, f), n=1)


# ----------------------------------------------------------------------------------------------- seams
def _solid_pose_stub(calls):
    """A device-free `_pose` for a solid: the overlay stub, with atoms_outside = 10 x the row's first coordinate (-1: failed)."""
    stub = _stub_overlay(lambda k: k + 1.0)

    def run(solid, coords, n, refine_steps=0):
        calls.append(("pose", solid))
        out = stub(None, coords, n)
        key = coords[:, 0, 0]
        out["atoms_outside"] = torch.where(torch.isnan(key), -1, (key * 10).round().nan_to_num(0).long()).to(torch.int32)
        return out
    return run


def test_proxy_path_takes_the_solid_seams_and_filters_on_atoms_outside():
    gen = _shell_generator()
    gen._generate_shard = _stub_shard()
    calls = []
    gen._pose = _solid_pose_stub(calls)
    gen._score = lambda solid, coords, n: (calls.append(("score", solid)), coords[:, 1, 0].clone())[1]
    gen._pair = lambda solid, coords, n: (calls.append(("pair", solid)), torch.zeros(len(coords), len(coords)))[1]
    kw = dict(reference_shape=C.pocket(), n_atoms=20, n_samples=8)
    plain = gen.generate_conformers(**kw)
    assert calls == [] and all(m.atoms_outside is None and m.pose is None for m in plain)
    posed = gen.generate_conformers(overlay=True, shape_scores=True, **kw)
    assert [c[0] for c in calls] == ["pose", "score"]
    assert all(isinstance(c[1], CH.SolidReference) and c[1].mesh is C.pocket() for c in calls)
    assert [m.sample_id for m in posed] == [0, 1, 2, 4, 5, 6, 7]                   # sample 3 is invalid
    want = {0: 0, 1: 7, 2: 4, 4: 8, 5: None, 6: 2, 7: 9}                             # x00 = (7 i % 10) / 10; 5 failed
    assert {m.sample_id: m.atoms_outside for m in posed} == want
    assert all((m.pose is None) == (m.sample_id == 5) for m in posed)
    for k in (0, 4, 9):
        kept = gen.generate_conformers(overlay=True, max_atoms_outside=k, **kw)
        assert [m.sample_id for m in kept] == [s for s, c in want.items() if R.passes(c, k)]
    calls.clear()
    diverse = gen.generate_conformers_sharded(overlay=True, max_pairwise_tanimoto=0.5, max_atoms_outside=8, **kw)
    assert [c[0] for c in calls] == ["pose", "score", "pair"]
    assert all(isinstance(c[1], CH.SolidReference) and c[1].mesh is C.pocket() for c in calls)
    assert sorted(m.sample_id for m in diverse) == [0, 1, 2, 4, 6]


def test_object_path_carries_atoms_outside_to_the_mols():
    from test_shape_overlay_host import PosedMol
    gen = _shell_generator(finisher="rdkit")
    calls = []
    gen._pose = _solid_pose_stub(calls)
    gen._score = lambda solid, coords, n: torch.full((coords.shape[0],), 0.25)
    req = postprocess.parse_request(gen, None, shape_scores=True, overlay=True, reference_shape=C.pocket(), max_atoms_outside=3)
    done = [PosedMol([[0.3, 0, 0]] * 4 + [[0, 0, 1.0]], z=[6] * 4 + [1]), None,
            PosedMol([[0.7, 0, 0]] * 5, z=[6] * 5), PosedMol([[float("nan"), 0, 0]] * 5, z=[6] * 5)]
    samples = postprocess.measure_finished(gen, req, done)
    assert [s.measured.atoms_outside for s in samples] == [3, None, 7, None] and len(calls) == 1
    assert calls[0][1].mesh is C.pocket()
    assert [s.measured.shape_tanimoto for s in samples] == [0.25, None, 0.25, 0.25]
    kept = postprocess.return_finished(gen, req, samples, None, 1)
    assert kept == [done[0]] and done[0].props["atoms_outside"] == 3 and done[2].props["atoms_outside"] == 7
    assert "atoms_outside" not in done[3].props


# ----------------------------------------------------------------------------------------------- restatement
def test_dropping_a_triangle_from_the_restatement_is_caught_at_its_probe_point():
    """The restatement the GPU tests compare against sees every triangle: without triangle 0, 255, 256 or the last one the
    winding number at that triangle's probe points moves by its contribution, far more than WINDING_TOL."""
    mesh = C.pocket()
    tri = C.triangles(mesh)
    F = mesh.faces.shape[0]
    for k in (0, C.TILE - 1, C.TILE, F - 1):
        pts, owners = C.probe_points(mesh, [k])
        w = R.winding(tri, pts)
        con = R.probe_contributions(tri, pts, owners)
        assert R.inside(w).tolist() == [False, True]                    # outside, then inside the outward surface
        mutant = R.winding(tri, pts, drop=k)
        np.testing.assert_allclose((w - mutant).numpy(), con.numpy(), atol=1e-12)
        assert float(con.abs().min()) > 10 * R.WINDING_TOL
        assert float((w - mutant).abs().min()) > 10 * R.WINDING_TOL
    assert [R.passes(c, 2) for c in (0, 2, 3, -1, None)] == [True, True, False, False, False]


def test_the_fp32_restatement_stays_within_the_tolerance():
    worst = 0.0
    for name in ("tetrahedron", "cube", "pocket"):
        mesh, pts, owners, p0 = C.test_points(name, 257, seed=1)
        tri = C.triangles(mesh)
        w = R.winding(tri, pts)
        assert float(((w.abs() - 0.5).abs()).min()) > 0.25              # no test point near the classification threshold
        worst = max(worst, float((R.winding(tri, pts, dtype=torch.float32).double() - w).abs().max()))
        con = R.probe_contributions(tri, pts[p0:], owners)
        assert R.WINDING_TOL < 0.1 * float(con.abs().min())
    mesh = C.pocket()                                                      # and the grid-mode run's points
    lo, hi = mesh.vertices.min(0) - 2.0, mesh.vertices.max(0) + 2.0
    pts = R.grid_points(torch.stack([torch.linspace(float(lo[k]), float(hi[k]), 8) for k in range(3)])).to(torch.float32)
    tri = C.triangles(mesh)
    worst = max(worst, float((R.winding(tri, pts, dtype=torch.float32).double() - R.winding(tri, pts)).abs().max()))
    print(f"MESH fp32 restatement: max |w32 - w64| = {worst:.3e} on the test points")
    assert 4 * worst <= R.WINDING_TOL


# ----------------------------------------------------------------------------------------------- C entries
def test_mesh_entries_refuse_bad_arguments_without_a_gpu():
    import ctypes
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check
    assert [h.mcg_mesh_splits(F) for F in (0, 1, 1024, 1025, 2048, 2049, 2488, 64 * 1024, 1 << 20, (1 << 20) + 1)] == \
        [0, 1, 1, 2, 2, 3, 3, 64, 64, 0]
    assert h.mcg_abi_version() == 4
    for args in ((None, 12, p, 5, None, 0, p, None), (p, 0, p, 5, None, 0, p, None), (p, (1 << 20) + 1, p, 5, None, 0, p, p),
                 (p, 12, p, 0, None, 0, p, None), (p, 12, p, (1 << 24) + 1, None, 0, p, None), (p, 12, p, 5, None, 0, None, None),
                 (p, 12, p, 5, p, 8, p, None), (p, 12, None, 0, None, 0, p, None),             # both / neither
                 (p, 12, None, 0, p, 1, p, None), (p, 12, None, 0, p, 257, p, None),           # n outside 2..256
                 (p, 2488, p, 5, None, 0, p, None)):                                           # three parts, no work space
        assert h.mcg_mesh_winding(*args, None) == 1, args
        assert b"mcg_mesh_winding" in h.mcg_last_error(), args
    for args in ((None, 12, p, 8, p, None), (p, 12, None, 8, p, None), (p, 12, p, 8, None, None), (p, 12, p, 1, p, None),
                 (p, 2488, p, 8, p, None)):
        assert h.mcg_mesh_occupancy(*args, None) == 1, args
        assert b"mcg_mesh_occupancy" in h.mcg_last_error(), args
    for args in ((None, 12, p, p, 2, 30, p, None), (p, 12, None, p, 2, 30, p, None), (p, 12, p, None, 2, 30, p, None),
                 (p, 12, p, p, 2, 30, None, None), (p, 0, p, p, 2, 30, p, None), (p, 12, p, p, 0, 30, p, None),
                 (p, 12, p, p, 2, 0, p, None), (p, 12, p, p, 2, 65, p, None), (p, 12, p, p, (1 << 18) + 1, 30, p, None)):
        assert h.mcg_mesh_atoms_outside(*args, None) == 1, args
        assert b"mcg_mesh_atoms_outside" in h.mcg_last_error(), args
    ok = dict(f=p, xf=p, frames=p, sxf=p, nn=p, B=3, N=27, rot=p, axes=p, n=40, best=p, which=p, flipped=p, pose=p, posed=p)
    for bad in (dict(f=None), dict(xf=None), dict(frames=None), dict(sxf=None), dict(nn=None), dict(rot=None), dict(axes=None),
                dict(best=None), dict(which=None), dict(flipped=None), dict(pose=None), dict(posed=None), dict(B=0),
                dict(N=0), dict(N=65), dict(n=1)):
        a = dict(ok, **bad)
        assert h.mcg_shape_overlay_field(a["f"], a["xf"], a["frames"], a["sxf"], a["nn"], a["B"], a["N"], a["rot"], a["axes"],
                                         a["n"], 0.8, 2.7, None, a["best"], a["which"], a["flipped"], a["pose"], a["posed"],
                                         None) == 1, bad
        assert b"mcg_shape_overlay_field" in h.mcg_last_error(), bad
    for args in ((None, p, p, 3, 27, p, 4, p, 40, p), (p, None, p, 3, 27, p, 4, p, 40, p), (p, p, p, 0, 27, p, 4, p, 40, p),
                 (p, p, p, 3, 0, p, 4, p, 40, p), (p, p, p, 3, 27, p, 0, p, 40, p), (p, p, p, 3, 27, p, 4, p, 1, p),
                 (p, p, p, 3, 27, p, 4, p, 40, None)):
        assert h.mcg_shape_tanimoto_field(*args[:9], 0.8, 2.7, args[9], None) == 1, args
        assert b"mcg_shape_tanimoto_field" in h.mcg_last_error(), args
