"""Pockets from the receptor without a GPU (DESIGN.md section 6 "Pockets from the receptor"): the host pipeline of
`pocket.py` on hand-made masks and on the restatement's masks of the carved block (tests/pocket_cases.py, tests/pocket_ref.py);
planted mistakes in the restatement, each caught by the comparison the GPU test applies to the kernel; `reference_shape=Pocket`
through `parse_request`; and the contracts of the third public header, include/mlconfgen_hip_pocket.h - the ones
tests/test_capi.py and tests/test_stream_contract_host.py hold the first header to."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import pocket_cases as PC
import pocket_ref as PR
import stream_probe as SP
from conftest import REPO
from ml_conformer_generator_amd import _lib, cheminformatics, postprocess
from ml_conformer_generator_amd import mesh as M
from ml_conformer_generator_amd import pocket as PK

HEADER = os.path.join(REPO, "include", "mlconfgen_hip_pocket.h")
FULL = np.uint32((1 << 26) - 1)               # every ray blocked, not occupied: a pocket point at any threshold
RECEPTOR = (np.array([[30.0, 0.0, 0.0], [0.0, 30.0, 0.0]]), np.array([6, 8]))


# ----------------------------------------------------------------------------------------------- hand-made masks
def _masks(n, cells, value=FULL):
    """Masks [n^3] that are 0 (buriedness 0: no pocket point) except `value` at `cells`, given relative to the centre."""
    m = np.zeros((n, n, n), dtype=np.uint32)
    c = n // 2
    for a, b, l in cells:
        m[c + a, c + b, c + l] = value
    return m.reshape(-1)


def _pocket(cells, radius=4.0, spacing=1.0, probe=0.5, center=(0.0, 0.0, 0.0), value=FULL, min_buriedness=14):
    n = PK.grid_size(radius, spacing)
    return PK.pocket_from_masks(_masks(n, cells, value), RECEPTOR, center, radius, spacing, probe, 8.0, min_buriedness)


def _holds(p, expected_cells):
    """What every produced pocket must satisfy: its mesh is what the unmodified `load_mesh` makes of its arrays, and the
    mesh's volume is the cells'."""
    again = M.load_mesh((p.vertices, p.faces))
    assert np.array_equal(again.vertices, p.mesh.vertices) and np.array_equal(again.faces, p.mesh.faces)
    assert M.load_mesh(p) is not None                                   # a Pocket is "an object with both"
    assert p.cells == expected_cells and p.volume == p.cells * p.spacing ** 3
    volume = M.mass_properties(p.mesh)["volume"]
    assert abs(volume - p.volume) <= 1e-9 * p.volume, (volume, p.volume)
    assert p.mesh.vertices.dtype == np.float32 and p.masks.dtype == np.uint32
    return p


def test_grid_and_directions():
    assert PK.grid_size(10.0, 1.0) == 21 and PK.grid_size(12.0, 1.0) == 25 and PK.grid_size(0.5, 1.0) == 1
    assert PK.grid_size(63.0, 1.0) == 127
    for radius, spacing in ((64.0, 1.0), (10.0, 0.1)):
        with pytest.raises(ValueError, match="grid points per axis"):
            PK.grid_size(radius, spacing)
    assert PK.DIRECTIONS.shape == (26, 3) and np.allclose(np.linalg.norm(PK.DIRECTIONS, axis=1), 1.0, atol=1e-15)
    assert np.array_equal(PK.DIRECTIONS, PR.directions())
    assert np.array_equal(PK.DIRECTIONS[::-1], -PK.DIRECTIONS)           # direction 25 - k is minus direction k
    assert np.array_equal(np.sign(PK.DIRECTIONS[0]), [-1, -1, -1]) and np.array_equal(np.sign(PK.DIRECTIONS[1]), [-1, -1, 0])
    pts = PK.grid_points(5, 0.5)
    assert np.array_equal(pts, PR.grid_points(5, 0.5)) and np.array_equal(pts[(2 * 5 + 2) * 5 + 2], [0, 0, 0])
    assert np.array_equal(pts[1], [-1.0, -1.0, -0.5])                    # the last index is the fastest
    assert PK.buriedness(np.array([0, 1, 0x80000003, 0x03FFFFFF, 0xFFFFFFFF], dtype=np.uint32)).tolist() == [0, 1, 2, 26, 26]


def test_the_centre_is_the_seed_and_one_cell_is_a_cube():
    p = _holds(_pocket([(0, 0, 0)]), 1)
    assert p.n_centres == 1 and p.cells_filled == 0 and len(p.faces) == 12 and p.mean_buriedness == 26.0
    assert np.array_equal(np.unique(p.vertices), [-0.5, 0.5])


def test_seed_snapping_and_its_refusal():
    # the centre is no pocket point; the nearest one is 2 A away, on both sides: the lower flat index is taken
    left, right = [(-2, 0, 0), (-3, 0, 0)], [(2, 0, 0), (3, 0, 0), (3, 1, 0)]
    p = _holds(_pocket(left + right), 2)
    assert p.n_centres == 2 and float(p.vertices[:, 0].max()) == -1.5
    assert _pocket(right).n_centres == 3
    p = _pocket([(0, 0, 0), (2, 0, 0), (3, 0, 0)])                       # the centre itself: nothing is snapped to
    assert p.n_centres == 1
    # beyond 3 A: refused, with the centre's buriedness and whether it is occupied
    with pytest.raises(ValueError, match=r"no pocket at the centre: its buriedness is 0 of 26 .* it is not occupied"):
        _pocket([(4, 0, 0)])
    occupied = _masks(9, [(4, 0, 0)])
    occupied[(4 * 9 + 4) * 9 + 4] = np.uint32(0x80000000 | 0x1F)
    with pytest.raises(ValueError, match=r"buriedness is 5 of 26 .* it is occupied"):
        PK.pocket_from_masks(occupied, RECEPTOR, (0, 0, 0), 4.0, 1.0, 0.5, 8.0, 14)
    with pytest.raises(ValueError, match="no pocket at the centre"):    # buried enough, but occupied: no pocket point
        _pocket([(0, 0, 0)], value=np.uint32(0x80000000) | FULL)
    with pytest.raises(ValueError, match="no pocket at the centre"):    # free, but under the threshold
        _pocket([(0, 0, 0)], value=np.uint32((1 << 13) - 1))
    assert _pocket([(0, 0, 0)], value=np.uint32((1 << 14) - 1)).n_centres == 1
    with pytest.raises(ValueError, match="masks holds"):
        PK.pocket_from_masks(np.zeros(8, dtype=np.uint32), RECEPTOR, (0, 0, 0), 4.0, 1.0, 0.5, 8.0, 14)


def test_a_diagonal_neighbour_is_not_joined():
    p = _holds(_pocket([(0, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 1)]), 2)
    assert p.n_centres == 2                                             # (0,0,0) - (0,0,1); the edge neighbours stay out


def test_the_radius_cap():
    path = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (3, 1, 0), (3, 2, 0), (3, 3, 0), (4, 0, 0), (4, 1, 0)]
    p = _holds(_pocket(path), 7)                                        # (3,3,0) and (4,1,0) lie beyond 4 A
    assert p.n_centres == 7 and float(p.vertices[:, 1].max()) == 2.5 and float(p.vertices[:, 0].max()) == 4.5


def test_dilation_is_not_clipped_at_the_grid_edge():
    line = [(k, 0, 0) for k in range(5)]                                # up to the last grid point of the axis
    p = _holds(_pocket(line, probe=1.4), 27)                            # pad 1: a "plus" of 7 cells on each centre
    assert p.n_centres == 5 and p.cells_filled == 0
    assert float(p.vertices[:, 0].max()) == 5.5 and float(p.vertices[:, 0].min()) == -1.5
    half = _holds(_pocket([(k, 0, 0) for k in range(9)], probe=0.7, spacing=0.5, center=(1.5, -2.0, 0.25)), 9 * 5 + 2)
    assert float(half.vertices[:, 0].max()) == 1.5 + 8 * 0.5 + 0.5 + 0.25 and half.volume == 47 * 0.125


def test_edge_repair_of_two_diagonal_cells():
    bare = np.zeros((2, 2, 1), dtype=bool)
    bare[0, 0, 0] = bare[1, 1, 0] = True
    with pytest.raises(ValueError, match="watertight"):                 # what the repair is for
        M.load_mesh(PK.cells_mesh(np.pad(bare, ((0, 0), (0, 0), (0, 1))), 0, 2, 1.0, (0, 0, 0)))
    fixed, added = PK.repair_edges(bare)
    assert added == 2 and bool(fixed.all()) and int(bare.sum()) == 2    # the input is left alone
    # through the pipeline: a 6-connected path whose ends touch along an edge in the plane below
    p = _holds(_pocket([(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (1, 1, 0)]), 7)
    assert p.n_centres == 5 and p.cells_filled == 2
    # a chain of repairs: each fill makes the next diagonal
    stair = np.zeros((3, 3, 3), dtype=bool)
    stair[0, 0, 0] = stair[1, 1, 0] = stair[2, 0, 1] = True
    fixed, added = PK.repair_edges(stair)
    assert added > 2 and PK.repair_edges(fixed)[1] == 0
    M.load_mesh(PK.cells_mesh(fixed, 0, 3, 1.0, (0, 0, 0)))


def test_a_vertex_only_contact_survives():
    cells = [(0, 0, 0), (-1, 0, 0), (-1, 0, 1), (-1, 0, 2), (0, 0, 2), (1, 0, 2), (1, 1, 2), (1, 1, 1)]
    p = _holds(_pocket(cells), 8)
    assert p.n_centres == 8 and p.cells_filled == 0
    corner = np.array([0.5, 0.5, 0.5], dtype=np.float32)                # where (0,0,0) and (1,1,1) touch, and nothing else
    at = np.flatnonzero((p.vertices == corner).all(axis=1))
    assert at.size == 1 and int((p.faces == at[0]).any(axis=1).sum()) >= 6


# ----------------------------------------------------------------------------------------------- the carved block
@functools.lru_cache(maxsize=None)
def _block_masks():
    xyz, z = PC.block()
    s = PC.BLOCK
    m, margin = PR.masks(xyz, PC.radii(z), PK.grid_size(s["radius"], s["spacing"]), s["spacing"], s["probe"], s["reach"])
    m.setflags(write=False)
    margin.setflags(write=False)
    return m, margin


def test_carved_block_figures():
    xyz, z = PC.block()
    assert len(z) == 2152
    m, margin = _block_masks()
    s = PC.BLOCK
    p = PK.pocket_from_masks(m, (xyz, z), (0.0, 0.0, 0.0), **s)
    _holds(p, 739)
    assert (p.n_centres, p.cells - p.cells_filled, p.cells_filled, len(p.faces), p.volume) == (405, 725, 14, 1448, 739.0)
    pic = M.mass_properties(p.mesh, 0.02)["principal_inertia_components"]
    assert np.round(pic).tolist() == [143.0, 250.0, 257.0]
    assert cheminformatics.solid_reference(p).mesh is p.mesh
    # the share of (point, test) pairs the GPU comparison leaves out at eps = 1e-3, and of points that hold one
    assert abs(float((margin < 1e-3).mean()) - 0.0021) < 1e-4 and abs(float((margin < 1e-3).any(axis=1).mean()) - 0.046) < 1e-3
    # every unfilled solid cell is clear of every van der Waals sphere
    n = PK.grid_size(s["radius"], s["spacing"])
    centres, seed = PK.pocket_centres(m, n, s["spacing"], s["radius"], s["min_buriedness"])
    assert seed == (n ** 3) // 2 and bool(centres[n // 2, n // 2, n // 2])
    solid, pad = PK.dilate(centres, s["spacing"], s["probe"])
    assert int(solid.sum()) == 725 and pad == 1
    cells = (np.argwhere(solid) - pad - (n - 1) / 2) * s["spacing"]
    gap = np.linalg.norm(cells[:, None, :] - xyz[None, :, :], axis=2) - PC.radii(z).astype(np.float64)[None, :]
    assert float(gap.min()) >= 0.0, float(gap.min())


# ----------------------------------------------------------------------------------------------- planted mistakes
EPS = 1e-3


@functools.lru_cache(maxsize=None)
def _small():
    xyz, z = PC.block()
    return PR.masks(xyz, PC.radii(z), 9, 1.0, 1.4, 8.0)


def test_the_restatement_passes_its_own_comparison():
    m, margin = _small()
    wrong, left_out = PR.compare(m, m, margin, EPS)
    assert wrong == 0 and left_out <= 0.01
    assert int((m & PK.OCCUPIED != 0).sum()) > 0 and int(PK.buriedness(m).min()) < int(PK.buriedness(m).max())


@pytest.mark.parametrize("planted", [dict(clamp=False), dict(probe_in_occupancy=False), dict(dropped_direction=7)],
                         ids=["no clamp of t", "probe left out of occupancy", "one direction dropped"])
def test_a_planted_mistake_is_caught(planted):
    xyz, z = PC.block()
    m, margin = _small()
    bad, _ = PR.masks(xyz, PC.radii(z), 9, 1.0, 1.4, 8.0, rules=PR.Rules(**planted))
    wrong, _ = PR.compare(bad, m, margin, EPS)
    assert wrong > 0, planted


# ----------------------------------------------------------------------------------------------- reference_shape=Pocket
GEN = types.SimpleNamespace(finisher=None)
RECEPTOR_OPTIONS = (dict(max_receptor_clashes=0), dict(relieve_clashes=4), dict(interaction_scores=True),
                    dict(max_interaction_score=0.0), dict(interaction_scores=True, rank_by="interaction"),
                    dict(optimise_pose=4), dict(optimise_pose="flexible"), dict(optimise_pose=("flexible", 8)))


def test_a_pocket_brings_its_own_receptor():
    p = _pocket([(0, 0, 0), (1, 0, 0)])
    with pytest.raises(ValueError, match="receptor cannot be combined with reference_shape"):
        postprocess.parse_request(GEN, None, reference_shape=p, receptor=RECEPTOR, overlay=True)
    want = RECEPTOR[0].astype(np.float32)
    for options in RECEPTOR_OPTIONS + (dict(add_hydrogens=True), {}):
        req = postprocess.parse_request(GEN, None, reference_shape=p, overlay=True, **options)
        assert isinstance(req.reference, cheminformatics.SolidReference) and req.reference.mesh is p.mesh
        assert np.array_equal(req.receptor[0].numpy(), want) and req.receptor[1].tolist() == [6, 8], options
        assert (req.typed_receptor is not None) == req.scores_interactions
    req = postprocess.parse_request(GEN, None, reference_shape=p, overlay=True, relieve_clashes=4, optimise_pose=("flexible", 8),
                                    max_receptor_clashes=2, max_atoms_outside=3)
    assert (req.relief_steps, req.optimise_steps, req.optimise_flexible, req.max_receptor_clashes) == (4, 8, True, 2)
    assert req.max_atoms_outside == 3 and req.scores_interactions
    # a typed triple is kept as given, so the interaction stage reads its types
    typed = dataclass_replace(p, receptor=(RECEPTOR[0], RECEPTOR[1], np.array([4, 2])))
    req = postprocess.parse_request(GEN, None, reference_shape=typed, overlay=True, interaction_scores=True)
    assert req.typed_receptor is not None and req.receptor[1].tolist() == [6, 8]


def dataclass_replace(p, **changes):
    import dataclasses
    return dataclasses.replace(p, **changes)


def test_a_pocket_without_receptor_options_is_a_mesh():
    p = _pocket([(0, 0, 0), (1, 0, 0)])
    req = postprocess.parse_request(GEN, None, reference_shape=p)       # the plain generation call: nothing reads the receptor
    assert req.reference.mesh is p.mesh and req.receptor is None and not req.measures
    req = postprocess.parse_request(GEN, None, reference_shape=p, shape_scores=True)
    assert req.receptor is None and req.scores_shape
    assert torch.equal(cheminformatics.solid_reference(p).triangles, cheminformatics.solid_reference(p.mesh).triangles)


def test_the_refusals_apply_unchanged():
    p = _pocket([(0, 0, 0), (1, 0, 0)])
    for options in RECEPTOR_OPTIONS:                                    # not posed: not in the receptor's frame
        with pytest.raises(ValueError, match="needs overlay=True"):
            postprocess.parse_request(GEN, None, reference_shape=p, **options)
    with pytest.raises(ValueError, match="refine_overlay cannot be combined with reference_shape"):
        postprocess.parse_request(GEN, None, reference_shape=p, overlay=True, refine_overlay=True)
    with pytest.raises(ValueError, match="finisher"):
        postprocess.parse_request(types.SimpleNamespace(finisher="rdkit"), None, reference_shape=p, overlay=True, optimise_pose=4)
    with pytest.raises(ValueError, match="rank_by='interaction' needs interaction_scores"):
        postprocess.parse_request(GEN, None, reference_shape=p, overlay=True, rank_by="interaction")
    with pytest.raises(ValueError, match="cannot be combined with reference_conformer"):
        postprocess.parse_request(GEN, torch.zeros(4, 3), reference_shape=p)
    for mesh in (p.mesh, (p.vertices, p.faces)):                       # a plain mesh refuses them exactly as before
        for options in RECEPTOR_OPTIONS:
            with pytest.raises(ValueError, match="needs a receptor|cannot be combined with reference_shape"):
                postprocess.parse_request(GEN, None, reference_shape=mesh, overlay=True, **options)
        with pytest.raises(ValueError, match="receptor cannot be combined with reference_shape"):
            postprocess.parse_request(GEN, None, reference_shape=mesh, overlay=True, receptor=RECEPTOR)
    assert len(postprocess.REQUEST_KEYWORDS) == 37


def test_find_pocket_checks_its_arguments_before_any_device_work():
    for bad in (dict(center=(0, 0)), dict(center=(0, 0, float("nan"))), dict(center="here"), dict(radius=0), dict(radius=-1.0),
                dict(spacing=0.0), dict(spacing=float("inf")), dict(probe=True), dict(probe=0), dict(reach=float("nan")),
                dict(min_buriedness=27), dict(min_buriedness=-1), dict(min_buriedness=14.0), dict(radius=64.0)):
        kw = dict(dict(center=(0.0, 0.0, 0.0)), **bad)
        with pytest.raises(ValueError):
            PK.find_pocket(RECEPTOR, **kw)
    with pytest.raises(ValueError, match="receptor"):
        PK.find_pocket("no atoms here", (0, 0, 0))
    with pytest.raises(ValueError, match="splits"):
        PK.ray_masks(RECEPTOR, (0, 0, 0), splits=257)
    assert PK.default_splits(21, 2152) == 9 and PK.default_splits(41, 100_000) == 3 and PK.default_splits(1, 1) == 1
    import ml_conformer_generator_amd as pkg
    assert pkg.find_pocket is PK.find_pocket and pkg.Pocket is PK.Pocket and "find_pocket" in pkg.__all__


# ----------------------------------------------------------------------------------------------- the third header
def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mcg_[a-z0-9_]+)\s*\(", text)))


def test_pocket_header_and_binding_agree():
    assert declared_symbols() == sorted(_lib.POCKET_SIGNATURES) == ["mcg_pocket_masks"]
    assert not set(_lib.POCKET_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.FLEX_SIGNATURES))
    text = open(HEADER).read()
    for name, value in (("MCG_POCKET_MAX_N", PK.MAX_N), ("MCG_POCKET_DIRECTIONS", PK.N_DIRECTIONS),
                        ("MCG_POCKET_MAX_SPLITS", PK.MAX_SPLITS)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value
    assert int(re.search(r"#define MCG_POCKET_OCCUPIED (0x[0-9a-f]+)u", text).group(1), 16) == int(PK.OCCUPIED)


def test_library_exports_the_pocket_symbols_with_their_signatures():
    h = _lib.lib()
    for name, (res, args) in _lib.POCKET_SIGNATURES.items():
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_pocket_header_is_plain_c_and_cxx(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mlconfgen_hip_pocket.h"\n'
                   "int main(void) {\n"
                   "  int (*a)(const float*, int, const float*, int, float, float, float, int, uint32_t*, void*) = mcg_pocket_masks;\n"
                   "  return a == 0 || MCG_POCKET_MAX_N == 0 || MCG_POCKET_OCCUPIED == 0 || mcg_abi_version() == 0;\n}\n")
    inc = os.path.join(REPO, "include")
    assert shutil.which("gcc") or shutil.which("g++")
    if shutil.which("gcc"):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    if shutil.which("g++"):
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_pocket_argument_errors_do_not_need_a_gpu():
    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = [p, 10, p, 21, 1.0, 1.4, 8.0, 4, p, None]
    for at, value in ((0, None), (8, None), (1, 0), (1, -1), (1, (1 << 17) + 1), (3, 0), (3, 128), (3, -5), (4, 0.0), (4, -1.0),
                      (4, float("nan")), (4, float("inf")), (5, 0.0), (5, float("nan")), (6, -0.0), (6, float("inf")),
                      (7, 0), (7, 257), (7, -1)):
        args = list(ok)
        args[at] = value
        assert h.mcg_pocket_masks(*args) == 1, (at, value)
        assert b"mcg_pocket_masks" in h.mcg_last_error()


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_pocket`: the entry's argument checks in a stand-alone program under host-side ASan + UBSan, on the CPU."""
    exe = str(tmp_path / "pocket_arg_check")
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_pocket", f"POCKET_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 not refused" in ran.stdout, ran.stdout + ran.stderr


def test_the_kernel_shares_the_tile_list_and_is_built():
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    text = open(os.path.join(csrc, "mcg_pocket.hip")).read()
    assert '#include "mcg_receptor_tiles.h"' in text and "build_tile_list(" in text
    assert "asm" not in text and "fp contract(off)" in text
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "mcg_pocket.hip" in make and "mlconfgen_hip_pocket.h" in make


# ----------------------------------------------------------------------------------------------- the stream contract
def test_every_stream_taking_pocket_entry_is_run_on_a_side_stream():
    import test_pocket_stream_gpu as G
    entries = SP.stream_entries(HEADER)
    assert entries == ["mcg_pocket_masks"]
    assert set(entries) == set(G.COVERAGE)
    for name, (test, arrangements) in G.COVERAGE.items():
        assert callable(getattr(G, test)) and arrangements == "AB", name
