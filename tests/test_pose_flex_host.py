"""Flexible pose without a GPU (DESIGN.md section 6 "Flexible pose"): the restatement's torsion tree on every case against
the hand-written expectations of `flex_cases`; planted mistakes in the restatement's own walk, each caught by a rule of the
teacher-forced check the GPU test applies to the kernel's trace; the two new values of `optimise_pose`; and the contracts
of the second public header, include/mlconfgen_hip_flex.h - the ones tests/test_capi.py and
tests/test_stream_contract_host.py hold the first header to."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import flex_cases as FC
import flex_pose_ref as FR
import interactions_ref as IR
import stream_probe as SP
from conftest import REPO
from ml_conformer_generator_amd import _lib, postprocess

HEADER = os.path.join(REPO, "include", "mlconfgen_hip_flex.h")


# ----------------------------------------------------------------------------------------------- the tree
@pytest.mark.parametrize("g", FC.cases() + FC.stereo_cases(), ids=lambda g: g.name)
def test_restated_tree_equals_the_hand_written_one(g):
    t = FR.tree(g.z, g.bonds, g.n)
    assert t["torsions"] == g.torsions
    assert [sorted(s) for s in t["sides"]] == g.sides
    assert (t["found"], t["used"]) == (g.found, len(g.torsions))
    for i in range(g.n):                                                        # near: i, 1-2 and 1-3, symmetric
        assert i in t["near"][i] and all(i in t["near"][j] for j in t["near"][i])
    for (a, b), side in zip(t["torsions"], t["sides"]):
        assert b in side and a not in side and g.bonds[a, b] == 1


def test_the_cases_cover_what_the_tree_can_get_wrong():
    by = FC.by_name()
    assert by["c19"].found == 16 and by["c20"].found == 17 and len(by["c20"].torsions) == 16
    assert by["c64"].n == 64 and by["empty"].n == 0 and by["one_atom"].n == 1
    assert by["n_methylacetamide"].torsions == [] and by["ring12"].torsions == []
    assert by["butane"].torsions == [(1, 2)] and by["biphenyl"].sides == [list(range(6, 12))]         # the ties
    assert by["two_fragments"].sides == [[5, 6]]
    tree = FR.tree(by["folded_heptane"].z, by["folded_heptane"].bonds, 7)
    assert FR.clash(by["folded_heptane"].x, FR.clash_radii(by["folded_heptane"].z), tree["near"])[0] > 0.05


def test_the_modules_clash_radii_are_the_definitions():
    """`interactions.clash_radii`, the table the generation path hands the kernel, against the restatement's own, bit for
    bit: every Z of 1..35, elements outside `config.ELEMENTS` (carbon's), and Z outside the table's range."""
    import torch
    from ml_conformer_generator_amd import config
    from ml_conformer_generator_amd import interactions as IX
    assert {z: v[1] for z, v in config.ELEMENTS.items()} == FR.RCOV and IX.CLASH_PAD == FR.CLASH_PAD
    zs = list(range(1, 36)) + [53, 118, 0, -3, 119, 1000, 36]
    got = IX.clash_radii(torch.tensor(zs).view(2, -1))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, len(zs) // 2)
    want = FR.clash_radii(zs)
    assert np.array_equal(got.reshape(-1).numpy().view(np.int32), want.view(np.int32))
    assert float(got.reshape(-1)[5]) == float(np.float32(0.76 + 0.45)) == float(got.reshape(-1)[0])      # C, and H as C
    assert float(got.reshape(-1)[7]) == float(np.float32(0.66 + 0.45))                                  # O


# ----------------------------------------------------------------------------------------------- planted mistakes
def _setting(name):
    g = FC.by_name()[name]
    c = IR.cases()[2]
    x = (g.x.astype(np.float64) - g.x.astype(np.float64).mean(axis=0) + np.array([0.6, -0.3, 0.2])).astype(np.float32)
    lig = (IR.radii(g.z), np.where(g.z == 6, 4, 3).astype(np.uint8))
    return g, x, lig, (c.rec, IR.radii(c.rec_z), c.rec_t)


STEPS = 12


def test_the_restatements_own_walk_passes_its_own_rule():
    for name in ("isopentylbenzene", "folded_heptane", "biphenyl", "toluene"):
        g, x, lig, rec = _setting(name)
        w = FR.run_walk(x, lig, rec, g.z, g.bonds, STEPS, 2.0)
        bad, end = FR.check_trace(w["trace"], x, lig, rec, g.z, g.bonds, STEPS, 2.0, coords=w["coords"], angles=w["angles"])
        assert bad == [], (name, bad[:3])
        assert end["kept"] == w["kept"] and w["kept"] > 0
        assert w["w_after"] + FR.W_REP * w["c_after"] < w["w_before"] + FR.W_REP * w["c_before"]
    assert end["twisted"] == 0                                                  # toluene: nothing to turn


@pytest.mark.parametrize("name, planted, rule", [
    ("isopentylbenzene", dict(tau_sign=-1.0), "tau"),
    ("isopentylbenzene", dict(side="a"), "tau"),
    ("biphenyl", dict(tie="lower"), "tau"),
    ("biphenyl", dict(near_13=False), "clash"),
    ("stacked_benzenes", dict(clash_frame="world"), "CLASH changed its bits"),
])
def test_a_planted_mistake_is_caught(name, planted, rule):
    g, x, lig, rec = _setting(name)
    w = FR.run_walk(x, lig, rec, g.z, g.bonds, STEPS, 2.0, rules=FR.Rules(**planted))
    bad, _ = FR.check_trace(w["trace"], x, lig, rec, g.z, g.bonds, STEPS, 2.0)
    assert any(rule in b for b in bad), (planted, bad[:4])


# ----------------------------------------------------------------------------------------------- the option's values
def _flags(value, receptor=object()):
    o = types.SimpleNamespace(interaction_scores=False, max_interaction_score=None, rank_by="shape", optimise_pose=value,
                              receptor=receptor)
    return postprocess._interaction_flags(o, None)


def test_optimise_pose_values():
    assert _flags(False) == (False, 0, False)
    assert _flags(True) == (True, 64, False) and _flags(8) == (True, 8, False) and _flags(1024) == (True, 1024, False)
    assert _flags("flexible") == (True, 64, True)
    assert _flags(("flexible", 8)) == (True, 8, True) and _flags(("flexible", 1024)) == (True, 1024, True)
    for bad in (("flexible", 0), ("rigid", 8), ("flexible", 1025), ("flexible", True), ("flexible",), "rigid", "Flexible",
                ("flexible", 8, 1), ("flexible", 2.0), 0, 1025, 2.5, None):
        with pytest.raises(ValueError, match="optimise_pose"):
            _flags(bad)
    with pytest.raises(ValueError, match="needs a receptor"):
        _flags("flexible", receptor=None)
    o = types.SimpleNamespace(interaction_scores=False, max_interaction_score=None, rank_by="shape",
                              optimise_pose=("flexible", 4), receptor=object())
    with pytest.raises(ValueError, match="finisher"):
        postprocess._interaction_flags(o, "rdkit")
    assert postprocess.Request.__dataclass_fields__["optimise_flexible"].default is False


# ----------------------------------------------------------------------------------------------- the second header
def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mcg_[a-z0-9_]+)\s*\(", text)))


def test_flex_header_and_binding_agree():
    assert declared_symbols() == sorted(_lib.FLEX_SIGNATURES) == ["mcg_receptor_optimise_flex", "mcg_torsion_tree"]
    assert not set(_lib.FLEX_SIGNATURES) & set(_lib.SIGNATURES)


def test_library_exports_the_flex_symbols_with_their_signatures():
    h = _lib.lib()
    for name, (res, args) in _lib.FLEX_SIGNATURES.items():
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_flex_header_is_plain_c_and_cxx(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mlconfgen_hip_flex.h"\nint main(void) { return MCG_FLEX_MAX_TORSIONS == 0 || mcg_abi_version() == 0; }\n')
    inc = os.path.join(REPO, "include")
    if shutil.which("gcc"):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    if shutil.which("g++"):
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_flex_argument_errors_do_not_need_a_gpu():
    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert h.mcg_torsion_tree(None, p, p, 1, 8, p, p, p, p, None) == 1 and b"mcg_torsion_tree" in h.mcg_last_error()
    assert h.mcg_torsion_tree(p, p, p, 1, 65, p, p, p, p, None) == 1
    assert h.mcg_torsion_tree(p, p, p, -1, 8, p, p, p, p, None) == 1
    assert h.mcg_torsion_tree(p, p, p, 0, 8, p, p, p, p, None) == 0             # B = 0 launches nothing
    ok = [p, p, p, p, 1, 8, p, p, 10, None, 4, 2.0, p, p, p, p, p, p, p, p, p, None, None, None]
    for at, value in ((0, None), (12, None), (16, None), (20, None), (4, 0), (5, 65), (8, 0), (10, 1025), (10, -1),
                      (11, -1.0), (11, float("nan")), (11, float("inf"))):
        args = list(ok)
        args[at] = value
        assert h.mcg_receptor_optimise_flex(*args) == 1, (at, value)
        assert b"mcg_receptor_optimise_flex" in h.mcg_last_error()


# ----------------------------------------------------------------------------------------------- the stream contract
def test_every_stream_taking_flex_entry_is_run_on_a_side_stream():
    import test_pose_flex_stream_gpu as G
    entries = SP.stream_entries(HEADER)
    assert entries == ["mcg_torsion_tree", "mcg_receptor_optimise_flex"]
    assert set(entries) == set(G.COVERAGE)
    for name, (test, arrangements) in G.COVERAGE.items():
        assert callable(getattr(G, test)) and arrangements == "AB", name
