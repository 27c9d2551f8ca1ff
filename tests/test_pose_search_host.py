"""Pose search without a GPU (DESIGN.md section 6 "Pose search"): the restatement's uniforms against Philox words computed by
hand; planted mistakes in the restatement's own starts and choice, each failing the pass rule the GPU test applies to the
kernels; the new values of `optimise_pose` and what `parse_request` refuses; and the contracts of the fourth public header,
include/mlconfgen_hip_search.h - the ones tests/test_pose_flex_host.py holds the second header to."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import flex_cases as FC
import flex_pose_ref as FR
import pose_search_ref as SR
from conftest import REPO
from ml_conformer_generator_amd import _lib, postprocess
from ml_conformer_generator_amd import interactions as IX
from test_interactions_host import _receptor
from test_shape_overlay_host import _ref, _shell_generator

HEADER = os.path.join(REPO, "include", "mlconfgen_hip_search.h")
F32 = np.float32
BY_NAME = FC.by_name()


# ----------------------------------------------------------------------------------------------- the uniforms
def _philox_by_hand(counter, key):
    """Philox4x32-10 in plain Python integers, written from the paper: no numpy, no shared text with `seeding`."""
    c, (k0, k1) = list(counter), key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
    return c


def test_the_hand_philox_gives_the_known_answers():
    assert _philox_by_hand((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _philox_by_hand((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _philox_by_hand((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


@pytest.mark.parametrize("seed, sid, s", [(0, 0, 1), (7, 5, 3), ((1 << 64) - 1, (1 << 32) - 1, 63), (0x1234567890ABCDEF, 17, 8)])
def test_uniforms_are_the_hand_computed_words(seed, sid, s):
    want = []
    for j in range(6):
        w = _philox_by_hand((sid, s, j, 0xFFFFFFFE), (seed & 0xFFFFFFFF, seed >> 32))
        want += [(v >> 8) / float(1 << 24) for v in w]
    got = SR.uniforms(seed, sid, s)
    assert got.dtype == F32 and got.tolist() == want and all(0.0 <= v < 1.0 for v in want)
    assert not SR.uniforms(seed, sid, 0).any()                                  # start 0 draws nothing
    # a planted wrong counter word (the size draw's) gives other uniforms: bit equality, the GPU test's rule, fails
    assert SR.uniforms(seed, sid, s, SR.Rules(counter_word=0xFFFFFFFF)).tolist() != want
    assert SR.COUNTER_WORD == IX.SEARCH_COUNTER_WORD == 0xFFFFFFFE


# ----------------------------------------------------------------------------------------------- the starts
def _row(name):
    g = BY_NAME[name]
    x = (g.x.astype(np.float64) - g.x.astype(np.float64).mean(axis=0) + np.array([0.6, -0.3, 0.2])).astype(F32)
    return g, x, FR.tree(g.z, g.bonds, g.n)


def _as_device(st):
    """A start rounded to what a kernel would hand back."""
    return dict(coords=st["coords"].astype(F32), xform=np.concatenate([st["R"].reshape(9), st["t"]]).astype(F32),
                angles=st["angles"].astype(F32))


@pytest.mark.parametrize("name", ["hexane", "isopentylbenzene", "toluene", "one_atom", "c20"])
def test_the_restatements_own_starts_pass_their_rule(name):
    g, x, t = _row(name)
    for s in (0, 1, 5):
        want = SR.start(x, t, 11, 3, s, 2.0, math.pi)
        bad, _ = SR.starts_pass(_as_device(want), want, SR.start_bound(x, t, want["u"], 2.0, s))
        assert bad == [], (s, bad)
        if s == 0:
            assert np.array_equal(want["coords"], x.astype(np.float64)) and not want["angles"].any()
        else:
            # a start is the input turned and shifted: the bond lengths survive, the centroid moves by at most `spread`
            for i in range(g.n):
                for j in range(i + 1, g.n):
                    if g.bonds[i, j]:
                        assert abs(np.linalg.norm(want["coords"][i] - want["coords"][j]) -
                                   np.linalg.norm(x[i].astype(np.float64) - x[j])) < 1e-9
            assert np.linalg.norm(want["coords"].mean(axis=0) - x.astype(np.float64).mean(axis=0)) <= 2.0 + 1e-9 or t["used"]
            assert (np.abs(want["angles"][: t["used"]]) <= math.pi).all() and not want["angles"][t["used"]:].any()


def test_torsions_turned_in_another_order():
    """Turns about CURRENT axes are changes of dihedral angles: in exact arithmetic they commute, so the descending order
    gives the same start and no rule on coordinates can tell it from the ascending one (the order is fixed for the bits,
    not for the geometry).  What an order-blind implementation does get wrong is the axis: turning, in ascending order,
    about the axes as they CAME fails the rule."""
    for name in ("isopentylbenzene", "hexane", "c20"):                         # nested sides, sides at both ends, 16 deep
        g, x, t = _row(name)
        want = SR.start(x, t, 11, 3, 2, 2.0, math.pi)
        bound = SR.start_bound(x, t, want["u"], 2.0, 2)
        other = SR.start(x, t, 11, 3, 2, 2.0, math.pi, SR.Rules(torsion_order="descending"))
        assert np.abs(other["coords"] - want["coords"]).max() < 1e-9, name
        wrong = SR.start(x, t, 11, 3, 2, 2.0, math.pi, SR.Rules(axes="input"))
        bad, _ = SR.starts_pass(_as_device(wrong), want, bound)
        assert any(b.startswith("start_xyz") for b in bad), (name, bad)


def test_spread_and_max_turn_of_zero():
    g, x, t = _row("hexane")
    st = SR.start(x, t, 2, 9, 4, 0.0, 0.0)
    assert np.array_equal(st["R"], np.eye(3)) and np.allclose(st["t"], 0, atol=1e-12)
    twisted = FR.twist(x.astype(np.float64) - x.astype(np.float64).mean(axis=0), st["angles"], t) + x.astype(np.float64).mean(axis=0)
    assert np.abs(st["coords"] - twisted).max() < 1e-9                         # the torsioned input, nothing else


# ----------------------------------------------------------------------------------------------- the choice
def test_the_choice_and_its_planted_mistakes():
    nan = float("nan")
    assert SR.choose([3.0, 1.0, 2.0]) == 1 and SR.choose([1.0, 1.0, 2.0]) == 0 and SR.choose([2.0, 1.0, 1.0]) == 1
    assert SR.choose([0.0, -0.0]) == 0 and SR.choose([-0.0, 0.0]) == 0         # the zeros are equal: the lower s
    assert SR.choose([nan, 5.0, nan]) == 1 and SR.choose([nan, nan]) == -1 and SR.choose([float("inf")]) == -1
    assert SR.choose([7.0]) == 0
    # a tie going to the highest s, NaN winning: each gives another winner, so equality - the GPU test's rule - fails
    assert SR.choose([1.0, 1.0, 2.0], SR.Rules(tie="highest")) == 1 != SR.choose([1.0, 1.0, 2.0])
    assert SR.choose([3.0, nan, 1.0], SR.Rules(nan_wins=True)) == 1 != SR.choose([3.0, nan, 1.0])
    # J is one fp32 product and one fp32 sum
    w, c = F32(-0.73219), F32(0.31871)
    assert SR.objective(w, c) == F32(w + F32(F32(0.840) * c))


def test_t_composed_the_wrong_way_round_fails_the_rule():
    g = np.random.default_rng(4)
    rot = lambda: SR.rotation_row_form(SR.sphere_point(g.random(), g.random()), g.random() * 3)    # noqa: E731
    a = np.concatenate([rot().reshape(9), g.normal(size=3) * 3]).astype(F32)
    b = np.concatenate([rot().reshape(9), g.normal(size=3) * 3]).astype(F32)
    want, wrong = SR.compose(a, b), SR.compose(a, b, SR.Rules(compose="tw@Rs"))
    bR, bt = SR.compose_bound(a, b)
    assert np.abs(want.astype(F32).astype(np.float64) - want)[:9].max() <= bR
    assert np.abs(want.astype(F32).astype(np.float64) - want)[9:].max() <= bt
    assert np.abs(wrong - want)[9:].max() > bt and np.array_equal(wrong[:9], want[:9])
    x = g.normal(size=(5, 3))
    assert np.abs((x @ a[:9].reshape(3, 3).astype(np.float64) + a[9:]) @ b[:9].reshape(3, 3).astype(np.float64) + b[9:]
                  - (x @ want[:9].reshape(3, 3) + want[9:])).max() < 1e-12


def test_select_gathers_start_0_and_computes_for_another_winner():
    g = np.random.default_rng(8)
    S, n = 3, 4
    coords = g.normal(size=(S, n, 3)).astype(F32)
    xf = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (S, 1)).astype(F32)
    stats = np.zeros((S, 12), dtype=F32)
    stats[:, 1] = [-1.0, -2.0, -0.5]
    stats[:, 0], stats[:, 6] = [9.0, 8.0, 7.0], [0.5, 0.25, 0.125]
    angles = g.normal(size=(S, 16)).astype(F32)
    out = SR.select(coords, xf, stats, angles, xf, angles, coords[0], n)
    assert out["best"] == 1 and out["stats"][0] == 9.0 and out["stats"][6] == 0.5 and out["stats"][1] == -2.0
    assert np.array_equal(out["coords"], coords[1]) and np.allclose(out["angles"], 2 * angles[1].astype(np.float64))
    assert abs(out["stats"][4] - math.sqrt(((coords[1].astype(np.float64) - coords[0]) ** 2).sum() / n)) < 1e-12
    stats[:, 1] = [-3.0, -2.0, -0.5]
    out = SR.select(coords, xf, stats, angles, xf, angles, coords[0], n)
    assert out["best"] == 0 and out["gathered"] and np.array_equal(out["stats"], stats[0].astype(np.float64))


# ----------------------------------------------------------------------------------------------- the option's values
def test_optimise_pose_search_values():
    value = postprocess._optimise_pose_value
    assert value("search") == (True, True, IX.SEARCH_STARTS) == (True, True, 8)
    assert value(("search", 4)) == (True, True, 4) and value(("search", 64, 1024)) == (1024, True, 64)
    assert value(("search", 1, 1)) == (1, True, 1) and value(["search", 2, 8]) == (8, True, 2)
    assert value("flexible") == (True, True, 0) and value(("flexible", 8)) == (8, True, 0) and value(12) == (12, False, 0)
    for bad in (("search", 0), ("search", 65), ("search", True), ("search", 2.0), ("search",), ("search", 8, True),
                ("search", 8, 4, 1), "Search", ("searches", 8)):
        with pytest.raises(ValueError, match="optimise_pose"):
            value(bad)
    assert postprocess.Request.__dataclass_fields__["optimise_starts"].default == 0
    assert IX.check_starts(1) == 1 and IX.check_starts(64) == 64
    for bad in (0, 65, True, 2.0, "8", None):
        with pytest.raises(ValueError):
            IX.check_starts(bad)


def test_parse_request_reads_and_refuses_search():
    from ml_conformer_generator_amd import host_pool as HP
    gen, parse, rec = _shell_generator(), postprocess.parse_request, _receptor()
    req = parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose="search")
    assert (req.optimise_starts, req.optimise_steps, req.optimise_flexible, req.scores_interactions) == (8, 64, True, True)
    req = parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose=("search", 4, 8))
    assert (req.optimise_starts, req.optimise_steps, req.optimise_flexible) == (4, 8, True)
    assert parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose=("search", 64)).optimise_starts == 64
    for value in (True, 8, "flexible", ("flexible", 8)):                        # the other values ask for no search
        assert parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose=value).optimise_starts == 0
    for bad in (("search", 0), ("search", 65), ("search", 8, 0), ("search", True)):
        with pytest.raises(ValueError, match="optimise_pose"):
            parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose=bad)
    with pytest.raises(ValueError, match="optimise_pose needs a receptor"):
        parse(gen, _ref(), overlay=True, optimise_pose="search")
    for finisher in ("rdkit", HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                                         "finish_tag_chunk")):
        gen.finisher = finisher
        with pytest.raises(ValueError, match="optimise_pose cannot be combined with a finisher"):
            parse(gen, _ref(), overlay=True, receptor=rec, optimise_pose="search")


def test_search_pose_refuses_before_any_device_work():
    g = BY_NAME["butane"]
    z, bonds, n, x = FC.padded([g])
    args = (_receptor(), torch.from_numpy(x), torch.from_numpy(n), torch.from_numpy(z), torch.from_numpy(bonds))
    for kw in (dict(starts=0), dict(starts=65), dict(starts=True), dict(spread=-1.0), dict(spread=float("nan")),
               dict(max_turn=-0.1), dict(max_turn=3.2), dict(steps=1025), dict(max_shift=-1.0), dict(seed=-1),
               dict(sample_ids=torch.tensor([1 << 32])), dict(sample_ids=torch.tensor([0, 1]))):
        with pytest.raises((ValueError, TypeError)):
            IX.search_pose(*args, **kw)


def test_optimise_rows_hands_the_seed_and_the_ids_to_the_search():
    gen, rec = _shell_generator(), _receptor()
    req = postprocess.parse_request(gen, _ref(), overlay=True, receptor=rec, optimise_pose=("search", 4, 8))
    seen = {}

    def search(prepared, coords, n_nodes, atomic_numbers, bond_orders, starts, steps, seed, sample_ids):
        seen.update(starts=starts, steps=steps, seed=seed, ids=sample_ids)
        B = coords.shape[0]
        zero = torch.zeros(B)
        return dict(coords=coords + 1.0, rotation=torch.eye(3).repeat(B, 1, 1), translation=torch.ones(B, 3),
                    moved=torch.tensor([True, False, True]), weighted_before=zero - 1, weighted_after=zero - 2,
                    kept=torch.tensor([2, 0, 0], dtype=torch.int32), rmsd=zero + 1.7, torsions=torch.ones(B, dtype=torch.int32),
                    torsion_angles=torch.ones(B, 16), conformer_rmsd=zero + 0.1, clash_before=zero, clash_after=zero,
                    best_start=torch.tensor([0, 0, 3], dtype=torch.int32))

    gen._search_pose = search
    gen._score_placed = lambda reference, x, n: torch.full((x.shape[0],), 0.25)
    x = torch.zeros(3, 4, 3)
    pose = torch.cat([torch.eye(3).reshape(1, 9), torch.zeros(1, 3)], dim=1).repeat(3, 1)
    ids = torch.tensor([10, 11, 12])
    out = postprocess.optimise_rows(gen, req, x, torch.tensor([4, 4, 4]), torch.full((3, 4), 6), torch.zeros(3, 4, 4),
                                    pose, torch.full((3,), 0.5), ids, 7)
    assert seen == dict(starts=4, steps=8, seed=7, ids=ids)
    assert out["pose_starts"].tolist() == [4, 4, 4] and out["pose_best_start"].tolist() == [0, 0, 3]
    assert out["coords"][0].eq(1).all() and out["coords"][1].eq(0).all() and out["coords"][2].eq(1).all()
    postprocess.optimise_rows(gen, req, x, torch.tensor([4, 4, 4]), torch.full((3, 4), 6), torch.zeros(3, 4, 4), pose,
                              torch.full((3,), 0.5))
    assert seen["seed"] == 0 and seen["ids"] is None                            # no sample_seed: 0; no ids: 0..B-1


# ----------------------------------------------------------------------------------------------- the fourth header
def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mcg_[a-z0-9_]+)\s*\(", text)))


def _c_arguments(name):
    """The ctypes of an entry's parameters as the header declares them."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    params = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    kinds = []
    for p in params.split(","):
        p = " ".join(p.split())
        if "*" in p:
            kinds.append(ctypes.c_void_p)
        else:
            kinds.append({"int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}[p.split()[0]])
    return kinds


def test_search_header_and_binding_agree():
    assert declared_symbols() == sorted(_lib.SEARCH_SIGNATURES) == ["mcg_pose_search_select", "mcg_pose_starts"]
    assert not set(_lib.SEARCH_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.FLEX_SIGNATURES) | set(_lib.POCKET_SIGNATURES))
    for name, (res, args) in _lib.SEARCH_SIGNATURES.items():                    # one to one, in order
        assert res is ctypes.c_int and args == _c_arguments(name), name
    text = open(HEADER).read()
    assert re.search(r"#define MCG_SEARCH_MAX_STARTS 64\b", text) and re.search(r"#define MCG_SEARCH_PARAMS 24\b", text)
    assert '#include "mlconfgen_hip.h"' in text and '#include "mlconfgen_hip_flex.h"' in text
    assert (IX.SEARCH_MAX_STARTS, IX.SEARCH_PARAMS) == (64, 24) == (SR.MAX_STARTS, SR.PARAMS)


def test_library_exports_the_search_symbols_with_their_signatures():
    h = _lib.lib()
    for name, (res, args) in _lib.SEARCH_SIGNATURES.items():
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_search_header_is_plain_c_and_cxx(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mlconfgen_hip_search.h"\nint main(void) { return MCG_SEARCH_MAX_STARTS == 0 || '
                   'MCG_SEARCH_PARAMS == 0 || MCG_FLEX_MAX_TORSIONS == 0 || mcg_abi_version() == 0; }\n')
    inc = os.path.join(REPO, "include")
    if shutil.which("gcc"):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    if shutil.which("g++"):
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_makefile_names_both_new_files():
    text = open(os.path.join(REPO, "ml_conformer_generator_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*?)\n\S", text, flags=re.S | re.M).group(1)
    hdrs = re.search(r"^HDRS = (.*?)\n\S", text, flags=re.S | re.M).group(1)
    assert "mcg_pose_search.hip" in srcs.split() and "../../include/mlconfgen_hip_search.h" in hdrs.split()
    assert "mcg_philox.h" in hdrs.split()
    assert os.path.exists(os.path.join(REPO, "ml_conformer_generator_amd", "csrc", "mcg_pose_search.hip"))


def test_search_argument_errors_do_not_need_a_gpu():
    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = [p, p, 1, 8, p, p, p, p, 3, 4, 2.0, 1.0, p, p, p, None, None]
    assert len(ok) == len(_lib.SEARCH_SIGNATURES["mcg_pose_starts"][1])
    for at, value in ((0, None), (1, None), (4, None), (5, None), (6, None), (7, None), (12, None), (13, None), (14, None),
                      (2, 0), (2, 16385), (3, 0), (3, 65), (9, 0), (9, 65), (10, -1.0), (10, float("nan")),
                      (10, float("inf")), (11, -0.5), (11, 3.2), (11, float("nan"))):
        args = list(ok)
        args[at] = value
        assert h.mcg_pose_starts(*args) == 1, (at, value)
        assert b"mcg_pose_starts" in h.mcg_last_error()
    ok = [p, p, p, p, p, p, p, p, 1, 8, 4, p, p, p, p, p, p, None]
    assert len(ok) == len(_lib.SEARCH_SIGNATURES["mcg_pose_search_select"][1])
    for at, value in [(k, None) for k in (0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15, 16)] + \
            [(8, 0), (8, 16385), (9, 0), (9, 65), (10, 0), (10, 65)]:
        args = list(ok)
        args[at] = value
        assert h.mcg_pose_search_select(*args) == 1, (at, value)
        assert b"mcg_pose_search_select" in h.mcg_last_error()


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_search`: both entries' argument checks in a stand-alone program under host-side ASan + UBSan, on the CPU."""
    exe = str(tmp_path / "search_arg_check")
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_search", f"SEARCH_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 not refused" in ran.stdout, ran.stdout + ran.stderr


# ----------------------------------------------------------------------------------------------- the stream contract
def test_every_stream_taking_search_entry_is_run_on_a_side_stream():
    import stream_probe as SP
    import test_pose_search_stream_gpu as G
    entries = SP.stream_entries(HEADER)
    assert entries == ["mcg_pose_starts", "mcg_pose_search_select"]
    assert set(entries) == set(G.COVERAGE)
    for name, (test, arrangements) in G.COVERAGE.items():
        assert callable(getattr(G, test)) and arrangements == "AB", name
