"""Clash relief, host side (no GPU): the fp64 restatement's own sanity (gradient against finite differences, a monotone
walk that clears every clashing case of the recipe), the pass rule's mutation check, the receptor sort and the tile
spheres (the far slab really yields tiles out of reach), every refusal of the function, the option and the C entry
before any device work, the pose composition, the two new values and the moved Mols through stubbed seams on the proxy
and the object path, the same molecules on both ranks of a world-size-2 gloo run, and the header as C99 and C++."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import relief_ref as RR
from conftest import REPO
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import receptor as RC
from test_receptor_host import _object_gen, _pocket, _proxy_gen
from test_shape_overlay_host import _free_port, _no_device, _ref, _shell_generator

CASES = RR.cases()
CLASHING = [c for c in CASES if c.name != "clean"]


# ----------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", [c for c in CASES if c.name in ("n1", "n26", "R1", "multi")], ids=lambda c: c.name)
def test_restatement_force_and_torque_are_the_gradient_of_the_penalty(case):
    ri, rj = case.radii()
    x = case.x.astype(np.float64)
    p = x.mean(0)
    v = RR.seven(x, ri, case.rec, rj)
    assert v[0] > 0
    eps = 1e-6
    for k in range(3):
        e = np.zeros(3)
        e[k] = eps
        dP = (RR.seven(x + e, ri, case.rec, rj)[0] - RR.seven(x - e, ri, case.rec, rj)[0]) / (2 * eps)
        assert -dP == pytest.approx(v[1 + k], rel=1e-5, abs=1e-7)                 # F = -dP/dp
        rot = RR._rodrigues_row(np.eye(3)[k], eps)                                  # row form of a turn about axis k
        plus, minus = (x - p) @ rot + p, (x - p) @ rot.T + p
        dP = (RR.seven(plus, ri, case.rec, rj)[0] - RR.seven(minus, ri, case.rec, rj)[0]) / (2 * eps)
        assert -dP == pytest.approx(v[4 + k], rel=1e-5, abs=1e-7)                 # tau = -dP/dtheta


def test_restatement_walk_is_monotone_and_clears_every_clashing_case_within_16_trials():
    for c in CLASHING:
        ri, rj = c.radii()
        w = RR.walk(c.x, ri, c.rec, rj, 16)
        hist = np.array(w["penalty"])
        assert hist[0] > 0, c                                                      # the recipe made it clash
        assert (np.diff(hist) <= 0).all() and hist[-1] == 0.0, (c, hist.tolist())
        assert 1 <= w["accepted"] <= w["trials"] <= 16
        moved = w["coords"]
        np.testing.assert_allclose(moved, c.x.astype(np.float64) @ w["rotation"] + w["translation"], atol=1e-12)
        assert np.linalg.norm(moved.mean(0) - c.x.astype(np.float64).mean(0)) <= RC.RELIEF_MAX_SHIFT
        overlap = RR.pairs(moved, ri, c.rec, rj, margin=0.0)[0].max(axis=1)        # the clash criterion's overlap
        assert (overlap < RC.CLASH_OVERLAP - 0.19).all()
        rmsd = math.sqrt(((moved - c.x) ** 2).sum(1).mean())
        print(f"RELIEF fp64 {c}: P {hist[0]:.4g} -> 0 in {w['trials']} trials ({w['accepted']} kept), rmsd {rmsd:.2f}, "
              f"worst overlap {overlap.max():.2f}")
    clean = next(c for c in CASES if c.name == "clean")
    w = RR.walk(clean.x, *clean.radii()[:1], clean.rec, clean.radii()[1], 16)
    assert w["penalty"] == [0.0] and w["trials"] == 0 and np.array_equal(w["rotation"], np.eye(3))
    assert [c.n for c in CASES[:4]] == [1, 3, 41, 64]
    assert [len(c.rec) for c in CASES[4:8]] == [1, 255, 256, 257] and len(CASES[8].rec) > 4 * RR.TILE


def _fp32_seven(x, ri, y, rj, slip=None):
    """The seven sums evaluated pair by pair in numpy fp32 (sequential sums): what an fp32 kernel computes, up to order.
    `slip` [n,R] of -1 / 0 / +1: h moved by that many fp32 ulps of the distance."""
    f = np.float32
    x, y, ri, rj = x.astype(f), y.astype(f), ri.astype(f), rj.astype(f)
    p = x.mean(0, dtype=f)
    acc = np.zeros(7, dtype=f)
    for i in range(len(x)):
        diff = x[i] - y
        d = np.sqrt((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        h = ((ri[i] - f(RR.MARGIN)) + rj) - d
        if slip is not None:
            h = h + slip[i].astype(f) * np.spacing(d)
        for j in np.nonzero(h > 0)[0]:
            g = (h[j] + h[j]) / d[j]
            fv = g * diff[j]
            acc[0] += h[j] * h[j]
            acc[1:4] += fv
            acc[4:7] += np.cross(x[i] - p, fv).astype(f)
    return acc


def test_the_pass_rule_passes_an_ulp_slip_and_fails_real_bugs():
    failed = {"tile": 0, "radius": 0, "atom": 0}
    g = np.random.default_rng(5)
    for c in CLASHING:
        ri, rj = c.radii()
        assert RR.passes(_fp32_seven(c.x, ri, c.rec, rj), c.x, ri, c.rec, rj), c
        slip = g.integers(-1, 2, size=(c.n, len(c.rec)))
        assert RR.passes(_fp32_seven(c.x, ri, c.rec, rj, slip), c.x, ri, c.rec, rj), c     # one ulp per pair: inside
        h = np.maximum(RR.pairs(c.x, ri, c.rec, rj)[0], 0.0)
        # a wrong radius: nitrogen's for carbon's on the ligand
        assert not RR.passes(_fp32_seven(c.x, np.full(c.n, 1.55), c.rec, rj), c.x, ri, c.rec, rj), c
        failed["radius"] += 1
        # a dropped tile: the sorted receptor without the 256 atoms of the tile that holds the deepest contact
        xyzr = RC.sort_receptor(*[torch.from_numpy(a) for a in (c.rec, rj.astype(np.float32))]).numpy()
        deep = RR.pairs(c.x, ri, xyzr[:, :3], xyzr[:, 3])[0].max(axis=0).argmax()
        keep = np.arange(len(xyzr)) // RR.TILE != deep // RR.TILE
        assert not RR.passes(_fp32_seven(c.x, ri, xyzr[keep, :3], xyzr[keep, 3]), c.x, ri, c.rec, rj), c
        failed["tile"] += 1
        # an off-by-one atom: the last ligand atom never visited (seen wherever that atom is in contact)
        if c.n > 1 and h[-1].max() > 1e-3:
            got = _fp32_seven(c.x[:-1], ri[:-1], c.rec, rj)
            got[4:] = 0                                      # (its torque is about another centroid: judge P and F)
            want, bound = RR.seven(c.x, ri, c.rec, rj), RR.bounds(c.x, ri, c.rec, rj)
            assert (np.abs(got[:4] - want[:4]) > bound[:4]).any(), c
            failed["atom"] += 1
    assert failed["atom"] >= 2 and failed["tile"] == failed["radius"] == len(CLASHING)


# ----------------------------------------------------------------------------------------------- sort and tile spheres
def test_receptor_sort_ignores_the_input_order_and_spheres_hold_their_tiles():
    c = next(c for c in CASES if c.name == "multi")
    xyz, r = torch.from_numpy(c.rec), RC.vdw_radii(torch.from_numpy(c.rec_z))
    base = RC.sort_receptor(xyz, r)
    assert base.shape == (len(c.rec), 4) and base.dtype == torch.float32
    assert sorted(map(tuple, base[:, :3].tolist())) == sorted(map(tuple, xyz.tolist()))
    perm = torch.randperm(len(c.rec), generator=torch.Generator().manual_seed(1))
    assert torch.equal(RC.sort_receptor(xyz[perm], r[perm]), base)
    spheres = RC.tile_spheres(base)
    T = -(-len(c.rec) // RR.TILE)
    assert spheres.shape == (T, 4)
    for t in range(T):
        tile = base[t * RR.TILE: (t + 1) * RR.TILE].double()
        far = (tile[:, :3] - spheres[t, :3].double()).norm(dim=1) + tile[:, 3]
        assert float(far.max()) <= float(spheres[t, 3])


def test_the_far_slab_yields_tiles_out_of_reach():
    c = next(c for c in CASES if c.name == "multi")
    spheres = RC.tile_spheres(RC.sort_receptor(torch.from_numpy(c.rec), RC.vdw_radii(torch.from_numpy(c.rec_z))))
    x = torch.from_numpy(c.x)
    centre = x.mean(0)
    reach = float((x - centre).norm(dim=1).max()) + RC.RELIEF_MAX_SHIFT + RR.CARBON + spheres[:, 3]
    reach = reach + (0.05 + 1e-3 * reach)                                          # the kernel's slack
    out = (spheres[:, :3] - centre).norm(dim=1) > reach
    print(f"RELIEF multi: {int(out.sum())} of {len(spheres)} tiles out of reach")
    assert 1 <= int(out.sum()) < len(spheres)


# ----------------------------------------------------------------------------------------------- refusals
def test_relieve_clashes_refusals_happen_before_any_device_work(monkeypatch):
    from ml_conformer_generator_amd import _lib
    monkeypatch.setattr(_lib, "lib", _no_device)
    rec = (torch.tensor([[0.0, 0.0, 0.0]]), [6])
    x = torch.zeros(3, 20, 3)
    n = torch.tensor([20, 5, 0], dtype=torch.int32)
    z = torch.full((3, 42), 6)
    for r, coords, nn, zz in (((torch.zeros(1, 3), [1]), x, n, z),                 # what `receptor_overlap` refuses
                              (rec, x, torch.tensor([21, 5, 0]), z),
                              (rec, x, torch.tensor([4, 5]), z),
                              (rec, torch.zeros(2, 65, 3), torch.tensor([3, 3]), torch.full((2, 65), 6)),
                              (rec, x, n, torch.full((3, 19), 6)),
                              (rec, x, n, torch.full((2, 42), 6))):
        with pytest.raises(ValueError):
            RC.relieve_clashes(r, coords, nn, zz, device="cpu")
    for steps in (-1, 1025, True, False, 1.0, "3", None):
        with pytest.raises(ValueError, match="steps"):
            RC.relieve_clashes(rec, x, n, z, steps=steps, device="cpu")
    for shift in (-0.5, float("nan"), float("inf"), None, True, "2"):
        with pytest.raises(ValueError, match="max_shift"):
            RC.relieve_clashes(rec, x, n, z, max_shift=shift, device="cpu")
    out = RC.relieve_clashes(rec, torch.zeros(0, 20, 3), torch.zeros(0, dtype=torch.int32), torch.zeros(0, 42),
                             device="cpu", return_gradient=True)
    assert out["coords"].shape == (0, 20, 3) and out["gradient"].shape == (0, 6) and out["moved"].shape == (0,)
    assert RC.check_relief_steps(0) == 0 and RC.check_relief_steps(1024) == 1024
    assert RC.check_relief_steps(True, "relieve_clashes", 1, RC.RELIEF_STEPS) == 32
    import ml_conformer_generator_amd as pkg
    assert pkg.relieve_clashes is RC.relieve_clashes and "relieve_clashes" in pkg.__all__


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_relieve_option_refusals_happen_before_any_device_work(entry):
    gen = _shell_generator()
    gen._generate_shard = gen._score = gen._pose = gen._pair = gen._receptor_coords = _no_device
    gen._relieve = gen._score_placed = _no_device
    call = getattr(gen, entry)
    pocket = _pocket()
    for kw in (dict(overlay=True, relieve_clashes=True),                           # no receptor
               dict(relieve_clashes=8),
               dict(receptor=pocket, relieve_clashes=True),                        # a receptor, but not posed
               dict(overlay=True, receptor=pocket, relieve_clashes=0),
               dict(overlay=True, receptor=pocket, relieve_clashes=-3),
               dict(overlay=True, receptor=pocket, relieve_clashes=1025),
               dict(overlay=True, receptor=pocket, relieve_clashes=8.0),
               dict(overlay=True, receptor=pocket, relieve_clashes="32"),
               dict(overlay=True, receptor=pocket, relieve_clashes=None)):
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    req = postprocess.parse_request(gen, _ref(), overlay=True, receptor=pocket, relieve_clashes=True)
    assert req.relief_steps == 32
    assert postprocess.parse_request(gen, _ref(), overlay=True, receptor=pocket, relieve_clashes=7).relief_steps == 7
    assert postprocess.parse_request(gen, _ref(), overlay=True, receptor=pocket).relief_steps == 0


def test_relieve_entry_refuses_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check
    ok = dict(x=p, r=p, nn=p, B=3, N=27, y=p, R=100, sph=p, steps=32, margin=0.4, shift=2.0, out=p, xf=p, st=p, g=p)

    def call(**kw):
        a = dict(ok, **kw)
        return h.mcg_receptor_relieve(a["x"], a["r"], a["nn"], a["B"], a["N"], a["y"], a["R"], a["sph"], a["steps"],
                                      a["margin"], a["shift"], a["out"], a["xf"], a["st"], a["g"], None)

    for bad in (dict(x=None), dict(r=None), dict(nn=None), dict(y=None), dict(out=None), dict(xf=None), dict(st=None),
                dict(B=0), dict(B=-1), dict(B=RC.MAX_BATCH + 1), dict(N=0), dict(N=65), dict(R=0), dict(R=-5),
                dict(R=RC.MAX_RECEPTOR_ATOMS + 1), dict(steps=-1), dict(steps=1025), dict(margin=-0.1),
                dict(margin=float("nan")), dict(margin=float("inf")), dict(shift=-1.0), dict(shift=float("nan")),
                dict(shift=float("inf")), dict(sph=None, x=None), dict(g=None, st=None)):
        assert call(**bad) == 1, bad                                     # MCG_ERR_ARG = hipErrorInvalidValue
        assert b"mcg_receptor_relieve" in h.mcg_last_error(), bad
    assert "mcg_receptor_relieve" in _lib.SIGNATURES and h.mcg_abi_version() == 4


def test_relieve_entry_states_its_bounds_in_the_refusal():
    """The whole message, as it read before the walk's shared text moved into headers."""
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: the call fails its host-side check
    assert h.mcg_receptor_relieve(p, p, p, 3, 27, p, 100, p, 1025, 0.4, 2.0, p, p, p, p, None) == 1
    assert h.mcg_last_error() == (b"mcg_receptor_relieve: bad arguments (non-null buffers, 1 <= B <= 16384, 1 <= N <= 64, "
                                  b"1 <= R <= 131072, 0 <= steps <= 1024, margin and max_shift finite and >= 0)")


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_relief`: the entry's argument checks in a stand-alone program under host-side ASan + UBSan, on the CPU."""
    exe = str(tmp_path / "relief_arg_check")
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_relief", f"RELIEF_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 not refused" in ran.stdout, ran.stdout + ran.stderr


def test_header_with_the_relief_entry_is_plain_c_and_cxx(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mlconfgen_hip.h"\n'
                   "int main(void) {\n"
                   "    float v[16] = {0};\n"
                   "    int32_t n = 1;\n"
                   "    if (mcg_abi_version() == 0)\n"
                   "        return mcg_receptor_relieve(v, v, &n, 1, 1, v, 1, 0, 32, 0.4f, 2.0f, v, v, v, 0, 0);\n"
                   "    return MCG_RECEPTOR_MAX_ATOMS == 0;\n"
                   "}\n")
    inc = os.path.join(REPO, "include")
    ran = 0
    if shutil.which("gcc"):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        ran += 1
    if shutil.which("g++"):
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        ran += 1
    text = open(os.path.join(inc, "mlconfgen_hip.h")).read()
    assert "mcg_receptor_relieve(" in text and ran >= 0


# ----------------------------------------------------------------------------------------------- pose composition
def test_compose_pose_is_the_pose_followed_by_the_move():
    g = torch.Generator().manual_seed(2)

    def rotation():
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        return (q * torch.sign(torch.linalg.det(q))).float()
    B = 6
    Q, R = torch.stack([rotation() for _ in range(B)]), torch.stack([rotation() for _ in range(B)])
    d, t = torch.randn(B, 3, generator=g) * 5, torch.randn(B, 3, generator=g)
    x = torch.randn(B, 9, 3, generator=g) * 4
    pose = torch.cat([Q.reshape(B, 9), d], dim=1)
    both = postprocess.compose_pose(pose, R, t)
    one = x.double() @ both[:, :9].reshape(B, 3, 3).double() + both[:, None, 9:].double()
    two = (x.double() @ Q.double() + d[:, None].double()) @ R.double() + t[:, None].double()
    torch.testing.assert_close(one, two, rtol=0, atol=2e-5)
    assert float(torch.linalg.det(both[:, :9].reshape(B, 3, 3).double()).sub(1).abs().max()) < 1e-5
    eye = torch.eye(3).expand(B, 3, 3)
    assert torch.equal(postprocess.compose_pose(pose, eye, torch.zeros(B, 3)), pose)      # the identity changes no bit


# ----------------------------------------------------------------------------------------------- stubbed seams
SHIFT = torch.tensor([0.0, 0.0, 1.0])


def _stub_relief(calls):
    """A device-free stand-in for `relieve_clashes`: a row whose posed coords[b, 0, 1] is >= 0.45 is moved by (0, 0, 1)."""
    def run(rec, coords, n, z, steps):
        calls.append(("relieve", int(coords.shape[0]), steps))
        B, N = coords.shape[0], coords.shape[1]
        moved = coords[:, 0, 1] >= 0.45
        real = (torch.arange(N).view(1, N) < torch.as_tensor(n).view(B, 1)).unsqueeze(2)
        out = torch.where(real, torch.where(moved.view(B, 1, 1), coords + SHIFT, coords), torch.zeros(()))
        t = torch.zeros(B, 3)
        t[moved] = SHIFT
        return dict(coords=out, rotation=torch.eye(3).expand(B, 3, 3).clone(), translation=t, rmsd=moved.float(),
                    penalty_before=moved.float(), penalty_after=torch.zeros(B), accepted_steps=moved.int(), moved=moved)
    return run


def _stub_placed(calls):
    def run(ref, coords, n):
        calls.append(("placed", int(coords.shape[0])))
        return torch.full((coords.shape[0],), 0.75)    # kept on the moved rows only
    return run


def test_proxy_path_records_carry_the_relief():
    calls, contacts = [], []
    gen = _proxy_gen(contacts)
    gen._relieve = gen._score_placed = _no_device
    kw = dict(reference_conformer=_ref(), n_samples=8, overlay=True, receptor=_pocket())
    plain = gen.generate_conformers(**kw)                                          # the option off: the seams are not touched
    assert all(m.relief_rmsd is None and m.receptor_clashes_before is None for m in plain)
    again = gen.generate_conformers(relieve_clashes=False, **kw)
    for a, b in zip(plain, again):
        torch.testing.assert_close(a.coords, b.coords, rtol=0, atol=0, equal_nan=True)
        assert (a.sample_id, a.receptor_contacts, a.overlay_tanimoto) == (b.sample_id, b.receptor_contacts,
                                                                           b.overlay_tanimoto) or a.sample_id == 5
    gen._relieve, gen._score_placed = _stub_relief(calls), _stub_placed(calls)
    pose, score = gen._pose, gen._score

    def posing(*a, **k):
        calls.append(("pose",))
        return pose(*a, **k)

    def scoring(*a, **k):
        calls.append(("score",))
        return score(*a, **k)
    gen._pose, gen._score = posing, scoring
    got = gen.generate_conformers(relieve_clashes=5, shape_scores=True, **kw)
    assert calls == [("pose",), ("relieve", 8, 5), ("placed", 8), ("score",)]       # behind the pose, before the rest
    assert [m.sample_id for m in got] == [m.sample_id for m in plain] == [0, 1, 2, 4, 5, 6, 7]
    n_moved = 0
    for a, b in zip(plain, got):
        k = (7 * b.sample_id) % 10
        if b.sample_id == 5:                                                       # pose failed: left alone, no values
            assert b.relief_rmsd is None and b.receptor_clashes_before is None and b.pose is None
            torch.testing.assert_close(a.coords, b.coords, rtol=0, atol=0, equal_nan=True)
            continue
        assert b.receptor_clashes_before == a.receptor_clashes == k
        assert b.receptor_clashes == k                                             # (the stub contacts ignore z)
        if k >= 5:
            n_moved += 1
            assert torch.equal(b.coords, a.coords + SHIFT) and b.relief_rmsd == 1.0
            assert torch.equal(b.pose[0], a.pose[0]) and torch.equal(b.pose[1], a.pose[1] + SHIFT)
            assert b.overlay_tanimoto == pytest.approx(0.75)
        else:                                                                      # unmoved: every bit it had
            assert torch.equal(b.coords, a.coords) and b.relief_rmsd == 0.0
            assert torch.equal(b.pose[0], a.pose[0]) and torch.equal(b.pose[1], a.pose[1])
            assert b.overlay_tanimoto == a.overlay_tanimoto
    assert n_moved == 3
    sharded = gen.generate_conformers_sharded(relieve_clashes=True, **kw)         # no process group: one rank
    assert [m.relief_rmsd for m in sharded] == [m.relief_rmsd for m in got]


def _relief_object_gen(calls):
    gen = _object_gen([])
    gen._relieve, gen._score_placed = _stub_relief(calls), _stub_placed(calls)
    return gen


def test_object_path_mols_carry_the_relief_and_move_with_their_hydrogens():
    calls = []
    gen = _relief_object_gen(calls)
    kw = dict(reference_conformer=_ref(), n_samples=9, sample_seed=5, overlay=True, receptor=_pocket())
    plain = gen.generate_conformers(**kw)
    assert calls == [] and all("relief_rmsd" not in m.props for m in plain)
    got = gen.generate_conformers(relieve_clashes=True, **kw)
    assert calls == [("relieve", 7, 32), ("placed", 7)]                            # the live Mols whose pose succeeded
    assert [m.props["sample_id"] for m in got] == [m.props["sample_id"] for m in plain] == [0, 1, 3, 4, 5, 6, 7, 8]
    for a, b in zip(plain, got):
        sid = b.props["sample_id"]
        if sid == 6:                                                               # pose failed
            assert "relief_rmsd" not in b.props and "receptor_clashes_before" not in b.props
            continue
        assert b.props["receptor_clashes_before"] == min(sid, 4)
        if sid >= 5:                                                               # all five positions, the hydrogen too
            np.testing.assert_allclose(b.conf.pos, a.conf.pos + SHIFT.numpy(), atol=1e-12)
            assert b.props["relief_rmsd"] == 1.0 and b.props["overlay_tanimoto"] == pytest.approx(0.75)
        else:
            np.testing.assert_array_equal(b.conf.pos, a.conf.pos)
            assert b.props["relief_rmsd"] == 0.0 and b.props["overlay_tanimoto"] == a.props["overlay_tanimoto"]


def _relief_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    gen = _relief_object_gen(calls)
    mols = gen.generate_conformers_sharded(reference_conformer=_ref(), n_samples=9, sample_seed=5, overlay=True,
                                           receptor=_pocket(), relieve_clashes=True, gather="all")
    q.put((rank, [(m.props["sample_id"], m.props.get("relief_rmsd"), m.props.get("receptor_clashes_before"),
                   repr(m.conf.pos.tolist())) for m in mols], sum(c[1] for c in calls if c[0] == "relieve")))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_gather_all_returns_the_same_relieved_molecules_on_both_ranks_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_relief_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res[0][1] == res[1][1]
    assert [(s, r, c) for s, r, c, _ in res[0][1]] == [(0, 0.0, 0), (1, 0.0, 1), (3, 0.0, 3), (4, 0.0, 4), (5, 1.0, 4),
                                                      (6, None, None), (7, 1.0, 4), (8, 1.0, 4)]
    assert sum(r[2] for r in res) == 7 and all(r[2] > 0 for r in res)               # each rank relieved its own shard
