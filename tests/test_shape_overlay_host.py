"""Posing generated molecules onto the reference, host side (no GPU): refusals before any device work, the C entries'
argument checks, the Mol-posing helper on a stand-in Mol, pose attachment on the proxy path, and the poses travelling next
to the Mols through a world-size-2 gloo gather."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ml_conformer_generator_amd.cheminformatics import pose_mols
from ml_conformer_generator_amd.handoff import molecules_from_tensors


def _shell_generator(finisher=None):
    from ml_conformer_generator_amd.conformer_generator import MLConformerGenerator
    gen = MLConformerGenerator.__new__(MLConformerGenerator)
    torch.nn.Module.__init__(gen)
    gen.device = torch.device("cpu")
    gen.dimension = 42
    gen.min_n_nodes, gen.max_n_nodes = 15, 39
    gen.last_batch = gen.last_valid_fraction = gen._timing = gen.last_noise_seed = gen.last_host_assembly_ms = None
    gen.atom_order_provider = None
    gen.finisher = finisher
    gen.n_host_workers = 0
    return gen


def _ref(n=17):
    return torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) * 0.37


def _no_device(*args, **kwargs):
    raise AssertionError("device work started before the arguments were checked")


def _rot_z(deg):
    a = np.deg2rad(deg)
    return torch.tensor([[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)


def _stub_overlay(shift_of):
    """A device-free stand-in for `shape_overlay`: rotation = 90 degrees about z, translation = (shift_of(x00), 0, 0) and
    tanimoto = shift_of(x00) per row, where x00 = the row's first coordinate; rows whose x00 is NaN fail."""
    def run(ref, coords, n, refine_steps=0):
        B = coords.shape[0]
        key = coords[:, 0, 0]
        R = _rot_z(90.0).expand(B, 3, 3).clone()
        t = torch.zeros(B, 3)
        t[:, 0] = shift_of(key)
        failed = torch.isnan(key)
        R[failed], t[failed] = float("nan"), float("nan")
        real = (torch.arange(coords.shape[1]).view(1, -1) < torch.as_tensor(n).view(B, 1)).unsqueeze(2)
        posed = torch.where(failed.view(B, 1, 1), coords, (coords @ R + t.unsqueeze(1)) * real)
        return dict(coords=posed, rotation=R, translation=t, tanimoto=shift_of(key),
                    orientation=torch.where(failed, -1, 0), flipped=torch.zeros(B, dtype=torch.bool))
    return run


# ----------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_overlay_refusals_happen_before_any_device_work(entry):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    gen._generate_shard = gen._score = gen._pose = _no_device
    call = getattr(gen, entry)
    ctx = torch.tensor([50.0, 100.0, 130.0])
    for kw in (dict(reference_context=ctx, n_atoms=17, overlay=True),            # nothing to pose onto
               dict(reference_conformer=_ref(65), overlay=True),                 # > 64 heavy atoms
               dict(reference_conformer=_ref(2), overlay=True),                  # < 3 heavy atoms
               dict(reference_conformer=_ref(), overlay=True, top_k=0)):
        with pytest.raises(ValueError):
            call(n_samples=4, **kw)
    gen.finisher = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                              "finish_tag_chunk")
    with pytest.raises(ValueError, match="custom finisher"):
        call(reference_conformer=_ref(), n_samples=4, overlay=True)


# ----------------------------------------------------------------------------------------------- C entries
def test_overlay_entries_refuse_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check

    def frames_tf(B=2, N=27, xform=p, terms=6):
        return h.mcg_shape_frames_tf(p, p, B, N, p, p, p, 0.8, 2.7, 5.4, terms, 1, p, p, xform, None)

    for bad in (dict(xform=None), dict(N=65), dict(N=0), dict(B=0), dict(terms=9)):
        assert frames_tf(**bad) == 1, bad
        assert b"mcg_shape_frames_tf" in h.mcg_last_error(), bad

    ok = dict(ref=p, n_ref=17, ref_xf=p, frames=p, xf=p, nn=p, B=3, N=27, rot=p, axes=p, n=40, f=p, score=None, best=p,
              which=p, flipped=p, pose=p, posed=p)

    def overlay(**kw):
        a = dict(ok, **kw)
        return h.mcg_shape_overlay(a["ref"], a["n_ref"], a["ref_xf"], a["frames"], a["xf"], a["nn"], a["B"], a["N"],
                                   a["rot"], a["axes"], a["n"], 0.8, 2.7, a["f"], a["score"], a["best"], a["which"],
                                   a["flipped"], a["pose"], a["posed"], None)

    for bad in (dict(ref=None), dict(ref_xf=None), dict(frames=None), dict(xf=None), dict(nn=None), dict(rot=None),
                dict(axes=None), dict(f=None), dict(best=None), dict(which=None), dict(flipped=None), dict(pose=None),
                dict(posed=None), dict(B=0), dict(N=0), dict(N=65), dict(n_ref=2), dict(n_ref=65), dict(n=1)):
        assert overlay(**bad) == 1, bad
        assert b"mcg_shape_overlay" in h.mcg_last_error(), bad
    assert "mcg_shape_frames_tf" in _lib.SIGNATURES and "mcg_shape_overlay" in _lib.SIGNATURES


# ----------------------------------------------------------------------------------------------- Mol posing helper
class _Atom:
    def __init__(self, z):
        self.z = z

    def GetAtomicNum(self):
        return self.z


class _Conf:
    def __init__(self, pos):
        self.pos = pos

    def GetPositions(self):
        return self.pos.copy()

    def SetAtomPosition(self, i, p):
        self.pos[i] = [float(p[0]), float(p[1]), float(p[2])]


class PosedMol:
    """A picklable Mol-like stand-in: ONE conformer that can be moved, atoms, double / int properties."""

    def __init__(self, pos, z=None):
        self.conf = _Conf(np.array(pos, dtype=np.float64))
        self.z = [6] * len(self.conf.pos) if z is None else list(z)
        self.props = {}

    def GetConformer(self):
        return self.conf

    def GetAtoms(self):
        return [_Atom(z) for z in self.z]

    def SetDoubleProp(self, k, v):
        self.props[k] = v

    def SetIntProp(self, k, v):
        self.props[k] = v


def test_pose_mols_moves_every_atom_by_one_rigid_transform():
    pos = np.array([[0.5, 1.0, 2.0], [1.1, 0.2, -0.3], [3.0, 4.0, 5.0], [-1.0, 0.5, 0.25]])
    m = PosedMol(pos, z=[6, 1, 8, 1])                       # two hydrogens
    failing = PosedMol([[float("nan"), 0, 0]] * 3)
    seen = []

    def overlay_fn(ref, coords, n):
        seen.append((coords.clone(), n.clone()))
        return _stub_overlay(lambda k: k * 2.0)(ref, coords, n)
    out = pose_mols(_ref(), [m, None, failing], overlay_fn=overlay_fn)
    assert len(seen) == 1 and seen[0][1].tolist() == [2, 3]                  # heavy atoms only, one batched call
    assert seen[0][0][0, :2].tolist() == [[0.5, 1.0, 2.0], [3.0, 4.0, 5.0]]
    R, t = _rot_z(90.0).double().numpy(), np.array([1.0, 0.0, 0.0])
    np.testing.assert_allclose(m.conf.pos, pos @ R + t, atol=1e-6)          # hydrogens moved with the heavy atoms
    assert m.props["overlay_tanimoto"] == pytest.approx(1.0)
    assert out[1] is None
    score, rot, trans = out[0]
    assert score == pytest.approx(1.0) and torch.allclose(rot, _rot_z(90.0)) and trans.tolist() == [1.0, 0.0, 0.0]
    assert out[2][1] is None and out[2][0] != out[2][0]                      # failed: NaN score, no pose, not moved
    assert np.isnan(failing.conf.pos[:, 0]).all() and not failing.conf.pos[:, 1:].any()


# ----------------------------------------------------------------------------------------------- proxy path (stub shard)
def _stub_shard(n_atoms=20):
    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        N = 22
        el = torch.full((n_samples, 42), 6, dtype=torch.int8)
        x = torch.zeros(n_samples, N, 3)
        x[:, :n_atoms] = torch.randn(n_atoms, 3, generator=torch.Generator().manual_seed(3))
        x[:, 0, 0] = torch.tensor([(7 * int(i)) % 10 / 10.0 for i in range(n_samples)])
        x[5, 0, 0] = float("nan")                      # a row whose pose fails
        n = torch.full((n_samples,), n_atoms, dtype=torch.int32)
        valid = torch.tensor([0 if i == 3 else 1 for i in range(n_samples)], dtype=torch.uint8)
        return dict(x=x, elements=el, bond=torch.zeros(n_samples, 42, 42, dtype=torch.int8), n_nodes=n, valid=valid)
    return run


def test_proxy_path_returns_posed_coordinates_with_their_pose():
    gen = _shell_generator()
    gen._generate_shard = _stub_shard()
    gen._pose = _stub_overlay(lambda k: k + 1.0)
    gen._score = lambda ref, coords, n: coords[:, 1, 0].clone()
    plain = gen.generate_conformers(reference_conformer=_ref(), n_samples=8)
    assert all(m.pose is None and m.overlay_tanimoto is None for m in plain)
    posed = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True)
    assert [m.sample_id for m in posed] == [m.sample_id for m in plain] == [0, 1, 2, 4, 5, 6, 7]
    for a, b in zip(plain, posed):
        if b.sample_id == 5:                          # failed: generated coordinates, no pose, NaN score
            assert b.pose is None and b.overlay_tanimoto != b.overlay_tanimoto
            assert torch.equal(b.coords[1:], a.coords[1:])
            continue
        R, t = b.pose
        assert torch.allclose(b.coords, a.coords @ R + t, atol=1e-6)
        assert b.overlay_tanimoto == pytest.approx(float(a.coords[0, 0]) + 1.0)
        assert b.shape_tanimoto is None
    # scored: the score of the RETURNED (posed) coordinates
    scored = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True, shape_scores=True)
    for a, b in zip(posed, scored):
        torch.testing.assert_close(a.coords, b.coords, rtol=0, atol=0, equal_nan=True)
        assert b.shape_tanimoto == pytest.approx(float(b.coords[1, 0]))


# ----------------------------------------------------------------------------------------------- object path, gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Stage:
    def __init__(self, mols):
        self.mols = mols

    def results(self):
        return list(self.mols)


def _object_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    gen = _shell_generator(finisher="rdkit")
    posed_on = []

    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist()
        # the finished "Mols": x[0, 0] = the sample id / 10, an H atom last; sample 2 was dropped by the finish
        gen._finish_stage = _Stage([None if i == 2 else PosedMol([[i / 10.0, 0, 0]] * 4 + [[0, 0, 1.0]], z=[6] * 4 + [1])
                                    for i in ids])
        return dict(x=torch.zeros(n_samples, 5, 3))

    stub = _stub_overlay(lambda k: k + 0.01 * rank)     # a rank-specific offset: shows WHERE each pose was made

    def pose(ref, coords, n, refine_steps=0):
        posed_on.append(int(coords.shape[0]))
        return stub(ref, coords, n)
    gen._generate_shard = run
    gen._pose = pose
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    from ml_conformer_generator_amd.distributed import assign_shards, keyed_global_sizes
    shards = assign_shards(keyed_global_sizes(7, 15, 19, 5), world)
    owner = {i: r for r, ix in enumerate(shards) for i in ix.tolist()}
    ok = True
    for gather in ("all", "rank0"):
        posed_on.clear()
        mols = gen.generate_conformers_sharded(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True,
                                               shape_scores=True, gather=gather)
        mine = [i for i in (range(7) if (gather == "all" or rank == 0) else shards[rank].tolist()) if i != 2]
        ok = ok and len(posed_on) == 1 and posed_on[0] == len([i for i in shards[rank].tolist() if i != 2])
        ok = ok and [m.props["sample_id"] for m in mols] == mine
        for m in mols:
            sid = m.props["sample_id"]
            shift = sid / 10.0 + 0.01 * owner[sid]
            ok = ok and abs(m.props["overlay_tanimoto"] - shift) < 1e-6
            # (x, 0, 0) @ rot_z(90) = (0, x, 0), then + (shift, 0, 0); the H atom (0, 0, 1) -> (shift, 0, 1)
            want = np.array([[shift, sid / 10.0, 0.0]] * 4 + [[shift, 0.0, 1.0]])
            ok = ok and np.allclose(m.conf.pos, want, atol=1e-5)
            ok = ok and abs(m.props["shape_tanimoto"] - sid / 10.0) < 1e-5      # scored after posing
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def test_object_path_poses_travel_next_to_the_mols_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_object_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True)]


def test_a_finished_sample_pickles_to_the_same_size_whatever_its_shard():
    """What crosses the object gather per sample owns its 12 pose values: its pickle does not carry the shard's other poses."""
    import pickle
    from ml_conformer_generator_amd import postprocess
    gen = _shell_generator(finisher="rdkit")
    gen._reference_coord = lambda r: torch.as_tensor(r, dtype=torch.float32)
    gen._pose = _stub_overlay(lambda k: k + 1.0)
    req = postprocess.parse_request(gen, _ref(), overlay=True)
    sizes = {}
    for B in (2, 64, 1000):
        samples = postprocess.measure_finished(gen, req, [PosedMol([[0.5, 0, 0]] * 4) for _ in range(B)])
        assert all(s.measured.pose is not None and s.measured.pose.shape == (12,) for s in samples)
        sizes[B] = len(pickle.dumps(postprocess.Finished(None, samples[B - 1].measured)))
        back = pickle.loads(pickle.dumps(samples[0]))
        assert torch.equal(back.measured.pose, samples[0].measured.pose) and back.mol.props == samples[0].mol.props
    assert sizes[2] == sizes[64] == sizes[1000] < 2048, sizes


def test_records_carry_a_pose_only_when_given():
    x = torch.randn(2, 4, 3)
    el = torch.full((2, 42), 6, dtype=torch.int8)
    bond = torch.zeros(2, 42, 42, dtype=torch.int8)
    n = torch.tensor([4, 3], dtype=torch.int32)
    valid = torch.ones(2, dtype=torch.uint8)
    plain = molecules_from_tensors(x, el, bond, n, valid)
    assert [(m.pose, m.overlay_tanimoto) for m in plain] == [(None, None), (None, None)]
    pose = torch.arange(24, dtype=torch.float32).reshape(2, 12)
    pose[1, 4] = float("nan")
    posed = molecules_from_tensors(x, el, bond, n, valid, overlay_tanimoto=torch.tensor([0.5, float("nan")]), pose=pose)
    R, t = posed[0].pose
    assert R.tolist() == pose[0, :9].reshape(3, 3).tolist() and t.tolist() == [9.0, 10.0, 11.0]
    assert posed[0].overlay_tanimoto == 0.5 and posed[1].pose is None and posed[1].overlay_tanimoto != 0.5
    assert [m.shape_tanimoto for m in posed] == [None, None]
