"""Shape scoring of generated molecules, host side (no GPU): selection, refusals before any device work, the C entries'
argument checks, score attachment on the proxy and the object (finished-Mol) paths, and coordinate extraction."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd.cheminformatics import mol_heavy_coords, padded_coords, select_scored
from ml_conformer_generator_amd.handoff import GeneratedMolecule, molecules_from_tensors


# ----------------------------------------------------------------------------------------------- selection
def test_selection_threshold_k_order_and_ties():
    scores = [0.5, 0.9, 0.7, 0.9, 0.2, 0.7]
    ids = [10, 11, 12, 3, 14, 5]
    assert select_scored(scores, ids) == [3, 1, 5, 2, 0, 4]             # descending, ties to the lower sample id
    assert select_scored(scores, ids, top_k=3) == [3, 1, 5]
    assert select_scored(scores, ids, min_shape_tanimoto=0.7) == [3, 1, 5, 2]     # >= threshold
    assert select_scored(scores, ids, top_k=1, min_shape_tanimoto=0.6) == [3]
    assert select_scored(scores, ids, top_k=100) == [3, 1, 5, 2, 0, 4]
    assert select_scored(scores, ids, min_shape_tanimoto=0.95) == []
    assert select_scored([], [], top_k=2) == []
    assert select_scored([float("nan"), 0.1, 0.3], [0, 1, 2]) == [2, 1, 0]      # NaN ranks last
    assert select_scored([float("nan"), 0.1], [0, 1], min_shape_tanimoto=0.0) == [1]


# ----------------------------------------------------------------------------------------------- stub generator
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


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_refusals_happen_before_any_device_work(entry):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    gen._generate_shard = gen._score = _no_device
    call = getattr(gen, entry)
    ctx = torch.tensor([50.0, 100.0, 130.0])
    cases = [
        dict(reference_context=ctx, n_atoms=17, shape_scores=True),                # nothing to score against
        dict(reference_context=ctx, n_atoms=17, top_k=3),
        dict(reference_context=ctx, n_atoms=17, min_shape_tanimoto=0.5),
        dict(reference_conformer=_ref(65), shape_scores=True),                      # > 64 heavy atoms
        dict(reference_conformer=_ref(2), shape_scores=True),                       # < 3 heavy atoms
        dict(reference_conformer=_ref(), top_k=0),
        dict(reference_conformer=_ref(), top_k=-2),
        dict(reference_conformer=_ref(), top_k=2.5),
        dict(reference_conformer=_ref(), top_k=True),
        dict(reference_conformer=_ref(), top_k=np.int64(0)),
        dict(reference_conformer=_ref(), min_shape_tanimoto=1.5),
        dict(reference_conformer=_ref(), min_shape_tanimoto=-0.1),
        dict(reference_conformer=_ref(), min_shape_tanimoto=float("nan")),
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            call(n_samples=4, **kw)
    gen.finisher = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                              "finish_tag_chunk")
    with pytest.raises(ValueError, match="custom finisher"):
        call(reference_conformer=_ref(), n_samples=4, shape_scores=True)


# ----------------------------------------------------------------------------------------------- C entries
def test_frame_entries_refuse_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check
    ok = dict(coords=p, n=p, B=2, N=27, alpha=0.8, amp=2.7, thr=5.4, terms=6)

    def moments(**kw):
        a = dict(ok, **kw)
        return h.mcg_shape_moments(a["coords"], a["n"], a["B"], a["N"], a["alpha"], a["amp"], a["thr"], a["terms"], 0,
                                   a.get("out", p), p, p, None, None)

    def frames(**kw):
        a = dict(ok, **kw)
        return h.mcg_shape_frames(a["coords"], a["n"], a["B"], a["N"], p, p, p, a["alpha"], a["amp"], a["thr"], a["terms"],
                                  0, a.get("out", p), p, None)

    for f, name in ((moments, b"mcg_shape_moments"), (frames, b"mcg_shape_frames")):
        for bad in (dict(N=65), dict(N=0), dict(B=0), dict(terms=1), dict(terms=9), dict(coords=None), dict(n=None),
                    dict(out=None), dict(alpha=0.0), dict(amp=-1.0), dict(thr=0.0)):
            assert f(**bad) == 1, bad
            assert name in h.mcg_last_error(), bad
    assert "mcg_shape_moments" in _lib.SIGNATURES and "mcg_shape_frames" in _lib.SIGNATURES


def test_atom_counts_outside_the_padded_width_are_refused():
    from ml_conformer_generator_amd.cheminformatics import check_n_nodes
    check_n_nodes(torch.tensor([0, 5, 27]), 3, 27)
    for n, B, N in (([28], 1, 27), ([-1, 3], 2, 27), ([3, 3], 3, 27)):
        with pytest.raises(ValueError):
            check_n_nodes(torch.tensor(n), B, N)


# ----------------------------------------------------------------------------------------------- records, extraction
def test_records_carry_scores_only_when_given():
    x = torch.randn(3, 5, 3)
    el = torch.full((3, 42), 6, dtype=torch.int8)
    bond = torch.zeros(3, 42, 42, dtype=torch.int8)
    n = torch.tensor([5, 4, 3], dtype=torch.int32)
    valid = torch.ones(3, dtype=torch.uint8)
    plain = molecules_from_tensors(x, el, bond, n, valid)
    assert [m.shape_tanimoto for m in plain] == [None, None, None]
    scored = molecules_from_tensors(x, el, bond, n, valid, shape_tanimoto=torch.tensor([0.25, 0.5, 0.75]))
    assert [m.shape_tanimoto for m in scored] == [0.25, 0.5, 0.75] and [m.sample_id for m in scored] == [0, 1, 2]
    assert scored == plain                                             # value equality ignores the score
    assert GeneratedMolecule([6, 6], torch.zeros(2, 3), torch.zeros(2, 2, dtype=torch.int8)).shape_tanimoto is None


class _Atom:
    def __init__(self, z):
        self.z = z

    def GetAtomicNum(self):
        return self.z


class _Conf:
    def __init__(self, pos):
        self.pos = pos

    def GetPositions(self):
        return self.pos


class FakeMol:
    """A picklable Mol-like stand-in: conformer positions, atoms, double / int properties."""

    def __init__(self, pos, z=None):
        self.pos = np.asarray(pos, dtype=np.float64)
        self.z = [6] * len(self.pos) if z is None else list(z)
        self.props = {}

    def GetConformer(self):
        return _Conf(self.pos)

    def GetAtoms(self):
        return [_Atom(z) for z in self.z]

    def SetDoubleProp(self, k, v):
        self.props[k] = v

    def SetIntProp(self, k, v):
        self.props[k] = v


def test_coordinates_come_from_the_conformer_heavy_atoms_only():
    pos = [[0.0, 1.0, 2.0], [0.5, 0.5, 0.5], [3.0, 4.0, 5.0]]
    m = FakeMol(pos, z=[6, 1, 8])
    c = mol_heavy_coords(m)
    assert c.dtype == torch.float32 and c.tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]
    coords, n = padded_coords([c, torch.ones(4, 3)])
    assert coords.shape == (2, 4, 3) and n.tolist() == [2, 4] and float(coords[0, 2:].abs().sum()) == 0.0
    # the generator scores every live Mol in ONE batched call and leaves dropped ones unscored
    gen = _shell_generator()
    seen = []

    def score(ref, coords, n):
        seen.append((coords.clone(), n.clone()))
        return coords[:, 0, 0] / 10.0
    gen._score = score
    out = postprocess.score_mols(gen, _ref(), [m, None, FakeMol([[7.0, 0, 0]] * 3)])
    assert out == [0.0, None, pytest.approx(0.7)] and len(seen) == 1 and seen[0][1].tolist() == [2, 3]


# ----------------------------------------------------------------------------------------------- proxy path (stub shard)
def _stub_shard(n_atoms=20):
    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        N = 22
        el = torch.full((n_samples, 42), 6, dtype=torch.int8)
        ids = torch.arange(n_samples) if len(rest) < 8 or rest[7] is None else torch.as_tensor(rest[7])
        # x[:, 0, 0] encodes the "score" of the sample (stubbed scorer below); sample 3 is invalid
        x = torch.zeros(n_samples, N, 3)
        x[:, 0, 0] = torch.tensor([(7 * int(i)) % 10 / 10.0 for i in range(n_samples)])
        n = torch.full((n_samples,), n_atoms, dtype=torch.int32)
        valid = torch.tensor([0 if i == 3 else 1 for i in range(n_samples)], dtype=torch.uint8)
        return dict(x=x, elements=el, bond=torch.zeros(n_samples, 42, 42, dtype=torch.int8), n_nodes=n, valid=valid)
    return run


def test_proxy_path_scores_and_selects_on_the_returned_rows():
    gen = _shell_generator()
    gen._generate_shard = _stub_shard()
    gen._score = lambda ref, coords, n: coords[:, 0, 0].clone()
    plain = gen.generate_conformers(reference_conformer=_ref(), n_samples=8)
    assert [m.shape_tanimoto for m in plain] == [None] * 7
    scored = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, shape_scores=True)
    expect = [(7 * i) % 10 / 10.0 for i in range(8)]
    assert [m.sample_id for m in scored] == [0, 1, 2, 4, 5, 6, 7]                    # sample order, invalid one dropped
    assert [m.shape_tanimoto for m in scored] == [pytest.approx(expect[i]) for i in (0, 1, 2, 4, 5, 6, 7)]
    top = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, top_k=np.int64(3))    # any integer type
    assert [m.sample_id for m in top] == [7, 4, 1]                                     # 0.9, 0.8, 0.7 (0.1 x 7 % 10)
    assert gen.last_valid_fraction == pytest.approx(7 / 8)                             # before the selection
    thr = gen.forward(reference_conformer=_ref(), n_samples=8, min_shape_tanimoto=0.5)
    assert [m.sample_id for m in thr] == [7, 4, 1, 5]
    none = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, min_shape_tanimoto=1.0)
    assert none == [] and gen.last_valid_fraction == pytest.approx(7 / 8)


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
    scored_on = []

    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist()
        # the finished "Mols": x[0, 0] = the sample id / 10; sample 2 was dropped by the finish
        gen._finish_stage = _Stage([None if i == 2 else FakeMol([[i / 10.0, 0, 0]] * 5) for i in ids])
        return dict(x=torch.zeros(n_samples, 5, 3))

    def score(ref, coords, n):
        scored_on.append(int(coords.shape[0]))
        return coords[:, 0, 0].clone() + 0.01 * rank        # a rank-specific offset: shows WHERE each score was made
    gen._generate_shard = run
    gen._score = score
    mols = gen.generate_conformers_sharded(reference_conformer=_ref(), n_samples=7, sample_seed=5, shape_scores=True)
    from ml_conformer_generator_amd.distributed import assign_shards, keyed_global_sizes
    shards = assign_shards(keyed_global_sizes(7, 15, 19, 5), world)
    owner = {i: r for r, ix in enumerate(shards) for i in ix.tolist()}
    ok = len(scored_on) == 1 and scored_on[0] == len([i for i in shards[rank].tolist() if i != 2])
    ok = ok and [m.props["sample_id"] for m in mols] == [0, 1, 3, 4, 5, 6]
    ok = ok and all(abs(m.props["shape_tanimoto"] - (m.props["sample_id"] / 10.0 + 0.01 * owner[m.props["sample_id"]]))
                    < 1e-6 for m in mols)
    top = gen.generate_conformers_sharded(reference_conformer=_ref(), n_samples=7, sample_seed=5, top_k=2)
    ok = ok and [m.props["sample_id"] for m in top] == [6, 5]
    mine = gen.generate_conformers_sharded(reference_conformer=_ref(), n_samples=7, sample_seed=5, top_k=2, gather="rank0")
    own = sorted((i for i in (range(7) if rank == 0 else shards[rank].tolist()) if i != 2), reverse=True)[:2]
    ok = ok and [m.props["sample_id"] for m in mine] == own
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def test_object_path_scores_travel_next_to_the_mols_world2_gloo():
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
