"""Shape-diverse selection, host side (no GPU): `select_diverse` against a brute-force restatement, refusals before any
device work on every generation entry and in `pairwise_shape_tanimoto`, the C entry's argument checks, selection through
a stub pair function on the proxy and the object path, and the same selection on both ranks of a world-size-2 gloo run."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ml_conformer_generator_amd.cheminformatics import (MAX_PAIR_BATCH, pairwise_shape_tanimoto, select_diverse,
                                                        select_scored)
from test_shape_overlay_host import (PosedMol, _free_port, _no_device, _ref, _shell_generator, _Stage, _stub_overlay,
                                     _stub_shard)


def _brute(scores, ids, pair, t, top_k, min_t):
    """The selection restated: filter, rank (NaN last, ties to the lower id), exclude against what is kept, cut."""
    cand = [i for i in range(len(scores)) if min_t is None or scores[i] >= min_t]
    order = sorted(cand, key=lambda i: (math.isnan(scores[i]), 0.0 if math.isnan(scores[i]) else -scores[i], ids[i]))
    kept = []
    for i in order:
        if t is None or not any(float(pair[i][j]) >= t for j in kept):   # a NaN entry compares False: excludes nothing
            kept.append(i)
    return kept if top_k is None else kept[:top_k]


def _case(seed, B):
    g = np.random.default_rng(seed)
    scores = g.choice([0.2, 0.35, 0.5, 0.5, 0.61, 0.8, float("nan")], size=B).tolist()     # ties and NaN scores
    ids = g.permutation(B * 3)[:B].tolist()
    p = g.choice([0.1, 0.3, 0.5, 0.7, 0.9, 1.0, float("nan")], size=(B, B)).astype(np.float32)
    p = np.triu(p, 1)
    p = p + p.T
    np.fill_diagonal(p, 1.0)
    return scores, ids, p


@pytest.mark.parametrize("seed", range(12))
def test_select_diverse_matches_the_restatement(seed):
    B = 5 + seed * 3
    scores, ids, p = _case(seed, B)
    for t in (None, 0.3, 0.5, 0.9, 1.0):
        for top_k in (None, 1, 3, B + 2):
            for min_t in (None, 0.0, 0.5, 0.8):
                want = _brute(scores, ids, p, t, top_k, min_t)
                assert select_diverse(scores, ids, p, t, top_k, min_t) == want, (t, top_k, min_t)
                assert select_diverse(scores, ids, torch.from_numpy(p), t, top_k, min_t) == want
                if t is None:
                    assert select_diverse(scores, ids, None, None, top_k, min_t) == select_scored(scores, ids, top_k,
                                                                                                  min_t)


def test_select_diverse_edge_cases():
    nan = float("nan")
    p = np.array([[1.0, 1.0, nan], [1.0, 1.0, 0.2], [nan, 0.2, 1.0]], dtype=np.float32)
    assert select_diverse([0.9, 0.8, 0.7], [0, 1, 2], p, 1.0) == [0, 2]            # >= 1 excludes an exact copy only
    assert select_diverse([0.9, 0.8, 0.7], [0, 1, 2], p, 0.1) == [0, 2]            # a NaN pair excludes nothing
    assert select_diverse([0.7, 0.8, 0.8], [0, 2, 1], p, 0.99) == [2, 1]           # tie to the lower id; 1 excludes 0
    assert select_diverse([nan, 0.8, 0.1], [0, 1, 2], p, None) == [1, 2, 0]        # a NaN score ranks last
    assert select_diverse([nan, 0.8, 0.1], [0, 1, 2], p, 0.99) == [1, 2]           # ... and 1 excludes it
    assert select_diverse([], [], np.zeros((0, 0)), 0.5) == []


# ----------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_diversity_refusals_happen_before_any_device_work(entry):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    gen._generate_shard = gen._score = gen._pose = _no_device
    gen._pair = _no_device
    call = getattr(gen, entry)
    ctx = torch.tensor([50.0, 100.0, 130.0])
    for kw in (dict(reference_conformer=_ref(), max_pairwise_tanimoto=0.5),               # not posed: no common frame
               dict(reference_conformer=_ref(), overlay=True, max_pairwise_tanimoto=True),
               dict(reference_conformer=_ref(), overlay=True, max_pairwise_tanimoto=float("nan")),
               dict(reference_conformer=_ref(), overlay=True, max_pairwise_tanimoto=0),
               dict(reference_conformer=_ref(), overlay=True, max_pairwise_tanimoto=0.0),
               dict(reference_conformer=_ref(), overlay=True, max_pairwise_tanimoto=1.0001),
               dict(reference_conformer=_ref(), overlay=True, max_pairwise_tanimoto=-0.5),
               dict(reference_conformer=_ref(), overlay=True, max_pairwise_tanimoto="0.5"),
               dict(reference_context=ctx, n_atoms=17, overlay=True, max_pairwise_tanimoto=0.5),
               dict(reference_conformer=_ref(65), overlay=True, max_pairwise_tanimoto=0.5),
               dict(reference_conformer=_ref(), overlay=True, max_pairwise_tanimoto=0.5, top_k=0)):
        with pytest.raises(ValueError):
            call(n_samples=4, **kw)
    gen.finisher = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                              "finish_tag_chunk")
    with pytest.raises(ValueError, match="custom finisher"):
        call(reference_conformer=_ref(), n_samples=4, overlay=True, max_pairwise_tanimoto=0.5)


def test_pairwise_refusals_happen_before_any_device_work():
    x = torch.zeros(3, 20, 3)
    n = torch.tensor([20, 5, 0], dtype=torch.int32)
    for ref, coords, nn in ((_ref(2), x, n), (_ref(65), x, n),                           # the reference checks
                            (_ref(), x, torch.tensor([21, 5, 0])), (_ref(), x, torch.tensor([4, 5])),   # check_n_nodes
                            (_ref(), torch.zeros(2, 65, 3), torch.tensor([3, 3])),        # padded width above 64
                            (_ref(), torch.zeros(MAX_PAIR_BATCH + 1, 1, 3),
                             torch.ones(MAX_PAIR_BATCH + 1, dtype=torch.int32))):         # above the batch cap
        with pytest.raises(ValueError):
            pairwise_shape_tanimoto(ref, coords, nn, device="cpu")
    out = pairwise_shape_tanimoto(_ref(), torch.zeros(0, 20, 3), torch.zeros(0, dtype=torch.int32), device="cpu")
    assert out.shape == (0, 0)


def test_pair_entry_refuses_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check
    ok = dict(coords=p, nn=p, B=3, N=27, xf=p, axes=p, n=40, f=p, g=p, t=p)

    def pair(**kw):
        a = dict(ok, **kw)
        return h.mcg_shape_pair_tanimoto(a["coords"], a["nn"], a["B"], a["N"], a["xf"], a["axes"], a["n"], 0.8, 2.7,
                                         a["f"], a["g"], a["t"], None)

    for bad in (dict(coords=None), dict(nn=None), dict(xf=None), dict(axes=None), dict(f=None), dict(g=None),
                dict(t=None), dict(B=0), dict(B=-1), dict(B=MAX_PAIR_BATCH + 1), dict(N=0), dict(N=65), dict(n=1),
                dict(n=257)):
        assert pair(**bad) == 1, bad
        assert b"mcg_shape_pair_tanimoto" in h.mcg_last_error(), bad
    assert "mcg_shape_pair_tanimoto" in _lib.SIGNATURES


# ----------------------------------------------------------------------------------------------- stub pair function
def _stub_pair(calls):
    """A device-free stand-in for `pairwise_shape_tanimoto`: T_ij = 1 - |k_i - k_j| with k = a row's coords[0, 1] (NaN
    rows give NaN), and a record of the batch sizes it was called with."""
    def run(ref, coords, n):
        calls.append(int(coords.shape[0]))
        k = coords[:, 0, 1].double()
        return (1.0 - (k.view(-1, 1) - k.view(1, -1)).abs()).float()
    return run


def test_proxy_path_selects_through_the_pair_function():
    gen = _shell_generator()
    gen._generate_shard = _stub_shard()
    gen._pose = _stub_overlay(lambda k: k + 1.0)        # (x, 0, 0) @ rot_z(90) -> (0, x, 0): coords[0, 1] = x
    gen._score = lambda ref, coords, n: coords[:, 1, 0].clone()
    calls = []
    gen._pair = _stub_pair(calls)
    base = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True, shape_scores=True)
    scores, ids = [m.shape_tanimoto for m in base], [m.sample_id for m in base]
    pair = _stub_pair([])(None, torch.stack([m.coords for m in base]), None)
    for t, top_k, min_t in ((0.75, None, None), (0.9, 3, None), (0.5, None, 0.0), (1.0, 2, None)):
        calls.clear()
        got = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True, max_pairwise_tanimoto=t,
                                      top_k=top_k, min_shape_tanimoto=min_t)
        assert calls == [len(base)]                              # one call over the kept (valid) records
        assert [m.sample_id for m in got] == [ids[i] for i in _brute(scores, ids, pair, t, top_k, min_t)]
    calls.clear()
    plain = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True, top_k=4)
    assert calls == [] and [m.sample_id for m in plain] == [ids[i] for i in select_scored(scores, ids, 4)]
    sharded = gen.generate_conformers_sharded(reference_conformer=_ref(), n_samples=8, overlay=True,
                                              max_pairwise_tanimoto=0.75)        # no process group: one rank
    assert [m.sample_id for m in sharded] == [ids[i] for i in _brute(scores, ids, pair, 0.75, None, None)]


class _StageGen:
    """`_generate_shard` for the object path: finished stand-in Mols with heavy atoms at (sid / 10, 0, 0); sample 2 is
    dropped by the finish."""
    def __init__(self, gen):
        self.gen = gen

    def __call__(self, ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
        self.gen._finish_stage = _Stage([None if i == 2 else PosedMol([[i / 10.0, 0, 0]] * 4 + [[0, 0, 1.0]],
                                                                      z=[6] * 4 + [1]) for i in ids])
        return dict(x=torch.zeros(n_samples, 5, 3))


def _object_gen(calls):
    gen = _shell_generator(finisher="rdkit")
    gen._generate_shard = _StageGen(gen)
    gen._pose = _stub_overlay(lambda k: k * 0 + 0.5)
    gen._score = lambda ref, coords, n: 1.0 - coords[:, 0, 1].clone()      # lower sample id: higher score
    gen._pair = _stub_pair(calls)
    return gen


def test_object_path_selects_through_the_pair_function():
    calls = []
    gen = _object_gen(calls)
    got = gen.generate_conformers(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True,
                                  max_pairwise_tanimoto=0.85)
    # ranking 0, 1, 3, 4, 5, 6 (2 was dropped); T = 1 - |sid_i - sid_j| / 10: a kept id excludes the ids within 1.5
    assert calls == [6] and [m.props["sample_id"] for m in got] == [0, 3, 5]
    calls.clear()
    got = gen.generate_conformers(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True, top_k=3)
    assert calls == [] and [m.props["sample_id"] for m in got] == [0, 1, 3]


def _diverse_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    gen = _object_gen(calls)
    mols = gen.generate_conformers_sharded(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True,
                                           max_pairwise_tanimoto=0.85, gather="all")
    q.put((rank, [m.props["sample_id"] for m in mols], calls))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_gather_all_selects_the_same_on_both_ranks_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_diverse_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    # every rank computes the pair matrix of the whole gathered batch (6 live Mols) and returns the same list
    assert res == [(0, [0, 3, 5], [6]), (1, [0, 3, 5], [6])]
