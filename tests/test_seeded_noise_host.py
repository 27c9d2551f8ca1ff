"""Keyed per-molecule randomness (`sample_seed`), the parts that need no GPU: the host Philox and the keyed sizes against
an independent restatement of Philox4x32-10, the sharded plumbing at gloo world size 2, and the C entry's argument
checks.  The restatement here is also what tests/test_seeded_generation.py checks the device noise against."""
import ctypes
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from ml_conformer_generator_amd import _lib, seeding
from ml_conformer_generator_amd.distributed import assign_shards, keyed_global_sizes
from ml_conformer_generator_amd.mol_utils import prepare_edm_input
from test_distributed_gloo import _free_port, _shell_generator

# ------------------------------------------------------------------------------------------------------------------
# Independent restatement of Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; Random123's philox4x32_R(10)):
# the 32x32 -> 64 multiply is split into 16-bit halves so that nothing of the product's own arithmetic is shared.
# ------------------------------------------------------------------------------------------------------------------
_M = (0xD2511F53, 0xCD9E8D57)
_W = (0x9E3779B9, 0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)


def _mul_hi_lo(a: int, b):
    """(hi, lo) 32-bit halves of a * b for a python constant a and a uint64 array b < 2^32, by 16-bit limbs."""
    b = b.astype(np.uint64)
    a_lo, a_hi = np.uint64(a & 0xFFFF), np.uint64(a >> 16)
    b_lo, b_hi = b & np.uint64(0xFFFF), b >> np.uint64(16)
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> np.uint64(16)) + (lh & np.uint64(0xFFFF)) + (hl & np.uint64(0xFFFF))
    lo = (ll & np.uint64(0xFFFF)) | ((mid & np.uint64(0xFFFF)) << np.uint64(16))
    hi = hh + (lh >> np.uint64(16)) + (hl >> np.uint64(16)) + (mid >> np.uint64(16))
    return hi & _MASK, lo & _MASK


def philox_ref(c0, c1, c2, c3, k0: int, k1: int) -> np.ndarray:
    """Words [..., 4] (uint64 holding 32-bit values) of Philox4x32-10 at counters (c0..c3) (arrays, broadcast)."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k = [np.uint64(k0), np.uint64(k1)]
    for r in range(10):
        hi0, lo0 = _mul_hi_lo(_M[0], c[0])
        hi1, lo1 = _mul_hi_lo(_M[1], c[2])
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(_W[0])) & _MASK, (k[1] + np.uint64(_W[1])) & _MASK]
    return np.stack(c, axis=-1)


def keyed_normals_ref(seed: int, sample_id: int, run: int, draw: int, n_atoms: int) -> np.ndarray:
    """[n_atoms, 11] float64: channel q of atom i = normal q of the stream (0..2 x, 3..10 h), restated from the spec."""
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    i = np.arange(n_atoms, dtype=np.uint64)[:, None]
    blk = np.arange(3, dtype=np.uint64)[None, :]
    w = philox_ref(np.uint64(sample_id), np.uint64(draw), i, (np.uint64(run) << np.uint64(8)) | blk, k0, k1)  # [n,3,4]
    w = w.astype(np.float64)
    z = np.empty(w.shape, dtype=np.float64)
    for e, o in ((0, 1), (2, 3)):
        u1 = (np.floor(w[..., e] / 256.0) + 1.0) * 2.0 ** -24
        u2 = np.floor(w[..., o] / 256.0) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[..., e], z[..., o] = r * np.cos(2.0 * math.pi * u2), r * np.sin(2.0 * math.pi * u2)
    return z.reshape(n_atoms, 12)[:, :11]


def keyed_sizes_ref(seed: int, ids, lo: int, hi: int) -> np.ndarray:
    ids = np.asarray(ids, dtype=np.uint64)
    w0 = philox_ref(ids, 0, 0, 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)[..., 0]
    return np.array([lo + ((int(w) * (hi - lo + 1)) >> 32) for w in w0.tolist()], dtype=np.int64)


KAT = [  # Random123 known-answer vectors of philox4x32_R(10): counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_restatement_reproduces_random123_vectors(ctr, key, out):
    assert tuple(int(v) for v in philox_ref(*ctr, *key)) == out


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_product_host_philox_reproduces_random123_vectors(ctr, key, out):
    assert tuple(int(v) for v in seeding.philox4x32_10(ctr, key)) == out


def test_product_philox_agrees_with_restatement_on_random_counters():
    rng = np.random.default_rng(3)
    ctr = rng.integers(0, 2 ** 32, size=(4096, 4), dtype=np.uint64)
    key = (int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)))
    got = seeding.philox4x32_10(ctr, key).astype(np.uint64)
    assert np.array_equal(got, philox_ref(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key))


def test_seed_key_split_and_refusals():
    assert seeding.philox_key(0x0123456789ABCDEF) == (0x89ABCDEF, 0x01234567)
    assert seeding.philox_key(2 ** 64 - 1) == (0xFFFFFFFF, 0xFFFFFFFF)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            seeding.check_seed(bad)
    for bad in (1.5, "7", True):
        with pytest.raises(TypeError):
            seeding.check_seed(bad)
    with pytest.raises(ValueError):
        seeding.check_sample_ids([0, 2 ** 32])
    with pytest.raises(ValueError):
        seeding.check_sample_ids([-1])
    with pytest.raises(ValueError):
        seeding.check_sample_ids([0, 1, 2], n_samples=2)


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 64 - 1, 0xDEADBEEF00C0FFEE])
def test_keyed_sizes_match_restatement_range_and_prefix(seed):
    ids = [0, 1, 2, 3, 7, 1_000_000, 2 ** 32 - 1]
    got = seeding.keyed_sizes(seed, ids, 15, 39)
    assert got.dtype == torch.int64
    assert got.tolist() == keyed_sizes_ref(seed, ids, 15, 39).tolist()
    big = seeding.keyed_sizes(seed, torch.arange(64), 15, 39)
    assert int(big.min()) >= 15 and int(big.max()) <= 39
    assert torch.equal(seeding.keyed_sizes(seed, torch.arange(4), 15, 39), big[:4])       # prefix-invariant
    assert torch.equal(seeding.keyed_sizes(seed, [9, 2], 27, 27), torch.tensor([27, 27]))  # a one-value range
    assert torch.equal(keyed_global_sizes(64, 15, 39, seed), big)


def test_keyed_sizes_are_uniform():
    lo, hi, n = 15, 39, 100_000
    sizes = seeding.keyed_sizes(77, torch.arange(n), lo, hi)
    counts = np.bincount(sizes.numpy() - lo, minlength=hi - lo + 1)
    assert counts.size == hi - lo + 1
    expect = n / (hi - lo + 1)
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    # 24 degrees of freedom: P(chi2 > 51.2) = 1e-3
    assert chi2 < 51.2, chi2


def test_prepare_edm_input_keyed_sizes_leave_the_global_rng_alone():
    state = torch.get_rng_state()
    norms = {"mean": torch.zeros(3), "mad": torch.ones(3)}
    node_mask, _, _ = prepare_edm_input(5, torch.tensor([1.0, 2.0, 3.0]), norms, 15, 39, "cpu", sample_seed=11,
                                        sample_ids=torch.tensor([4, 0, 9, 9, 2]))
    assert torch.equal(torch.get_rng_state(), state)
    assert node_mask.sum(1).reshape(-1).long().tolist() == keyed_sizes_ref(11, [4, 0, 9, 9, 2], 15, 39).tolist()


def test_edm_tensors_refuses_ids_without_a_seed_and_a_tape_with_one():
    gen = _shell_generator()
    gen.generative_model = types.SimpleNamespace(noise_fn=None)
    with pytest.raises(ValueError, match="sample_ids needs a sample_seed"):
        gen.edm_tensors(torch.tensor([1.0, 2.0, 3.0]), n_samples=2, sample_ids=torch.tensor([0, 1]))
    gen.generative_model.noise_fn = lambda shape: torch.zeros(shape)
    with pytest.raises(ValueError, match="noise_fn"):
        gen.edm_tensors(torch.tensor([1.0, 2.0, 3.0]), n_samples=2, sample_seed=3)


# ------------------------------------------------------------------------------------------------------------------
# Sharded plumbing: `generate_conformers_sharded(sample_seed=...)` at world size 2 with only `_generate_shard` stubbed
# ------------------------------------------------------------------------------------------------------------------
def _keyed_stub(calls):
    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        seed, ids = rest[-2], rest[-1]
        calls.append((sizes.clone(), n_samples, seed, ids.clone()))
        N, D = min(ref_n_atoms + variance, 39), 42
        el = torch.zeros(n_samples, D, dtype=torch.int8)
        for b in range(n_samples):
            el[b, : int(sizes[b])] = 6
        x = ids.float().view(-1, 1, 1).repeat(1, N, 3)        # x encodes the sample id the shard was asked for
        return dict(x=x, elements=el, bond=torch.zeros(n_samples, D, D, dtype=torch.int8),
                    n_nodes=sizes.to(torch.int32), valid=(sizes % 2 == 0).to(torch.uint8))
    return run


def _keyed_shard_worker(rank, world, port, n_samples, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(1000 + 17 * rank)            # ranks disagree on purpose: nothing may depend on their RNGs
    seeded = []
    torch.cuda.manual_seed = seeded.append         # the default path seeds the device generator through this
    seed = 0xC0FFEE12345
    expect = torch.from_numpy(keyed_sizes_ref(seed, range(n_samples), 15, 39))
    results = []
    for balance in ("cost", "count", "cost"):
        gen = _shell_generator()
        calls = []
        gen._generate_shard = _keyed_stub(calls)
        state = torch.get_rng_state()
        gather = "rank0" if len(results) == 2 else "all"
        mols = gen.generate_conformers_sharded(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=27,
                                               variance=12, n_samples=n_samples, balance=balance, sample_seed=seed,
                                               gather=gather)
        mine = assign_shards(expect, world, balance)[rank]
        ok = len(calls) == 1 and torch.equal(calls[0][0], expect[mine]) and calls[0][1] == mine.numel()
        ok = ok and calls[0][2] == seed and torch.equal(calls[0][3], mine)       # the shard's GLOBAL ids
        ok = ok and torch.equal(torch.get_rng_state(), state) and gen.last_noise_seed is None and not seeded
        rows = list(range(n_samples)) if (gather == "all" or rank == 0) else mine.tolist()
        kept = [i for i in rows if int(expect[i]) % 2 == 0]
        ok = ok and [m.sample_id for m in mols] == kept
        ok = ok and all(float(m.coords[0, 0]) == m.sample_id and m.GetNumAtoms() == int(expect[m.sample_id]) for m in mols)
        results.append(bool(ok))
    gen = _shell_generator()
    try:
        gen.generate_conformers_sharded(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=27, n_samples=4,
                                        seed=3, sample_seed=seed)
        results.append(False)
    except ValueError:
        results.append(True)
    seen = [None] * world
    dist.all_gather_object(seen, keyed_global_sizes(n_samples, 15, 39, seed).tolist())
    results.append(seen[0] == seen[1] == expect.tolist())
    q.put((rank, results))
    dist.barrier()
    dist.destroy_process_group()


def test_keyed_sharded_plumbing_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_keyed_shard_worker, args=(r, 2, port, 13, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, [True] * 5), (1, [True] * 5)]


def test_keyed_sharded_call_without_a_process_group_uses_ids_0_to_n():
    gen = _shell_generator()
    calls = []
    gen._generate_shard = _keyed_stub(calls)
    state = torch.get_rng_state()
    mols = gen.generate_conformers_sharded(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=27, variance=2,
                                           n_samples=6, sample_seed=5)
    expect = torch.from_numpy(keyed_sizes_ref(5, range(6), 25, 29))
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(calls[0][0], expect) and torch.equal(calls[0][3], torch.arange(6))
    assert [m.sample_id for m in mols] == [i for i in range(6) if int(expect[i]) % 2 == 0]


# ------------------------------------------------------------------------------------------------------------------
# C entry: argument errors without a GPU, header as C99
# ------------------------------------------------------------------------------------------------------------------
def test_keyed_noise_entry_refuses_bad_arguments_without_a_gpu():
    h = _lib.lib()
    fake_plan = ctypes.create_string_buffer(4096)        # never dereferenced: the checks come first
    ids = (ctypes.c_int64 * 4)()
    bx, bh = (ctypes.c_float * 12)(), (ctypes.c_float * 32)()
    f = h.mcg_sampler_noise_keyed
    assert f(None, 1, ids, 0, 0, bx, bh, None) == 1
    assert b"mcg_sampler_noise_keyed" in h.mcg_last_error()
    assert f(fake_plan, 1, None, 0, 0, bx, bh, None) == 1
    assert f(fake_plan, 1, ids, 0, 0, None, bh, None) == 1
    assert f(fake_plan, 1, ids, 0, 0, bx, None, None) == 1
    assert f(fake_plan, 1, ids, 1 << 24, 0, bx, bh, None) == 1
    assert b"24 bits" in h.mcg_last_error()
    assert h.mcg_abi_version() == 4


def test_header_declares_the_keyed_entry_as_plain_c(tmp_path):
    src = tmp_path / "k.c"
    src.write_text('#include "mlconfgen_hip.h"\n'
                   "int main(void) {\n"
                   "    int64_t ids[1] = {0}; float x[3], h[8];\n"
                   "    return mcg_sampler_noise_keyed((const mcg_plan*)0, (uint64_t)1 << 40, ids, 1u, 2u, x, h, (void*)0);\n"
                   "}\n")
    inc = os.path.join(REPO, "include")
    compilers = [c for c in ("gcc", "cc", "clang", "/opt/rocm/lib/llvm/bin/clang") if shutil.which(c)]
    if not compilers:
        pytest.skip("no C compiler")
    r = subprocess.run([compilers[0], "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "mcg_sampler_noise_keyed" in _lib.SIGNATURES
