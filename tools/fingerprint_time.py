#!/usr/bin/env python3
"""Cost of the chemical fingerprints (`chemical_scores`, `unique`, `max_pairwise_chemical_tanimoto`) on one MI355X.

  kernels:    at B = 2 048 and 16 384 molecule-like graphs of 42 atoms (random trees of degree <= 3 with 0-3 ring
              closures) the fingerprint launch (`mcg_graph_fingerprint`), the pair launch (`mcg_fingerprint_pair_tanimoto`)
              and, beside it, the same matrix from a torch formulation on the same GPU: the bits unpacked to a [B, 2048]
              bf16 0/1 matrix (unpacking not timed), F @ F.T with fp32 accumulation (exact: counts <= 2 048), then the
              elementwise division.  Timed with device events: `--warmup` untimed launches, then the median, min and max
              of `--runs` runs of `--passes` launches each.  The two matrices must agree bit for bit.
  generation: one `generate_conformers` call at the benchmark's headline configuration (bench.py configs[1]: 64
              molecules, 27 atoms, 100 steps, fp32) with and without `chemical_scores=True, unique=True`, the two
              interleaved run by run (host clock around a synchronised call).
Nothing else should run on the GPU.  Prints one JSON line."""
import argparse
import json
import os
import random
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ml_conformer_generator_amd import MLConformerGenerator, weights as W  # noqa: E402
from ml_conformer_generator_amd import fingerprint as FP  # noqa: E402
from shape_score_time import SEED, stat, timed  # noqa: E402


def molecule_like_batch(B: int, n: int, seed: int):
    """(z [B,n] int32, bonds [B,n,n] int8, n_nodes [B]) of B random molecule-like graphs of n atoms."""
    rng = random.Random(seed)
    z = np.zeros((B, n), np.int32)
    bonds = np.zeros((B, n, n), np.int8)
    for b in range(B):
        z[b] = rng.choices([6, 6, 6, 7, 8, 9, 16], k=n)
        deg = [0] * n
        for a in range(1, n):
            j = rng.choice([k for k in range(a) if deg[k] < 3])
            bonds[b, a, j] = bonds[b, j, a] = rng.choice([1, 1, 2, 4])
            deg[a] += 1
            deg[j] += 1
        for _ in range(rng.randint(0, 3)):
            a, j = rng.sample(range(n), 2)
            if bonds[b, a, j] == 0:
                bonds[b, a, j] = bonds[b, j, a] = 1
    return torch.from_numpy(z), torch.from_numpy(bonds), torch.full((B,), n, dtype=torch.int32)


def event_times(fn, dev, warmup: int, runs: int, passes: int):
    """ms per launch: `runs` device-event windows of `passes` launches each, after `warmup` untimed launches."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(runs):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(passes):
            fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end) / passes)
    return out


def unpack_bits(fp: torch.Tensor, dtype) -> torch.Tensor:
    shifts = torch.arange(32, device=fp.device, dtype=torch.int32)
    return ((fp.unsqueeze(2) >> shifts) & 1).reshape(fp.shape[0], -1).to(dtype)


def bf16_mm_to_fp32() -> bool:
    """Whether this torch multiplies bf16 matrices into an fp32 result (`out_dtype`); else the 0/1 matrix is fp32."""
    a = torch.ones(16, 16, dtype=torch.bfloat16, device="cuda:0")
    try:
        return torch.mm(a, a.t(), out_dtype=torch.float32).dtype == torch.float32
    except (TypeError, RuntimeError, NotImplementedError):
        return False


def torch_pair(bits: torch.Tensor) -> torch.Tensor:
    """T = c / (p_i + p_j - c), [B,B] fp32, from the 0/1 matrix `bits` [B, 2048] (bf16 or fp32); the counts are exact."""
    c = torch.mm(bits, bits.t(), out_dtype=torch.float32) if bits.dtype == torch.bfloat16 else torch.mm(bits, bits.t())
    p = c.diagonal()
    union = p.view(-1, 1) + p.view(1, -1)
    union -= c
    return c.div_(union)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="one pass of everything (for the rocprofv3 kernel trace)")
    ap.add_argument("--no-generation", action="store_true")
    args = ap.parse_args()
    runs, passes, warmup = (1, 1, 1) if args.quick else (args.runs, args.passes, args.warmup)
    dev = torch.device("cuda:0")
    result = {"kernels": {}, "generation": {}}
    bf16 = bf16_mm_to_fp32()
    for B in (2048, 16384):
        z, bonds, n = (t.to(dev) for t in molecule_like_batch(B, 42, B))
        fp, key, _ = FP.graph_fingerprints(z, bonds, n, dev)
        row = {"fingerprint": stat(event_times(lambda: FP.graph_fingerprints(z, bonds, n, dev, check=False), dev, warmup,
                                               runs, passes)),
               "distinct_keys": int(torch.unique(key).numel())}
        pair = FP.pairwise_fingerprint_tanimoto(fp)
        row["pair_hip"] = stat(event_times(lambda: FP.pairwise_fingerprint_tanimoto(fp), dev, warmup, runs, passes))
        bits = unpack_bits(fp, torch.bfloat16 if bf16 else torch.float32)
        row["pair_torch"] = dict(stat(event_times(lambda: torch_pair(bits), dev, warmup, runs, passes)),
                                 formulation=("bf16" if bf16 else "fp32") + " 0/1 matrix, F @ F.T into fp32, division")
        row["pair_matrices_bit_equal"] = bool(torch.equal(torch_pair(bits).view(torch.int32), pair.view(torch.int32)))
        row["pair_word_operations"] = B * B * 64
        row["pair_output_bytes"] = B * B * 4
        del pair, bits
        result["kernels"][f"B={B}"] = row
        print(B, row, file=sys.stderr, flush=True)
    if not args.no_generation:
        ref = torch.as_tensor(np.load(os.path.join(REPO, "tests", "golden", "shape_quadrupole.npz"))["xyz_walk27"])
        gen = MLConformerGenerator(diffusion_steps=100, device=dev, edm_weights=W.synth_edm_state_dict(1234, recipe="v2d"),
                                   adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321), atom_order_provider=None)
        kw = dict(reference_conformer=ref, n_samples=64, variance=0, optimise_geometry=False, sample_seed=SEED)
        graph = ([6] * 6, [[4 if abs(i - j) in (1, 5) else 0 for j in range(6)] for i in range(6)])      # benzene
        chem_kw = dict(kw, chemical_scores=True, unique=True, reference_graph=graph)
        for _ in range(max(1, warmup - 1)):
            gen.generate_conformers(**kw)
            gen.generate_conformers(**chem_kw)
        plain, chem = [], []
        for _ in range(runs):
            plain += timed(lambda: gen.generate_conformers(**kw), dev, 1, passes)
            chem += timed(lambda: gen.generate_conformers(**chem_kw), dev, 1, passes)
        result["generation"] = {"workload": "generate_conformers n_samples=64, 27 atoms, diffusion_steps=100, fp32",
                                "plain": stat(plain), "chemical_scores+unique": stat(chem),
                                "added_ms": round(statistics.median(chem) - statistics.median(plain), 3),
                                "overhead_pct": round(100.0 * (statistics.median(chem) / statistics.median(plain) - 1.0), 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
