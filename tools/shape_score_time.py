#!/usr/bin/env python3
"""Cost of shape scoring on one MI355X.

  frames:     principal shape frames of a batch by the HIP kernels (`cheminformatics.shape_frames_hip`) against the tensor
              path (`shape_quadrupole_batch`) on the device, at 64 and 256 molecules of the configs[1] (27 atoms) and
              configs[2] (27 +- 12 atoms, ragged) shapes from a seeded generation, and of compact synthetic 39-atom clouds
              (every pair within the neighbour threshold: the worst case of the clique enumeration);
  generation: a full `generate_conformers` call (64 molecules, 27 atoms, 100 steps) with and without `shape_scores=True`,
              the two interleaved run by run.
Every figure is the median of `--runs` runs (each the mean of `--passes` host-synchronised passes) with its min and max.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (`--quick`).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ml_conformer_generator_amd import MLConformerGenerator, weights as W  # noqa: E402
from ml_conformer_generator_amd.cheminformatics import shape_frames_hip, shape_quadrupole_batch  # noqa: E402

SEED = 20261015


def timed(fn, dev, runs, passes):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(passes):
            fn()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) * 1e3 / passes)
    return out


def stat(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="one pass of everything (for the rocprofv3 kernel trace)")
    args = ap.parse_args()
    runs, passes = (1, 1) if args.quick else (args.runs, args.passes)
    dev = torch.device("cuda:0")
    ref = torch.as_tensor(np.load(os.path.join(REPO, "tests", "golden", "shape_quadrupole.npz"))["xyz_walk27"])
    gen = MLConformerGenerator(diffusion_steps=100, device=dev, edm_weights=W.synth_edm_state_dict(1234, recipe="v2d"),
                               adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321), atom_order_provider=None)
    kw = dict(reference_conformer=ref, optimise_geometry=False, sample_seed=SEED)
    result = {"frames": {}, "generation": {}}

    batches = {}
    for B in (64, 256):
        for name, variance in (("configs[1]", 0), ("configs[2]", 12)):
            gen.generate_conformers(n_samples=B, variance=variance, **kw)
            lb = gen.last_batch
            batches[f"{name} B={B}"] = (lb["x_ordered"].contiguous(), lb["n_nodes"].to(torch.int32))
        g = torch.Generator().manual_seed(B)
        batches[f"compact39 B={B}"] = ((torch.rand(B, 39, 3, generator=g) * 3.0).to(dev),
                                       torch.full((B,), 39, dtype=torch.int32, device=dev))
    for key, (x, n) in batches.items():
        _, _, counts = shape_frames_hip(x, n, dev, with_counts=True)
        hip = timed(lambda: shape_frames_hip(x, n, dev), dev, runs, passes)
        row = {"hip": stat(hip), "cliques_per_molecule_max": int(counts.sum(1).max()),
               "cliques_total": int(counts.sum())}
        compact = key.startswith("compact39")
        if not (compact and (args.quick or x.shape[0] > 64)):      # 256 x 3.3 M index rows do not fit the tensor path
            try:
                ten = timed(lambda: shape_quadrupole_batch(x, n, dev), dev, 1 if compact else runs,
                            1 if compact else passes)
                row["tensor"] = stat(ten)
                row["speedup"] = round(statistics.median(ten) / statistics.median(hip), 2)
            except torch.cuda.OutOfMemoryError:
                row["tensor"] = "out of device memory"
                torch.cuda.empty_cache()
        result["frames"][key] = row
        print(key, row, file=sys.stderr, flush=True)

    plain, scored = [], []
    for _ in range(runs):
        plain += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, **kw), dev, 1, passes)
        scored += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, shape_scores=True, **kw), dev, 1, passes)
    result["generation"] = {"workload": "generate_conformers n_samples=64, 27 atoms, diffusion_steps=100, fp32",
                            "plain": stat(plain), "shape_scores": stat(scored),
                            "overhead_pct": round(100.0 * (statistics.median(scored) / statistics.median(plain) - 1.0), 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
