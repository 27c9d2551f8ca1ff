#!/usr/bin/env python3
"""Cost of posing generated molecules onto the reference on one MI355X.

  batches:    `cheminformatics.shape_overlay` against `cheminformatics.shape_scores` (the scoring pass it is compared with)
              at 64 and 256 molecules of the configs[1] (27 atoms) and configs[2] (27 +- 12 atoms, ragged) shapes from a
              seeded generation;
  generation: a full `generate_conformers` call (64 molecules, 27 atoms, 100 steps) with and without `overlay=True`, the
              two interleaved run by run.
Every figure is the median of `--runs` runs (each the mean of `--passes` host-synchronised passes) with its min and max.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (`--quick`).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ml_conformer_generator_amd import MLConformerGenerator, weights as W  # noqa: E402
from ml_conformer_generator_amd.cheminformatics import shape_overlay, shape_scores  # noqa: E402
from shape_score_time import SEED, stat, timed  # noqa: E402


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
    result = {"batches": {}, "generation": {}}
    for B in (64, 256):
        for name, variance in (("configs[1]", 0), ("configs[2]", 12)):
            gen.generate_conformers(n_samples=B, variance=variance, **kw)
            lb = gen.last_batch
            x, n = lb["x_ordered"].contiguous(), lb["n_nodes"].to(torch.int32)
            pose = timed(lambda: shape_overlay(ref, x, n, dev), dev, runs, passes)
            score = timed(lambda: shape_scores(ref, x, n, dev), dev, runs, passes)
            row = {"overlay": stat(pose), "shape_scores": stat(score)}
            result["batches"][f"{name} B={B}"] = row
            print(name, B, row, file=sys.stderr, flush=True)
    plain, posed = [], []
    for _ in range(runs):
        plain += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, **kw), dev, 1, passes)
        posed += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, overlay=True, **kw), dev, 1, passes)
    result["generation"] = {"workload": "generate_conformers n_samples=64, 27 atoms, diffusion_steps=100, fp32",
                            "plain": stat(plain), "overlay": stat(posed),
                            "overhead_pct": round(100.0 * (statistics.median(posed) / statistics.median(plain) - 1.0), 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
