#!/usr/bin/env python3
"""Cost of the refined pose (`shape_overlay(refine_steps=64)`) on one MI355X.

  batches:    `cheminformatics.shape_overlay` with refine_steps=64 against the unrefined call, at 64 and 256 molecules of the
              configs[1] (27 atoms) and configs[2] (27 +- 12 atoms, ragged) shapes from a seeded generation, and the
              number of rows the refinement replaced with the mean gain in overlay Tanimoto;
  generation: a full `generate_conformers` call (64 molecules, 27 atoms, 100 steps) with `overlay=True` and with
              `overlay=True, refine_overlay=True`, the two interleaved run by run.
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
from ml_conformer_generator_amd.cheminformatics import shape_overlay  # noqa: E402
from shape_score_time import SEED, stat, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--quick", action="store_true", help="one pass of everything (for the rocprofv3 kernel trace)")
    args = ap.parse_args()
    runs, passes = (1, 1) if args.quick else (args.runs, args.passes)
    dev = torch.device("cuda:0")
    ref = torch.as_tensor(np.load(os.path.join(REPO, "tests", "golden", "shape_quadrupole.npz"))["xyz_walk27"])
    gen = MLConformerGenerator(diffusion_steps=100, device=dev, edm_weights=W.synth_edm_state_dict(1234, recipe="v2d"),
                               adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321), atom_order_provider=None)
    kw = dict(reference_conformer=ref, optimise_geometry=False, sample_seed=SEED)
    result = {"steps": args.steps, "batches": {}, "generation": {}}
    for B in (64, 256):
        for name, variance in (("configs[1]", 0), ("configs[2]", 12)):
            gen.generate_conformers(n_samples=B, variance=variance, **kw)
            lb = gen.last_batch
            x, n = lb["x_ordered"].contiguous(), lb["n_nodes"].to(torch.int32)
            plain = timed(lambda: shape_overlay(ref, x, n, dev), dev, runs, passes)
            refined = timed(lambda: shape_overlay(ref, x, n, dev, refine_steps=args.steps), dev, runs, passes)
            res = shape_overlay(ref, x, n, dev, refine_steps=args.steps)
            gain = (res["tanimoto"] - res["start_tanimoto"]).double()
            row = {"overlay": stat(plain), "overlay_refined": stat(refined),
                   "added_ms": round(statistics.median(refined) - statistics.median(plain), 3),
                   "rows_refined": int(res["refined"].sum()), "mean_gain": round(float(gain.nanmean()), 4)}
            result["batches"][f"{name} B={B}"] = row
            print(name, B, row, file=sys.stderr, flush=True)
    posed, refined = [], []
    for _ in range(runs):
        posed += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, overlay=True, **kw), dev, 1, passes)
        refined += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, overlay=True,
                                                         refine_overlay=args.steps, **kw), dev, 1, passes)
    result["generation"] = {"workload": "generate_conformers n_samples=64, 27 atoms, diffusion_steps=100, fp32",
                            "overlay": stat(posed), "overlay_refined": stat(refined),
                            "overhead_pct": round(100.0 * (statistics.median(refined) / statistics.median(posed) - 1.0), 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
