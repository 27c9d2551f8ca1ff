#!/usr/bin/env python3
"""Cost of the pairwise shape Tanimoto (shape-diverse selection) on one MI355X.

  batches:    `cheminformatics.pairwise_shape_tanimoto` at 64, 256 and 2 048 molecules of the configs[1] (27 atoms) and
              configs[2] (27 +- 12 atoms, ragged) shapes, posed onto the reference by `shape_overlay` (a seeded generation
              of 256 molecules, repeated row by row to reach 2 048), for every Gram tile size (MCG_SHAPE_PAIR_TILE = 1,
              2, 4: the same bits whichever runs) and the one the library picks;
  generation: a full `generate_conformers` call (64 molecules, 27 atoms, 100 steps) with `overlay=True` alone and with
              `max_pairwise_tanimoto` as well, the two interleaved run by run.
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
from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto, shape_overlay  # noqa: E402
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
    for name, variance in (("configs[1]", 0), ("configs[2]", 12)):
        gen.generate_conformers(n_samples=256, variance=variance, **kw)
        lb = gen.last_batch
        x0, n0 = lb["x_ordered"].contiguous(), lb["n_nodes"].to(torch.int32)
        x0 = shape_overlay(ref, x0, n0, dev)["coords"].contiguous()
        for B in (64, 256, 2048):
            rows = torch.arange(B, device=dev) % x0.shape[0]
            x, n = x0[rows].contiguous(), n0.to(dev)[rows].contiguous()
            row = {}
            for tile in ("1", "2", "4", None):
                if tile is None:
                    os.environ.pop("MCG_SHAPE_PAIR_TILE", None)
                else:
                    os.environ["MCG_SHAPE_PAIR_TILE"] = tile
                if args.quick and tile is not None:
                    continue
                row["auto" if tile is None else f"tile{16 * int(tile)}"] = stat(
                    timed(lambda: pairwise_shape_tanimoto(ref, x, n, dev), dev, runs, passes))
            result["batches"][f"{name} B={B}"] = row
            print(name, B, row, file=sys.stderr, flush=True)
    os.environ.pop("MCG_SHAPE_PAIR_TILE", None)
    posed, diverse = [], []
    for _ in range(runs):
        posed += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, overlay=True, **kw), dev, 1, passes)
        diverse += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, overlay=True,
                                                         max_pairwise_tanimoto=0.9, **kw), dev, 1, passes)
    result["generation"] = {"workload": "generate_conformers n_samples=64, 27 atoms, diffusion_steps=100, fp32",
                            "overlay": stat(posed), "overlay+max_pairwise_tanimoto": stat(diverse),
                            "overhead_pct": round(100.0 * (statistics.median(diverse) / statistics.median(posed) - 1.0), 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
