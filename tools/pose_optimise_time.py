#!/usr/bin/env python3
"""Cost of the pose optimisation (`optimise_pose`) on one MI355X.

  kernel:     one `mcg_receptor_optimise` launch (`interactions.optimise_typed`: the ligand already typed, the receptor
              prepared and uploaded outside the timed region) over 2 048 molecules of 27 atoms - the workload of
              tools/interaction_time.py: random walks placed at random inside a ball of synthetic receptor atoms of protein
              density - against receptors of 2 000, 20 000 and 100 000 atoms, `steps = 64`, with tile skipping on and off;
              timed with device events: `--warmup` untimed launches, then the median, min and max of `--runs` runs of
              `--passes` launches each;
  yardstick:  one `mcg_receptor_interactions` launch (`interactions.score_typed`) on the same inputs, times (the mean number
              of trials a molecule used + 1): what the walk's evaluations would cost as scoring launches.  A molecule of 27
              atoms leaves 37 of a workgroup's 64 atom slots idle in either kernel.
Nothing else should run on the GPU.  No threshold: a record.  Prints one JSON line."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from ml_conformer_generator_amd import interactions as IX  # noqa: E402
from fingerprint_time import event_times  # noqa: E402
from interaction_time import ball_receptor, walks  # noqa: E402
from shape_score_time import stat  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-samples", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n = args.n_samples, 27
    g = torch.Generator().manual_seed(7)
    z = torch.tensor([6, 6, 6, 7, 8])[torch.randint(0, 5, (B, n), generator=g)].to(dev)
    types = torch.randint(0, 8, (B, n), generator=g).to(dev, torch.uint8)
    radii = IX.interaction_radii(z)
    nn = torch.full((B,), n, dtype=torch.int32, device=dev)
    rot = torch.zeros(B, dtype=torch.int32, device=dev)
    timing = (dev, args.warmup, args.runs, args.passes)
    result = {"rows": B, "atoms": n, "steps": args.steps, "max_shift": IX.OPTIMISE_MAX_SHIFT, "kernel": {}}
    for R in (2000, 20000, 100000):
        rec, radius = ball_receptor(R, R)
        prepared = IX.prepare_receptor(rec)
        on_device = IX.PreparedReceptor(*(t.to(dev) for t in prepared))       # uploaded once, outside the timed region
        x = walks(B, n, max(radius - 6.0, 1.0), R + 1).to(dev)
        row = {"tiles": int(prepared.spheres.shape[0])}
        outs = {}
        for skip in (True, False):
            def launch():
                return IX.optimise_typed(on_device, x, nn, radii, types, args.steps, IX.OPTIMISE_MAX_SHIFT, skip, dev)
            outs[skip] = launch()
            row["skip_tiles" if skip else "every_tile"] = stat(event_times(launch, *timing))
        stats = outs[True]["stats"]
        row["identical"] = all(torch.equal(outs[True][k].view(torch.int32), outs[False][k].view(torch.int32)) for k in outs[True])
        trials = float(stats[:, 2].mean())
        row.update(mean_trials=round(trials, 2), mean_kept=round(float(stats[:, 3].mean()), 2),
                   mean_w_before=round(float(stats[:, 0].mean()), 3), mean_w_after=round(float(stats[:, 1].mean()), 3),
                   mean_rmsd=round(float(stats[:, 4].mean()), 3))
        for skip in (True, False):
            one = stat(event_times(lambda: IX.score_typed(on_device, x, nn, radii, types, rot, skip_tiles=skip, device=dev),
                                   *timing))
            key = "skip_tiles" if skip else "every_tile"
            row[f"score_launch_{key}"] = one
            row[f"yardstick_{key}_ms"] = round(one["median_ms"] * (trials + 1.0), 3)
        result["kernel"][f"R={R}"] = row
        print({R: row}, file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
