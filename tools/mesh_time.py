#!/usr/bin/env python3
"""Cost of the solid-reference kernels (`csrc/mcg_mesh.hip`) on one MI355X, on the demo pocket (2 488 triangles,
tests/golden/pocket_6q8k_mesh.npz):
  occupancy:      the `mcg_mesh_occupancy` launch a `reference_shape` call makes once - 40^3 = 64 000 grid points;
  atoms_outside:  one `mcg_mesh_atoms_outside` launch at 256 molecules x 39 atoms placed around the pocket.
Device events: `--warmup` untimed launches, then the median, min and max of `--runs` windows of `--passes` launches.  For
kernel times run it under `rocprofv3 --kernel-trace --stats` (a run of its own).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ml_conformer_generator_amd import cheminformatics as CH  # noqa: E402
from ml_conformer_generator_amd import mesh as M  # noqa: E402


def event_times(fn, dev, warmup, runs, passes):
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
        torch.cuda.synchronize(dev)
        out.append(start.elapsed_time(end) / passes)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--passes", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(REPO, "tests", "golden", "pocket_6q8k_mesh.npz"))
    solid = CH.solid_reference(M.load_mesh((z["v"], z["f"].astype(np.int64))))
    d = solid.on(dev)
    g = np.random.default_rng(0)
    v = solid.mesh.vertices
    x = torch.from_numpy((v[g.integers(0, len(v), (256, 39))] + g.normal(size=(256, 39, 3)) * 1.5).astype(np.float32)).to(dev)
    n = torch.full((256,), 39, dtype=torch.int32, device=dev)
    F = int(d["triangles"].shape[0])
    out = dict(triangles=F, grid_points=solid.n ** 3, atoms=256 * 39,
               occupancy=event_times(lambda: CH.mesh_occupancy(d["triangles"], d["axes"], dev), dev, args.warmup, args.runs,
                                     args.passes),
               atoms_outside=event_times(lambda: CH.mesh_atoms_outside(d["triangles_own"], x, n, dev), dev, args.warmup,
                                         args.runs, args.passes))
    out["inside_points"] = int(d["f"].sum())
    out["outside_counts_mean"] = float(CH.mesh_atoms_outside(d["triangles_own"], x, n, dev).float().mean())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
