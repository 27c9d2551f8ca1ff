#!/usr/bin/env python3
"""Cost of the pocket kernel (`csrc/mcg_pocket.hip`, entry `mcg_pocket_masks`) on one MI355X, in two cases:
  block:      21^3 grid points (radius 10 A, spacing 1 A) against the 2 152-atom carved block of tests/pocket_cases.py;
  synthetic:  41^3 grid points (radius 20 A, spacing 1 A) against a 100 000-atom synthetic receptor at a protein's density.
Per case: the launch alone on device-resident inputs (device events: `--warmup` untimed launches, then the median, min and
max of `--runs` single launches), at the default split count and at one split, how many receptor tiles the skip keeps per
workgroup, and the wall time of `find_pocket` end to end (host sort, copy, launch, host pipeline).  For kernel times run it
under `rocprofv3 --kernel-trace --stats` (a run of its own).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pocket_cases as PC  # noqa: E402
from ml_conformer_generator_amd import _lib  # noqa: E402
from ml_conformer_generator_amd import pocket as PK  # noqa: E402
from ml_conformer_generator_amd import receptor as RC  # noqa: E402


def event_times(fn, dev, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(runs):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize(dev)
        out.append(start.elapsed_time(end))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def case(xyz, z, radius, dev, warmup, runs, find=True):
    probe, reach, spacing = PK.DEFAULT_PROBE, PK.DEFAULT_REACH, PK.DEFAULT_SPACING
    n = PK.grid_size(radius, spacing)
    r = RC.vdw_radii(torch.from_numpy(z))
    xyzr = RC.sort_receptor(torch.from_numpy(xyz).to(torch.float32), r)
    spheres = RC.tile_spheres(xyzr)
    R = int(xyzr.shape[0])
    rec, sph = xyzr.to(dev), spheres.to(dev)
    out = torch.zeros(n ** 3, dtype=torch.int32, device=dev)
    S = PK.default_splits(n, R)

    def launch(splits, tiles=sph):
        _lib.check(_lib.lib().mcg_pocket_masks(_lib.dptr(rec), R, _lib.dptr(tiles), n, spacing, probe, reach, splits,
                                               _lib.dptr(out), _lib.current_stream_ptr(dev)), "mcg_pocket_masks")

    kept = PK.kept_tiles(spheres, n, spacing, probe, reach)
    res = dict(atoms=R, grid_points=n ** 3, workgroups=int(kept.size), tiles=-(-R // 256), default_splits=S,
               tiles_kept=dict(min=int(kept.min()), mean=float(kept.mean()), max=int(kept.max())),
               default=event_times(lambda: launch(S), dev, warmup, runs),
               one_split=event_times(lambda: launch(1), dev, warmup, runs),
               no_skip=event_times(lambda: launch(S, None), dev, warmup, runs))
    launch(S)
    masks = out.cpu().numpy().view(np.uint32)
    res["occupied_points"] = int((masks >> 31).sum())
    res["mean_buriedness_free"] = float(PK.buriedness(masks[(masks >> 31) == 0]).mean()) if (masks >> 31 == 0).any() else None
    if find:
        t0 = time.perf_counter()
        try:
            p = PK.find_pocket((xyz, z), (0.0, 0.0, 0.0), radius=radius, device=dev)
            res["pocket"] = dict(cells=p.cells, n_centres=p.n_centres, cells_filled=p.cells_filled, faces=int(len(p.faces)))
        except ValueError as e:                   # "no pocket at the centre": the masks were still computed and read
            res["pocket"] = str(e)
        res["find_pocket_wall_ms"] = (time.perf_counter() - t0) * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = dict(block=case(*PC.block(), 10.0, dev, args.warmup, args.runs),
               synthetic=case(*PC.synthetic_receptor(), 20.0, dev, args.warmup, args.runs))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
