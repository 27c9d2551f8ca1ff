#!/usr/bin/env python3
"""Cost of the receptor interaction score (`interaction_scores`, `max_interaction_score`) on one MI355X.

  kernel:     one `mcg_receptor_interactions` launch (`interactions.score_typed`: the ligand already typed, the receptor
              prepared and uploaded outside the timed region) over 2 048 molecules of 27 atoms - random walks placed at
              random inside a ball of synthetic receptor atoms of protein density - against receptors of 2 000, 20 000
              and 100 000 atoms, with tile skipping on and off; timed with device events: `--warmup` untimed launches,
              then the median, min and max of `--runs` runs of `--passes` launches each;
  yardstick:  `receptor.receptor_overlap` (`k_receptor_overlap`) over the same molecules and receptors;
  prepare:    host time of `interactions.prepare_receptor` (typing, sorting, tile spheres) per receptor, once;
  generation: a full `generate_conformers` call (64 molecules, 27 atoms, 100 steps, `overlay=True`, a 5 000-atom receptor
              as a (coords, atomic numbers) pair) with and without `interaction_scores=True`, the two interleaved run by
              run, host-synchronised.
Nothing else should run on the GPU.  No threshold: a record.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ml_conformer_generator_amd import interactions as IX  # noqa: E402
from ml_conformer_generator_amd import receptor as RC  # noqa: E402
from fingerprint_time import event_times  # noqa: E402
from shape_score_time import SEED, stat, timed  # noqa: E402

DENSITY = 0.05                                    # heavy atoms per cubic angstrom: roughly a protein's


def ball_receptor(R: int, seed: int):
    """R atoms (C, N, O, S) uniform in a ball of protein density round the origin, with random types."""
    g = np.random.default_rng(seed)
    radius = (3.0 * R / (4.0 * np.pi * DENSITY)) ** (1.0 / 3.0)
    v = g.normal(size=(R, 3))
    v *= (radius * g.random((R, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    return (torch.tensor(v, dtype=torch.float32), torch.tensor(g.choice([6, 6, 6, 7, 8, 16], R)),
            torch.tensor(g.integers(0, 8, R), dtype=torch.uint8)), float(radius)


def walks(B: int, n: int, reach: float, seed: int) -> torch.Tensor:
    """B random walks of n steps of 1.5 A, each started at a random point within `reach` of the origin."""
    g = np.random.default_rng(seed)
    step = g.normal(size=(B, n, 3))
    step *= 1.5 / np.linalg.norm(step, axis=2, keepdims=True)
    start = g.normal(size=(B, 1, 3))
    start *= (reach * g.random((B, 1, 1)) ** (1.0 / 3.0)) / np.linalg.norm(start, axis=2, keepdims=True)
    return torch.tensor(start + np.cumsum(step, axis=1), dtype=torch.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-samples", type=int, default=2048)
    ap.add_argument("--no-generation", action="store_true", help="the kernel figures only")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n = args.n_samples, 27
    g = torch.Generator().manual_seed(7)
    z = torch.tensor([6, 6, 6, 7, 8])[torch.randint(0, 5, (B, n), generator=g)].to(dev)
    types = torch.randint(0, 8, (B, n), generator=g).to(dev, torch.uint8)
    radii = IX.interaction_radii(z)
    nn = torch.full((B,), n, dtype=torch.int32, device=dev)
    rot = torch.randint(0, 9, (B,), generator=g).to(dev, torch.int32)
    timing = (dev, args.warmup, args.runs, args.passes)
    result = {"rows": B, "atoms": n, "kernel": {}}
    for R in (2000, 20000, 100000):
        rec, radius = ball_receptor(R, R)
        t0 = time.perf_counter()
        prepared = IX.prepare_receptor(rec)
        prepare_ms = (time.perf_counter() - t0) * 1e3
        on_device = IX.PreparedReceptor(*(t.to(dev) for t in prepared))       # uploaded once, outside the timed region
        x = walks(B, n, max(radius - 6.0, 1.0), R + 1).to(dev)
        row = {"prepare_host_ms": round(prepare_ms, 1), "tiles": int(prepared.spheres.shape[0])}
        outs = {}
        for skip in (True, False):
            def launch():
                return IX.score_typed(on_device, x, nn, radii, types, rot, skip_tiles=skip, device=dev)
            outs[skip] = launch()
            row["skip_tiles" if skip else "every_tile"] = stat(event_times(launch, *timing))
        row["identical"] = all(torch.equal(outs[True][k].view(torch.int32), outs[False][k].view(torch.int32)) for k in outs[True])
        row["mean_score_before_division"] = round(float(outs[True]["mol_terms"][:, 5].mean()), 3)
        row["receptor_overlap"] = stat(event_times(lambda: RC.receptor_overlap(rec[:2], x, nn, z, dev), *timing))
        result["kernel"][f"R={R}"] = row
        print({R: row}, file=sys.stderr, flush=True)
    if not args.no_generation:
        from ml_conformer_generator_amd import MLConformerGenerator, weights as W
        from receptor_overlap_time import synthetic_receptor
        ref = torch.as_tensor(np.load(os.path.join(REPO, "tests", "golden", "shape_quadrupole.npz"))["xyz_walk27"])
        gen = MLConformerGenerator(diffusion_steps=100, device=dev, edm_weights=W.synth_edm_state_dict(1234, recipe="v2d"),
                                   adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321), atom_order_provider=None)
        kw = dict(reference_conformer=ref, optimise_geometry=False, sample_seed=SEED, n_samples=64, variance=0, overlay=True,
                  receptor=synthetic_receptor(ref, 5000, 5))
        plain, scored = [], []
        for _ in range(args.runs):
            plain += timed(lambda: gen.generate_conformers(**kw), dev, 1, 3)
            scored += timed(lambda: gen.generate_conformers(interaction_scores=True, **kw), dev, 1, 3)
        result["generation"] = {"workload": "generate_conformers n_samples=64, 27 atoms, diffusion_steps=100, fp32, overlay, "
                                            "5000-atom receptor", "receptor": stat(plain),
                                "receptor+interaction_scores": stat(scored),
                                "overhead_pct": round(100.0 * (statistics.median(scored) / statistics.median(plain) - 1.0), 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
