#!/usr/bin/env python3
"""Cost of the receptor contacts (`receptor=`, `max_receptor_clashes`) on one MI355X.

  batches:    `receptor.receptor_overlap` at 64 and 256 molecules of the configs[1] (27 atoms) and configs[2]
              (27 +- 12 atoms, ragged) shapes, posed onto the reference by `shape_overlay` (a seeded generation of 256
              molecules), against synthetic receptors of 2 000, 20 000 and 100 000 heavy atoms (brute force: the cost
              depends on the counts only);
  generation: a full `generate_conformers` call (64 molecules, 27 atoms, 100 steps) with `overlay=True` alone and with a
              5 000-atom receptor given as a PDB string (parsed on every call) as well, the two interleaved run by run.
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
from ml_conformer_generator_amd.receptor import receptor_overlap  # noqa: E402
from shape_score_time import SEED, stat, timed  # noqa: E402


def synthetic_receptor(ref: torch.Tensor, R: int, seed: int):
    """R heavy atoms (C, N, O, S) spread through a shell 4-25 A beyond the reference's atoms (never within 0.5 A of one)."""
    g = np.random.default_rng(seed)
    c = ref.double().mean(0).numpy()
    r0 = float((ref.double() - ref.double().mean(0)).norm(dim=1).max()) + 4.0
    v = g.normal(size=(R, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    xyz = c + v * (r0 + 21.0 * g.random((R, 1)))
    return torch.tensor(xyz, dtype=torch.float32), torch.tensor(g.choice([6, 6, 6, 7, 8, 16], R))


def pdb_string(xyz: torch.Tensor, z: torch.Tensor) -> str:
    sym = {6: "C", 7: "N", 8: "O", 16: "S"}
    lines = [f"ATOM  {k % 100000:5d}  {sym[int(e)]:<3} ALA A{k // 10 % 10000:4d}    {x:8.3f}{y:8.3f}{w:8.3f}  1.00 20.00"
             f"          {sym[int(e)]:>2}" for k, ((x, y, w), e) in enumerate(zip(xyz.tolist(), z.tolist()))]
    return "\n".join(lines + ["END"]) + "\n"


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
    receptors = {R: synthetic_receptor(ref, R, R) for R in (2000, 20000, 100000)}
    result = {"batches": {}, "generation": {}}
    for name, variance in (("configs[1]", 0), ("configs[2]", 12)):
        gen.generate_conformers(n_samples=256, variance=variance, **kw)
        lb = gen.last_batch
        x0, n0 = lb["x_ordered"].contiguous(), lb["n_nodes"].to(torch.int32)
        x0 = shape_overlay(ref, x0, n0, dev)["coords"].contiguous()
        z0 = lb["elements"].to(torch.long)
        for B in (64, 256):
            x, n, z = x0[:B].contiguous(), n0[:B].to(dev).contiguous(), z0[:B].contiguous()
            row = {}
            for R, rec in receptors.items():
                pairs = int(n.sum()) * R
                t = timed(lambda: receptor_overlap(rec, x, n, z, dev), dev, runs, passes)
                row[f"R={R}"] = dict(stat(t), pair_terms=pairs,
                                     gpairs_per_s=round(pairs / (statistics.median(t) * 1e-3) / 1e9, 1))
            result["batches"][f"{name} B={B}"] = row
            print(name, B, row, file=sys.stderr, flush=True)
    pocket = pdb_string(*synthetic_receptor(ref, 5000, 5))
    posed, contacts = [], []
    for _ in range(runs):
        posed += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, overlay=True, **kw), dev, 1, passes)
        contacts += timed(lambda: gen.generate_conformers(n_samples=64, variance=0, overlay=True, receptor=pocket,
                                                          max_receptor_clashes=0, **kw), dev, 1, passes)
    result["generation"] = {"workload": "generate_conformers n_samples=64, 27 atoms, diffusion_steps=100, fp32",
                            "overlay": stat(posed), "overlay+receptor(5000 atoms, PDB)": stat(contacts),
                            "overhead_pct": round(100.0 * (statistics.median(contacts) / statistics.median(posed) - 1.0),
                                                  2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
