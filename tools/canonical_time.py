#!/usr/bin/env python3
"""Cost of the canonical labelling (`smiles`, `unique="exact"`, `exclude_graphs`) on one MI355X.

  generated:     one `mcg_canonical_order` launch over the graphs of 2 048 generated molecules - one
                 `generate_conformers` call at the benchmark's headline shape (bench.py: 27 atoms, 100 steps, fp32,
                 synthetic weights) with every record kept - and, as the yardstick, `mcg_graph_fingerprint` over the same
                 tensors.  The synthetic weights write dense graphs, most of which the labelling refuses with DEGREE
                 before any search: the status counts are printed beside the times.
  molecule-like: the same two launches over 2 048 molecule-like graphs of 42 atoms (`fingerprint_time.molecule_like_batch`:
                 random trees of degree <= 3 with 0-3 ring closures), where every row is searched.
Timed with device events: `--warmup` untimed launches, then the median, min and max of `--runs` runs of `--passes`
launches each.  Nothing else should run on the GPU.  Prints one JSON line."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ml_conformer_generator_amd import MLConformerGenerator, weights as W  # noqa: E402
from ml_conformer_generator_amd import canonical as CN  # noqa: E402
from ml_conformer_generator_amd import conformer_generator as CG  # noqa: E402
from ml_conformer_generator_amd import fingerprint as FP  # noqa: E402
from fingerprint_time import event_times, molecule_like_batch  # noqa: E402
from shape_score_time import SEED, stat  # noqa: E402


def measure(z, bonds, n, dev, warmup, runs, passes):
    out = CN.canonical_order(z, bonds, n, dev, check=False)
    status = out["status"].cpu()
    return {"rows": int(status.numel()),
            "canonical_order": stat(event_times(lambda: CN.canonical_order(z, bonds, n, dev, check=False), dev, warmup, runs,
                                                passes)),
            "graph_fingerprint": stat(event_times(lambda: FP.graph_fingerprints(z, bonds, n, dev, check=False), dev, warmup,
                                                  runs, passes)),
            "status_counts": {CN.describe_status(s): int((status == s).sum()) for s in sorted(set(status.tolist()))},
            "largest_leaves": int(out["leaves"].max()), "distinct_keys": int(torch.unique(out["key"]).numel())}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-samples", type=int, default=2048)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {}
    z, bonds, n = (t.to(dev) for t in molecule_like_batch(args.n_samples, 42, 2048))
    result["molecule-like, 42 atoms"] = measure(z, bonds, n, dev, args.warmup, args.runs, args.passes)
    print(result, file=sys.stderr, flush=True)
    ref = torch.as_tensor(np.load(os.path.join(REPO, "tests", "golden", "shape_quadrupole.npz"))["xyz_walk27"])
    gen = MLConformerGenerator(diffusion_steps=100, device=dev, edm_weights=W.synth_edm_state_dict(1234, recipe="v2d"),
                               adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321), atom_order_provider=None)
    CG._finish = lambda mols, og, use_rdkit=None: (list(mols), 1.0)           # keep every record, valid or not
    mols = gen.generate_conformers(reference_conformer=ref, n_samples=args.n_samples, variance=0, optimise_geometry=False,
                                   sample_seed=SEED)
    z, bonds, n = FP.pad_graphs([FP.mol_graph(m) for m in mols])
    result["generated, 27 atoms"] = measure(z.to(dev), bonds.to(dev), n.to(dev), dev, args.warmup, args.runs, args.passes)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
