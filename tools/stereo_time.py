#!/usr/bin/env python3
"""Cost of the stereo identity (`smiles="isomeric"`, `unique="stereo"`) on one MI355X.

One `mcg_stereo_order` launch beside one `mcg_canonical_order` launch over the same 2 048 molecule-like graphs of 42 atoms
(`fingerprint_time.molecule_like_batch`: random trees of degree <= 3 with 0-3 ring closures, every row searched), with
seeded random coordinates: the stereo launch adds the fp32 prepass, one byte store and - on certificate ties - one wave
minimum per leaf, and visits the leaves the graph search's twin rule skips for non-terminal twins.
Timed with device events, protocol as `canonical_time.py`: `--warmup` untimed launches, then the median, min and max of
`--runs` runs of `--passes` launches each.  Nothing else should run on the GPU.  Prints one JSON line."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from ml_conformer_generator_amd import canonical as CN  # noqa: E402
from ml_conformer_generator_amd import stereo as ST  # noqa: E402
from fingerprint_time import event_times, molecule_like_batch  # noqa: E402
from shape_score_time import stat  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-samples", type=int, default=2048)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    z, bonds, n = (t.to(dev) for t in molecule_like_batch(args.n_samples, 42, 2048))
    x = (torch.rand(args.n_samples, 42, 3, generator=torch.Generator().manual_seed(2048)) * 8.0 - 4.0).to(dev)
    graph = CN.canonical_order(z, bonds, n, dev, check=False)
    out = ST.stereo_order(x, z, bonds, n, dev, check=False)
    both = (graph["status"] == 0) & (out["status"] == 0)
    status = out["status"].cpu()
    result = {"rows": int(status.numel()),
              "stereo_order": stat(event_times(lambda: ST.stereo_order(x, z, bonds, n, dev, check=False), dev, args.warmup,
                                               args.runs, args.passes)),
              "canonical_order": stat(event_times(lambda: CN.canonical_order(z, bonds, n, dev, check=False), dev, args.warmup,
                                                  args.runs, args.passes)),
              "status_counts": {CN.describe_status(s): int((status == s).sum()) for s in sorted(set(status.tolist()))},
              "graph_keys_equal": bool((graph["key"][both] == out["key"][both]).all()),
              "leaves": {"stereo": int(out["leaves"].sum()), "canonical": int(graph["leaves"].sum()),
                         "largest_stereo": int(out["leaves"].max())},
              "counts": dict(zip(("tetrahedral", "double_bonds", "undefined"), out["counts"].sum(dim=0).tolist())),
              "distinct_stereo_keys": int(torch.unique(out["stereo_key"]).numel()),
              "distinct_graph_keys": int(torch.unique(out["key"]).numel())}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
