#!/usr/bin/env python3
"""Cost of the substructure matching (`require_substructures`, `exclude_substructures`, `substructure_counts`) on one
MI355X.

Input: the 2 048 molecule-like graphs of 42 atoms the fingerprint and canonical tools time
(`fingerprint_time.molecule_like_batch`: random trees of degree <= 3 with 0-3 ring closures).
  catalogue:  one `mcg_substructure_match` launch of the graphs against `substructure.CATALOGUE` (its patterns constrain
              hydrogens: the counts are computed once, outside the timed region, and passed in);
  scaffold:   one launch against ONE 12-atom pattern, `substructure.from_graph` of the first 12 atoms of the first graph
              (a connected piece by construction: atom a of the tree bonds to an earlier atom);
  yardstick:  `mcg_canonical_order` over the same tensors.
Timed with device events: `--warmup` untimed launches, then the median, min and max of `--runs` runs of `--passes`
launches each.  Nothing else should run on the GPU.  No threshold: a record.  Prints one JSON line."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from ml_conformer_generator_amd import canonical as CN  # noqa: E402
from ml_conformer_generator_amd import hydrogens as HY  # noqa: E402
from ml_conformer_generator_amd import substructure as SUB  # noqa: E402
from fingerprint_time import event_times, molecule_like_batch  # noqa: E402
from shape_score_time import stat  # noqa: E402


def summary(out):
    count, status = out["count"].cpu(), out["status"].cpu()
    return {"pairs_with_a_match": int((count > 0).sum()), "pairs": int(count.numel()),
            "budget_pairs": int((status != 0).sum()), "largest_count": int(count.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-samples", type=int, default=2048)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    z, bonds, n = molecule_like_batch(args.n_samples, 42, 2048)
    nh = HY.implicit_counts(z, bonds, n).to(dev)
    scaffold = SUB.compile_patterns([(z[0, :12].tolist(), bonds[0, :12, :12])])
    catalogue = SUB.compile_patterns(list(SUB.CATALOGUE.values()))
    z, bonds, n = z.to(dev), bonds.to(dev), n.to(dev)
    timing = (dev, args.warmup, args.runs, args.passes)
    result = {"rows": args.n_samples, "atoms": 42}
    for name, compiled, h in (("catalogue", catalogue, nh), ("scaffold", scaffold, False)):
        def launch():
            return SUB.match_substructures(z, bonds, n, compiled, hydrogens=h, device=dev, check=False)
        result[name] = dict(summary(launch()), patterns=len(compiled.patterns), ms=stat(event_times(launch, *timing)))
        print({name: result[name]}, file=sys.stderr, flush=True)
    result["canonical_order"] = stat(event_times(lambda: CN.canonical_order(z, bonds, n, dev, check=False), *timing))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
