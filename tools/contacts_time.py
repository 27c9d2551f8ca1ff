#!/usr/bin/env python3
"""Cost of the receptor contact fingerprint (`contacts.py`, `interaction_scores="contacts"`) on one MI355X, beside the
interaction score on the same inputs.

  kernels:   one `mcg_receptor_contacts` launch and one `mcg_receptor_interactions` launch, each the raw C entry on buffers
             allocated outside the timed region, over 2 048 molecules of 42 atoms - random walks placed at random inside a
             ball of synthetic receptor atoms of protein density (`interaction_time.ball_receptor`, `walks`) - against the
             100 000-atom receptor, every atom its own residue-sized group of eight, with tile skipping on and off;
  timing:    device events round single launches: `--warmup` untimed launches, then the median, min and max of `--runs`
             (21) timed ones; the two kernels interleaved launch by launch, so a drifting clock meets both alike;
  also:      the same contacts launch with a 40-entry reference list joined in the epilogue, and how many groups and
             contacting receptor atoms a molecule has (what the sort epilogue works on).
Nothing else should run on the GPU.  No threshold: a record.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from ml_conformer_generator_amd import _lib  # noqa: E402
from ml_conformer_generator_amd import contacts as CT  # noqa: E402
from ml_conformer_generator_amd import interactions as IX  # noqa: E402
from interaction_time import ball_receptor, walks  # noqa: E402
from shape_score_time import stat  # noqa: E402


def one_launch_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-samples", type=int, default=2048)
    ap.add_argument("--atoms", type=int, default=42)
    ap.add_argument("--receptor-atoms", type=int, default=100000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n, R = args.n_samples, args.atoms, args.receptor_atoms
    g = torch.Generator().manual_seed(7)
    z = torch.tensor([6, 6, 6, 7, 8])[torch.randint(0, 5, (B, n), generator=g)].to(dev)
    types = torch.randint(0, 8, (B, n), generator=g).to(dev, torch.uint8)
    radii = IX.interaction_radii(z).contiguous()
    nn = torch.full((B,), n, dtype=torch.int32, device=dev)
    rot = torch.randint(0, 9, (B,), generator=g).to(dev, torch.int32)
    rec, radius = ball_receptor(R, R)
    typed = IX.prepare_receptor(rec)
    prepared = CT.PreparedReceptor(typed.xyzr, typed.types, typed.spheres, torch.arange(R, dtype=torch.int32) // 8)
    x = walks(B, n, max(radius - 6.0, 1.0), R + 1).to(dev).contiguous()
    xyzr, rec_t, rec_g, spheres = (t.to(dev) for t in (prepared.xyzr, prepared.types, prepared.groups, prepared.spheres))
    out = dict(groups=torch.zeros(B, 256, dtype=torch.int32, device=dev), kinds=torch.zeros(B, 256, dtype=torch.uint8, device=dev),
               n_groups=torch.zeros(B, dtype=torch.int32, device=dev), atom_kinds=torch.zeros(B, n, dtype=torch.uint8, device=dev),
               status=torch.zeros(B, dtype=torch.int32, device=dev), counts=torch.zeros(B, 3, dtype=torch.int32, device=dev))
    terms = dict(atoms=torch.zeros(B, n, 6, device=dev), mol=torch.zeros(B, 8, device=dev),
                 hbonds=torch.zeros(B, dtype=torch.int32, device=dev))
    lib, p, stream = _lib.lib(), _lib.dptr, _lib.current_stream_ptr(dev)
    ref_g = (torch.arange(40, dtype=torch.int32) * 7).to(dev)
    ref_k = torch.full((40,), 14, dtype=torch.uint8, device=dev)

    def contacts(skip, join=False):
        _lib.check(lib.mcg_receptor_contacts(
            p(x), p(radii), p(types), p(nn), B, n, p(xyzr), p(rec_t), p(rec_g), R, p(spheres) if skip else None,
            p(ref_g) if join else None, p(ref_k) if join else None, 40 if join else 0, CT.DEFAULT_KINDS, p(out["groups"]),
            p(out["kinds"]), p(out["n_groups"]), p(out["atom_kinds"]), p(out["status"]), p(out["counts"]) if join else None,
            stream), "mcg_receptor_contacts")

    def interactions(skip):
        _lib.check(lib.mcg_receptor_interactions(
            p(x), p(radii), p(types), p(nn), p(rot), B, n, p(xyzr), p(rec_t), R, p(spheres) if skip else None,
            p(terms["atoms"]), p(terms["mol"]), p(terms["hbonds"]), stream), "mcg_receptor_interactions")

    result = {"rows": B, "atoms": n, "receptor_atoms": R, "tiles": int(prepared.spheres.shape[0]), "runs": args.runs}
    for skip in (True, False):
        for _ in range(args.warmup):
            contacts(skip), contacts(skip, True), interactions(skip)
        torch.cuda.synchronize(dev)
        t = {"contacts": [], "contacts_with_reference": [], "interactions": []}
        for _ in range(args.runs):
            t["interactions"].append(one_launch_ms(lambda: interactions(skip)))
            t["contacts"].append(one_launch_ms(lambda: contacts(skip)))
            t["contacts_with_reference"].append(one_launch_ms(lambda: contacts(skip, True)))
        row = {k: stat(v) for k, v in t.items()}
        row["ratio"] = round(statistics.median(t["contacts"]) / statistics.median(t["interactions"]), 3)
        result["skip_tiles" if skip else "every_tile"] = row
        print({skip: row}, file=sys.stderr, flush=True)
    contacts(True)
    torch.cuda.synchronize(dev)
    status = out["status"].cpu()
    result["status_counts"] = {name: int((status == k).sum()) for k, name in enumerate(CT.STATUS_NAMES)}
    result["mean_groups"] = round(float(out["n_groups"].float().mean()), 1)
    result["max_groups"] = int(out["n_groups"].max())
    kept = {k: v.clone() for k, v in out.items() if k != "counts"}
    contacts(False)
    torch.cuda.synchronize(dev)
    result["identical"] = all(torch.equal(kept[k], out[k]) for k in kept)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
