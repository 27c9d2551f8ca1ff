#!/usr/bin/env python3
"""Every output bit of the receptor and rigid-body walk entries (`mcg_receptor_relieve`, `mcg_receptor_optimise`,
`mcg_receptor_interactions`, `mcg_shape_overlay_refined`) over the tests' own case sets, for comparing two builds of the
library (MCG_LIB_PATH selects one):

  MCG_LIB_PATH=<a.so> python tools/walk_bits.py --out a.npz      one MI355X, a fresh process per library
  MCG_LIB_PATH=<b.so> python tools/walk_bits.py --out b.npz
  python tools/walk_bits.py --compare a.npz b.npz                no GPU: one line per entry, exit status 1 on a difference

The inputs are `relief_ref.cases()` (steps 0, 1, 32; padded widths n, 41, 64; tile skipping on and off; with the
gradient), `pose_optimise_ref.cases()` (steps 0, 1, 8, 64 with the trace; the same widths and skipping), the interaction
cases and hand pairs, the golden pairs of the refined overlay (steps 0 and 64, with the objective and the refined scores),
and per entry one batch of 70 mixed-size rows with one empty and one non-finite row.  Arrays are compared as int32 views,
so NaN rows compare by their bits too."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

WIDTHS = (None, 41, 64)                       # None: the case's own atom count


def _bits(t):
    """A tensor as the int32 (or wider integer) array of its bits."""
    a = t.detach().cpu().contiguous().numpy()
    if a.dtype == np.float32:
        return a.view(np.int32)
    return a.astype(np.int64) if a.dtype.kind in "bui" else a


def _widths(n):
    return sorted({max(n, 1) if w is None else w for w in WIDTHS if w is None or w >= n})


def _spoilt(case, value):
    """A copy of `case` with one non-finite coordinate."""
    import copy
    bad = copy.copy(case)
    bad.x = case.x.copy()
    bad.x[min(4, case.n - 1), 1] = np.float32(value)
    return bad


def dump_relief(out, dev):
    import relief_ref as RR
    from ml_conformer_generator_amd import receptor as RC
    cases = RR.cases()
    for c in cases:
        for steps in (0, 1, 32):
            for width in _widths(c.n):
                for skip in (True, False):
                    x, n, z = RR.pad([c], width)
                    got = RC.relieve_clashes(c.receptor, x, n, z, steps=steps, device=dev, return_gradient=True,
                                             skip_tiles=skip)
                    for k, v in got.items():
                        out[f"relieve/{c.name}/steps{steps}/w{width}/skip{int(skip)}/{k}"] = _bits(v)
    host = next(c for c in cases if c.name == "multi")
    batch = [RR.Case(f"o{k}", 5000 + k, 5 + k % 36) for k in range(70)]
    batch[37] = host
    batch[11] = _spoilt(batch[11], "nan")
    x, n, z = RR.pad(batch, 41)
    n[53] = 0
    got = RC.relieve_clashes(host.receptor, x, n, z, steps=32, device=dev, return_gradient=True)
    for k, v in got.items():
        out[f"relieve/batch70/{k}"] = _bits(v)


def _typed(case_list, width, radii):
    import torch
    B = len(case_list)
    x = np.full((B, width, 3), 7.5, dtype=np.float32)
    r = np.full((B, width), 1.9, dtype=np.float32)
    t = np.full((B, width), 7, dtype=np.uint8)
    for b, c in enumerate(case_list):
        x[b, : c.n], r[b, : c.n], t[b, : c.n] = c.x, radii(c.z), c.t
    return (torch.from_numpy(x), torch.tensor([c.n for c in case_list], dtype=torch.int32), torch.from_numpy(r),
            torch.from_numpy(t), torch.tensor([c.n_rot for c in case_list], dtype=torch.int32))


def dump_optimise(out, dev):
    import interactions_ref as IR
    import pose_optimise_ref as P
    from ml_conformer_generator_amd import interactions as IX
    cases = P.cases()
    for c in cases:
        prepared = IX.prepare_receptor(c.receptor)
        for steps in (0, 1, 8, 64):
            for width in _widths(c.n):
                for skip in (True, False):
                    x, n, r, t, _ = _typed([c], width, IR.radii)
                    got = IX.optimise_typed(prepared, x, n, r, t, steps, 2.0, skip, dev, trace=True)
                    for k, v in got.items():
                        out[f"optimise/{c.name}/steps{steps}/w{width}/skip{int(skip)}/{k}"] = _bits(v)
    host = cases[2]
    batch = [IR.Case(f"o{k}", 5000 + k, 1 + k % 40) for k in range(70)]
    batch[37] = host
    batch[53] = IR.Case("empty", 51, 0)
    batch[11] = _spoilt(batch[11], "inf")
    x, n, r, t, _ = _typed(batch, 41, IR.radii)
    got = IX.optimise_typed(host.receptor, x, n, r, t, 64, 2.0, True, dev, trace=True)
    for k, v in got.items():
        out[f"optimise/batch70/{k}"] = _bits(v)


def dump_interactions(out, dev):
    import interactions_cases as K
    import interactions_ref as IR
    from ml_conformer_generator_amd import interactions as IX
    cases = IR.cases()
    for name, (pair, _) in K.HAND.items():
        c = IR.Case("hand", 1, 1)
        c.x, c.z, c.t, c.n_rot = pair["x"], np.array(pair["z"]), np.array(pair["t"], dtype=np.uint8), 0
        c.rec, c.rec_z, c.rec_t = pair["y"], np.array(pair["zr"]), np.array(pair["tr"], dtype=np.uint8)
        cases.append(c)
        c.name = "hand_" + "".join(ch if ch.isalnum() else "_" for ch in name)
    for c in cases:
        prepared = IX.prepare_receptor(c.receptor)
        for width in _widths(c.n):
            for skip in (True, False):
                x, n, r, t, rot = _typed([c], width, IR.radii)
                got = IX.score_typed(prepared, x, n, r, t, rot, skip_tiles=skip, device=dev)
                for k, v in got.items():
                    out[f"interactions/{c.name}/w{width}/skip{int(skip)}/{k}"] = _bits(v)
    host = cases[2]
    batch = [IR.Case(f"o{k}", 5000 + k, 1 + k % 40) for k in range(70)]
    batch[37] = host
    batch[53] = IR.Case("empty", 51, 0)
    batch[11] = _spoilt(batch[11], "nan")
    x, n, r, t, rot = _typed(batch, 41, IR.radii)
    got = IX.score_typed(host.receptor, x, n, r, t, rot, device=dev)
    for k, v in got.items():
        out[f"interactions/batch70/{k}"] = _bits(v)


def dump_refine(out, dev):
    import torch
    import overlay_refine_ref as RR
    from ml_conformer_generator_amd import cheminformatics as CH
    z = np.load(os.path.join(REPO, "tests", "golden", "shape_quadrupole.npz"), allow_pickle=False)
    golden = {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind == "f" and z[k].ndim > 0}

    def pad(mols, N=None):
        N = N or max(int(m.shape[0]) for m in mols)
        x = torch.zeros(len(mols), N, 3)
        for b, m in enumerate(mols):
            x[b, : m.shape[0]] = m.to(torch.float32)
        return x, torch.tensor([int(m.shape[0]) for m in mols], dtype=torch.int32)

    def run(tag, ref, x, n, steps):
        # the refined entry itself, also at steps = 0, with the objective and the refined scores
        got = CH._overlay(ref, x, n, device=dev, with_scores=True, steps=steps, refined_entry=True)
        for k, v in got.items():
            out[f"refine/{tag}/steps{steps}/{k}"] = _bits(v)

    for ref_name in RR.TABLE_REFERENCES:
        pairs = [p for p in RR.table_pairs(golden) if p[0] == ref_name]
        x, n = pad([p[3] for p in pairs])
        for steps in (0, 64):
            run(ref_name, pairs[0][2], x, n, steps)
    g = torch.Generator().manual_seed(5)
    mols = []
    for k in torch.randint(1, 64, (70,), generator=g):             # random chains, 1.5 A steps
        d = torch.randn(int(k), 3, generator=g)
        mols.append(torch.cumsum(1.5 * d / d.norm(dim=1, keepdim=True), 0))
    mols[11] = mols[11].clone()
    mols[11][0, 2] = float("nan")
    x, n = pad(mols, 64)
    n[53] = 0
    for steps in (0, 64):
        run("batch70", golden["xyz_ceyyag"].to(torch.float32), x, n, steps)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    worst = 0
    if set(a.files) != set(b.files):
        print(f"DIFFERENT key sets: {sorted(set(a.files) ^ set(b.files))[:5]} ...")
        worst = 1
    for entry in sorted({k.split("/")[0] for k in a.files}):
        keys = [k for k in a.files if k.split("/")[0] == entry and k in b.files]
        differing = [k for k in keys if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]
        words = sum(int(a[k].size) for k in keys)
        print(f"{entry}: {len(keys)} arrays, {words} words, {'EQUAL' if not differing else 'DIFFERENT'}"
              + (f" in {len(differing)}: {differing[:3]}" if differing else ""))
        worst |= bool(differing)
    return worst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="write every output to this .npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two dumps, no GPU")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("--out or --compare")
    import torch
    dev = torch.device("cuda:0")
    out = {}
    for part in (dump_interactions, dump_relief, dump_optimise, dump_refine):
        part(out, dev)
        torch.cuda.synchronize()
        print(f"{part.__name__}: {len(out)} arrays so far", file=sys.stderr, flush=True)
    np.savez_compressed(args.out, **out)
    print(f"{len(out)} arrays from {os.environ.get('MCG_LIB_PATH') or 'the package library'} -> {args.out}")


if __name__ == "__main__":
    main()
