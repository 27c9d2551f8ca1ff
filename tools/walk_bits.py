#!/usr/bin/env python3
"""Every output bit of the receptor and rigid-body walk entries (`mcg_receptor_relieve`, `mcg_receptor_optimise`,
`mcg_receptor_interactions`, `mcg_shape_overlay_refined`, `mcg_torsion_tree` + `mcg_receptor_optimise_flex`, the pose
search) over the tests' own case sets, for comparing two builds of the library (MCG_LIB_PATH selects one):

  MCG_LIB_PATH=<a.so> python tools/walk_bits.py --out a.npz      one MI355X, a fresh process per library
  MCG_LIB_PATH=<b.so> python tools/walk_bits.py --out b.npz
  python tools/walk_bits.py --compare a.npz b.npz                no GPU: one line per entry, exit status 1 on a difference

The inputs are `relief_ref.cases()` (steps 0, 1, 32; padded widths n, 41, 64; tile skipping on and off; with the
gradient), `pose_optimise_ref.cases()` (steps 0, 1, 8, 64 with the trace; the same widths and skipping), the interaction
cases and hand pairs, the golden pairs of the refined overlay (steps 0 and 64, with the objective and the refined scores),
`flex_cases.cases()` through the tree and the flexible walk (steps, widths and skipping as the optimiser's, with the trace),
a few of the search tests' pools through `search_pose` with 1 and 5 starts (every returned tensor, `starts` included), and
per entry one batch of 70 mixed-size rows with one empty and one non-finite row.  `--parts` dumps some entries only.
Arrays are compared as int32 views, so NaN rows compare by their bits too."""
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


FLEX_OFFSET = np.array([0.6, -0.3, 0.2])      # out of the middle of the pocket, as the flexible-pose tests place a graph


def _graph_batch(graphs, width, spoil=None):
    """(coords, n_nodes, atomic numbers, bond codes) of `flex_cases` graphs placed as the flexible-pose tests place them;
    `spoil`: a row that gets one non-finite coordinate."""
    import torch
    import flex_cases as FC
    z, bonds, n, _ = FC.padded(graphs, width)
    x = np.zeros((len(graphs), width, 3), dtype=np.float32)
    for b, g in enumerate(graphs):
        if g.n:
            x[b, : g.n] = (g.x.astype(np.float64) - g.x.astype(np.float64).mean(axis=0) + FLEX_OFFSET).astype(np.float32)
    if spoil is not None:
        x[spoil, min(4, graphs[spoil].n - 1), 1] = np.float32("inf")
    return tuple(torch.from_numpy(v) for v in (x, n, z, bonds))


def dump_flex(out, dev):
    import flex_cases as FC
    import interactions_ref as IR
    from ml_conformer_generator_amd import interactions as IX
    receptors = IR.cases()
    graphs = FC.cases()
    for g in graphs:
        # each graph in its own receptor, by the flexible-pose tests' rule: 1, 255, 256, 257, 4 097 atoms and the pockets
        prepared = IX.prepare_receptor(receptors[(2, 4, 5, 6, 7, 8, 3)[sum(map(ord, g.name)) % 7]].receptor)
        for width in _widths(g.n):
            x, n, z, bonds = _graph_batch([g], width)
            for k, v in IX.torsion_tree(z, bonds, n, dev).items():
                out[f"flex/{g.name}/w{width}/tree/{k}"] = _bits(v)
            for steps in (0, 1, 8, 64):
                for skip in (True, False):
                    got = IX.optimise_pose_flexible(prepared, x, n, z, bonds, steps, 2.0, dev, trace=True, skip_tiles=skip)
                    for k, v in got.items():
                        out[f"flex/{g.name}/steps{steps}/w{width}/skip{int(skip)}/{k}"] = _bits(v)
    pool = [g for g in graphs if 1 <= g.n <= 41]
    batch = [pool[(3 * k) % len(pool)] for k in range(70)]
    batch[53] = FC.by_name()["empty"]
    x, n, z, bonds = _graph_batch(batch, 41, spoil=11)
    got = IX.optimise_pose_flexible(receptors[2].receptor, x, n, z, bonds, 64, 2.0, dev, trace=True)
    for k, v in got.items():
        out[f"flex/batch70/{k}"] = _bits(v)


def dump_search(out, dev):
    import flex_cases as FC
    import interactions_ref as IR
    from ml_conformer_generator_amd import interactions as IX
    by_name, pocket = FC.by_name(), IR.cases()[5].receptor
    pools = (("pool5", ("hexane", "isopentylbenzene", "toluene", "folded_heptane", "empty"), 14, 6, 3, None),
             ("pool8", ("hexane", "isopentylbenzene", "toluene", "folded_heptane", "empty", "biphenyl", "c20", "one_atom"),
              20, 8, 5, 5),
             ("pool3", ("hexane", "toluene", "isopentylbenzene"), 11, 64, 9, None))
    for tag, names, width, steps, seed, spoil in pools:
        x, n, z, bonds = _graph_batch([by_name[k] for k in names], width, spoil)
        for S in (1, 5):
            got = IX.search_pose(pocket, x, n, z, bonds, starts=S, steps=steps, seed=seed, device=dev)
            for k, v in got.items():
                for kk, vv in (v.items() if isinstance(v, dict) else ((None, v),)):
                    out[f"search/{tag}/S{S}/{k}" + (f"/{kk}" if kk else "")] = _bits(vv)


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


PARTS = dict(interactions=dump_interactions, relieve=dump_relief, optimise=dump_optimise, refine=dump_refine, flex=dump_flex,
             search=dump_search)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="write every output to this .npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two dumps, no GPU")
    ap.add_argument("--parts", nargs="+", choices=sorted(PARTS), default=sorted(PARTS), help="the entries to dump")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("--out or --compare")
    import torch
    dev = torch.device("cuda:0")
    out = {}
    for part in (PARTS[k] for k in args.parts):
        part(out, dev)
        torch.cuda.synchronize()
        print(f"{part.__name__}: {len(out)} arrays so far", file=sys.stderr, flush=True)
    np.savez_compressed(args.out, **out)
    print(f"{len(out)} arrays from {os.environ.get('MCG_LIB_PATH') or 'the package library'} -> {args.out}")


if __name__ == "__main__":
    main()
