"""Wall time of `standardize.standardize_graphs` on the MI355X ("Standardised graphs"): B = 2 048
molecules of 27 heavy atoms (the configs[1] size; 64 distinct drug-like graphs - an aromatic core of
tests/standardize_cases.py, a side chain, every eighth with a stray atom - repeated), inputs resident on the device.
Prints the median of `--repeats` timed calls (the launch and its allocations, ending in a device synchronise), of the
launch alone (device events), and what the batch held."""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def grown(k, atoms):
    """Graph k of `atoms` atoms: a core, a chain of C / N / O from one of its two-bond carbons, and for every eighth k a
    last atom left unbonded."""
    import numpy as np
    import standardize_cases as C
    cores = ["benzene", "pyridine", "indole", "benzimidazole", "naphthalene", "2-pyridone", "pyrazine", "furan"]
    z, codes, n = C.cases()[cores[k % len(cores)]]["mol"]
    z = list(z)
    bonds = [(i, j, codes[i][j]) for i in range(n) for j in range(i) if codes[i][j]]
    rng = np.random.RandomState(900 + k)
    anchor = max(a for a in range(n) if z[a] == 6 and sum(1 for c in codes[a] if c) == 2)
    stray = k % 8 == 7
    while len(z) < atoms - (1 if stray else 0):       # a plain chain: every atom in it has at most two bonds
        z.append(int(rng.choice([6, 6, 6, 7, 8])))
        bonds.append((anchor, len(z) - 1, 1))
        anchor = len(z) - 1
    if stray:
        z.append(8)
    xyz = (rng.standard_normal((len(z), 3)) * 3.0).astype(np.float32)
    return dict(mol=C.mol(z, bonds), xyz=xyz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=2048)
    ap.add_argument("--atoms", type=int, default=27)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import standardize_cases as C
    from ml_conformer_generator_amd import _lib
    from ml_conformer_generator_amd import standardize as S
    dev = torch.device("cuda:0")
    base = [grown(k, args.atoms) for k in range(64)]
    items = [base[k % 64] for k in range(args.molecules)]
    x, z, bonds, n = (torch.from_numpy(t).to(dev) for t in C.pad_batch(items, 42, 42))
    out = S.standardize_graphs(x, z, bonds, n, dev)
    torch.cuda.synchronize()
    wall = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        S.standardize_graphs(x, z, bonds, n, dev, check=False)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    B, W = args.molecules, 42
    i32 = dict(dtype=torch.int32, device=dev)
    bufs = [torch.empty(B, 42, 3, device=dev), torch.empty(B, W, **i32), torch.empty(B, W, W, dtype=torch.int8, device=dev),
            torch.empty(B, W, W, dtype=torch.int8, device=dev), torch.empty(B, W, **i32)] + [torch.empty(B, **i32) for _ in range(4)]
    kernel = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for lo in range(0, B, S.MAX_BATCH):
            hi = min(B, lo + S.MAX_BATCH)
            _lib.check(_lib.lib().mcg_standardize_graphs(_lib.dptr(x[lo:hi]), _lib.dptr(z[lo:hi]), _lib.dptr(bonds[lo:hi]),
                                                         _lib.dptr(n[lo:hi]), hi - lo, 42, W,
                                                         *[_lib.dptr(t[lo:hi]) for t in bufs],
                                                         _lib.current_stream_ptr(dev)), "mcg_standardize_graphs")
        e1.record()
        torch.cuda.synchronize()
        kernel.append(e0.elapsed_time(e1))
    print(f"STANDARDIZE_TIME molecules={B} atoms={args.atoms} valid={int(out['valid'].sum())} "
          f"atoms_removed={int(out['atoms_removed'].sum())} aromatic_bonds={int((out['bond_orders'] == 4).sum()) // 2} "
          f"standardize_wall_ms={statistics.median(wall):.3f} launch_ms={statistics.median(kernel):.3f}")


if __name__ == "__main__":
    main()
