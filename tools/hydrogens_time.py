"""Wall time of `hydrogens.add_hydrogens` on the MI355X ("Explicit hydrogens"): B = 2 048 molecules of
27 heavy atoms (the configs[1] size; 64 distinct grown molecules of tests/hydrogens_cases.py, repeated), inputs resident
on the device.  Prints the median of `--repeats` timed calls (perceive + place + the host read of the largest count), of
the placement launch alone (events), and the batch's hydrogen and rotor counts."""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=2048)
    ap.add_argument("--atoms", type=int, default=27)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import hydrogens_cases as C
    from ml_conformer_generator_amd import _lib
    from ml_conformer_generator_amd import hydrogens as HY
    from ml_conformer_generator_amd import pharmacophore as PH
    dev = torch.device("cuda:0")
    base = [C.grown(500 + k, args.atoms) for k in range(64)]
    items = [base[k % 64] for k in range(args.molecules)]
    x, z, bonds, n = (torch.from_numpy(t).to(dev) for t in C.pad_batch(items, 42, 42))
    out = HY.add_hydrogens(x, z, bonds, n, dev, return_rotors=True)
    torch.cuda.synchronize()
    wall = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        HY.add_hydrogens(x, z, bonds, n, dev, check=False)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    # the placement launch alone
    types, rings, count = PH.perceive_features(z, bonds, n, dev)
    B, W, HW = args.molecules, 42, HY.slots(42)
    bufs = [torch.empty(B, HW, 3, device=dev), torch.empty(B, HW, dtype=torch.int32, device=dev),
            torch.empty(B, W, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev)]
    zi = z.to(torch.int32).contiguous()
    kernel = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for lo in range(0, B, HY.MAX_BATCH):
            hi = min(B, lo + HY.MAX_BATCH)
            _lib.check(_lib.lib().mcg_hydrogens_place(_lib.dptr(x[lo:hi]), _lib.dptr(zi[lo:hi]), _lib.dptr(bonds[lo:hi]),
                                                      _lib.dptr(n[lo:hi]), _lib.dptr(types[lo:hi]), _lib.dptr(rings[lo:hi]),
                                                      _lib.dptr(count[lo:hi]), hi - lo, 42, W, HW,
                                                      *[_lib.dptr(t[lo:hi]) for t in bufs], None,
                                                      _lib.current_stream_ptr(dev)), "mcg_hydrogens_place")
        e1.record()
        torch.cuda.synchronize()
        kernel.append(e0.elapsed_time(e1))
    print(f"HYDROGENS_TIME molecules={B} atoms={args.atoms} hydrogens={int(out['n_hydrogens'].sum())} "
          f"rotors={int((out['rotor_delta'] >= 0).sum())} unplaced={int(out['unplaced'].sum())} "
          f"add_hydrogens_wall_ms={statistics.median(wall):.3f} place_launch_ms={statistics.median(kernel):.3f}")


if __name__ == "__main__":
    main()
