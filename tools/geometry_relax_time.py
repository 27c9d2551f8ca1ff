"""What `relax_geometry` costs on the MI355X ("Relaxed geometry").

  kernel:    `mcg_geometry_relax` alone, 200 steps, 64 and 256 molecules of 27 and 39 atoms (noisy carbon chains: the cost
             depends on the atom count and the step budget, not on the graph), device events around `--repeats` launches;
  generator: a 64-molecule, 100-step `generate_conformers` on synthetic weights with and without the option, the two
             interleaved in one process (host clock around a call that ends in a device synchronise).
Prints one JSON line.  Needs the GPU: there is no other way to get a time.

    python tools/geometry_relax_time.py [--repeats 20] [--calls 5]
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402


def chains(B, n, seed):
    """B noisy zigzag chains of n carbons: coords [B,n,3], z [B,n], bonds [B,n,n], n_nodes [B]."""
    g = torch.Generator().manual_seed(seed)
    half = math.radians(109.47) / 2.0
    step = torch.tensor([[1.52 * math.sin(half), 1.52 * math.cos(half) * (1 if m % 2 == 0 else -1), 0.0]
                         for m in range(n)])
    x = torch.cumsum(step, dim=0).unsqueeze(0).repeat(B, 1, 1) + 0.05 * torch.randn(B, n, 3, generator=g)
    bonds = torch.zeros(B, n, n, dtype=torch.int8)
    idx = torch.arange(n - 1)
    bonds[:, idx, idx + 1] = 1
    bonds[:, idx + 1, idx] = 1
    return x.float(), torch.full((B, n), 6, dtype=torch.int32), bonds, torch.full((B,), n, dtype=torch.int32)


def kernel_times(repeats):
    from ml_conformer_generator_amd import geometry
    dev = torch.device("cuda:0")
    out = {}
    for B in (64, 256):
        for n in (27, 39):
            args = [t.to(dev) for t in chains(B, n, 7 * B + n)]
            for _ in range(3):
                res = geometry.relax_geometry(*args, steps=200, check=False)
            torch.cuda.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(repeats):
                res = geometry.relax_geometry(*args, steps=200, check=False)
            end.record()
            torch.cuda.synchronize()
            out[f"B{B}_n{n}"] = {"ms_per_call": start.elapsed_time(end) / repeats,
                                 "accepted_mean": float(res["accepted_steps"].float().mean()),
                                 "energy_before_mean": float(res["energy_before"].mean()),
                                 "energy_after_mean": float(res["energy_after"].mean())}
    return out


def generator_times(calls):
    from ml_conformer_generator_amd import MLConformerGenerator
    from ml_conformer_generator_amd import weights as W
    dev = torch.device("cuda:0")
    gen = MLConformerGenerator(diffusion_steps=100, device=dev, edm_weights=W.synth_edm_state_dict(1234, weight_gain=0.3),
                               adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321), atom_order_provider=None,
                               finisher=None)
    ctx = torch.tensor([105.0766, 473.1938, 537.4675])
    kw = dict(reference_context=ctx, n_atoms=33, variance=6, n_samples=64, optimise_geometry=False, sample_seed=11)

    def call(relax):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen.generate_conformers(relax_geometry=relax, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for relax in (False, True):
        call(relax)                                   # warm-up: code objects, plans, graphs
    off, on = [], []
    for _ in range(calls):                            # interleaved: both see the same box
        off.append(call(False))
        on.append(call(True))
    med = lambda v: sorted(v)[len(v) // 2]            # noqa: E731
    return {"off_ms": off, "on_ms": on, "off_median_ms": med(off), "on_median_ms": med(on),
            "added_median_ms": med(on) - med(off), "added_share": (med(on) - med(off)) / med(off)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("geometry_relax_time.py needs the GPU: a time measured anywhere else says nothing")
    print(json.dumps({"kernel_200_steps": kernel_times(a.repeats), "generate_conformers_64x100": generator_times(a.calls)}))


if __name__ == "__main__":
    main()
