#!/usr/bin/env python3
"""Cost of the keyed noise stream (`sample_seed`) on one MI355X: ms per generation pass with and without a sample seed.

Workloads: BASELINE configs[1] (n_samples=64, 27 heavy atoms, diffusion_steps=100, fp32) and the same with 4 molecules.
Per workload and mode: `--runs` runs of `--passes` timed `generate_conformers` passes each (after `--warmup` passes), the
two modes interleaved run by run so that clock drift hits both alike.  Reported: wall ms per pass (host-synchronised) and
the sampler's own ms per pass (HIP events around `edm_tensors`' sampler, the window `bench.py` reports as sampler time).
The keyed kernel's own time per launch comes from a separate `rocprofv3 --kernel-trace --stats` run of this script
(kernel `k_noise_keyed`).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ml_conformer_generator_amd import MLConformerGenerator, weights as W  # noqa: E402
from ml_conformer_generator_amd.synthetic import DUMMY_CONTEXT  # noqa: E402


def one_run(gen, dev, ctx, n_samples, passes, sample_seed):
    walls, samplers = [], []
    for _ in range(passes):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        gen.generate_conformers(reference_context=ctx, n_atoms=27, variance=0, n_samples=n_samples,
                                optimise_geometry=False, sample_seed=sample_seed)
        torch.cuda.synchronize(dev)
        walls.append((time.perf_counter() - t0) * 1e3)
        samplers.append(gen._timing["sampler_start"].elapsed_time(gen._timing["sampler_end"]))
    return statistics.mean(walls), statistics.mean(samplers)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=str, default="64,4", help="n_samples of the workloads, comma separated")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = MLConformerGenerator(diffusion_steps=100, device=dev, edm_weights=W.synth_edm_state_dict(1234, recipe="v2d"),
                               adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321), atom_order_provider=None,
                               n_host_workers=0)
    gen._timing = {"sampler_start": torch.cuda.Event(enable_timing=True),
                   "sampler_end": torch.cuda.Event(enable_timing=True)}
    ctx = torch.tensor(DUMMY_CONTEXT)
    out = {"workload": "generate_conformers(n_atoms=27, variance=0), diffusion_steps=100, fp32", "results": {}}
    for n_samples in (int(v) for v in args.sizes.split(",")):
        modes = {"default": None, "seeded": 20261015}
        for seed in modes.values():
            for _ in range(args.warmup):
                one_run(gen, dev, ctx, n_samples, 1, seed)
        res = {m: {"wall_ms": [], "sampler_ms": []} for m in modes}
        for _ in range(args.runs):
            for m, seed in modes.items():
                wall, samp = one_run(gen, dev, ctx, n_samples, args.passes, seed)
                res[m]["wall_ms"].append(round(wall, 3))
                res[m]["sampler_ms"].append(round(samp, 3))
        d, s = res["default"], res["seeded"]
        res["seeded_over_default_wall"] = round(statistics.median(s["wall_ms"]) / statistics.median(d["wall_ms"]) - 1, 5)
        res["seeded_over_default_sampler"] = round(
            statistics.median(s["sampler_ms"]) / statistics.median(d["sampler_ms"]) - 1, 5)
        out["results"][f"n_samples={n_samples}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
