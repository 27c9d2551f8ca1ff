#!/usr/bin/env python3
"""Benchmark of the mlconfgen denoising hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W [--full]

A "step" is ONE call of the public path `MLConformerGenerator.generate_conformers_sharded` over one batch of
synthetic input: the full ancestral sampler (T = 100 denoising steps = 101 EGNN calls), the device-side
EDM->GCN hand-off, the AdjMatSeer GCN pass, bond argmax + write-back + validity proxy, the RCCL gather to
rank 0 (N > 1), the final D2H copy and the host-side assembly of the molecule records.
Workload at N = 1: BASELINE.json configs[1] (n_samples = 64, 27 heavy atoms, diffusion_steps = 100,
fp32).  For N > 1 every rank generates its contiguous shard of 64 x N molecules (weak scaling, 64 per GPU)
on its own weight replica; the results are gathered once with RCCL at the end of each step.

A plain run does only what the headline needs: set-up, the W warm-up and K timed steps, `--dump-outputs`, the line.
`--full` adds everything else, measured after the timed steps: the edge-kernel `roofline`, `aggregate_roofline` and the
host-stage probe; at N = 1 `cpu_baseline` and (fp32) `f32x6_candidate`, and with the default workload, each timed in the
same run, `config2_ragged256` (BASELINE configs[2] shape), `config0_plumbing` (configs[0]: ceyyag context, 4 samples,
T = 20, with the CPU oracle run IN FULL beside it) and `config4_share_bf16_inpaint` (one GPU's share of configs[4]: 256
ragged, bf16 operands, fixed fragment, rs = 1, T = 250); for N > 1 `config3_ragged256_per_gpu` (configs[3]: 256 ragged
molecules per rank).  The `--no-*` and `--cpu-*` options narrow what `--full` adds.

`--gpus N` with N > 1 and no launcher environment (WORLD_SIZE unset): this process never touches a GPU (devices are
counted from the KFD topology in sysfs, no HIP call); it starts N child ranks of itself (RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* set), polls them, ends all of them as soon as one fails, relays rank 0's JSON line and exits
with the worst child status.  Fewer than N devices -> non-zero exit, no JSON line.

Prints ONE JSON line on rank 0.  Weights are seeded synthetic tensors in the reference checkpoint
layout (the trained checkpoints are not available offline) - timing does not depend on weight values.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

H = 420
PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 matrix peak
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n-samples", type=int, default=64, help="molecules per GPU")
    ap.add_argument("--n-atoms", type=int, default=27)
    ap.add_argument("--variance", type=int, default=0, help=">0: ragged batch n_atoms +- variance (config 3: 27 +- 12)")
    ap.add_argument("--diffusion-steps", type=int, default=100)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything beyond the headline: rooflines, host-stage probe, "
                         "f32x6 probe, the configs[0] / [2] / [4] objects and the CPU baseline (N = 1), configs[3] (N > 1); "
                         "the --no-* and --cpu-* options narrow it")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-phi-calls", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="threads of the CPU baseline; 0 (default) = the best of a bounded sweep over 8 / 16 / 32 / 64 on one B/8 call")
    ap.add_argument("--cpu-all-cores", action="store_true",
                    help="also time one denoiser call at B/8 with torch.set_num_threads(os.cpu_count()) (BASELINE.md section 3's "
                         "rule; ~80 s on the 256-core GPU box, where it is 229x slower than 16 threads)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f32x6"],
                    help="bf16 = opt-in reduced-precision MFMA operands (configs[4]); the default bench line is fp32")
    ap.add_argument("--no-config2", action="store_true",
                    help="skip the second object of the default line (BASELINE configs[2] shape: 256 ragged molecules)")
    ap.add_argument("--no-config0", action="store_true", help="skip the configs[0] object (ceyyag context, 4 samples, T = 20, HIP + CPU oracle in full)")
    ap.add_argument("--no-config4", action="store_true", help="skip the configs[4]-share object (256 ragged, bf16, fixed fragment, rs = 1, T = 250)")
    ap.add_argument("--no-config3", action="store_true", help="N > 1: skip the configs[3] object (256 ragged molecules per GPU)")
    ap.add_argument("--no-x6-probe", action="store_true",
                    help="skip the extra (untimed-for-`value`) pass in the opt-in f32x6 mode that is reported beside the fp32 line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0: its batch and the molecules "
                         "returned) as float32 DIR/<name>.npy, at most 64 MB")
    ap.add_argument("--fragment", action="store_true",
                    help="configs[4] sampler: inpainting around a fixed 8-atom fragment (6 C + 2 Cl), resample_steps=1, "
                         "inertial_fragment_matching=False -> 2 denoiser calls per step + 1")
    return ap.parse_args()


def edge_flops_per_launch(n_edges):
    """Algorithmic FLOPs of one fused edge-MLP launch: per real edge the
    420x420 second layer, the factorised first-layer finish (2 adds + 2 FMA per channel) and the
    gate / coordinate-head dot product."""
    return 2.0 * n_edges * (H * H + 3 * H)


def time_edge_kernel(gen, plan, dev, iters=20):
    """Duration of the dominant kernel (k_edge, GCL variant) measured live with events on the stream it is launched on:
    three batches of `iters` back-to-back launches -> (mean over the batches, best batch)."""
    from ml_conformer_generator_amd import _lib
    L = _lib.lib()
    dyn = gen.generative_model.dynamics
    stream = _lib.current_stream_ptr(dev)
    _lib.check(L.mcg_bench_edge(dyn.handle, plan.handle, 4, 0, 3, stream), "bench_edge")
    secs = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        _lib.check(L.mcg_bench_edge(dyn.handle, plan.handle, 4, 0, iters, stream), "bench_edge")
        e1.record()
        torch.cuda.synchronize(dev)
        secs.append(e0.elapsed_time(e1) / iters * 1e-3)
    return sum(secs) / len(secs), min(secs)


def time_aggregate_kernel(plan, dev, iters=20):
    """Stand-alone aggregate (HBM-bound probe): algorithmic bytes = 4*(421*E_r + 420*M_r)."""
    from ml_conformer_generator_amd import _lib
    L = _lib.lib()
    n_nodes = plan.n_nodes_host.tolist()
    first, cnt, off = [], [], 0
    for n in n_nodes:
        for i in range(n):
            first.append(off + i * (n - 1))
            cnt.append(n - 1)
        off += n * (n - 1)
    E, M = off, len(first)
    first_d = torch.tensor(first, dtype=torch.int32, device=dev)
    cnt_d = torch.tensor(cnt, dtype=torch.int32, device=dev)
    # rotate over enough distinct m buffers to exceed the 256 MiB Infinity Cache
    nbuf = max(2, int(600e6 // (E * H * 4)) + 1)
    ms = [torch.randn(E, H, device=dev) for _ in range(nbuf)]
    gate = torch.rand(E, device=dev)
    out = torch.empty(M, H, device=dev)
    stream = _lib.current_stream_ptr(dev)

    def run(k):
        m = ms[k % nbuf]
        _lib.check(L.mcg_egnn_aggregate(m.data_ptr(), gate.data_ptr(), first_d.data_ptr(), cnt_d.data_ptr(),
                                        out.data_ptr(), M, H, stream), "aggregate")
    for k in range(nbuf):
        run(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for k in range(iters):
        run(k)
    e1.record()
    torch.cuda.synchronize(dev)
    sec = e0.elapsed_time(e1) / iters * 1e-3
    byts = 4.0 * (421 * E + 420 * M)
    return sec, byts


def _cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(args, sd, gsd):
    """CPU oracle (a port of the reference's op sequence, parity-pinned to it) timed on this box's
    host cores on a bounded sample: `cpu_phi_calls` denoiser calls + 1 GCN pass at the bench
    workload, extrapolated to 101 calls (every call has identical cost).

    Threads: BASELINE.md section 3 says `torch.set_num_threads(os.cpu_count())`.  On the GPU box's 256-core host
    that rule makes the aten kernels ~20x SLOWER than 16 threads (8: 0.68 s, 16: 0.40 s, 32: 0.70 s, 128: 2.7 s per
    call at B=16; one call at B=8: 0.36 s with 16 threads, 81.9 s with 256 - profiles/round2_bench_c2.json): the
    headline baseline therefore uses the thread count that is best for the CPU on THIS host: the winner of a bounded sweep
    (8 / 16 / 32 / 64 threads, one warm + one timed denoiser call at B/8 each, stopped past the knee; `thread_sweep_...` in
    the line) unless --cpu-threads fixes it;
    --cpu-all-cores measures the os.cpu_count() rule beside it on a B/8 slice (`all_cores`), so both numbers are on
    record."""
    from ml_conformer_generator_amd.synthetic import synth_gcn_inputs
    from oracle import egnn_oracle as EO
    from oracle import gcn_oracle as GO
    from oracle import host_oracle as HO
    n_all = os.cpu_count() or 1
    B, n = args.n_samples, args.n_atoms
    g = torch.Generator().manual_seed(3)
    sizes = torch.full((B,), n)
    nm, em = HO.masks_from_sizes(sizes, n)
    z = torch.randn(B, n, 11, generator=g) * nm
    ctx = torch.tensor([-0.99, -1.66, -1.66]).view(1, 1, 3).repeat(B, n, 1) * nm
    t = torch.full((B, 1), 0.5)
    # thread count: the best of a bounded sweep (one denoiser call at B/8 per candidate, a few seconds in all) unless
    # --cpu-threads fixes it - the baseline is quoted at the count that is best for the CPU on THIS host
    sweep = None
    if args.cpu_threads > 0:
        cores = min(n_all, args.cpu_threads)
    else:
        Bs = max(1, B // 8)
        nms, ems = HO.masks_from_sizes(sizes[:Bs], n)
        sweep = {}
        with torch.no_grad():
            for cand in sorted({c for c in (8, 16, 32, 64) if c <= n_all} | ({n_all} if n_all < 8 else set())):
                torch.set_num_threads(cand)
                EO.egnn_dynamics(sd, t[:Bs], z[:Bs], nms, ems, ctx[:Bs])          # warm this pool size
                t0 = time.time()
                EO.egnn_dynamics(sd, t[:Bs], z[:Bs], nms, ems, ctx[:Bs])
                sweep[cand] = time.time() - t0
                if sweep[cand] > 3.0 * min(sweep.values()):
                    break                                                         # past the knee: more threads only get slower
        cores = min(sweep, key=sweep.get)
    torch.set_num_threads(cores)
    with torch.no_grad():
        t0 = time.time()
        for _ in range(args.cpu_phi_calls):
            EO.egnn_dynamics(sd, t, z, nm, em, ctx)
        phi_s = (time.time() - t0) / args.cpu_phi_calls
        el, dm, am = synth_gcn_inputs(B, [n] * B, seed=1)
        t0 = time.time()
        GO.adj_mat_seer(gsd, el, dm, am)
        gcn_s = time.time() - t0
        # the os.cpu_count() rule, on 1/8 of the batch (bounded: the full batch would take minutes per call)
        all_cores = {"skipped": "opt-in (--cpu-all-cores): one denoiser call at B/8 with torch.set_num_threads(os.cpu_count()) "
                                "takes ~80 s on the 256-core GPU box, too long for the default run",
                     "last_measured": "profiles/round2_bench_c2_all_cores.json: 81.9 s with 256 threads vs 0.357 s with 16 "
                                      "(229x slower) - the headline baseline uses the thread count that is best for the CPU"}
        if n_all == cores:
            all_cores = {"threads": n_all, "note": "the headline baseline already uses every core of this host"}
        if n_all != cores and args.cpu_all_cores:
            Bs = max(1, B // 8)
            nms, ems = HO.masks_from_sizes(sizes[:Bs], n)
            t0 = time.time()
            EO.egnn_dynamics(sd, t[:Bs], z[:Bs], nms, ems, ctx[:Bs])
            small_best = time.time() - t0
            torch.set_num_threads(n_all)
            t0 = time.time()
            EO.egnn_dynamics(sd, t[:Bs], z[:Bs], nms, ems, ctx[:Bs])
            small_all = time.time() - t0
            torch.set_num_threads(cores)
            all_cores = {"threads": n_all, "sample": f"1 denoiser call at B={Bs}", "phi_call_s": small_all,
                         f"phi_call_s_at_{cores}_threads": small_best, "slowdown_vs_headline_threads": small_all / small_best}
    calls = args.diffusion_steps + 1
    total = phi_s * calls + gcn_s
    return {"value": B / total, "unit": "molecules/s", "cores": cores, "kind": "port", "cpu_model": _cpu_model(),
            "host_cores": n_all,
            "thread_sweep_s_per_call_at_B_over_8": sweep,
            "sample": f"{args.cpu_phi_calls} of {calls} denoiser calls ({phi_s:.2f} s each) + 1 GCN pass "
                      f"({gcn_s:.2f} s) at B={B}, n={n}; extrapolated x{calls}", "phi_call_s": phi_s,
            "all_cores": all_cores}


def make_generator(args, dev, dtype, sd, gsd):
    from ml_conformer_generator_amd import MLConformerGenerator
    gen = MLConformerGenerator(diffusion_steps=args.diffusion_steps, device=dev, edm_weights=sd,
                               adj_mat_seer_weights=gsd, compute_dtype=dtype)
    gen._timing = {"sampler_start": torch.cuda.Event(enable_timing=True), "sampler_end": torch.cuda.Event(enable_timing=True)}
    return gen


def timed_passes(gen, ctx, n_total, n_atoms, variance, frag_kw, steps, warmup, fence, seed=7, ref_conformer=None,
                 vary_sizes=False, last_out=None):
    """`steps` timed calls of the public sharded path after `warmup` untimed ones.
    `vary_sizes`: every pass (warm-up included) draws its molecule sizes from seed + pass index, the way a caller of a
    ragged workload runs it (the reference's protocol generates for 1 000 different references,
    research_scripts/evaluation.py:47-54,98-103): every timed pass then meets a size vector it has never seen and pays
    the plan for it - host tables, uploads, workspace, HIP-graph capture - inside the timed region.  Otherwise every pass
    re-draws the SAME sizes (fixed-size workloads: the draw is constant anyway).
    Returns (elapsed seconds on this rank, mean sampler ms per pass, whether EVERY coordinate this rank generated in the
    timed passes is finite - checked after the clock stops, last valid fraction).  `last_out` (a dict): receives the
    molecules the last timed pass returned ("molecules") and the tensors of its whole batch ("batch")."""
    from ml_conformer_generator_amd.conformer_generator import HAVE_RDKIT     # (MMFF94 runs only where RDKit exists)
    sampler_ms = []
    kept = []
    pass_index = [0]
    mols = None

    def one_pass():
        # sizes: CPU generator only (torch.manual_seed would also reseed every device generator and give all ranks
        # the same noise); noise: per-rank device generator, seed + rank, set inside the sharded path
        torch.default_generator.manual_seed(seed + (pass_index[0] if vary_sizes else 0))
        pass_index[0] += 1
        if ref_conformer is not None:
            mols = gen.generate_conformers_sharded(reference_conformer=ref_conformer, variance=variance, n_samples=n_total,
                                                   seed=seed, optimise_geometry=HAVE_RDKIT, gather="rank0", **frag_kw)
        else:
            mols = gen.generate_conformers_sharded(reference_context=ctx, n_atoms=n_atoms, variance=variance,
                                                   n_samples=n_total, seed=seed, optimise_geometry=HAVE_RDKIT,
                                                   gather="rank0", **frag_kw)
        torch.cuda.synchronize(gen.device)
        sampler_ms.append(gen._timing["sampler_start"].elapsed_time(gen._timing["sampler_end"]))
        if gen.last_batch is not None:
            kept.append(gen.last_batch["x"])
        return mols

    for _ in range(warmup):
        one_pass()
    sampler_ms.clear()
    kept.clear()
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        mols = one_pass()
    fence()
    elapsed = time.perf_counter() - t0
    if last_out is not None and mols is not None:
        last_out.update(molecules=mols, batch=gen.last_batch)
    finite = all(bool(torch.isfinite(x).all()) for x in kept)
    return elapsed, sum(sampler_ms) / max(1, len(sampler_ms)), finite, gen.last_valid_fraction


def cold_call_cost(gen, dev, n_samples=256, n_atoms=27, variance=12, seed=9001):
    """What the FIRST denoiser call over a never-seen size vector costs beyond a warm one: `plan_ms` = `EGNNDynamics.plan`
    (host tables, uploads, workspace - `mcg_plan_create_ex`), `first_call_ms` = the first `mcg_egnn_dynamics` on it (HIP
    graph capture + instantiate + launch), `warm_call_ms` = the second (graph replay); cold_call_ms = plan + first - warm.
    Mean over three fresh size vectors; everything synchronised."""
    dyn = gen.generative_model.dynamics
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(3):
        lo, hi = max(n_atoms - variance, gen.min_n_nodes), min(n_atoms + variance, gen.max_n_nodes)
        sizes = torch.randint(lo, hi + 1, (n_samples,), generator=g)
        N = hi
        nm = (torch.arange(N).unsqueeze(0) < sizes.unsqueeze(1)).float().unsqueeze(2).to(dev)
        xh = torch.randn(n_samples, N, 11, device=dev) * nm
        cx = torch.tensor([-0.99, -1.66, -1.66], device=dev).view(1, 1, 3).repeat(n_samples, N, 1) * nm
        t = torch.full((n_samples,), 0.5, device=dev)
        out = torch.empty_like(xh)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        plan = dyn.plan(sizes, N)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        dyn.run(plan, t, xh, cx, out)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        dyn.run(plan, t, xh, cx, out)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        rows.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    plan_ms, first_ms, warm_ms = (sum(r[k] for r in rows) / len(rows) for k in range(3))
    return {"cold_call_ms": plan_ms + first_ms - warm_ms, "plan_ms": plan_ms, "first_call_ms": first_ms,
            "warm_call_ms": warm_ms, "plans_cached": len(dyn._plans),
            "what": "first denoiser call over a never-seen size vector minus a warm one: plan (host tables, uploads, "
                    "workspace) + HIP-graph capture; mean of 3 fresh vectors"}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(last, out_dir):
    """What the last timed step computed, as float32 arrays DIR/<name>.npy (64 MB in all at most):
      batch_<key>    every tensor of the whole generated batch (`gen.last_batch`, this rank's: sampled coordinates `x`,
                     features `h`, `n_nodes`, GCN element types / bond orders, coordinates in GCN order `x_ordered`) -
                     with synthetic weights the validity gate may drop every molecule, this is what was computed;
      returned_<f>   the molecule records the call returned (those that passed the validity gate), padded:
                     coords [K, n, 3], atomic_numbers [K, n], bond_orders [K, n, n] (padding 0), n_atoms [K], and
                     batch_row [K] (the record's row in the batch, -1 if it does not name one) - only when K > 0: with
                     synthetic weights the gate may return nothing, and then no returned_* file is written.
    Past the limit, both are a fixed seeded sample of their molecules in order, named by `*_molecule_index`."""
    import numpy as np
    mols, batch = last.get("molecules") or [], last.get("batch") or {}
    batch = {k: v.detach().float().cpu().numpy() for k, v in batch.items() if torch.is_tensor(v)}
    B = min((a.shape[0] for a in batch.values()), default=0)
    n_max = max((m.GetNumAtoms() for m in mols), default=0)
    batch_bytes = sum(a.nbytes for a in batch.values())
    rec_per_mol = 4 * (3 * n_max + n_max + n_max * n_max + 2)
    frac = min(1.0, DUMP_LIMIT_BYTES / max(1, batch_bytes + B * 4 + len(mols) * rec_per_mol))

    def sample(n, seed):
        idx = np.arange(n)
        if frac < 1.0:
            idx = np.sort(np.random.default_rng(seed).choice(n, max(1, int(n * frac)), replace=False))
        return idx
    arrs = {}
    bi = sample(B, 0)
    for k, a in batch.items():
        arrs["batch_" + k] = np.ascontiguousarray(a[bi] if a.shape[0] == B else a)
    arrs["batch_molecule_index"] = bi.astype(np.float32)
    ri = sample(len(mols), 1) if mols else np.zeros(0, np.int64)
    k = len(ri)
    rec = {"coords": np.zeros((k, n_max, 3), np.float32), "atomic_numbers": np.zeros((k, n_max), np.float32),
           "bond_orders": np.zeros((k, n_max, n_max), np.float32), "n_atoms": np.zeros(k, np.float32),
           "molecule_index": ri.astype(np.float32), "batch_row": np.full(k, -1.0, np.float32)}
    for j, b in enumerate(ri):
        m = mols[b]
        n = m.GetNumAtoms()
        row = getattr(m, "_b", None)               # a record's row in the host batch it views (generation order)
        if row is not None and row >= 0:
            rec["batch_row"][j] = row
        rec["coords"][j, :n] = m.coords.numpy()
        rec["atomic_numbers"][j, :n] = m.atomic_numbers
        rec["bond_orders"][j, :n, :n] = m.bond_orders.numpy()
        rec["n_atoms"][j] = n
    if k and n_max:
        arrs.update({"returned_" + name: a for name, a in rec.items()})
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrs.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32, copy=False))


def synthetic_fragment():
    """configs[4] fixed fragment: 8 heavy atoms, a 1.45 A zig-zag chain, 6 C + 2 Cl."""
    fx = torch.tensor([[1.25 * i, 0.72 * (i % 2), 0.3 * ((i // 2) % 2)] for i in range(8)], dtype=torch.float32)
    return dict(fixed_fragment=(fx - fx.mean(0), [6, 6, 6, 6, 6, 6, 17, 17]), inertial_fragment_matching=False,
                resample_steps=1, blend_power=3)


def config0_plumbing(args, gen, sd, gsd, dev, fence):
    """BASELINE configs[0]: generate_conformers on the ceyyag reference conformer (17 heavy atoms; coordinates from
    tests/golden/context_shape.npz - the reference's asset itself does not travel), n_samples = 4, variance = 2,
    diffusion_steps = 20.  HIP path: 1 warm-up + 3 timed passes of the public call.  CPU: the oracle pipeline (port of the
    reference's op sequence) run IN FULL - 21 denoiser calls, hand-off tensors, GCN, bond argmax - as BASELINE.md
    section 3 says; no extrapolation."""
    import numpy as np
    xyz = torch.from_numpy(np.load(os.path.join(REPO, "tests", "golden", "context_shape.npz"))["ceyyag_xyz"]).float()
    T0 = 20
    gen.set_diffusion_steps(T0)
    try:
        el, ms, fin, vf = timed_passes(gen, None, 4, None, 2, {}, 3, 1, fence, ref_conformer=xyz)
    finally:
        gen.set_diffusion_steps(args.diffusion_steps)
    out = {"workload": "configs[0]: generate_conformers(ceyyag heavy atoms, n_samples=4, variance=2), diffusion_steps=20, fp32",
           "value": 4 * 3 / el, "unit": "molecules/s", "steps": 3, "warmup": 1, "ms_per_step": el / 3 * 1e3,
           "ms_per_denoiser_call": ms / (T0 + 1), "outputs_finite": fin, "valid_proxy_fraction": vf}
    if not args.no_cpu_baseline:
        from ml_conformer_generator_amd.config import CONTEXT_NORMS
        from oracle import diffusion_oracle as DO
        from oracle import gcn_oracle as GO
        from oracle import host_oracle as HO
        cores = min(os.cpu_count() or 1, args.cpu_threads if args.cpu_threads > 0 else 16)
        torch.set_num_threads(cores)
        norms = {k: torch.tensor(v) for k, v in CONTEXT_NORMS.items()}
        t0 = time.time()
        with torch.no_grad():
            torch.manual_seed(7)
            c, _ = HO.context_shape(xyz - xyz.mean(0))
            nm, em, cx = HO.edm_input(4, c, norms, 15, 19)
            orc = DO.SamplerOracle(sd, T0)
            x, h = orc.forward(nm, em, cx, 0)
            n_nodes = nm.sum(1).reshape(-1).to(torch.long)
            e_, d_, a_ = HO.adj_mat_seer_input(x, h, n_nodes)
            bond = GO.adj_mat_seer(gsd, e_, d_, a_).argmax(-1)
            HO.bond_writeback(bond, e_, n_nodes)
        cpu_s = time.time() - t0
        out["cpu_oracle_full_run"] = {"value": 4 / cpu_s, "unit": "molecules/s", "seconds": cpu_s, "cores": cores,
                                      "kind": "port", "sample": "the whole configs[0] job: 21 denoiser calls + hand-off + GCN + "
                                                                "bond write-back, no extrapolation"}
        out["gpu_over_cpu"] = out["value"] / out["cpu_oracle_full_run"]["value"]
    return out


def config4_share(args, gsd, ctx, dev, fence):
    """One GPU's share of BASELINE configs[4]: 256 ragged molecules (15..39 atoms), bf16 MFMA operands, fixed 8-atom
    fragment inpainting, resample_steps = 1, diffusion_steps = 250 (501 denoiser calls).  1 warm-up pass at T = 10 (plan,
    graph capture) + 1 timed pass, with the bf16 edge kernel's own roofline."""
    import argparse as _ap
    from ml_conformer_generator_amd import weights as W
    a4 = _ap.Namespace(**vars(args))
    a4.diffusion_steps, a4.dtype = 250, "bf16"
    sd4 = W.synth_edm_state_dict(1234, weight_gain=0.3)       # contractive: resampling repeats the 1/alpha_ts amplification
    g4 = make_generator(a4, dev, "bf16", sd4, gsd)
    frag = synthetic_fragment()
    g4.set_diffusion_steps(10)
    timed_passes(g4, ctx, 256, 27, 12, frag, 1, 0, fence, seed=7)
    g4.set_diffusion_steps(250)
    # TWO timed passes, reported one by one (round-5 review: one pass could not tell box-to-box spread from pass-to-pass noise);
    # each draws sizes nobody has seen before it (its own seed): both pay their plan + graph capture inside the timed region
    passes = [timed_passes(g4, ctx, 256, 27, 12, frag, 1, 0, fence, seed=8 + k) for k in range(2)]
    el = sum(p[0] for p in passes)
    ms = sum(p[1] for p in passes) / len(passes)
    fin = all(p[2] for p in passes)
    vf = passes[-1][3]
    _, roof = edge_roofline(a4, g4, dev, "bf16")
    # "fraction of the bf16 MFMA peak" is the wrong yardstick for this kernel: beside it, from committed rocprofv3 --pmc passes of
    # this kernel at this shape (they cannot be taken inside this run): HBM-side traffic per launch, the kernel's ISSUE-BOUND
    # time (matrix pipe + VALU issue that do not overlap, at the per-instruction issue costs the SQ_ACTIVE_INST counters give)
    # and where its wave-cycles go (`stall_breakdown`)
    try:
        e = json.load(open(os.path.join(REPO, "profiles", "pmc_traffic.json")))["configs[4] share, bf16 edge kernel: n_samples=256, n=27+-12"]
        cyc = e["issue_cycles_per_instruction"]
        plain = e["sq_insts_valu"] - e["sq_insts_mfma"] - e["sq_insts_valu_trans_f32"]
        cycles = e["sq_valu_mfma_busy_cycles"] + cyc["valu"] * plain + cyc["valu_trans_f32"] * e["sq_insts_valu_trans_f32"]
        bound_us = cycles / (1024 * 2.4e9) * 1e6
        roof["traffic"] = e["traffic_bytes_corrected"]
        roof["traffic_source"] = ("profiles/pmc_traffic.json (static: separate FETCH_SIZE / WRITE_SIZE passes, " + e["round"] + "; FETCH_SIZE x2 gfx950 "
                                  "correction; algorithmic " + e["algorithmic_bytes"] + ")")
        roof["issue_bound"] = {"issue_bound_us": bound_us, "measured_us": roof["avg_launch_us"],
                               "frac": bound_us / roof["avg_launch_us"], "mfma_issue_us": e["sq_valu_mfma_busy_cycles"] / (1024 * 2.4e9) * 1e6,
                               "valu_issue_us": (cycles - e["sq_valu_mfma_busy_cycles"]) / (1024 * 2.4e9) * 1e6,
                               "counters": {k: e[k] for k in ("sq_insts_valu", "sq_insts_mfma", "sq_insts_valu_trans_f32", "sq_valu_mfma_busy_cycles")},
                               "cycles_per_instruction": cyc,
                               "source": "profiles/pmc_traffic.json (static: separate rocprofv3 --pmc passes of this kernel at this shape, "
                                         + e["round"] + "); matrix and vector issue of a SIMD do not overlap in this kernel, so they add"}
        roof["stall_breakdown"] = e["stall_breakdown"]
    except Exception:  # noqa: BLE001
        pass
    return {"workload": "configs[4] per-GPU share: n_samples=256, 27+-12 heavy atoms (ragged), fixed 8-atom fragment "
                        "(inpainting, resample_steps=1), diffusion_steps=250, bf16-operand MFMA HIP EGNN (fp32 "
                        "accumulate/state) + fp32 GCN",
            "value": 256 * len(passes) / el, "unit": "molecules/s", "steps": len(passes), "warmup": "1 pass at T=10",
            "ms_per_step": el / len(passes) * 1e3,
            "passes": [{"molecules_per_s": 256 / p[0], "ms": p[0] * 1e3, "egnn_step_ms_per_batch": p[1] / 501} for p in passes],
            "dtype": "bf16", "egnn_step_ms_per_batch": ms / 501, "denoiser_calls": 501, "outputs_finite": fin,
            "valid_proxy_fraction": vf, "roofline": roof,
            "weights": "synthetic, reference checkpoint layout, seed 1234, nn.Linear-family init x 0.3"}


def x6_probe(args, gen, sd, gsd, ctx, dev):
    """The same workload in the opt-in "f32x6" mode (edge-MLP contraction as six bf16 partial products of three-part
    fp32 operands, fp32 accumulate - DESIGN.md): one warm-up + one timed pass, plus the deviation of ONE denoiser
    call from the exact-fp32 kernel on identical inputs.  Reported beside the fp32 line; never part of `value`."""
    B = args.n_samples
    g6 = make_generator(args, dev, "f32x6", sd, gsd)
    torch.manual_seed(11)
    n = torch.randint(args.n_atoms - args.variance, args.n_atoms + args.variance + 1, (B,))
    N = int(n.max())
    nm = (torch.arange(N).unsqueeze(0) < n.unsqueeze(1)).float().unsqueeze(2).to(dev)
    z = torch.randn(B, N, 11, device=dev) * nm
    c = torch.randn(B, 1, 3, device=dev).repeat(1, N, 1) * nm
    t = torch.full((B, 1), 0.5, device=dev)
    o32 = gen.generative_model.dynamics(t, z, nm, None, c)
    o6 = g6.generative_model.dynamics(t, z, nm, None, c)
    dev_rel = float((o6 - o32).abs().max() / o32.abs().max())
    el, ms, fin6, _ = timed_passes(g6, ctx, B, args.n_atoms, args.variance, {}, 1, 1, lambda: torch.cuda.synchronize(dev))
    return {"value": B / el, "unit": "molecules/s", "egnn_step_ms_per_batch": ms / (args.diffusion_steps + 1),
            "outputs_finite": fin6,
            "max_rel_deviation_of_one_denoiser_call_from_exact_fp32": dev_rel,
            "note": "opt-in mode, NOT the judged number: multiplies in bf16 (6 partial products of 3-part fp32 operands), "
                    "accumulates in fp32; passes the same fp32 parity tolerance as the exact kernel (DESIGN.md)"}


def time_edge_kernel_in_call(gen, plan, dev, calls=8):
    """Mean duration of the GCL edge kernel INSIDE whole denoiser calls: the kernel's own begin / end timestamps
    (hipExtLaunchKernelGGL events on the launching stream, `mcg_bench_edge_incall`), 18 launches per call behind and in
    front of the node GEMMs - the context the sampler runs it in, and the figure a rocprofv3 kernel trace of the timed
    region reports.  (Back-to-back launches of this one kernel for milliseconds draw more power than the sampler's mix and
    run 1-10 % slower on some boxes: reported beside it as `standalone_*`.)"""
    import numpy as np
    from ml_conformer_generator_amd import _lib
    L = _lib.lib()
    dyn = gen.generative_model.dynamics
    B, N = plan.B, plan.N
    nm = plan.node_mask()
    g = torch.Generator(device=dev).manual_seed(5)
    xh = torch.randn(B, N, 11, device=dev, generator=g) * nm
    ctx = torch.tensor([-0.99, -1.66, -1.66], device=dev).view(1, 1, 3).repeat(B, N, 1) * nm
    t = torch.full((B,), 0.5, device=dev)
    out = torch.empty_like(xh)
    us = np.zeros(4, dtype=np.float32)
    stream = _lib.current_stream_ptr(dev)
    for n_calls in (2, calls):            # two warm calls (clocks, caches), then the measured ones
        _lib.check(L.mcg_bench_edge_incall(dyn.handle, plan.handle, _lib.dptr(t), _lib.dptr(xh), _lib.dptr(ctx), _lib.dptr(out),
                                           n_calls, us.ctypes.data, stream), "mcg_bench_edge_incall")
    return float(us[0]) * 1e-6, float(us[1]) * 1e-6, int(us[2]), plan.n_ranges


def last_plan(gen):
    """The denoiser plan the generator used last (its plan cache is ordered by recency)."""
    return next(reversed(gen.generative_model.dynamics._plans.values()))


def edge_roofline(args, gen, dev, dtype, traffic=None, traffic_source=None):
    plan = last_plan(gen)
    sa_mean, sa_best = time_edge_kernel(gen, plan, dev)
    edge_s, equiv_s, n_timed, n_ranges = time_edge_kernel_in_call(gen, plan, dev)
    timing = ("mean of the GCL edge launches of 8 whole denoiser calls issued as plain launches, each launch's own begin / end "
              "timestamps (hipExtLaunchKernelGGL events on the launching stream)")
    in_run = None
    if n_ranges != 1:
        # the plan cuts the batch into molecule ranges whose edge kernels OVERLAP on separate streams: a per-launch time of
        # one range is not the time of the batch's edge layer.  The roofline figure is then the kernel over the WHOLE batch
        # launched alone (mcg_bench_edge on the parent plan's own tables); the in-run per-range figure is reported beside it
        # (round-5 review), as a LOWER bound: ranges that share the chip each look longer than they would alone.
        fl_all = edge_flops_per_launch(plan.n_real_edges) * (6.0 if dtype == "f32x6" else 1.0)
        pk = PEAK_F32_MFMA_TFLOPS if dtype == "f32" else 2500.0
        in_run = {"per_range_avg_launch_us": edge_s * 1e6, "per_range_coordinate_variant_avg_launch_us": equiv_s * 1e6 if equiv_s else None,
                  "molecule_ranges": n_ranges, "launches_timed": n_timed,
                  "frac_lower_bound": fl_all / (n_ranges * edge_s) / 1e12 / pk,
                  "what": "GCL edge launches of the ranges INSIDE 8 whole denoiser calls (each range's own begin / end timestamps); the "
                          "ranges overlap on separate streams, so n_ranges x this time over-counts the layer's edge time"}
        edge_s, equiv_s = sa_mean, None
        timing = (f"the plan runs {n_ranges} molecule ranges on separate streams (overlapping edge kernels); timed instead: the "
                  "kernel over the whole batch alone, HIP events around 3 batches of 20 back-to-back launches, mean")
    fl = edge_flops_per_launch(plan.n_real_edges)
    if dtype == "f32x6":
        fl *= 6.0          # executed bf16 FLOPs: six partial products per fp32 product (K padded 420 -> 448 not counted)
    achieved = fl / edge_s / 1e12
    peak_tf = PEAK_F32_MFMA_TFLOPS if dtype == "f32" else 2500.0      # dense bf16 MFMA peak
    return plan, {"kernel": "k_edge (fused edge MLP: layer-1 finish + 420x420 MFMA + gate + per-node sum)",
                  "bound": "mfma", "achieved": achieved, "peak": peak_tf, "unit": "TFLOP/s",
                  "frac": achieved / peak_tf, "traffic": traffic, "traffic_source": traffic_source,
                  "avg_launch_us": edge_s * 1e6, "launches_timed": n_timed,
                  "launch_timing": timing, "molecule_ranges": n_ranges, "in_run": in_run,
                  "coordinate_variant_avg_launch_us": equiv_s * 1e6 if equiv_s else None,
                  "standalone_avg_launch_us": sa_mean * 1e6, "standalone_best_launch_us": sa_best * 1e6,
                  "standalone_timing": "HIP events around 3 batches of 20 back-to-back launches of this kernel alone: mean / best batch",
                  "flops_per_launch": fl}


def host_stage_report(gen, probe=True):
    """The two RDKit-owned host stages around the GCN (canonical order + connectivity before it, `redefine_bonds` +
    `standardize_mol` / MMFF behind it; `host_pool.py`).  Where RDKit imports they run inside the timed region, fanned out
    over `n_host_workers` worker processes, and their wall times are reported; RDKit exists on none of this project's
    boxes, so there (with `probe`) the object carries a labelled PROBE instead: the same pipeline (`rdkit_order.OrderStage`
    -> per-group 'launch' -> `rdkit_finish.FinishStage`) over 256 molecules with a fake 2 ms-per-molecule function in each
    stage (tests/fake_host_tasks.py), pooled against serial, warm."""
    from ml_conformer_generator_amd import host_pool as HP
    from ml_conformer_generator_amd import rdkit_finish as RF
    from ml_conformer_generator_amd import rdkit_order as RO
    from ml_conformer_generator_amd.conformer_generator import HAVE_RDKIT
    from ml_conformer_generator_amd.handoff import molecules_from_tensors
    out = {"rdkit": HAVE_RDKIT, "n_host_workers": gen.n_host_workers,
           "host_order_ms": gen.last_host_order_ms, "host_finish_ms": gen.last_host_finish_ms}
    fake = os.path.join(REPO, "tests", "fake_host_tasks.py")
    if not probe or HAVE_RDKIT or not os.path.exists(fake):
        return out
    try:
        B, N = 256, 27
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B, N, 3, generator=g) * 1.7
        h = torch.nn.functional.one_hot(torch.randint(0, 7, (B, N), generator=g), 8).float()
        n = torch.full((B,), N)
        recs = molecules_from_tensors(x, torch.full((B, 42), 6, dtype=torch.int8),
                                      torch.randint(0, 3, (B, 42, 42), generator=g).to(torch.int8), n.to(torch.int32),
                                      torch.ones(B, dtype=torch.uint8))
        groups = RO.launch_groups(B)

        def run(ex):
            t0 = time.perf_counter()
            st = RO.OrderStage(HP.TaskRef(fake, "order_chunk"), x, h, n, ex, groups)
            fin = RF.FinishStage(HP.TaskRef(fake, "finish_chunk"), True, ex)
            for gi, (lo, hi) in enumerate(groups):
                st.result(gi)
                fin.add(recs[lo:hi])
            fin.results()
            return (time.perf_counter() - t0) * 1e3
        # a pool of its own (the generator's shared one may be warm already): started the way `_generate_shard` starts it -
        # `prestart` with the task file BEFORE the sampler - then a stand-in for the sampler (0.45 s at configs[1]) and the first use
        pool = HP.HostPool(gen.n_host_workers, task_timeout_s=gen.task_timeout_s)
        t0 = time.perf_counter()
        pool.prestart([HP.TaskRef(fake, "order_chunk")])
        prestart_call_ms = (time.perf_counter() - t0) * 1e3
        time.sleep(0.45)
        warm = min(run(pool) for _ in range(1))
        first = warm                                   # the first use IS a warm run: start-up and imports hid under the "sampler"
        pooled = min(run(pool) for _ in range(3))
        start_ms = pool.last_start_ms
        pool.close()
        cold_pool = HP.HostPool(gen.n_host_workers, task_timeout_s=gen.task_timeout_s)
        t0 = time.perf_counter()
        run(cold_pool)                                 # round 5's behaviour: workers start at the first submit
        cold = (time.perf_counter() - t0) * 1e3
        cold_pool.close()
        serial = run(HP.SerialExecutor())
        out["probe_fake_2ms_per_molecule"] = {
            "what": "NOT RDKit (absent here): 256 molecules through the order -> launch -> finish pipeline with a fake 2 ms-per-"
                    "molecule function in each stage, worker processes vs the reference's one-molecule-at-a-time loop",
            "serial_ms": serial, "pooled_ms": pooled, "speedup": serial / pooled, "workers": gen.n_host_workers,
            "first_use_ms_incl_worker_start": cold,
            "first_use_ms_after_prestart": first, "first_use_critical_path_ms": max(0.0, first - pooled) + prestart_call_ms,
            "prestart_call_ms": prestart_call_ms, "worker_start_ms_in_background": start_ms,
            "task_timeout_s": gen.task_timeout_s}
    except Exception as e:  # noqa: BLE001 - a probe must not take the bench line down
        out["probe_error"] = f"{type(e).__name__}: {e}"
    return out


def count_gpus_without_hip():
    """GPUs of this box WITHOUT any HIP / HSA call: KFD topology nodes with SIMDs (CPU nodes have simd_count 0),
    narrowed by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES when set.  Returns None when sysfs has no KFD topology."""
    import glob
    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not nodes:
        return None
    n = 0
    for f in nodes:
        try:
            for ln in open(f):
                k, _, v = ln.partition(" ")
                if k == "simd_count" and int(v) > 0:
                    n += 1
        except (OSError, ValueError):
            pass
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def spawn_ranks(n):
    """`--gpus N` without a launcher: start N child ranks of this script BEFORE anything here touches a GPU (devices are
    counted from sysfs; only if that is absent with `torch.cuda.device_count()`, which does not initialise a device on
    this image), poll them, end every rank as soon as one exits non-zero or the overall limit (MCG_BENCH_TIMEOUT, default
    3600 s) passes, relay rank 0's JSON line, exit with the worst child status.  The children are fresh processes (no
    exec of a process that has touched a GPU)."""
    import socket
    import subprocess
    import tempfile
    have = count_gpus_without_hip()
    if have is None:
        have = torch.cuda.device_count()
    # (MCG_DIST_BACKEND=gloo: dry run of the N-rank control flow with the ranks sharing the GPUs that exist - labelled
    #  `dist_backend: gloo` in the line, never a scaling measurement)
    if have < n and os.environ.get("MCG_DIST_BACKEND") != "gloo":
        sys.stderr.write(f"bench.py: --gpus {n} but this box has {have} GPU(s); refusing to report a smaller run\n")
        sys.exit(3)
    s = socket.socket()
    s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    limit = float(os.environ.get("MCG_BENCH_TIMEOUT", "3600"))
    procs = []
    with tempfile.TemporaryFile(mode="w+") as out0:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL))
        t0 = time.time()
        why = None
        while True:
            rcs = [p.poll() for p in procs]
            if all(rc is not None for rc in rcs):
                break
            if any(rc not in (None, 0) for rc in rcs):
                why = f"rank(s) {[r for r, rc in enumerate(rcs) if rc not in (None, 0)]} failed"
            elif time.time() - t0 > limit:
                why = f"no result after {limit:.0f} s"
            if why:
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
                t1 = time.time()
                while any(p.poll() is None for p in procs) and time.time() - t1 < 10:
                    time.sleep(0.1)
                for p in procs:
                    if p.poll() is None:
                        p.kill()
                rcs = [p.wait() for p in procs]
                break
            time.sleep(0.2)
        out0.seek(0)
        line = [ln for ln in out0.read().splitlines() if ln.startswith("{")]
    if why or any(rcs) or not line:
        sys.stderr.write(f"bench.py: child ranks exited with {rcs}" + (f" ({why}; the others were ended)" if why else "") + "\n")
        sys.exit(max(1, max(abs(r) for r in rcs)))
    print(line[-1], flush=True)
    sys.exit(0)


def pin_this_rank(world, local_rank):
    """Placement (round 6): a rank - its torch threads and, by inheritance, its host-pool worker processes - is pinned to the cores
    of its GPU's NUMA node, shared between the ranks of that node (ml_conformer_generator_amd/affinity.py: sysfs only, no HIP call;
    loaded BY PATH - the package's __init__ would load the HIP library first).  On by default for N > 1, off for a lone rank;
    MCG_BENCH_AFFINITY=0 / 1 overrides.  Returns the cores now in force (None = not pinned)."""
    if os.environ.get("MCG_BENCH_AFFINITY", "1" if world > 1 else "0") == "0":
        return None
    import importlib.util as _ilu
    spec = _ilu.spec_from_file_location("_mcg_affinity", os.path.join(REPO, "ml_conformer_generator_amd", "affinity.py"))
    aff = _ilu.module_from_spec(spec)
    spec.loader.exec_module(aff)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    return aff.pin(aff.rank_cpus(local_rank, local_world)) or None


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args.gpus)             # never returns
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}\n")
        sys.exit(2)
    use_dist = world > 1 or bool(os.environ.get("MCG_FORCE_COLLECTIVE"))
    # N rank processes share one host: without a cap each keeps torch's default intra-op pool of EVERY core (256 threads per
    # rank on the GPU box; the CPU thread sweep below shows what oversubscription costs).  The hot path needs the host for
    # launches, the size draw and the record assembly only.
    rank_cpus = pin_this_rank(world, local_rank)
    n_cores = len(rank_cpus) if rank_cpus else (os.cpu_count() or 1) // max(1, world)
    host_threads = max(1, min(16, n_cores))
    torch.set_num_threads(host_threads)
    backend = os.environ.get("MCG_DIST_BACKEND", "nccl")
    if world > 1 and backend == "nccl" and torch.cuda.device_count() < world:
        sys.stderr.write(f"bench.py: {world} ranks but {torch.cuda.device_count()} GPU(s)\n")
        sys.exit(3)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if os.environ.get("NCCL_DEBUG", "").upper() == "VERSION":
            os.environ["NCCL_DEBUG"] = ""        # the version banner goes to stdout, where only the JSON line belongs
        # MCG_DIST_BACKEND=gloo: dry run of the N > 1 control flow with several ranks on ONE GPU
        dev_index = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(dev_index)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        assert dist.get_world_size() == world
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", torch.cuda.current_device())

    lib_path = os.path.join(REPO, "ml_conformer_generator_amd", "libmlconfgen_hip.so")
    need_build = not os.path.exists(lib_path)
    if use_dist and world > 1:
        # every rank must agree BEFORE local rank 0 starts writing the file (the linker creates it early)
        flag = torch.tensor([1 if need_build else 0], device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        need_build = bool(flag.item())
    if need_build:          # fresh checkout: the library is git-ignored; local rank 0 builds it, the others wait at the barrier
        if local_rank == 0:
            import subprocess
            subprocess.run(["make", "-C", os.path.join(REPO, "ml_conformer_generator_amd", "csrc"), "-j4"], check=True,
                           stdout=sys.stderr)
        if use_dist and world > 1:
            dist.barrier()
    from ml_conformer_generator_amd import weights as W
    from ml_conformer_generator_amd.synthetic import DUMMY_CONTEXT

    # Weights: the mutation-checked gains with the squared-distance columns damped ("v2d").  The undamped default
    # ("v2", the parity fixtures' recipe at T = 20 / B = 4) overflows the UNTRAINED sampler at this workload - x -> d^2 ->
    # x feeds back through the coordinate head and the trajectory is NaN from step ~30 of 100 (tools/finite_probe.py) -
    # and a benchmark must not time NaN arithmetic.  `outputs_finite` below is checked on EVERY generated coordinate.
    # (fragment modes: contractive legacy weights - resampling repeats the 1/alpha_ts amplification of the first step)
    sd = W.synth_edm_state_dict(1234, weight_gain=0.3) if args.fragment else W.synth_edm_state_dict(1234, recipe="v2d")
    gsd = W.synth_adj_mat_seer_state_dict(4321)
    gen = make_generator(args, dev, args.dtype, sd, gsd)
    ctx = torch.tensor(DUMMY_CONTEXT)
    B = args.n_samples
    frag_kw = {}
    if args.fragment:
        frag_kw = synthetic_fragment()

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    last_step = {}
    elapsed, sampler_ms, finite, valid_frac = timed_passes(gen, ctx, B * world, args.n_atoms, args.variance, frag_kw,
                                                           args.steps, args.warmup, fence, last_out=last_step)
    if args.dump_outputs and rank == 0:
        dump_outputs(last_step, args.dump_outputs)
    head_assembly_ms = gen.last_host_assembly_ms          # D2H of the (gathered) result tensors + molecule records, last pass
    if use_dist:
        tt = torch.tensor([elapsed, 0.0 if finite else 1.0], dtype=torch.float64,
                          device=dev if dist.get_backend() == "nccl" else torch.device("cpu"))
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt[0].item())
        finite = float(tt[1].item()) == 0.0            # every rank's shard

    headline_default = (B == 64 and args.variance == 0 and args.n_atoms == 27 and args.dtype == "f32" and not args.fragment
                        and args.diffusion_steps == 100)
    head_roof = None
    if rank == 0 and args.full:
        # dominant kernel of the HEADLINE workload, timed now: later sub-runs add plans of other shapes
        # HBM bytes per launch of the dominant kernel come from separate rocprofv3 --pmc passes (they cannot be taken
        # inside this run); quoted from the committed summary only for the exact workload it was measured on, and tagged
        traffic = traffic_source = None
        try:
            pmc = json.load(open(os.path.join(REPO, "profiles", "pmc_traffic.json")))
            key = f"configs[1]: n_samples={B}, n={args.n_atoms}"
            if args.variance == 0 and key in pmc and args.dtype == "f32":
                traffic = pmc[key]["traffic_bytes_corrected"]
                traffic_source = "profiles/pmc_traffic.json (static: rocprofv3 --pmc passes of an earlier run of this workload, " + pmc[key].get("round", "round 1") + ")"
        except Exception:  # noqa: BLE001
            pass
        head_roof = edge_roofline(args, gen, dev, args.dtype, traffic, traffic_source)
    c3 = None
    if args.full and world > 1 and headline_default and not args.no_config3:
        # BASELINE configs[3]: 256 ragged molecules PER GPU (n_samples = 256 x N in total), every rank, 1 warm-up + 2 passes
        el3, ms3, fin3, vf3 = timed_passes(gen, ctx, 256 * world, 27, 12, {}, 2, 1, fence, vary_sizes=True)
        asm3 = gen.last_host_assembly_ms
        t3 = torch.tensor([el3, 0.0 if fin3 else 1.0], dtype=torch.float64,
                          device=dev if dist.get_backend() == "nccl" else torch.device("cpu"))
        dist.all_reduce(t3, op=dist.ReduceOp.MAX)
        c3 = (float(t3[0].item()), ms3, float(t3[1].item()) == 0.0, vf3, asm3)


    if rank == 0:
        total_mols = B * world * args.steps
        value = total_mols / elapsed
        n_calls = (2 * args.diffusion_steps if args.fragment else args.diffusion_steps) + 1
        egnn_step_ms = sampler_ms / n_calls
        if args.full:
            plan, roof = head_roof
            agg_s, agg_b = time_aggregate_kernel(plan, dev)
        else:
            plan = last_plan(gen)
        if B == 64 and args.variance == 0 and args.n_atoms == 27:
            cfg_label = "configs[1]"
        elif B == 256 and args.variance == 12 and args.n_atoms == 27:
            cfg_label = "configs[2] shape" if world == 1 else "configs[3] shape (256/GPU)"
        elif B == 4 and args.variance == 2 and args.n_atoms == 17 and args.diffusion_steps == 20:
            cfg_label = "configs[0] shape (ceyyag: 17 heavy atoms +-2, 4 samples, T=20)"
        else:
            cfg_label = "custom"
        if args.fragment:
            cfg_label = ("configs[4] per-GPU share" if (B == 256 and args.variance == 12 and args.diffusion_steps == 250
                                                         and args.dtype == "bf16") else "custom") + " (fragment inpainting, rs=1)"
        mode_text = {"f32": "fp32 HIP EGNN + GCN",
                     "bf16": "bf16-operand MFMA HIP EGNN (fp32 accumulate/state) + fp32 GCN",
                     "f32x6": "fp32 HIP EGNN with the edge-MLP contraction as 6 bf16 partial products of "
                              "3-part fp32 operands (fp32-accurate, fp32 accumulate) + fp32 GCN"}[args.dtype]
        out = {
            "metric": f"valid molecules/sec @{args.diffusion_steps} diffusion steps (`value` = RAW molecules/s through the whole "
                      "public path: the reference's validity gate needs RDKit + trained weights, unavailable offline; see `validity`)",
            "value": value, "unit": "molecules/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{cfg_label}: n_samples={B}/GPU, {args.n_atoms}"
                                   f"{'+-' + str(args.variance) if args.variance else ''} heavy atoms, "
                                   f"diffusion_steps={args.diffusion_steps}, " + mode_text,
                       "parallelism": (f"batch-sharded x{world}, " + ("RCCL" if backend == "nccl" else backend + " (dry run, ranks share the GPU)")
                                       + " gather to rank 0 at end (the only data-path collective)") if world > 1 else "single GPU",
                       "edge_rows_per_wave": 16 * plan.edge_mt, "real_edges": plan.n_real_edges,
                       "real_nodes": plan.n_real_nodes,
                       "weights": "synthetic, reference checkpoint layout, seed 1234, " +
                                  ("nn.Linear-family init x 0.3" if args.fragment else "recipe v2d (ml_conformer_generator_amd/weights.py)")},
            "dist_world_size": dist.get_world_size() if use_dist else 1,
            "dist_backend": (dist.get_backend() if use_dist else None),
            "timed_region": "MLConformerGenerator.generate_conformers_sharded: size draw, sampler, hand-off, GCN, bond "
                            "write-back + validity proxy, gather, D2H, molecule records",
            "validity": "`value` counts every molecule that went through the whole public path (raw); trained weights and "
                        "RDKit are unavailable offline, so the reference's gate cannot run: `valid_proxy_fraction` is the "
                        "share passing the labelled valence / single-fragment PROXY on synthetic-weight outputs "
                        "(meaningless chemistry, reported for completeness), and the reference's published valid "
                        "fraction is 0.48 (README.md:115)",
            "valid_proxy_fraction": valid_frac,
            "value_x_reference_valid_fraction": value * 0.48,
            "egnn_step_ms_per_batch": egnn_step_ms,
            "host_assembly_ms": head_assembly_ms,
            "host_threads_per_rank": host_threads,
            "host_cpus_per_rank": ({"count": len(rank_cpus), "first": rank_cpus[0], "last": rank_cpus[-1],
                                    "how": "pinned to the cores of this rank's GPU's NUMA node, shared between the ranks of the node "
                                           "(affinity.py, sysfs only); rank 0 shown"}
                                   if rank_cpus else {"count": (os.cpu_count() or 1) // max(1, world), "how": "not pinned"}),
            "host_stages": host_stage_report(gen, probe=args.full),
            "outputs_finite": finite,
        }
        if args.full:
            out["roofline"] = roof
            out["aggregate_roofline"] = {"kernel": "k_aggregate (stand-alone gate*mask*segment-sum probe)", "bound": "hbm",
                                         "achieved": agg_b / agg_s / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                         "frac": agg_b / agg_s / 1e9 / PEAK_HBM_GBS, "avg_launch_us": agg_s * 1e6,
                                         "bytes_per_launch": agg_b}
        default_line = args.full and headline_default and world == 1
        if c3 is not None:
            _, roof3 = edge_roofline(args, gen, dev, args.dtype)
            out["config3_ragged256_per_gpu"] = {
                "workload": f"configs[3]: n_samples={256 * world} sharded 256/GPU, 27+-12 heavy atoms (ragged), diffusion_steps=100, "
                            + mode_text + ", gather at end",
                "value": 256 * world * 2 / c3[0], "unit": "molecules/s", "n_gpus": world, "steps": 2, "warmup": 1,
                "ms_per_step": c3[0] / 2 * 1e3, "egnn_step_ms_per_batch": c3[1] / (args.diffusion_steps + 1),
                "valid_proxy_fraction": c3[3], "outputs_finite": c3[2], "roofline": roof3,
                "host_assembly_ms": c3[4],
                "sizes": "a different global size vector every pass (seed + pass index)",
                "timing": "max over ranks, barrier + synchronize on both sides"}
            finite = finite and c3[2]
        if default_line and not args.no_config2:
            # BASELINE configs[2] (256 ragged molecules, 15..39 atoms) timed in the same run: 1 warm-up + 2 passes
            el2, ms2, fin2, vf2 = timed_passes(gen, ctx, 256, 27, 12, {}, 2, 1, fence, vary_sizes=True)
            tr2 = ts2 = None
            try:
                e2 = json.load(open(os.path.join(REPO, "profiles", "pmc_traffic.json")))["configs[2] shape: n_samples=256, n=27+-12"]
                tr2 = e2["traffic_bytes_corrected_per_layer"]
                ts2 = ("profiles/pmc_traffic.json (static: separate rocprofv3 --pmc passes, " + e2["round"] + "; three range-launches "
                       "per layer summed, FETCH_SIZE x2 gfx950 correction)")
            except Exception:  # noqa: BLE001
                pass
            _, roof2 = edge_roofline(args, gen, dev, args.dtype, tr2, ts2)
            out["config2_ragged256"] = {
                "workload": "configs[2] shape: n_samples=256, 27+-12 heavy atoms (ragged), diffusion_steps=100, " + mode_text,
                "value": 256 * 2 / el2, "unit": "molecules/s", "steps": 2, "warmup": 1, "ms_per_step": el2 / 2 * 1e3,
                "egnn_step_ms_per_batch": ms2 / (args.diffusion_steps + 1), "valid_proxy_fraction": vf2,
                "outputs_finite": fin2, "roofline": roof2,
                "sizes": "a different size vector every pass (seed + pass index): each timed pass builds its plan and captures "
                         "its HIP graph inside the timed region",
                "cold_call": cold_call_cost(gen, dev)}
        if default_line and not args.no_config0:
            out["config0_plumbing"] = config0_plumbing(args, gen, sd, gsd, dev, fence)
            finite = finite and out["config0_plumbing"]["outputs_finite"]
        if default_line and not args.no_config4:
            out["config4_share_bf16_inpaint"] = config4_share(args, gsd, ctx, dev, fence)
            finite = finite and out["config4_share_bf16_inpaint"]["outputs_finite"]
        if args.full and args.dtype == "f32" and world == 1 and not args.no_x6_probe and not args.fragment:
            out["f32x6_candidate"] = x6_probe(args, gen, sd, gsd, ctx, dev)
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(args, sd, gsd)
            out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
        line = json.dumps(out)
    else:
        line = None
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if line is not None:
        # the JSON line is the LAST thing on stdout: RCCL writes its banner / warnings through C stdio
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:  # noqa: BLE001
            pass
        print(line, flush=True)
        if not finite:
            sys.stderr.write("bench.py: the timed passes produced non-finite coordinates (`outputs_finite`: false) - "
                             "the line above is NOT a valid measurement\n")
            sys.exit(5)


if __name__ == "__main__":
    main()
