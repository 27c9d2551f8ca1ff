"""What `pharmacophore_scores` costs on the MI355X ("Pharmacophore overlap").

  kernels:   `mcg_pharm_perceive` and `mcg_pharm_score` alone at 64 x 27, 64 x 39 and 256 x 39 (molecule-like graphs grown
             from aromatic rings, coordinates from a Gaussian cloud, a reference of ten features), device events around
             `--repeats` launches after warm-up; beside them `mcg_graph_fingerprint` on the same graphs, the stage this
             one sits next to;
  generator: a 64-molecule, 100-step `generate_conformers` on synthetic weights - plain, with `overlay=True` (which the
             option needs) and with `overlay=True, pharmacophore_scores=True` - interleaved in one process (host clock
             around a call that ends in a device synchronise).
Prints one JSON line.  Needs the GPU: there is no other way to get a time.

    python tools/pharmacophore_time.py [--repeats 20] [--calls 5]
"""
import argparse
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FEATURES = [("ring", (0.0, 0.0, 0.0)), ("donor", (2.4, 0.3, 0.0)), ("acceptor", (-2.1, 1.0, 0.4)),
            ("acceptor", (1.0, -2.2, 0.1)), ("cation", (3.6, 1.1, -0.5)), ("anion", (-3.4, -0.8, 0.2)),
            ("hydrophobe", (0.2, 2.9, 0.6)), ("hydrophobe", (-1.2, -2.8, -0.4)), ("ring", (3.9, -2.0, 0.3)),
            ("donor", (-0.6, 0.9, 2.2))]


def graphs(B, n, seed):
    """(z [B,n] int32, bonds [B,n,n] int8, n_nodes [B]) of B molecule-like graphs of n atoms: one or two aromatic rings,
    then a random tree of degree <= 3 with elements from C N O F S and codes from 1 1 2."""
    rng = random.Random(seed)
    z = np.zeros((B, n), np.int32)
    bonds = np.zeros((B, n, n), np.int8)
    for b in range(B):
        z[b] = rng.choices([6, 6, 6, 7, 8, 9, 16], k=n)
        deg = [0] * n
        at = 0
        for _ in range(rng.randint(1, 2)):
            size = rng.choice([5, 6])
            for k in range(size):
                i, j = at + k, at + (k + 1) % size
                bonds[b, i, j] = bonds[b, j, i] = 4
                deg[i] += 1
                deg[j] += 1
            z[b, at:at + size] = rng.choices([6, 6, 6, 7], k=size)
            at += size
        for a in range(at, n):
            j = rng.choice([k for k in range(a) if deg[k] < 3])
            bonds[b, a, j] = bonds[b, j, a] = rng.choice([1, 1, 2])
            deg[a] += 1
            deg[j] += 1
    return torch.from_numpy(z), torch.from_numpy(bonds), torch.full((B,), n, dtype=torch.int32)


def events(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / repeats


def kernel_times(repeats):
    from ml_conformer_generator_amd import _lib
    from ml_conformer_generator_amd import fingerprint as FP
    from ml_conformer_generator_amd import pharmacophore as PH
    dev = torch.device("cuda:0")
    lib, stream = _lib.lib(), _lib.current_stream_ptr(dev)
    xyz, typ = (t.to(dev) for t in PH.load_reference_features(FEATURES))
    o_rr = PH.reference_self_overlap((xyz, typ), dev)
    out = {}
    for B, n in ((64, 27), (64, 39), (256, 39)):
        z, bonds, nn = (t.to(dev).contiguous() for t in graphs(B, n, 31 * B + n))
        coords = (torch.randn(B, n, 3, generator=torch.Generator().manual_seed(B + n)) * 2.5).to(dev)
        types, rings, count = PH.perceive_features(z, bonds, nn, dev)
        res = PH.score_features((xyz, typ), coords, nn, types, rings, count, dev)
        buf = {k: torch.empty_like(v) for k, v in res.items()}

        def perceive():
            _lib.check(lib.mcg_pharm_perceive(_lib.dptr(z), _lib.dptr(bonds), _lib.dptr(nn), B, n, _lib.dptr(types),
                                              _lib.dptr(count), _lib.dptr(rings), stream), "mcg_pharm_perceive")

        def score():
            _lib.check(lib.mcg_pharm_score(_lib.dptr(coords), _lib.dptr(nn), _lib.dptr(types), _lib.dptr(rings),
                                           _lib.dptr(count), B, n, n, _lib.dptr(xyz), _lib.dptr(typ), int(typ.numel()),
                                           _lib.dptr(o_rr), _lib.dptr(buf["o_rm"]), _lib.dptr(buf["o_mm"]),
                                           _lib.dptr(buf["tanimoto"]), _lib.dptr(buf["matches"]), None, stream),
                       "mcg_pharm_score")
        out[f"B{B}_n{n}"] = {"perceive_ms": events(perceive, repeats), "score_ms": events(score, repeats),
                             "python_perceive_plus_score_ms": events(
                                 lambda: PH.pharmacophore_tanimoto((xyz, typ), coords, z, bonds, nn, dev), repeats),
                             "fingerprint_ms": events(lambda: FP.graph_fingerprints(z, bonds, nn, dev, check=False), repeats),
                             "features_mean": float((types.cpu().to(torch.int32).apply_(lambda v: bin(v).count("1")).sum()
                                                     + count.sum().cpu()) / B),
                             "tanimoto_mean": float(res["tanimoto"].mean())}
    return out


def generator_times(calls):
    from ml_conformer_generator_amd import MLConformerGenerator
    from ml_conformer_generator_amd import weights as W
    dev = torch.device("cuda:0")
    gen = MLConformerGenerator(diffusion_steps=100, device=dev, edm_weights=W.synth_edm_state_dict(1234, recipe="v2d"),
                               adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321), atom_order_provider=None,
                               finisher=None)
    ref = torch.as_tensor(np.load(os.path.join(REPO, "tests", "golden", "shape_quadrupole.npz"))["xyz_walk27"])
    kw = dict(reference_conformer=ref, n_samples=64, variance=0, optimise_geometry=False, sample_seed=11)
    variants = {"plain": {}, "overlay": dict(overlay=True),
                "overlay_pharmacophore": dict(overlay=True, pharmacophore_scores=True, reference_pharmacophore=FEATURES)}

    def call(extra):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen.generate_conformers(**kw, **extra)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for extra in variants.values():
        call(extra)                                   # warm-up: code objects, plans, graphs
    times = {k: [] for k in variants}
    for _ in range(calls):                            # interleaved: all see the same box
        for k, extra in variants.items():
            times[k].append(call(extra))
    med = lambda v: sorted(v)[len(v) // 2]            # noqa: E731
    out = {k + "_ms": v for k, v in times.items()}
    out.update({k + "_median_ms": med(v) for k, v in times.items()})
    out["added_median_ms"] = med(times["overlay_pharmacophore"]) - med(times["overlay"])
    out["added_share"] = out["added_median_ms"] / med(times["overlay"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pharmacophore_time.py needs the GPU: a time measured anywhere else says nothing")
    print(json.dumps({"kernels": kernel_times(a.repeats), "generate_conformers_64x100": generator_times(a.calls)}))


if __name__ == "__main__":
    main()
