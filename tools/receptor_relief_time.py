"""Wall time of one `receptor.relieve_clashes` call on the MI355X ("Clash relief"): B = 2 048
molecules of N = 42 atoms - copies of one random walk, displaced as in the tests - in a carved lattice pocket of 4 000
atoms, 32 trials, with tile skipping on and off (two rounds of each, alternating).  Host clock around the whole call
ending in a synchronise, median and minimum of 15 after 3 warm-up calls; beside it the device span between two events.
Prints one JSON line.  Run from the repository root: python tools/receptor_relief_time.py"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import relief_ref as RR
from ml_conformer_generator_amd import receptor as RC
dev = torch.device("cuda:0")
g = np.random.default_rng(1)
lig = RR.ligand(42, g)
k = 12
axis = np.arange(-k, k + 1) * 2.6
pts = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3) + g.normal(size=((2 * k + 1) ** 3, 3)) * 0.3
near = np.linalg.norm(pts[:, None, :] - lig[None, :, :], axis=2).min(axis=1)
pts = pts[near > 3.8]
pts = pts[np.argsort(np.linalg.norm(pts, axis=1))[:4000]]
rec = (torch.from_numpy(pts.astype(np.float32)), torch.full((4000,), 6))
B = 2048
x = torch.from_numpy(np.stack([RR.displaced(lig, g) for _ in range(B)]).astype(np.float32))
n = torch.full((B,), 42, dtype=torch.int32)
z = torch.full((B, 42), 6)
xd, nd, zd = x.to(dev), n.to(dev), z.to(dev)
res = {}
outs = {}
for skip in (True, False, True, False):
    for _ in range(3):
        out = RC.relieve_clashes(rec, xd, nd, zd, steps=32, device=dev, skip_tiles=skip)
    torch.cuda.synchronize()
    ts, ks = [], []
    for _ in range(15):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); t0 = time.perf_counter(); e0.record()
        out = RC.relieve_clashes(rec, xd, nd, zd, steps=32, device=dev, skip_tiles=skip)
        e1.record(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3); ks.append(e0.elapsed_time(e1))
    res.setdefault(skip, []).append((float(np.median(ts)), float(np.min(ts)), float(np.median(ks))))
    outs[skip] = out
same = all(torch.equal(outs[True][k2], outs[False][k2]) for k2 in outs[True])
sp = RC.tile_spheres(RC.sort_receptor(rec[0], RC.vdw_radii(rec[1])))
o = outs[True]
print(json.dumps(dict(wall_ms_median_min_devspan={str(k2): v for k2, v in res.items()}, identical=same, tiles=int(sp.shape[0]),
                      moved=int(o["moved"].sum()), cleared=int((o["penalty_after"] == 0).sum()),
                      clashing=int((o["penalty_before"] > 0).sum()), mean_accepted=float(o["accepted_steps"].float().mean()),
                      mean_rmsd=float(o["rmsd"][o["moved"]].mean()))))
