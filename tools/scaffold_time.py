#!/usr/bin/env python3
"""Time of the ring and scaffold step (`scaffold.ring_perception` + `scaffold.murcko_scaffolds`) for 2 048 molecules of 42
atoms (GPU box): seeded, molecule-like graphs - two or three 5- / 6-rings joined by chains, the rest substituents, every
degree at most 4.  Warm-up, then the median of repeated runs: the device part (the three launches, device events) and the
whole call with its host half (the identity bytes, a host clock round a synchronise).  Prints one line per figure."""
import os, random, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ml_conformer_generator_amd import canonical, scaffold

B, N, WARM, REPS = 2048, 42, 3, 21
dev = torch.device("cuda:0")


def molecule(rng):
    z, bonds, deg = [], {}, []

    def atom():
        z.append(rng.choice([6, 6, 6, 6, 7, 8]))
        deg.append(0)
        return len(z) - 1

    def bond(a, b, c=1):
        bonds[(a, b)] = c
        deg[a] += 1
        deg[b] += 1
    anchors = []
    for r in range(rng.choice([2, 3])):
        k, code = rng.choice([(5, 1), (6, 1), (6, 4)])
        ring = [atom() for _ in range(k)]
        for i in range(k):
            bond(ring[i], ring[(i + 1) % k], code)
        if anchors:                                   # a chain of 0..3 atoms to the ring before
            last = rng.choice(anchors[-1])
            for _ in range(rng.randint(0, 3)):
                nxt = atom()
                bond(last, nxt)
                last = nxt
            bond(last, ring[0])
        anchors.append(ring[1:])
    while len(z) < N:                                 # substituents, some doubly bonded
        free = [a for a in range(len(z)) if deg[a] < 3]
        a = rng.choice(free)
        plain = all(c == 1 for (i, j), c in bonds.items() if a in (i, j))      # room for a double bond: C=O on a ring
        bond(a, atom(), 2 if rng.random() < 0.25 and plain else 1)
    return z, bonds


rng = random.Random(20261020)
zs = torch.zeros(B, N, dtype=torch.int32)
codes = torch.zeros(B, N, N, dtype=torch.int8)
for b in range(B):
    z, bonds = molecule(rng)
    zs[b] = torch.tensor(z[:N], dtype=torch.int32)
    for (i, j), c in bonds.items():
        codes[b, i, j] = codes[b, j, i] = c
n = torch.full((B,), N, dtype=torch.int32)
zd, bd, nd = zs.to(dev), codes.to(dev), n.to(dev)


def device_part():
    per = scaffold.ring_perception(zd, bd, nd, dev, check=False)
    sub = scaffold.induced_subgraph(zd, bd, nd, per["masks"][:, scaffold.MASK_SCAFFOLD].contiguous(), scaffold.MODE_KEEP, dev)
    return per, canonical.canonical_order(sub["atomic_numbers"], sub["bond_orders"], sub["n"], dev, check=False)


for _ in range(WARM):
    device_part()
    found = scaffold.murcko_scaffolds(zd, bd, nd, dev, check=False)
torch.cuda.synchronize(dev)
ms, wall = [], []
for _ in range(REPS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    per, ordered = device_part()
    end.record()
    torch.cuda.synchronize(dev)
    ms.append(start.elapsed_time(end))
    t0 = time.perf_counter()
    found = scaffold.murcko_scaffolds(zd, bd, nd, dev, check=False)
    torch.cuda.synchronize(dev)
    wall.append(1e3 * (time.perf_counter() - t0))
counts = per["counts"].cpu()
print(f"{B} molecules of {N} atoms: {float(counts[:, 0].float().mean()):.2f} rings, {float(counts[:, 5].float().mean()):.2f} "
      f"linker and {float(counts[:, 6].float().mean()):.2f} exo atoms each on average; "
      f"{len(scaffold.group_by_scaffold(found['identity']))} scaffolds, "
      f"{sum(1 for e in found['identity'] if e is None)} without a canonical order")
print(f"ring_perception + induced_subgraph + canonical_order of the scaffolds, device events: median {statistics.median(ms):.3f} ms "
      f"(min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs)")
print(f"murcko_scaffolds with its host half (identity bytes), host clock: median {statistics.median(wall):.2f} ms "
      f"(min {min(wall):.2f}, max {max(wall):.2f})")
