#!/usr/bin/env python3
"""Time of the pose search (`interactions.search_pose`) beside the flexible walk alone on the same start rows, in the same
process (GPU box): the 2 048 molecules of 42 atoms and the 100 000-atom ball receptor of tools/flex_pose_time.py, 8 starts,
64 trials - 16 384 start rows, one `mcg_receptor_optimise_flex` launch.  The whole `search_pose` (perceive, torsion tree,
`mcg_pose_starts`, the replication, the walk, `mcg_pose_search_select`), then `mcg_receptor_optimise_flex` alone on the
starts that call made, its operands replicated outside the timed region, then the two new kernels each alone.  Receptor
uploaded outside the timed region.  Warm-up, then the median of 21 runs by device events.  No threshold: a record.  Prints
one line per figure and the ratio."""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from ml_conformer_generator_amd import interactions as IX  # noqa: E402
from interaction_time import ball_receptor, walks  # noqa: E402

B, N, R, S, STEPS, WARM, REPS = 2048, 42, 100000, 8, 64, 3, 21
dev = torch.device("cuda:0")

g = torch.Generator().manual_seed(7)
z = torch.tensor([6, 6, 6, 7, 8])[torch.randint(0, 5, (B, N), generator=g)].to(dev)
bonds = torch.zeros(B, N, N, dtype=torch.int8)
idx = torch.arange(N - 1)
bonds[:, idx, idx + 1] = 1
bonds[:, idx + 1, idx] = 1
bonds = bonds.to(dev)
nn = torch.full((B,), N, dtype=torch.int32, device=dev)
ids = torch.arange(B)
rec, radius = ball_receptor(R, R)
prepared = IX.prepare_receptor(rec)
on_device = IX.PreparedReceptor(*(t.to(dev) for t in prepared))
x = walks(B, N, max(radius - 6.0, 1.0), R + 1).to(dev)


def search():
    return IX.search_pose(on_device, x, nn, z, bonds, starts=S, steps=STEPS, seed=7, sample_ids=ids, device=dev)


first = search()
rows = first["starts"]["coords"].reshape(B * S, N, 3).contiguous()
pick = torch.arange(B, device=dev).repeat_interleave(S)
types = IX.ligand_types(z, bonds, nn, dev)
tree = IX.torsion_tree(z, bonds, nn, dev, check=False)
rep = dict(nn=nn[pick].contiguous(), radii=IX.interaction_radii(z)[pick].contiguous(), types=types[pick].contiguous(),
           clash=IX.clash_radii(z)[pick].contiguous(), tree=IX._repeat_tree(tree, pick))


def walk_alone():
    return IX._walk_typed(on_device, rows, rep["nn"], B * S, N, rep["radii"], rep["types"], STEPS, IX.OPTIMISE_MAX_SHIFT, True,
                          dev, False, rep["clash"], rep["tree"])


def starts_alone():
    return IX.pose_starts(x, nn, tree, ids, 7, S, device=dev)


st = first["starts"]


def select_alone():
    return IX.select_starts(st["walk_coords"], st["walk_xform"], st["walk_stats"], st["walk_angles"], st["xform"],
                            st["angles"], x, nn, dev)


def timed(call):
    for _ in range(WARM):
        out = call()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(REPS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = call()
        end.record()
        torch.cuda.synchronize(dev)
        ms.append(start.elapsed_time(end))
    return out, ms


def line(ms):
    return f"median {statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs)"


out_s, ms_s = timed(search)
out_w, ms_w = timed(walk_alone)
_, ms_a = timed(starts_alone)
_, ms_c = timed(select_alone)
best = out_s["best_start"]
j = out_s["start_scores"]
print(f"{B} molecules of {N} atoms, receptor of {R} atoms ({int(prepared.spheres.shape[0])} tiles), {S} starts, {STEPS} trials: "
      f"{B * S} start rows; torsions used {float(tree['counts'][:, 1].float().mean()):.1f}")
print(f"search_pose, whole:                        {line(ms_s)}; a start >= 1 won in {int((best > 0).sum())} of {B} rows; mean J "
      f"{float(j[:, 0].mean()):.3f} (start 0) -> {float(j.min(dim=1).values.mean()):.3f} (winner)")
print(f"mcg_receptor_optimise_flex on its {B * S} rows: {line(ms_w)}; mean trials {float(out_w['stats'][:, 2].mean()):.1f}, "
      f"kept {float(out_w['stats'][:, 3].mean()):.1f}")
print(f"mcg_pose_starts alone:                     {line(ms_a)}")
print(f"mcg_pose_search_select alone:              {line(ms_c)}")
print(f"ratio search_pose / walk alone: {statistics.median(ms_s) / statistics.median(ms_w):.3f}")
