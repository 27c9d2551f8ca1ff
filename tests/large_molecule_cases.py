"""Molecules above 42 atoms: the cases shared by tests/test_large_molecules_host.py (CPU) and
tests/test_large_molecules_gpu.py (MI355X), as plain data with the regime each one is there to cover.

A plan lays the real directed edges of all molecules out as one flat row list (atom i of an n-atom molecule owns n - 1
consecutive rows) and cuts it into units of R rows: R = 16 for the exact-fp32 kernels (edge_mt 1), R = 64 for the bf16 /
f32x6 kernels (edge_mt 4).  How many units an atom's rows run through decides which kernels can serve the batch:

  R = 16 span <= 4   unit tables exist: exact-fp32 throughput kernel, node GEMM gathers the workgroup-level sums
  R = 16 span 5..8   no unit tables: column-split kernel k_edge_ns, eight-slot combine, coordinate-update kernel
  R = 16 span > 8    refused at plan creation
  R = 64 span <= 2   bf16: node GEMM gathers the per-unit partial sums, fused node launch possible
  R = 64 span 3..4   bf16: gather, unfused;  f32x6: combine
  R = 64 span 5..8   combine + coordinate-update kernel in both modes

The expected routes below were read from route() (csrc/mcg_egnn_api.hip); every GPU case asserts the one it names through
`mcg_debug_route`, so a heuristic that later moves a size into another regime fails the test instead of emptying it.
"""
import torch

WEIGHT_SEED, WEIGHT_RECIPE = 1234, "v2"


def unit_spans(sizes, R):
    """Units of R rows that the edge rows of each molecule's atoms run through, most per molecule: atom i of molecule b
    owns rows first .. first + n - 2 with first = row_off[b] + i * (n - 1) (csrc/mcg_plan_host.cpp)."""
    spans, row_off = [], 0
    for n in sizes:
        worst = 0
        for i in range(n if n > 1 else 0):
            first = row_off + i * (n - 1)
            worst = max(worst, (first + n - 2) // R - first // R + 1)
        spans.append(worst)
        row_off += n * (n - 1)
    return spans


def span16(sizes):
    return max(unit_spans(sizes, 16))


def span64(sizes):
    return max(unit_spans(sizes, 64))


def build_inputs(sizes, N, seed):
    """The per-test recipe of tests/test_hip_parity.py: seeded randn times the mask, one context vector per molecule
    repeated over its atoms, and a t column that differs between molecules.  Returns fp32 CPU tensors
    (t[B,1], z[B,N,11], node_mask[B,N,1], edge_mask[B*N*N,1], context[B,N,3])."""
    from oracle import host_oracle as HO
    g = torch.Generator().manual_seed(seed)
    sz = torch.tensor(sizes)
    B = len(sizes)
    nm, em = HO.masks_from_sizes(sz, N)
    z = torch.randn(B, N, 11, generator=g) * nm
    ctx = torch.randn(B, 1, 3, generator=g).repeat(1, N, 1) * nm
    t = (0.3 + 0.4 * torch.arange(B, dtype=torch.float32) / max(B, 1)).reshape(B, 1)
    return t, z, nm, em, ctx


def oracle_per_molecule(sd, t, z, node_mask, context):
    """oracle.egnn_oracle.egnn_dynamics evaluated molecule by molecule at each molecule's own width (B = 1, N = n_b) and
    put back into [B, N, 11]: the same function - a padded slot contributes exact zeros to every sum, and molecules do not
    interact - at sum(n_b^2) dense edges instead of B * N^2 (case H: 37 000 instead of 182 000).  dtype follows `sd`.
    tests/test_large_molecules_host.py holds it against the whole-batch evaluation."""
    from oracle import egnn_oracle as EO
    from oracle import host_oracle as HO
    dt = next(iter(sd.values())).dtype
    out = torch.zeros(z.shape, dtype=dt)
    for b, n in enumerate(node_mask.reshape(node_mask.shape[0], -1).sum(1).round().long().tolist()):
        if n == 0:
            continue
        nm, em = HO.masks_from_sizes(torch.tensor([n]), n)
        out[b, :n] = EO.egnn_dynamics(sd, t[b:b + 1].to(dt), z[b:b + 1, :n].to(dt), nm.to(dt), em.to(dt),
                                      context[b:b + 1, :n].to(dt))[0]
    return out


def route(edge, agg, coord, **more):
    return dict(edge=edge, agg=agg, coord=coord, **more)


_NS = route("Ns", "Combine", "Kernel")

# name -> sizes, pad width N, input seed, host regime and the route of every (mode, variant) the GPU module runs.
#   sets:     unit-table sets of the 16-row plan (mcg_plan_check_tables info[0]); None = the 16-row plan is refused
#   span16/64: most units an atom's rows run through
#   routes:   (mode, variant) -> expected mcg_debug_route fields.  Variants of f32: "auto", "lat0", "lat1"
#             (mcg_plan_set_latency_mode -1 / 0 / 1; the latter two only where the plan has tables).  bf16 / f32x6 run on
#             edge_mt = 4 plans when no molecule is below 6 atoms, as EGNNDynamics.plan chooses.
#             Cases A, B and H have ONE table set, so latency mode 0 selects the tables mode -1 selects and their "lat0" runs
#             repeat "auto" bit for bit (the issue asks for them); case I has two sets and is where mode 0 switches tables.
CASES = {
    "A": dict(sizes=[52, 60, 47, 55], N=60, seed=101, sets=1, span16=5, span64=2, edge_mt_wide=4, routes={
        ("f32", "auto"): route("Exact", "GatherU", "PendingU", unit_span=2),
        ("f32", "lat0"): route("Exact", "GatherU", "PendingU", unit_span=2),
        ("f32", "lat1"): route("Ns", "Combine", "Kernel", pspan=5, unit_span=0),
        ("f32x6", "auto"): route("W64X6", "Combine", "Kernel", pspan=2),
        ("bf16", "auto"): route("W64Bf16", "GatherP", "PendingP", pspan=2, fused=False),
    }),
    "B": dict(sizes=[64, 65, 66, 67, 20], N=67, seed=102, sets=1, span16=5, span64=2, edge_mt_wide=4, routes={
        ("f32", "auto"): route("Exact", "GatherU", "PendingU", unit_span=2),
        ("f32", "lat0"): route("Exact", "GatherU", "PendingU", unit_span=2),
        ("f32", "lat1"): route("Ns", "Combine", "Kernel", pspan=5, unit_span=0),
        ("f32x6", "auto"): route("W64X6", "Combine", "Kernel", pspan=2),
        ("bf16", "auto"): route("W64Bf16", "GatherP", "PendingP", pspan=2, fused=False),
    }),
    "C": dict(sizes=[68, 80, 9, 101], N=101, seed=103, sets=0, span16=7, span64=3, edge_mt_wide=4, routes={
        ("f32", "auto"): dict(_NS, pspan=7, unit_span=0),
        ("f32x6", "auto"): route("W64X6", "Combine", "Kernel", pspan=3),
        ("bf16", "auto"): route("W64Bf16", "GatherP", "PendingP", pspan=3, fused=False),
    }),
    "D": dict(sizes=[114, 43, 65, 20, 90], N=114, seed=104, sets=0, span16=8, span64=3, edge_mt_wide=4, routes={
        ("f32", "auto"): dict(_NS, pspan=8, unit_span=0),
        ("f32x6", "auto"): route("W64X6", "Combine", "Kernel", pspan=3),
        ("bf16", "auto"): route("W64Bf16", "GatherP", "PendingP", pspan=3, fused=False),
    }),
    # a molecule below 6 atoms keeps the split-operand modes on 16-row tiles: bf16 on its 16-row kernel with eight partial
    # sums per atom, f32x6 on the exact fp32 kernels
    "E": dict(sizes=[114, 1, 2, 70], N=114, seed=105, sets=0, span16=8, span64=3, edge_mt_wide=1, routes={
        ("f32", "auto"): dict(_NS, pspan=8, unit_span=0),
        ("f32x6", "auto"): dict(_NS, pspan=8, unit_span=0),
        ("bf16", "auto"): route("Bf16Rows16", "Combine", "Kernel", pspan=8),
    }),
    # beyond the 16-row plans' limit: exact fp32 is refused at plan creation, the 64-row modes run with five slots per atom
    "F": dict(sizes=[200, 130, 12], N=200, seed=106, sets=None, span16=14, span64=5, edge_mt_wide=4, routes={
        ("f32x6", "auto"): route("W64X6", "Combine", "Kernel", pspan=5),
        ("bf16", "auto"): route("W64Bf16", "Combine", "Kernel", pspan=5),
    }),
    "G": dict(sizes=[115, 115], N=115, seed=107, sets=0, span16=8, span64=3, edge_mt_wide=4, routes={
        ("f32", "auto"): dict(_NS, pspan=8, unit_span=0),
        ("f32x6", "auto"): route("W64X6", "Combine", "Kernel", pspan=3),
        ("bf16", "auto"): route("W64Bf16", "GatherP", "PendingP", pspan=3, fused=False),
    }),
    # 43..51 atoms: the only sizes above 42 with TWO table sets - quarter-tile units (an atom's rows span four) and four-tile
    # units (two) - so latency mode 0 runs other tables, and another gather width, than mode -1
    "I": dict(sizes=[48, 51, 45, 50], N=51, seed=109, sets=2, span16=4, span64=2, edge_mt_wide=4, routes={
        ("f32", "auto"): route("Exact", "GatherU", "PendingU", unit_span=4),
        ("f32", "lat0"): route("Exact", "GatherU", "PendingU", unit_span=2),
        ("f32", "lat1"): route("Ns", "Combine", "Kernel", pspan=4, unit_span=0),
        ("f32x6", "auto"): route("W64X6", "Combine", "Kernel", pspan=2),
        ("bf16", "auto"): route("W64Bf16", "GatherP", "PendingP", pspan=2, fused=False),
    }),
    # One complete round of a 256-CU chip (512 four-tile units) and a tail: the two 114-atom molecules fall into four-tile
    # units (64 rows: their atoms span three), the quarter-tile tail holds 30-atom molecules, so this batch HAS unit tables -
    # one mixed set - and exact fp32 runs the throughput kernel with a three-row gather.  2 263 tiles: below the 3 600 from
    # which a plan is cut into molecule ranges.  (Another device size cuts the round elsewhere: the route assertion says so.)
    "H": dict(sizes=[114, 114] + [30] * 12, N=114, seed=108, sets=1, span16=8, span64=3, edge_mt_wide=4, cus=256, routes={
        ("f32", "auto"): route("Exact", "GatherU", "PendingU", unit_span=3),
        ("f32", "lat0"): route("Exact", "GatherU", "PendingU", unit_span=3),
        ("f32", "lat1"): dict(_NS, pspan=8, unit_span=0),
        ("f32x6", "auto"): route("W64X6", "Combine", "Kernel", pspan=3),
        ("bf16", "auto"): route("W64Bf16", "GatherP", "PendingP", pspan=3, fused=False),
    }),
}
