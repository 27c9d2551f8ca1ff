"""Plain torch restatement of `oracle/gcn_oracle.py` (AdjMatSeer, adj_mat_seer.py:104-165) that returns every stage the
library's `mcg_gcn_peek` can copy out, runs at whatever dtype it is given and takes a `mutation=` argument: one planted
arithmetic mistake of the kind a kernel could make.  Shared by `tools/parity_sensitivity.py --gcn`,
`tests/test_gcn_host.py` (CPU) and `tests/test_gcn_gpu.py`.

Unmutated and in fp32 its logits are `torch.equal` to `oracle.gcn_oracle.adj_mat_seer` (the same torch calls in the same
order; `tests/test_gcn_host.py` asserts it), so the restatement inherits the oracle's pin to the reference.

Also here: the input sets and weight sets the three users share, and the per-stage tolerances of the GPU pins.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from ml_conformer_generator_amd.synthetic import synth_gcn_inputs
from ml_conformer_generator_amd.weights import synth_adj_mat_seer_state_dict
from parity_tolerance import ATOL, RTOL, violation

D, EMB, HID, NB, NEMB = 42, 64, 2048, 5, 36

# `mcg_gcn_peek` order (include/mlconfgen_hip.h), then the public output
STAGES = ("L_dm", "L_adj", "bottleneck", "scale", "e0", "xb", "res")
QUANTITIES = STAGES + ("logits",)

DM_LAYERS = ("gcn1_dm", "gcn2_dm", "gcn3_dm")
MAIN_LAYERS = ("gcn1", "gcn2", "gcn3", "gcn4")
# "distance branch" = everything up to and including nodes_coord_fc, "main branch" = everything behind it
DM_WEIGHTS = tuple(n + ".linear.weight" for n in DM_LAYERS) + ("dm_resize.weight", "nodes_coord_fc.weight")
MAIN_WEIGHTS = tuple(n + ".linear.weight" for n in MAIN_LAYERS) + ("resize.weight",)

# name[:branch or layer] - what a kernel would have to get wrong
MUTATIONS: Tuple[str, ...] = (
    "Lt:dm", "Lt:main",                    # k_propagate multiplies by L^T
    "coldeg:dm", "coldeg:main",            # k_lnorm sums columns for the degree
    "rownorm:dm", "rownorm:main",          # D^-1 A instead of D^-1/2 A D^-1/2
    "noI:dm", "noI:main",                  # the +I of the input matrix missing
    "rowdot_drop4",                        # dm_resize drops the last 4 of K = 2048
    "rowdot_nobias",                       # dm_resize bias dropped
    "coordfc_k40", "coordfc_k41",          # nodes_coord_fc reads 40 / 41 of the 42 bottlenecks (K = 42 -> 44 padding edge)
    "pad_bottleneck_zero",                 # padded atoms' bottleneck zeroed
    "emb_swap",                            # the two embedding tables swapped
    "emb_shift:dm", "emb_shift:main",      # embedding rows shifted by one
    "bf16:dm", "bf16:main",                # Linear weights rounded to bf16
    "bias_after:gcn2_dm", "bias_after:gcn3",   # a GraphConv bias added behind L instead of in front of it
    "dist_noise",                          # every distance off by a random 0.1 % (symmetric)
)


def _sym_norm(a: torch.Tensor, mut: Optional[str]) -> torch.Tensor:
    if mut == "noI":
        a = a - torch.eye(a.size(-1), dtype=a.dtype)
    if mut == "coldeg":
        inv = torch.rsqrt(a.sum(dim=-2).clamp(min=1e-12))
    else:
        inv = torch.rsqrt(a.sum(dim=-1).clamp(min=1e-12))
    if mut == "rownorm":
        return (inv * inv).unsqueeze(-1) * a
    return inv.unsqueeze(-1) * a * inv.unsqueeze(-2)


def _graph_conv(sd, name: str, x: torch.Tensor, L: torch.Tensor, transpose: bool, bias_after: bool) -> torch.Tensor:
    if transpose:
        L = L.transpose(1, 2)
    if bias_after:
        return torch.bmm(L, F.linear(x, sd[name + ".linear.weight"])) + sd[name + ".linear.bias"]
    return torch.bmm(L, F.linear(x, sd[name + ".linear.weight"], sd[name + ".linear.bias"]))


def gcn_forward(sd: Dict[str, torch.Tensor], elements: torch.Tensor, dist_mat: torch.Tensor, adj_mat: torch.Tensor,
                dtype: torch.dtype = torch.float32, mutation: Optional[str] = None,
                n_nodes: Optional[Sequence[int]] = None) -> Dict[str, torch.Tensor]:
    """-> {stage: tensor} for every name in QUANTITIES, computed in `dtype`.  `n_nodes` (real atoms per molecule) is
    needed by the `pad_bottleneck_zero` mutation only."""
    if mutation is not None and mutation not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutation!r}")
    name, _, where = (mutation or "").partition(":")
    dm_mut = name if where == "dm" else None
    main_mut = name if where == "main" else None
    B = elements.size(0)
    sd = {k: v.to(dtype) for k, v in sd.items()}
    if name == "bf16":
        for k in (DM_WEIGHTS if where == "dm" else MAIN_WEIGHTS):
            sd[k] = sd[k].to(torch.bfloat16).to(dtype)
    dist_mat, adj_mat = dist_mat.to(dtype), adj_mat.to(dtype)
    if name == "dist_noise":
        u = torch.rand(dist_mat.shape, generator=torch.Generator().manual_seed(77), dtype=torch.float64) * 2 - 1
        u = torch.triu(u) + torch.triu(u, 1).transpose(1, 2)
        dist_mat = dist_mat * (1 + 1e-3 * u).to(dtype)
    emb_dm, emb_main = sd["dm_nodes_embedding.weight"], sd["nodes_embedding.weight"]
    if name == "emb_swap":
        emb_dm, emb_main = emb_main, emb_dm
    if name == "emb_shift":
        if where == "dm":
            emb_dm = torch.roll(emb_dm, 1, 0)
        else:
            emb_main = torch.roll(emb_main, 1, 0)
    out: Dict[str, torch.Tensor] = {}
    # distance-graph branch -> per-atom scalar bottleneck
    L_dm = _sym_norm(dist_mat, dm_mut)
    y = F.embedding(elements, emb_dm)
    for layer in DM_LAYERS:
        y = F.relu(_graph_conv(sd, layer, y, L_dm, dm_mut == "Lt", mutation == "bias_after:" + layer))
    w, b = sd["dm_resize.weight"], sd["dm_resize.bias"]
    if name == "rowdot_drop4":
        bottleneck = F.linear(y[..., :HID - 4], w[:, :HID - 4], b).squeeze(-1)
    elif name == "rowdot_nobias":
        bottleneck = F.linear(y, w).squeeze(-1)
    else:
        bottleneck = F.linear(y, w, b).squeeze(-1)
    if name == "pad_bottleneck_zero":
        n = torch.as_tensor(list(n_nodes)).reshape(B, 1)
        bottleneck = bottleneck * (torch.arange(D).reshape(1, D) < n).to(dtype)
    # main branch
    if name in ("coordfc_k40", "coordfc_k41"):
        k = int(name[-2:])
        scale = F.linear(bottleneck[:, :k], sd["nodes_coord_fc.weight"][:, :k], sd["nodes_coord_fc.bias"])
    else:
        scale = F.linear(bottleneck, sd["nodes_coord_fc.weight"], sd["nodes_coord_fc.bias"])
    v = F.embedding(elements, emb_main) + scale.reshape(B, D, EMB)
    out["L_dm"], out["bottleneck"], out["scale"], out["e0"] = L_dm, bottleneck, scale, v
    L = _sym_norm(adj_mat, main_mut)
    out["L_adj"] = L
    for layer in MAIN_LAYERS:
        v = F.relu(_graph_conv(sd, layer, v, L, main_mut == "Lt", mutation == "bias_after:" + layer))
    out["xb"] = v.reshape(B * D, HID)
    res = F.linear(v, sd["resize.weight"], sd["resize.bias"]).reshape(B, D, D, NB)
    out["res"] = res
    out["logits"] = res.transpose(1, 2) + res
    return out


# ------------------------------------------------------------------------------------------------- shared inputs
EDGE_SIZES = [1, 2, 15, 27, 41, 42]


def _ragged(k: int, start: int = 0) -> List[int]:
    return [15 + ((start + i) * 7) % 25 for i in range(k)]


def sym_inputs(B: int = 16):
    """The edge sizes plus ragged rows, symmetric matrices, elements from {6, 7, 8} (the suite's classic GCN input)."""
    sizes = (EDGE_SIZES + _ragged(10))[:B]
    return synth_gcn_inputs(len(sizes), sizes, seed=3) + (sizes,)


def asym_inputs(B: int = 16):
    """Independent upper and lower triangles: every distance x (1 + 0.3 U) per entry, ~3 % extra one-way bonds."""
    sizes = (EDGE_SIZES[::-1] + _ragged(10, 3))[:B]
    el, dm, am = synth_gcn_inputs(len(sizes), sizes, seed=5)
    g = torch.Generator().manual_seed(11)
    dm = dm * (1 + 0.3 * torch.rand(dm.shape, generator=g))
    extra = (torch.rand(am.shape, generator=g) < 0.03).float()
    for b, n in enumerate(sizes):
        am[b, :n, :n] = torch.maximum(am[b, :n, :n], extra[b, :n, :n])
    return el, dm, am, sizes


def element_inputs():
    """Every id 0..35 in a real position (35 = the last table row), in two different arrangements."""
    sizes = [42, 36, 39, 17]
    el, dm, am = synth_gcn_inputs(len(sizes), sizes, seed=7)
    g = torch.Generator().manual_seed(13)
    for b, n in enumerate(sizes):
        el[b, :n] = torch.randint(0, NEMB, (n,), generator=g)
    el[0, :NEMB] = torch.randperm(NEMB, generator=g)
    el[1, :NEMB] = torch.arange(NEMB - 1, -1, -1)
    assert sorted(set(el[0, :42].tolist())) == list(range(NEMB)) and int(el[1, 0]) == NEMB - 1
    return el, dm, am, sizes


JUNK_SIZES = [1, 2, 15, 27, 41, 42, 20, 33, 38]


def junk_inputs(junk: bool = True):
    """Junk in the padded rows and columns (i >= n or j >= n) of dist_mat and adj_mat: the reference reads it, so the
    kernels must too.  Positive, so that degrees stay away from the 1e-12 clamp.  `junk=False`: the control (zero
    padding + I) on the same molecules."""
    sizes = JUNK_SIZES
    el, dm, am = synth_gcn_inputs(len(sizes), sizes, seed=9)
    if junk:
        g = torch.Generator().manual_seed(17)
        jd = 0.5 + 2.5 * torch.rand(dm.shape, generator=g)
        ja = (torch.rand(am.shape, generator=g) < 0.3).float()
        eye = torch.eye(D)
        for b, n in enumerate(sizes):
            pad = torch.ones(D, D, dtype=torch.bool)
            pad[:n, :n] = False
            dm[b][pad] = jd[b][pad]
            am[b][pad] = torch.maximum(ja[b], eye)[pad]
    return el, dm, am, sizes


def input_sets(B: int = 16) -> Dict[str, tuple]:
    """name -> (elements, dist_mat, adj_mat, sizes); every set the GPU test compares with fp64."""
    j = junk_inputs()
    j = tuple(t[:B] for t in j[:3]) + (j[3][:B],)
    return {"sym": sym_inputs(B), "asym": asym_inputs(B), "elements": element_inputs(), "junk": j}


WEIGHT_SETS = {"gain1": dict(), "gain2.45": dict(weight_gain=2.45)}     # 2.45 ~ sqrt(6): variance-preserving under ReLU


def weight_set(name: str) -> Dict[str, torch.Tensor]:
    return synth_adj_mat_seer_state_dict(4321, **WEIGHT_SETS[name])


# ------------------------------------------------------------------------------------------------- stage tolerances
# Fraction of the project's tolerance (rtol 1e-4 / atol 1e-5 of the stage's own maximum) each quantity is held to on the
# GPU.  MEASURED_FP32 is the worst violation of this restatement run in fp32 on the CPU against itself in fp64, over
# all four input sets at B = 16 and both weight sets (`python tools/parity_sensitivity.py --gcn` prints it);
# the tolerance is 16 x that, for a different summation order over K = 2048, capped at 1.  Nothing here comes from a
# kernel's output.
MEASURED_FP32 = {"L_dm": 0.0026, "L_adj": 0.0012, "bottleneck": 0.018, "scale": 0.045, "e0": 0.040, "xb": 0.053,
                 "res": 0.050, "logits": 0.049}
MARGIN = 16.0
# = L_dm 0.0416, L_adj 0.0192, bottleneck 0.288, scale 0.72, e0 0.64, xb 0.848, res 0.8, logits 0.784 of rtol 1e-4 / atol 1e-5
STAGE_TOL = {q: min(1.0, MARGIN * v) for q, v in MEASURED_FP32.items()}


def stage_violation(got: torch.Tensor, ref64: torch.Tensor, q: str) -> float:
    """violation in units of the stage's own tolerance (<= 1 passes)."""
    f = STAGE_TOL[q]
    return violation(got.reshape(ref64.shape), ref64, rtol=RTOL * f, atol=ATOL * f)


def table(sets: Dict[str, tuple], weights: Sequence[str] = tuple(WEIGHT_SETS), mutations: Sequence[str] = MUTATIONS):
    """-> {(weights, set): {"ref": {q: tensor64}, "base": {q: v}, mutation: {q: v}}} with v = the violation of the fp32
    restatement (unmutated = "base", or mutated) against the unmutated fp64 one in units of the PROJECT's tolerance
    (rtol 1e-4 / atol 1e-5 of the stage's maximum); v / STAGE_TOL[q] is in units of what the GPU test asserts."""
    out = {}
    with torch.no_grad():
        for wn in weights:
            sd = weight_set(wn)
            for sn, (el, dm, am, sizes) in sets.items():
                ref = gcn_forward(sd, el, dm, am, torch.float64)
                rows = {"ref": ref}
                for m in (None,) + tuple(mutations):
                    got = gcn_forward(sd, el, dm, am, torch.float32, mutation=m, n_nodes=sizes)
                    rows[m or "base"] = {q: violation(got[q], ref[q]) for q in QUANTITIES}
                out[(wn, sn)] = rows
    return out
