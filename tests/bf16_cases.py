"""Shapes, inputs and the mutation table of the bf16 stage pins, shared by tests/test_bf16_stages_host.py (CPU),
tests/test_bf16_stages_gpu.py (MI355X) and `tools/parity_sensitivity.py --bf16-stages`.

One layer is gcl_0 of block 3 (layer index 6), the coordinate layer that of block 3; "v2" weights, random compact h, x, x0 as
in test_one_gcl_layer_at_case_d_vs_fp64.  Each shape names the operand mode, the plan's edge_mt, the rounding model of its
aggregate and the route the GPU module asserts (read from route(), csrc/mcg_egnn_api.hip).
"""
import functools

import torch

import bf16_ref as R

WEIGHT_SEED, WEIGHT_RECIPE = 1234, "v2"
BLOCK, LAYER = 3, 6
P_GCL = f"dynamics.egnn.e_block_{BLOCK}.gcl_0."
P_GCL1 = f"dynamics.egnn.e_block_{BLOCK}.gcl_1."
P_EQ = f"dynamics.egnn.e_block_{BLOCK}.gcl_equiv."
P_NEXT_GCL = f"dynamics.egnn.e_block_{BLOCK + 1}.gcl_0."

# name -> sizes, input seed, mode, edge_mt, R (rows per unit), aggregate model, expected route (keep_agg = 0)
SHAPES = {
    "a": dict(sizes=[19, 27, 15, 33], seed=501, mode="bf16", edge_mt=4, rounded=True,
              route=dict(edge="W64Bf16", agg="GatherP", coord="PendingP", pspan=2)),
    "b": dict(sizes=[3, 17, 5, 1, 22], seed=502, mode="bf16", edge_mt=1, rounded=False,
              route=dict(edge="Bf16Rows16", agg="GatherP", coord="PendingP", pspan=3)),
    "c": dict(sizes=[19, 27, 15, 33], seed=501, mode="bf16", edge_mt=1, rounded=False,
              route=dict(edge="Bf16Rows16", agg="GatherP", coord="PendingP", pspan=3)),
    "d": dict(sizes=[70, 9], seed=504, mode="bf16", edge_mt=4, rounded=True,
              route=dict(edge="W64Bf16", agg="GatherP", coord="PendingP", pspan=3, fused=False)),
    "e": dict(sizes=[200, 12], seed=505, mode="bf16", edge_mt=4, rounded=True,
              route=dict(edge="W64Bf16", agg="Combine", coord="Kernel", pspan=5)),
    "f33": dict(sizes=[33], seed=506, mode="bf16", edge_mt=4, rounded=True,
                route=dict(edge="W64Bf16", agg="GatherP", coord="PendingP", pspan=1)),
    "f31": dict(sizes=[31], seed=507, mode="bf16", edge_mt=4, rounded=True,
                route=dict(edge="W64Bf16", agg="GatherP", coord="PendingP", pspan=2)),
    "g": dict(sizes=[19, 27, 15, 33], seed=501, mode="f32x6", edge_mt=4, rounded=False,
              route=dict(edge="W64X6", agg="Combine", coord="Kernel", pspan=2)),
}


def rows_per_unit(shape):
    return 16 * SHAPES[shape]["edge_mt"]


def rnd_of(shape):
    return R.identity if SHAPES[shape]["mode"] == "f32x6" else R.bf16_rne


@functools.lru_cache(maxsize=None)
def weights():
    from ml_conformer_generator_amd.weights import synth_edm_state_dict
    return synth_edm_state_dict(WEIGHT_SEED, recipe=WEIGHT_RECIPE)


@functools.lru_cache(maxsize=None)
def layer(prefix, dtype):
    key = "coord_mlp" if prefix.endswith("gcl_equiv.") else "edge_mlp"
    return R.cast(R.layer_weights(weights(), prefix, key), dtype)


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(Geometry, h[M,420], x[M,3], x0[M,3]) fp32, seeded per shape."""
    c = SHAPES[shape]
    geo = R.Geometry(c["sizes"])
    g = torch.Generator().manual_seed(c["seed"])
    return geo, torch.randn(geo.M, 420, generator=g), torch.randn(geo.M, 3, generator=g), torch.randn(geo.M, 3, generator=g)


@functools.lru_cache(maxsize=None)
def free_run(shape, dtype):
    """The restatement of the GCL layer and of the coordinate layer from the shape's inputs, every stage fed the one before."""
    geo, h, x, x0 = inputs(shape)
    c, rnd = SHAPES[shape], rnd_of(shape)
    g = R.gcl_stages(geo, h.to(dtype), x.to(dtype), x0.to(dtype), layer(P_GCL, dtype), rnd, c["rounded"])
    e = R.equiv_stages(geo, h.to(dtype), x.to(dtype), x0.to(dtype), layer(P_EQ, dtype), rnd)
    return dict(pab=g["pab"], m=g["m"], agg=g["agg"], hidden=g["hidden"], h=g["h"], pab_eq=e["pab"], m_eq=e["m"], x=e["x"])


def forced(shape, bufs, dtype, stages=("pab", "agg", "hidden", "h", "pab_next", "pab_eq", "x"), rounded=None):
    """Teacher-forced stages in `dtype`: each stage evaluated from the fp32 buffer `bufs` holds for the stage before it (the
    device's, or on the host the fp32 restatement's), never from this evaluation's own previous stage - a rounding flip in one
    stage cannot leak into the next one's budget.  bufs: pab [M,840], agg, hidden, h [M,420] (the layer's OUTPUT), pab_eq [M,840].
    pab_next = the projections gcl_1 of the block reads from the new h."""
    geo, h, x, x0 = inputs(shape)
    c, rnd = SHAPES[shape], rnd_of(shape)
    rounded = c["rounded"] if rounded is None else rounded
    h, x, x0 = h.to(dtype), x.to(dtype), x0.to(dtype)
    w, we = layer(P_GCL, dtype), layer(P_EQ, dtype)
    out = {}
    if "pab" in stages:
        out["pab"] = R.projections(h, w, rnd)
    if "agg" in stages:
        m = R.messages(geo, bufs["pab"].to(dtype), x, x0, w, rnd)
        out["agg"] = R.aggregate(geo, m, R.gate_of(m, w), rnd, rounded)
    if "hidden" in stages:
        out["hidden"] = R.hidden_of(h, bufs["agg"].to(dtype), w, rnd)
    if "h" in stages:
        out["h"] = R.h_next(h, bufs["hidden"].to(dtype), w, rnd)
    if "pab_next" in stages:
        out["pab_next"] = R.projections(bufs["h"].to(dtype), layer(P_GCL1, dtype), rnd)
    if "pab_eq" in stages:
        out["pab_eq"] = R.projections(h, we, rnd)
    if "x" in stages:
        m = R.messages(geo, bufs["pab_eq"].to(dtype), x, x0, we, rnd)
        out["x"] = R.coord_next(geo, x, m, R.pair_terms(geo, x, x0)[2], we)
    return out


def reference_alone(shape):
    """stage -> figures of the restatement's fp32 evaluation against its fp64 one, teacher-forced with the fp32 free run's
    buffers: what the GPU tests do with the device's buffers."""
    bufs = free_run(shape, torch.float32)
    a, b = forced(shape, bufs, torch.float32), forced(shape, bufs, torch.float64)
    return {s: R.judge(a[s], b[s], a[s]) for s in a}


# ------------------------------------------------------------------------------------------------------------ mutation table
def _atom_with_two_units(geo, Ru):
    """(atom, unit): an atom whose rows run through two units, and the second of them"""
    u = geo.unit(Ru)
    for v in range(geo.M):
        rows = (geo.ei == v).nonzero().reshape(-1)
        if rows.numel() and int(u[rows[0]]) != int(u[rows[-1]]):
            return v, int(u[rows[-1]])
    raise AssertionError("no atom spans two units")


def mutation_table(shape="a"):
    """[(label, stage, required, figures, excess)]: each mutation applied to the fp64 restatement of ONE stage (its inputs are
    the fp32 restatement's buffers of the stage before it, as the GPU tests feed the device's) and scored against the unmutated fp64 value under the acceptance rule, with the
    restatement's own fp32 evaluation as the denominator.  `excess` >= 10 = seen."""
    f64, f32 = torch.float64, torch.float32
    geo, h, x, x0 = inputs(shape)
    c, rnd = SHAPES[shape], rnd_of(shape)
    bufs = free_run(shape, f32)              # the stand-in for the device's buffers
    b, r = forced(shape, bufs, f64), forced(shape, bufs, f32)
    w, we = layer(P_GCL, f64), layer(P_EQ, f64)
    h64, x64, x064 = h.double(), x.double(), x0.double()
    pab64, pabeq64, agg_in = bufs["pab"].double(), bufs["pab_eq"].double(), bufs["agg"].double()
    b["m"] = R.messages(geo, pab64, x64, x064, w, rnd)
    b["m_eq"] = R.messages(geo, pabeq64, x64, x064, we, rnd)
    unit = R.pair_terms(geo, x64, x064)[2]
    gate = R.gate_of(b["m"], w)
    Ru = rows_per_unit(shape)
    one_edge = torch.ones(geo.E, dtype=torch.bool)
    one_edge[geo.E // 2] = False
    atom, un = _atom_with_two_units(geo, Ru)
    one_unit = ~((geo.ei == atom) & (geo.unit(Ru) == un))
    K4 = (416, 417, 418, 419)

    def agg_from(m, g=None, **kw):
        return R.aggregate(geo, m, R.gate_of(m, w) if g is None else g, rnd, kw.pop("rounded", c["rounded"]), **kw)

    def msgs(ww=w, **kw):
        return R.messages(geo, pab64 if ww is w else pabeq64, x64, x064, ww, rnd, **kw)

    # the exact-aggregate model of the same messages, for the mutation that rounds where the 16-row kernel does not
    exact64 = R.aggregate(geo, b["m"], gate, rnd, False)
    m32 = R.messages(geo, bufs["pab"], x, x0, layer(P_GCL, f32), rnd)
    exact32 = R.aggregate(geo, m32, R.gate_of(m32, layer(P_GCL, f32)), rnd, False)
    rows = [("aggregate operands left unrounded (64-row model)", "agg", True, R.aggregate(geo, b["m"], gate, rnd, False), b["agg"], r["agg"])] \
        if c["rounded"] else []
    rows += [
        ("aggregate operands rounded (16-row model)", "agg", True, R.aggregate(geo, b["m"], gate, rnd, True), exact64, exact32),
        ("A left unrounded", "agg", True, agg_from(msgs(rnd_a=R.identity)), b["agg"], r["agg"]),
        ("gate computed from the rounded m", "agg", True, agg_from(b["m"], R.gate_of(b["m"], w, rnd_m=rnd)), b["agg"], r["agg"]),
        ("[h | agg] left unrounded", "hidden", True, R.hidden_of(h64, agg_in, w, rnd, rnd_in=R.identity), b["hidden"], r["hidden"]),
        ("k = 416..419 of the 420-contraction dropped (W2)", "agg", True, agg_from(msgs(k_drop=K4)), b["agg"], r["agg"]),
        ("k = 416..419 of the 840-contraction dropped (W3)", "hidden", True, R.hidden_of(h64, agg_in, w, rnd, k_drop=K4), b["hidden"], r["hidden"]),
        ("one edge dropped", "agg", True, agg_from(b["m"], gate, keep=one_edge), b["agg"], r["agg"]),
        (f"one {Ru}-row unit's partial row of one atom dropped", "agg", True, agg_from(b["m"], gate, keep=one_unit), b["agg"], r["agg"]),
        ("gate bias dropped", "agg", True, agg_from(b["m"], R.gate_of(b["m"], w, drop_bias=True)), b["agg"], r["agg"]),
        ("d0 column dropped", "agg", True, agg_from(msgs(drop_d0=True)), b["agg"], r["agg"]),
        ("d2 column dropped", "agg", True, agg_from(msgs(drop_d2=True)), b["agg"], r["agg"]),
        ("/ 100 dropped", "agg", True, agg_from(b["m"], gate, norm=1.0), b["agg"], r["agg"]),
        ("coordinate head knocked out", "x", True, R.coord_next(geo, x64, b["m_eq"], unit, we, head=False), b["x"], r["x"]),
        ("one atom's coordinate slot dropped", "x", True, R.coord_next(geo, x64, b["m_eq"], unit, we, drop_atom=atom), b["x"], r["x"]),
        ("one edge dropped (coordinates)", "x", True, R.coord_next(geo, x64, b["m_eq"], unit, we, keep=one_edge), b["x"], r["x"]),
        ("d0 column dropped (coordinates)", "x", True, R.coord_next(geo, x64, msgs(we, drop_d0=True), unit, we), b["x"], r["x"]),
        ("A left unrounded (coordinates)", "x", False, R.coord_next(geo, x64, msgs(we, rnd_a=R.identity), unit, we), b["x"], r["x"]),
    ]
    out = []
    for label, stage, required, mut, ref, ref32 in rows:
        fig = R.judge(mut, ref, ref32)
        out.append((label, stage, required, fig, R.excess(fig, stage in R.STRICT_STAGES)))
    return out


def least_visible(shape):
    """class of stage -> smallest rms ratio of a required mutation scored in it"""
    out = {}
    for label, stage, required, f, _ in mutation_table(shape):
        if required:
            k = R.stage_class(stage, SHAPES[shape]["rounded"] and "16-row model" not in label)
            out[k] = min(out.get(k, float("inf")), f["rms_ratio"])
    return out


def table_text(shape="a"):
    lines = [f"bf16 stage pins: mutations of the fp64 restatement, shape ({shape}) sizes {SHAPES[shape]['sizes']}, block {BLOCK} gcl_0 / "
             f"coordinate layer, \"{WEIGHT_RECIPE}\" weights seed {WEIGHT_SEED}.",
             "Figures are shares of the stage's max|ref|; excess = the largest figure / limit of the acceptance rule "
             "(tests/bf16_ref.py; >= 10 = seen); rms ratio = rms(mutated - fp64) / rms(fp32 restatement - fp64).", "",
             "reference alone (fp32 restatement against fp64, every stage fed the same fp32 buffer of the stage before it):"]
    for s, f in reference_alone(shape).items():
        lines.append(f"    {s:8s} viol {f['viol']:9.3g}  share {f['share']:.4f}  max {f['max']:.2e}  rms {f['rms']:.2e}")
    lines += ["", f"    {'mutation':54s} {'stage':6s} {'share':>7s} {'max':>9s} {'rms ratio':>10s} {'excess':>10s}"]
    for label, stage, required, f, e in mutation_table(shape):
        flag = "" if e >= 10 else ("   <-- BLIND" if required else "   (informational)")
        lines.append(f"    {label:54s} {stage:6s} {f['share']:7.4f} {f['max']:9.2e} {f['rms_ratio']:10.3g} {e:10.3g}{flag}")
    for k, v in sorted(least_visible(shape).items()):
        lines.append(f"    -> least visible required mutation by rms ratio, class {k}: {v:.3g}; a fifth of it {v / 5:.3g} >= "
                     f"the class's rms bound {R.RMS_BOUND[k]:g}")
    return "\n".join(lines)
