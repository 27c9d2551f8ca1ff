"""The bf16 operand mode on the MI355X, stage by stage against its rounding model (tests/bf16_ref.py) evaluated in fp64.

One GCL layer (block 3, gcl_0) and the coordinate layer of block 3 run through the debug hooks (mcg_egnn_gcl_debug_ex,
mcg_egnn_equiv_debug) on the shapes of tests/bf16_cases.py.  Every stage is TEACHER-FORCED: the fp64 value of a stage is
computed from the device's buffer of the stage before it (pab -> aggregate -> hidden -> h' -> Pab', pab -> x'), so a bf16
rounding flip in one stage never reaches the next one's budget, and is judged by the acceptance rule of bf16_ref
(`judge` / `excess`): the stated per-call tolerance on every element of the stages without a rounding inside them; on the
aggregate and x' at most 2 % of the elements outside it, those within 4 x the restatement's own fp32 maximum; and the rms
distance from fp64 at most the stage class's RMS_BOUND x the restatement's own.  The host half (tests/test_bf16_stages_host.py) shows the rule
leaves the restatement 4 x room and sees every planted mistake tenfold.

Every run asserts its route through mcg_debug_route.  Each comparison prints one line
    BF16-STAGES <shape> <stage> route=... viol .. share .. max .. rms .. ratio ..
(profiles/bf16_stage_pins.txt holds them as measured).  The fp64 values are computed once per shape and module.
Shape (d), [70, 9] with three partial rows gathered per atom, is the bf16 counterpart of
test_large_molecules_gpu.py::test_one_gcl_layer_at_case_d_vs_fp64 (which stays on f32 / f32x6).
"""
import functools

import pytest
import torch

import bf16_cases as Cs
import bf16_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16_SHAPES = [s for s in sorted(Cs.SHAPES) if Cs.SHAPES[s]["mode"] == "bf16"]
FUSED_SHAPES = [s for s in BF16_SHAPES if Cs.SHAPES[s]["edge_mt"] == 4 and Cs.SHAPES[s]["route"].get("pspan", 9) <= 2]
_DYN = {}


def dyn_for(mode):
    from ml_conformer_generator_amd.egnn import EGNNDynamics
    if mode not in _DYN:
        d = EGNNDynamics(device=DEV)
        d.load_reference_state_dict(Cs.weights())
        d.set_precision(mode)
        _DYN[mode] = d
    return _DYN[mode]


def plan_for(shape):
    c = Cs.SHAPES[shape]
    d = dyn_for(c["mode"])
    plan = d.plan(torch.tensor(c["sizes"], dtype=torch.int32), max(c["sizes"]), edge_mt=c["edge_mt"], n_ranges=1)
    assert plan.edge_mt == c["edge_mt"] and plan.n_ranges == 1 and plan.n_real_nodes == Cs.inputs(shape)[0].M
    return d, plan


def assert_route(d, plan, expected, keep_agg):
    from ml_conformer_generator_amd import _lib
    got = _lib.debug_route(d.handle, plan.handle, keep_agg)
    wrong = {k: (got[k], v) for k, v in expected.items() if got[k] != v}
    assert not wrong, f"route (got, expected) differs in {wrong}; full route {got}"
    return got


def route_text(r):
    return f"{r['edge']}/{r['agg']}/{r['coord']}/pab={r['pab']}/node={r['node']}/fused={int(r['fused'])}/pspan={r['pspan']}"


def pab_of(shape, raw, M):
    blocked = Cs.SHAPES[shape]["mode"] == "bf16" and Cs.SHAPES[shape]["edge_mt"] == 4
    return (R.unblock_pab if blocked else R.rowmajor_pab)(raw.cpu(), M)[0]


def run_gcl(shape, keep_agg, layer=Cs.LAYER, expect=None):
    """One run of the layer through the hook: the route it took and the plan's buffers on the CPU."""
    d, plan = plan_for(shape)
    geo, h, x, x0 = Cs.inputs(shape)
    exp = dict(Cs.SHAPES[shape]["route"]) if expect is None else dict(expect)
    if keep_agg:
        exp.update(agg="Combine", fused=False)
    r = assert_route(d, plan, exp, keep_agg)
    got = d.gcl_debug_ex(plan, layer, h, x, x0, keep_agg)
    torch.cuda.synchronize()
    hi, xi, x0i = got["inputs"]
    assert torch.equal(hi.cpu(), h) and torch.equal(xi.cpu(), x) and torch.equal(x0i.cpu(), x0), "inputs were written"
    assert got["fused"] == r["fused"] and got["pab_is_next"] == r["fused"]
    out = {k: got[k].cpu() for k in ("h_out", "agg", "hidden")}
    out.update(pab=pab_of(shape, got["pab_raw"], geo.M), route=r, fused=got["fused"])
    return out


@functools.lru_cache(maxsize=None)
def combine_run(shape):
    """keep_agg = 1 (every buffer materialised), and the stages' fp64 / fp32 values teacher-forced with its buffers."""
    g = run_gcl(shape, True)
    bufs = dict(pab=g["pab"], agg=g["agg"][:, :R.H], hidden=g["hidden"][:, :R.H], h=g["h_out"][:, :R.H])
    stages = ("pab", "agg", "hidden", "h", "pab_next")
    return g, bufs, Cs.forced(shape, bufs, torch.float64, stages), Cs.forced(shape, bufs, torch.float32, stages)


def check(shape, stage, a, b, r, route):
    fig = R.judge(a, b, r)
    strict = stage in R.STRICT_STAGES
    print(f"\nBF16-STAGES {shape} {stage} route={route_text(route)} {R.figures_text(fig)} excess {R.excess(fig, strict):.3g}")
    assert bool(torch.isfinite(a).all()), (shape, stage)
    bound = R.RMS_BOUND[R.stage_class(stage, Cs.SHAPES[shape]["rounded"])]
    assert R.accepted(fig, strict, bound), (shape, stage, bound, fig)
    return fig


@pytest.mark.parametrize("shape", sorted(Cs.SHAPES))
def test_gcl_stages_vs_fp64_teacher_forced(shape):
    """pab, the aggregate, hidden and h' of the layer with every buffer materialised (the Combine route), each against the
    fp64 stage fed the device's previous buffer; padding columns exactly zero; a second run bit-identical."""
    g, bufs, b, r = combine_run(shape)
    for stage, a in (("pab", bufs["pab"]), ("agg", bufs["agg"]), ("hidden", bufs["hidden"]), ("h", bufs["h"])):
        check(shape, stage, a, b[stage], r[stage], g["route"])
    for name in ("h_out", "agg", "hidden"):
        assert float(g[name][:, R.H:].abs().max()) == 0.0, f"padding columns of {name} are not exactly zero"
    again = run_gcl(shape, True)
    for name in ("h_out", "agg", "hidden", "pab"):
        assert torch.equal(again[name], g[name]), f"second run differs in {name}"
    if shape == "b":          # the one-atom molecule has no edges
        v = sum(Cs.SHAPES["b"]["sizes"][:3])
        assert Cs.SHAPES["b"]["sizes"][3] == 1 and float(g["agg"][v].abs().max()) == 0.0


@pytest.mark.parametrize("shape", BF16_SHAPES)
def test_the_pin_tells_the_two_aggregate_models_apart_on_the_device(shape):
    """The device's aggregate scored against the OTHER kernel's rounding model (64-row kernel against the exact aggregate,
    16-row kernel against the rounded one) fails the rule."""
    g, bufs, _, _ = combine_run(shape)
    other = not Cs.SHAPES[shape]["rounded"]
    b = Cs.forced(shape, bufs, torch.float64, ("agg",), rounded=other)["agg"]
    r = Cs.forced(shape, bufs, torch.float32, ("agg",), rounded=other)["agg"]
    fig = R.judge(bufs["agg"], b, r)
    print(f"\nBF16-STAGES {shape} agg-vs-other-model {R.figures_text(fig)} excess {R.excess(fig, False):.3g}")
    assert not R.accepted(fig, False), (shape, fig)


def _set(d, option, value):
    from ml_conformer_generator_amd import _lib
    d.set_option(getattr(_lib, option), value)


@pytest.mark.parametrize("shape", BF16_SHAPES)
def test_production_route_gives_bit_identical_h_and_a_pinned_next_pab(shape):
    """keep_agg = 0 - what a denoiser call runs: the gathering node GEMM, with MCG_OPT_GEMM_BF16_LDS 1 and 2, and the fused node
    launch (MCG_OPT_NODE_FUSED 2 against 1) where atoms span at most two units - against the Combine route: h' and, unfused,
    hidden bit for bit.  After a fused launch pab holds the NEXT layer's projections: pinned against rnd(h'_device) rnd(W')^T + b'
    for gcl_0 (read by gcl_1) and gcl_1 (read by the coordinate layer)."""
    d, _ = plan_for(shape)
    g, bufs, b, r = combine_run(shape)
    c = Cs.SHAPES[shape]
    try:
        for lds in (1, 2):
            for fused_opt in ((1, 2) if shape in FUSED_SHAPES else (1,)):
                _set(d, "OPT_GEMM_BF16_LDS", lds)
                _set(d, "OPT_NODE_FUSED", fused_opt)
                want_fused = fused_opt == 2 and lds != 1
                p = run_gcl(shape, False, expect=dict(c["route"], fused=want_fused))
                assert torch.equal(p["h_out"], g["h_out"]), f"h' differs from the Combine route (lds {lds}, fused {fused_opt})"
                if not p["fused"]:
                    assert torch.equal(p["hidden"], g["hidden"]) and torch.equal(p["pab"], g["pab"])
                    continue
                check(shape, "pab_next", p["pab"], b["pab_next"], r["pab_next"], p["route"])
                # the other parity of layer & 1: gcl_1, whose fused launch writes the coordinate layer's projections
                q = run_gcl(shape, False, layer=Cs.LAYER + 1, expect=dict(c["route"], fused=True))
                assert q["fused"]
                hq = q["h_out"][:, :R.H]
                bq = R.projections(hq.double(), Cs.layer(Cs.P_EQ, torch.float64), Cs.rnd_of(shape))
                rq = R.projections(hq, Cs.layer(Cs.P_EQ, torch.float32), Cs.rnd_of(shape))
                check(shape, "pab_next", q["pab"], bq, rq, q["route"])
    finally:
        _set(d, "OPT_GEMM_BF16_LDS", 0)
        _set(d, "OPT_NODE_FUSED", 0)


@pytest.mark.parametrize("shape", sorted(Cs.SHAPES))
def test_coordinate_layer_vs_fp64_and_both_ways_of_applying_the_update(shape):
    """x' of the coordinate layer with the pending update applied by its own launch (apply = 0) and consumed as the side job of
    the next block's first first-layer GEMM (apply = 1): bit-identical to each other, both against fp64 (teacher-forced with the
    device's projections); the projections themselves, and those the consuming GEMM writes, against fp64."""
    d, plan = plan_for(shape)
    geo, h, x, x0 = Cs.inputs(shape)
    route = assert_route(d, plan, Cs.SHAPES[shape]["route"], False)
    runs = []
    for apply in (0, 1, 0):
        got = d.equiv_debug(plan, Cs.BLOCK, h, x, x0, apply)
        torch.cuda.synchronize()
        hi, xi, x0i = got["inputs"]
        assert torch.equal(hi.cpu(), h) and torch.equal(xi.cpu(), x) and torch.equal(x0i.cpu(), x0), "inputs were written"
        runs.append((got["x_out"].cpu(), pab_of(shape, got["pab_raw"], geo.M)))
    (x_a0, pab_eq), (x_a1, pab_nx), (x_again, pab_again) = runs
    assert torch.equal(x_a0, x_a1), "x' differs between the stand-alone apply and the GEMM's side job"
    assert torch.equal(x_a0, x_again) and torch.equal(pab_eq, pab_again), "second run differs"
    assert float(x_a0[:, 3].abs().max()) == 0.0
    bufs = dict(pab_eq=pab_eq)
    b = Cs.forced(shape, bufs, torch.float64, ("pab_eq", "x"))
    r = Cs.forced(shape, bufs, torch.float32, ("pab_eq", "x"))
    check(shape, "pab", pab_eq, b["pab_eq"], r["pab_eq"], route)
    check(shape, "x", x_a0[:, :3], b["x"], r["x"], route)
    check(shape, "x", x_a1[:, :3], b["x"], r["x"], route)
    rnd = Cs.rnd_of(shape)
    check(shape, "pab", pab_nx, R.projections(h.double(), Cs.layer(Cs.P_NEXT_GCL, torch.float64), rnd),
          R.projections(h, Cs.layer(Cs.P_NEXT_GCL, torch.float32), rnd), route)
    if shape == "b":
        v = sum(Cs.SHAPES["b"]["sizes"][:3])
        assert torch.equal(x_a0[v, :3], x[v]), "the one-atom molecule moved"


def test_the_hooks_refuse_arguments_out_of_range():
    """MCG_ERR_ARG with a message, nothing launched: layer / block beyond the model, keep_agg / apply that are no flags, apply = 1
    on the last block (no next first-layer GEMM to carry the update)."""
    from ml_conformer_generator_amd import _lib
    d, plan = plan_for("f31")
    geo, h, x, x0 = Cs.inputs("f31")
    with pytest.raises(_lib.McgError, match="mcg_egnn_gcl_debug_ex"):
        d.gcl_debug_ex(plan, 2 * d.n_blocks, h, x, x0, False)
    hd, xd = h.to(DEV), x.to(DEV)
    st = _lib.current_stream_ptr(DEV)
    L = _lib.lib()
    assert L.mcg_egnn_gcl_debug_ex(d.handle, plan.handle, Cs.LAYER, _lib.dptr(hd), _lib.dptr(xd), _lib.dptr(xd), 2, None, st) != 0
    assert L.mcg_egnn_equiv_debug(d.handle, plan.handle, Cs.BLOCK, _lib.dptr(hd), _lib.dptr(xd), _lib.dptr(xd), 2, st) != 0
    with pytest.raises(_lib.McgError, match="apply = 1 needs a next block"):
        d.equiv_debug(plan, d.n_blocks - 1, h, x, x0, 1)
    with pytest.raises(_lib.McgError, match="mcg_egnn_equiv_debug"):
        d.equiv_debug(plan, d.n_blocks, h, x, x0, 0)
    two = d.plan(torch.tensor([27] * 160, dtype=torch.int32), 27, n_ranges=2)
    if two.n_ranges > 1:
        hh = torch.zeros(two.n_real_nodes, 420)
        xx = torch.zeros(two.n_real_nodes, 3)
        with pytest.raises(_lib.McgError, match="molecule ranges"):
            d.gcl_debug_ex(two, Cs.LAYER, hh, xx, xx, False)
    torch.cuda.synchronize()
