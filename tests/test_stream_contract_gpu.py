"""Every stream-taking entry point on a stream that is not the default one (tests/stream_probe.py: the two arrangements, the
coverage table).  Run with `-m gpu`.

One test per kernel family, at the smallest shapes that still reach every launch of its entries; each arranged call must
  * hand every stream-taking C entry the CURRENT stream (seen through `stream_probe.Recorder`),
  * leave the default stream's spin running when the side stream has finished (A) / not wait for its own stream's spin on
    the host (B, raw entries),
  * give the bits of the same call on the default stream.
The controls at the top call `mcg_bond_writeback` with stream 0 on purpose inside each arrangement and must come out wrong.

Each arranged call prints one line `STREAM <label>: ...` with the baseline time and the spin asked for; the module ends with
the calibrated spin rate and the longest spin."""
import functools
import time

import numpy as np
import pytest
import torch

import stream_probe as P
from conftest import TapeNoise

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 20261020


def _lib():
    from ml_conformer_generator_amd import _lib as L
    return L


def _st():
    return _lib().current_stream_ptr(DEV)


def _show(res):
    print(f"\nSTREAM {res.label}: baseline {res.t_call_ms:.2f} ms, spin {res.delay_ms:.0f} ms, "
          f"{'default stream still busy' if res.busy else 'side stream still busy at return' if res.pending else 'NOT busy'}, "
          f"{'equal' if res.equal else 'DIFFERENT'}, entries {sorted({n for n, _ in res.calls})}"
          + (f", enqueued in {res.enqueue_ms:.2f} ms" if res.enqueue_ms is not None else ""))
    return res


_HELD = {"A": set(), "B": set()}          # entries an arrangement has held for in the CURRENT test (`_fresh_claims`)


@pytest.fixture(autouse=True)
def _fresh_claims():
    """What an earlier test held for does not count towards a later test's claim."""
    _HELD["A"].clear()
    _HELD["B"].clear()
    yield


def run_a(call, label, entries, **kw):
    res = _show(P.arrangement_a(call, label + " [A]", **kw)).ok(entries)
    _HELD["A"].update(entries)
    return res


def run_b(call, true, poison, label, entries, raw=False, refill=()):
    res = _show(P.arrangement_b(call, true, poison, label + " [B]", raw=raw, refill=refill)).ok(entries, raw=raw)
    _HELD["B"].update(entries)
    return res


def run_ab(call, true, label, entries, poison=None, raw=False):
    run_a(lambda: call(true), label, entries)
    run_b(call, true, P.rolled(true) if poison is None else poison, label, entries, raw=raw)


def claims(test_name):
    """Every entry the table gives to `test_name` has been through the arrangements the table states for it."""
    for entry in P.covered_by(test_name):
        for arrangement in P.COVERAGE[entry][1]:
            assert entry in _HELD[arrangement], f"{test_name} is the table's test of {entry} under {arrangement}: it did not run"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if P._RATE:
        print(f"\nSTREAM-PROBE summary: {P._RATE[0]:.0f} cycles per ms; longest spin {P.LARGEST['delay_ms']:.0f} ms "
              f"({P.LARGEST['entry']})")


# ---- the hand-off batch: B = 3, one molecule of 42 atoms and one of 1 atom ----------------------------------------------
SIZES = [42, 15, 1]


def _handoff_batch(seed, sizes=SIZES):
    g = torch.Generator().manual_seed(seed)
    B, N = len(sizes), 42
    x = torch.randn(B, N, 3, generator=g) * 2.5
    h = torch.zeros(B, N, 8)
    cls = torch.randint(0, 8, (B, N), generator=g)
    h.scatter_(2, cls.unsqueeze(2), 1.0)
    order = torch.zeros(B, 42, dtype=torch.int32)
    conn = torch.zeros(B, 42, 42, dtype=torch.uint8)
    for b, n in enumerate(sizes):
        order[b, :n] = torch.randperm(n, generator=g).to(torch.int32)
        c = (torch.rand(n, n, generator=g) < 0.15)
        conn[b, :n, :n] = (c | c.t()).to(torch.uint8)
    return {k: v.to(DEV).contiguous() for k, v in dict(x=x, h=h, n=torch.tensor(sizes, dtype=torch.int32), order=order,
                                                       conn=conn).items()}


def _writeback_batch(seed, sizes=SIZES):
    g = torch.Generator().manual_seed(seed)
    B = len(sizes)
    bond = torch.randint(0, 5, (B, 42, 42), generator=g).to(torch.int8)
    zs = torch.tensor([6, 7, 8, 9, 15, 16, 17, 35])
    el = torch.zeros(B, 42, dtype=torch.int64)
    for b, n in enumerate(sizes):
        el[b, :n] = zs[torch.randint(0, 8, (n,), generator=g)]
    return {k: v.to(DEV).contiguous() for k, v in dict(bond=bond, el=el, n=torch.tensor(sizes, dtype=torch.int32)).items()}


class _Writeback:
    """`mcg_bond_writeback` itself into buffers of this object; `stream`: None = the current one."""

    def __init__(self, B=len(SIZES)):
        self.B = B
        self.sym = torch.empty(B, 42, 42, dtype=torch.int8, device=DEV)
        self.valid = torch.empty(B, dtype=torch.uint8, device=DEV)

    def __call__(self, inp, stream=None):
        L = _lib()
        L.check(L.lib().mcg_bond_writeback(L.dptr(inp["bond"]), L.dptr(inp["el"]), L.dptr(inp["n"]), self.B, L.dptr(self.sym),
                                           L.dptr(self.valid), _st() if stream is None else stream), "mcg_bond_writeback")
        return [self.sym, self.valid]


# ---- the controls: the probe can fail --------------------------------------------------------------------------------------
def test_control_a_work_on_stream_0_is_seen_as_the_sentinel():
    """`mcg_bond_writeback` given stream 0 under a side stream whose default stream spins: the side stream reads the
    sentinel, not the answer."""
    wb, true = _Writeback(), _writeback_batch(1)
    res = _show(P.arrangement_a(lambda: wb(true, stream=0), "control mcg_bond_writeback on stream 0 [A]", refill=[wb.sym, wb.valid]))
    assert res.busy and not res.equal
    assert all(P.is_sentinel(t) for t in res.got)
    assert res.calls == [("mcg_bond_writeback", 0)]
    with pytest.raises(AssertionError, match="another stream"):
        res.ok(["mcg_bond_writeback"])
    assert P.same_bits(res.base, [wb.sym, wb.valid])          # (it ran in the end, behind the spin: ordering only)
    run_a(lambda: wb(true), "mcg_bond_writeback", ["mcg_bond_writeback"], refill=[wb.sym, wb.valid])       # and on S it holds


def test_control_b_work_on_stream_0_computes_the_poison():
    """The control of arrangement B, in a process of its own.  What it needs of the DEVICE - a launch on stream 0 runs while a
    side stream spins with a copy queued behind the spin - holds in a fresh process and behind most of the suite's files, but
    not behind all of them: behind the `test_s*` files the same launch starts only when the spin is over (measured on an
    MI355X: enqueued in 0.07 ms behind a 20 ms spin, and it still read the copied inputs), although
    `stream_probe.independent_stream` finds both directions free for plain fills and copies in that very process.  What this
    means for the arranged calls of this file: arrangement B never reports a defect that is not there; in such a process it
    can miss work misplaced onto STREAM 0 (arrangement A, whose control holds in every process tried, still sees that), and it
    is not known to miss work on any other unordered stream.  The in-process outcome is printed, not asserted."""
    import os
    import subprocess
    import sys
    try:
        _control_b()
        print("\nSTREAM control [B] in this process: discriminates")
    except AssertionError as e:
        print(f"\nSTREAM control [B] in this process: does NOT discriminate stream 0 here ({str(e)[:120]})")
    finally:
        torch.cuda.synchronize()
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_stream_contract_gpu as T; "
            "T._control_b()")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)   # (a child that runs out of time is killed)
    print(done.stdout[-3000:], done.stderr[-3000:])
    assert done.returncode == 0, f"the control failed in a fresh process (exit {done.returncode})"


def _control_b():
    """`mcg_bond_writeback` given stream 0 while its true inputs are still behind the side stream's spin: it computes the
    poison's answer."""
    wb, true, poison = _Writeback(), _writeback_batch(1), _writeback_batch(2)
    of_poison = [t.clone() for t in wb(poison)]
    torch.cuda.synchronize()
    res = _show(P.arrangement_b(lambda inp: wb(inp, stream=0), true, poison, "control mcg_bond_writeback on stream 0 [B]", raw=True,
                                refill=[wb.sym, wb.valid]))
    assert res.enqueue_ms < res.delay_ms / 2, f"the host took {res.enqueue_ms:.1f} ms to enqueue behind a {res.delay_ms:.0f} ms spin"
    assert res.pending and not res.equal
    assert not any(P.is_sentinel(t) for t in res.got), "the stream-0 launch had not run when the side stream's spin was over"
    assert P.same_bits(res.got, of_poison) and not P.same_bits(of_poison, res.base)
    assert res.calls == [("mcg_bond_writeback", 0)]
    run_b(wb, true, poison, "mcg_bond_writeback", ["mcg_bond_writeback"], raw=True, refill=[wb.sym, wb.valid])


# ---- the denoiser -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dyn(mode):
    from conftest import sd_for
    from ml_conformer_generator_amd.egnn import EGNNDynamics
    d = EGNNDynamics(device=DEV)
    d.load_reference_state_dict(sd_for({"weight_seed": 1234, "weight_recipe": "v2"}))
    d.set_precision(mode)
    return d


def _denoiser_inputs(sizes, N, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(sizes)
    nm = (torch.arange(N).unsqueeze(0) < torch.tensor(sizes).unsqueeze(1)).float().unsqueeze(2)
    return {k: v.to(DEV).contiguous() for k, v in dict(t=torch.rand(B, generator=g), xh=torch.randn(B, N, 11, generator=g) * nm,
                                                       ctx=torch.randn(B, 1, 3, generator=g).repeat(1, N, 1) * nm).items()}


DENOISER = [("one range", [9, 27, 20, 1], 0, 1, "f32"), ("one range", [9, 27, 20, 1], 0, 1, "bf16"),
            ("one range", [9, 27, 20, 1], 0, 1, "f32x6"), ("two ranges", [27] * 6, 2, 2, "f32"),
            ("three ranges, plain launches", [27] * 6, 3, 3, "f32")]


@pytest.mark.parametrize("name,sizes,n_ranges,ranges,mode", DENOISER, ids=[f"{c[0]}-{c[4]}" for c in DENOISER])
def test_denoiser_on_a_side_stream(name, sizes, n_ranges, ranges, mode):
    """`mcg_egnn_dynamics` through `EGNNDynamics.run`: a replay on S of a plan first run on the default stream, the first
    call of a plan on S (planned and captured there), its replay on S, and the late producer; `mcg_plan_peek` on the
    one-range exact plan.  The two-range plan is the smallest the library cuts (4 374 edge rows against a floor of 4 096)."""
    d = _dyn(mode)
    N = max(sizes)
    sz = torch.tensor(sizes, dtype=torch.int32)
    true, poison = _denoiser_inputs(sizes, N, 5), _denoiser_inputs(sizes, N, 6)
    out = torch.empty_like(true["xh"])
    label = f"mcg_egnn_dynamics {name} {mode}"
    ran = ["mcg_egnn_dynamics"]

    def make_plan():
        p = d.plan(sz, N, n_ranges=n_ranges)
        assert p.n_ranges == ranges, (p.n_ranges, ranges)
        return p

    def call(inp=true):
        return [d.run(make_plan(), inp["t"], inp["xh"], inp["ctx"], out=out)]

    d._plans.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    base = [call()[0].clone()]
    torch.cuda.synchronize()
    first = (base, (time.perf_counter() - t0) * 1e3)          # plan, capture, run: what the first call on S does again
    assert bool(torch.isfinite(base[0]).all()) and float(base[0].abs().max()) > 0
    run_a(call, label + ", first run on the default stream, replay on S", ran, baseline=first, refill=[out])
    if ranges == 1 and mode == "f32":
        plan = make_plan()
        run_a(lambda: [d._peek(plan, 0, 432)], "mcg_plan_peek", ["mcg_plan_peek"])
        ran.append("mcg_plan_peek")
    d._plans.clear()                                          # the next call plans anew
    run_a(call, label + ", planned and captured on S", ran[:1], baseline=first, refill=[out])
    run_a(call, label + ", replay on S", ran[:1], baseline=first, refill=[out])
    run_b(call, true, poison, label, ran[:1], raw=True, refill=[out])
    if ranges == 1 and mode == "f32":
        claims("test_denoiser_on_a_side_stream")


# ---- the sampler --------------------------------------------------------------------------------------------------------
def test_sampler_entries_on_a_side_stream():
    """The raw sampler entries at sizes [65, 9, 1] (the 64-lane loop wraps once), then one sample of T = 5 at B = 3 wholly
    under S with a recorded noise tape."""
    from ml_conformer_generator_amd.egnn import BatchPlan
    L = _lib()
    lib = L.lib
    d = _dyn("f32")
    sizes, N = [65, 9, 1], 65
    B = len(sizes)
    plan = BatchPlan(torch.tensor(sizes, dtype=torch.int32), N, DEV, edge_mt=1)
    nm = (torch.arange(N).unsqueeze(0) < torch.tensor(sizes).unsqueeze(1)).float().unsqueeze(2)

    def draws(seed):
        g = torch.Generator().manual_seed(seed)
        v = dict(rx=torch.randn(B, N, 3, generator=g), rh=torch.randn(B, N, 8, generator=g),
                 z=torch.randn(B, N, 11, generator=g) * nm, zk=torch.randn(B, N, 11, generator=g),
                 ctx=torch.randn(B, 1, 3, generator=g).repeat(1, N, 1) * nm, t=torch.rand(B, generator=g))
        fm = torch.zeros(B, N, 1)
        for b, n in enumerate(sizes):
            fm[b, torch.randint(0, n, (2,), generator=g)] = 1.0
        fm[0, 64] = 1.0                                        # an atom of the fixed fragment in the loop's second trip
        v["fm"] = fm
        v["ids"] = torch.randint(0, 2 ** 31, (B,), generator=g)
        return {k: t.to(DEV).contiguous() for k, t in v.items()}
    true, poison = draws(11), draws(12)
    eps, zbuf, scratch = (torch.empty(B, N, 11, device=DEV) for _ in range(3))
    kx, kh = torch.empty(B, N, 3, device=DEV), torch.empty(B, N, 8, device=DEV)
    xo, ho = torch.empty(B, N, 3, device=DEV), torch.empty(B, N, 8, device=DEV)

    def sub(keys):
        return {k: true[k] for k in keys}, {k: poison[k] for k in keys}

    def noise(i):
        L.check(lib().mcg_sampler_noise(plan.handle, L.dptr(i["rx"]), L.dptr(i["rh"]), L.dptr(eps), _st()), "mcg_sampler_noise")
        return [eps]

    def keyed(i):
        L.check(lib().mcg_sampler_noise_keyed(plan.handle, 0x1234567890ABCDEF, L.dptr(i["ids"]), 3, 7, L.dptr(kx), L.dptr(kh),
                                              _st()), "mcg_sampler_noise_keyed")
        return [kx, kh]

    def blend(mode):
        def f(i):
            zbuf.copy_(i["z"])
            L.check(lib().mcg_sampler_blend(plan.handle, L.dptr(zbuf), L.dptr(i["zk"]), L.dptr(i["fm"]) if mode else None,
                                            L.dptr(i["rx"]), L.dptr(i["rh"]), 0.8125, 0.59375, 0.421875 if mode else 0.0, mode,
                                            _st()), "mcg_sampler_blend")
            return [zbuf]
        return f

    def step(i):
        zbuf.copy_(i["z"])
        L.check(lib().mcg_sampler_step(d.handle, plan.handle, L.dptr(zbuf), L.dptr(i["ctx"]), L.dptr(i["t"]), L.dptr(i["rx"]),
                                       L.dptr(i["rh"]), 0.96875, 0.21875, 0.15625, L.dptr(scratch), _st()), "mcg_sampler_step")
        return [zbuf]

    def decode(i):
        L.check(lib().mcg_sampler_decode(d.handle, plan.handle, L.dptr(i["z"]), L.dptr(i["ctx"]), L.dptr(i["t"]), L.dptr(i["rx"]),
                                         1.0009765625, 0.03125, 0.03125, 1.0, 4.0, L.dptr(scratch), L.dptr(xo), L.dptr(ho),
                                         _st()), "mcg_sampler_decode")
        return [xo, ho]

    for entry, fn, keys, bufs in (("mcg_sampler_noise", noise, ("rx", "rh"), [eps]),
                                  ("mcg_sampler_noise_keyed", keyed, ("ids",), [kx, kh]),
                                  ("mcg_sampler_blend", blend(0), ("z", "zk", "rx", "rh"), [zbuf]),
                                  ("mcg_sampler_blend", blend(1), ("z", "zk", "fm", "rx", "rh"), [zbuf]),
                                  ("mcg_sampler_step", step, ("z", "ctx", "t", "rx", "rh"), [zbuf, scratch]),
                                  ("mcg_sampler_decode", decode, ("z", "ctx", "t", "rx"), [xo, ho, scratch])):
        t, p = sub(keys)
        run_a(lambda: fn(t), entry, [entry], refill=bufs)
        run_b(fn, t, p, entry, [entry], raw=True, refill=bufs)

    # one whole sample under S
    from ml_conformer_generator_amd.equivariant_diffusion import EquivariantDiffusion, PredefinedNoiseSchedule
    T, sz = 5, [9, 27, 20]
    gm = EquivariantDiffusion(dynamics=d, in_node_nf=8, timesteps=1000, noise_precision=1e-5)
    gm.gamma = PredefinedNoiseSchedule(timesteps=T, precision=1e-5)
    gm.T = T
    g = torch.Generator().manual_seed(21)
    nm3 = (torch.arange(27).unsqueeze(0) < torch.tensor(sz).unsqueeze(1)).float().unsqueeze(2)
    ctx = (torch.randn(3, 1, 3, generator=g).repeat(1, 27, 1) * nm3).to(DEV)
    tape = torch.randn((T + 2) * 3 * 27 * 11, generator=g)
    nmd = nm3.to(DEV)

    def sample():
        gm.noise_fn = TapeNoise(tape, DEV)
        try:
            x, h = gm(nmd, None, ctx, 0)
            assert gm.noise_fn.pos == tape.numel()
        finally:
            gm.noise_fn = None
        return [x, h]
    run_a(sample, "EquivariantDiffusion sample T=5 B=3", ["mcg_sampler_noise", "mcg_sampler_step", "mcg_sampler_decode"])
    claims("test_sampler_entries_on_a_side_stream")


# ---- the GCN and the hand-off -----------------------------------------------------------------------------------------------
def _gcn(gcn_sd):
    from ml_conformer_generator_amd.adj_mat_seer import AdjMatSeer
    g = AdjMatSeer(device=DEV)
    g.load_state_dict(gcn_sd)
    return g


def _gcn_inputs(sizes, seed):
    from ml_conformer_generator_amd.synthetic import synth_gcn_inputs
    el, dm, am = synth_gcn_inputs(len(sizes), sizes, seed=seed)
    return dict(el=el.to(DEV).contiguous(), dm=dm.to(DEV).contiguous(), am=am.to(DEV).contiguous())


def _forward(g):
    def f(i):
        bond, logits = g.bond_orders(i["el"], i["dm"], i["am"], with_logits=True)
        return [bond, logits]
    return f


def test_gcn_and_handoff_on_a_side_stream(gcn_sd):
    L = _lib()
    lib = L.lib
    B = len(SIZES)
    # mcg_gcn_forward: a fresh handle sizes its workspace under S, a larger batch regrows it under S
    small, large = _gcn_inputs(SIZES, 9), _gcn_inputs(SIZES + [27, 8], 10)
    serial = _gcn(gcn_sd)
    base = {}
    for key, inp in (("small", small), ("large", large)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [t.clone() for t in _forward(serial)(inp)]
        torch.cuda.synchronize()
        base[key] = (out, (time.perf_counter() - t0) * 1e3)
    fresh = _gcn(gcn_sd)
    def workspace(g, rows):
        return [g._peek(w, rows) for w in (2, 3, 5, 6)]
    run_a(lambda: _forward(fresh)(small), "mcg_gcn_forward, fresh handle (workspace sized on S)", ["mcg_gcn_forward"],
          baseline=base["small"])
    # ... and the zero fill of the new workspace ran IN FRONT of the forward: behind it, it would have wiped what the forward left
    _forward(serial)(small)
    assert P.same_bits(workspace(fresh, B), workspace(serial, B)), "the fresh workspace is not as the forward left it"
    run_a(lambda: _forward(fresh)(large), "mcg_gcn_forward, larger batch (workspace regrown on S)", ["mcg_gcn_forward"],
          baseline=base["large"])
    _forward(serial)(large)
    assert P.same_bits(workspace(fresh, B + 2), workspace(serial, B + 2)), "the regrown workspace is not as the forward left it"
    run_a(lambda: _forward(fresh)(small), "mcg_gcn_forward, smaller batch in the regrown workspace", ["mcg_gcn_forward"],
          baseline=base["small"])
    run_b(_forward(_gcn(gcn_sd)), small, P.rolled(small), "mcg_gcn_forward, fresh handle", ["mcg_gcn_forward"], raw=True)
    fresh.check_inputs_seen()                                  # clean inputs: no IndexError
    _forward(serial)(small)
    run_a(lambda: [serial._peek(w, B) for w in (2, 5, 6)], "mcg_gcn_peek", ["mcg_gcn_peek"])

    # mcg_handoff_ex with an order and a connectivity
    el, dm, am = (torch.empty(B, 42, dtype=torch.int64, device=DEV), torch.empty(B, 42, 42, device=DEV),
                  torch.empty(B, 42, 42, device=DEV))
    xo, flag = torch.empty(B, 42, 3, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)

    def handoff(i):
        flag.zero_()                                           # (the entry only ever sets it)
        L.check(lib().mcg_handoff_ex(L.dptr(i["x"]), L.dptr(i["h"]), L.dptr(i["n"]), B, 42, 1.3, L.dptr(i["order"]),
                                     L.dptr(i["conn"]), L.dptr(el), L.dptr(dm), L.dptr(am), L.dptr(xo), L.dptr(flag), _st()),
                "mcg_handoff_ex")
        return [el, dm, am, xo, flag]
    true = _handoff_batch(3)
    run_a(lambda: handoff(true), "mcg_handoff_ex", ["mcg_handoff_ex"], refill=[el, dm, am, xo])
    run_b(handoff, true, _handoff_batch(4), "mcg_handoff_ex", ["mcg_handoff_ex"], raw=True, refill=[el, dm, am, xo])
    assert int(flag) == 0 and int(el[2, 0]) > 0 and int(el[2, 1]) == 0

    wb = _Writeback()
    run_a(lambda: wb(_writeback_batch(1)), "mcg_bond_writeback", ["mcg_bond_writeback"], refill=[wb.sym, wb.valid])
    run_b(wb, _writeback_batch(1), _writeback_batch(2), "mcg_bond_writeback", ["mcg_bond_writeback"], raw=True,
          refill=[wb.sym, wb.valid])

    # mcg_ifm_merge through its wrapper (no host read in it)
    from ml_conformer_generator_amd.mol_utils import ifm_merge_hip

    def frag(seed):
        g = torch.Generator().manual_seed(seed)
        return {k: v.to(DEV).contiguous() for k, v in dict(
            ffx=torch.randn(5, 3, generator=g), ffh=torch.randn(5, 8, generator=g), gx=torch.randn(B, 37, 3, generator=g),
            gh=torch.randn(B, 37, 8, generator=g), shift=torch.randn(B, 3, generator=g),
            rot=torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]).items()}

    def merge(i):
        return list(ifm_merge_hip(i["ffx"], i["ffh"], i["gx"], i["gh"], i["shift"], i["rot"], DEV, 42))
    run_a(lambda: merge(frag(1)), "mcg_ifm_merge", ["mcg_ifm_merge"])
    run_b(merge, frag(1), frag(2), "mcg_ifm_merge", ["mcg_ifm_merge"], raw=True)

    # mcg_egnn_aggregate over the compact edge list of the same three molecules
    n_rows = torch.tensor([n - 1 for n in SIZES for _ in range(n)], dtype=torch.int32)
    first_row = (torch.cumsum(n_rows, 0) - n_rows).to(torch.int32)
    E, M, D = int(n_rows.sum()), int(n_rows.numel()), 420
    agg = torch.empty(M, D, device=DEV)
    fr, nr = first_row.to(DEV), n_rows.to(DEV)

    def edges(seed):
        g = torch.Generator().manual_seed(seed)
        return dict(m=torch.randn(E, D, generator=g).to(DEV), gate=torch.rand(E, generator=g).to(DEV))

    def aggregate(i):
        L.check(lib().mcg_egnn_aggregate(L.dptr(i["m"]), L.dptr(i["gate"]), L.dptr(fr), L.dptr(nr), L.dptr(agg), M, D, _st()),
                "mcg_egnn_aggregate")
        return [agg]
    run_a(lambda: aggregate(edges(1)), "mcg_egnn_aggregate", ["mcg_egnn_aggregate"], refill=[agg])
    run_b(aggregate, edges(1), edges(2), "mcg_egnn_aggregate", ["mcg_egnn_aggregate"], raw=True, refill=[agg])
    claims("test_gcn_and_handoff_on_a_side_stream")


def test_an_element_outside_the_table_is_reported_behind_a_delayed_side_stream_forward(gcn_sd):
    """`AdjMatSeer.check_inputs_seen()` right behind a forward on S whose true input - element id 36, one past the embedding
    table - is still behind S's spin, the poison in its place being clean: the reference's IndexError must not be lost.
    (Before `mcg_gcn_check` waited for the forward's completion event it read the flag through the legacy stream, which a
    side stream does not order with, and returned 0 here.)"""
    g = _gcn(gcn_sd)
    clean = _gcn_inputs(SIZES, 9)
    bad = {k: v.clone() for k, v in clean.items()}
    bad["el"][1, 3] = 36
    work = P.rolled(clean)
    S = P.independent_stream(DEV)
    torch.cuda.synchronize()
    try:
        P.quiet_host(True)
        g.bond_orders(clean["el"], clean["dm"], clean["am"])     # sizes the workspace; clean: the flag stays down
        g.check_inputs_seen()
        with torch.cuda.stream(S):
            P.delay(S, P.MIN_DELAY_MS, "mcg_gcn_check")
            for k in work:
                work[k].copy_(bad[k])
            bond = g.bond_orders(work["el"], work["dm"], work["am"])
            pending = not S.query()
            with pytest.raises(IndexError):
                g.check_inputs_seen()
        assert pending                                          # the forward itself did not wait for its stream
        S.synchronize()
        assert bond.shape == (3, 42, 42)
        with pytest.raises(IndexError):                         # and the flag stays up
            g.check_inputs_seen()
    finally:
        torch.cuda.synchronize()
        P.quiet_host(False)


# ---- the post-generation modules: one batch of known molecules --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _molecules():
    """A single-atom row, a full-width row (the 14-atom reference molecule at W = 14) and two ordinary rows of
    `composed_cases.batch()`, on the device: coords [4,14,3], z [4,14] int32, bonds [4,14,14] int8, n [4] int32."""
    import composed_cases as CC
    import standardize_cases as SC
    items = {it["name"]: it for it in CC.batch()}
    rows = [items[k] for k in ("one atom", "reference molecule", "phenol", "indole")]
    xyz, z, bonds, n = (torch.from_numpy(t) for t in SC.pad_batch(rows, 14, 14))
    assert n.tolist() == [1, 14, 7, 9]
    return dict(coords=xyz.to(DEV), z=z.to(DEV), bonds=bonds.to(DEV), n=n.to(DEV))


def _mol(*keys):
    m = _molecules()
    return {k: m[k] for k in keys}


def _reference_coords():
    import composed_cases as CC
    return CC.reference()[0]


def test_shape_entries_on_a_side_stream():
    from ml_conformer_generator_amd import cheminformatics as CH
    ref = _reference_coords()
    xn = _mol("coords", "n")

    def frames_tf(i):
        xf = torch.empty(i["coords"].shape[0], 12, device=DEV)
        return [CH.shape_frames_hip(i["coords"], i["n"], DEV, centre_atoms=True, xform_out=xf), xf]
    run_ab(lambda i: CH.shape_tanimoto_batch(ref, i["coords"], i["n"], DEV), xn, "shape_tanimoto_batch", ["mcg_shape_tanimoto"])
    run_ab(lambda i: CH.shape_frames_hip(i["coords"], i["n"], DEV, centre_atoms=True, with_counts=True), xn, "shape_frames_hip",
           ["mcg_shape_moments", "mcg_shape_frames"])
    run_ab(frames_tf, xn, "shape_frames_hip(xform_out=)", ["mcg_shape_moments", "mcg_shape_frames_tf"])
    run_ab(lambda i: CH.shape_overlay(ref, i["coords"], i["n"], DEV, with_scores=True), xn, "shape_overlay",
           ["mcg_shape_frames_tf", "mcg_shape_overlay"])
    run_ab(lambda i: CH.shape_overlay(ref, i["coords"], i["n"], DEV, with_scores=True, refine_steps=4), xn,
           "shape_overlay(refine_steps=4)", ["mcg_shape_frames_tf", "mcg_shape_overlay_refined"])
    run_ab(lambda i: CH.pairwise_shape_tanimoto(ref, i["coords"], i["n"], DEV), xn, "pairwise_shape_tanimoto",
           ["mcg_shape_pair_tanimoto"])
    claims("test_shape_entries_on_a_side_stream")


def test_mesh_entries_on_a_side_stream():
    import mesh_cases as MC
    from ml_conformer_generator_amd import cheminformatics as CH
    from ml_conformer_generator_amd import mesh as M
    mesh = M.load_mesh(MC.box(9.0, 7.0, 6.0, origin=(-4.0, -4.0, -3.0)))
    tri = MC.triangles(mesh)
    solid = CH.SolidReference(mesh, n=16)
    solid.on(DEV)                                              # the solid's device side (its occupancy launch) is built once
    torch.cuda.synchronize()
    xn = _mol("coords", "n")
    pts = {"points": MC.random_points(mesh, 300, 1).to(DEV)}
    axes = {"axes": solid.axes.to(DEV).contiguous()}
    run_ab(lambda i: CH.mesh_winding(tri, points=i["points"], device=DEV), pts, "mesh_winding", ["mcg_mesh_winding"],
           poison={"points": MC.random_points(mesh, 300, 2).to(DEV)})
    run_ab(lambda i: CH.mesh_occupancy(tri, i["axes"], DEV), axes, "mesh_occupancy", ["mcg_mesh_occupancy"],
           poison={"axes": (axes["axes"] + 0.75).contiguous()})
    run_ab(lambda i: CH.mesh_atoms_outside(tri, i["coords"], i["n"], DEV, with_winding=True), xn, "mesh_atoms_outside",
           ["mcg_mesh_atoms_outside"])
    run_ab(lambda i: CH.shape_scores_solid(solid, i["coords"], i["n"], DEV), xn, "shape_scores_solid",
           ["mcg_shape_tanimoto_field"])
    run_ab(lambda i: CH.shape_overlay_solid(solid, i["coords"], i["n"], DEV, with_scores=True), xn, "shape_overlay_solid",
           ["mcg_shape_overlay_field", "mcg_mesh_atoms_outside"])
    claims("test_mesh_entries_on_a_side_stream")


def test_receptor_entries_on_a_side_stream():
    import interactions_cases as IK
    from ml_conformer_generator_amd import interactions as IX
    from ml_conformer_generator_amd import receptor as RC
    m = _molecules()
    g = np.random.default_rng(8)
    R = 257                                                    # one receptor atom above a tile of 256: with splits = 2 the second range runs
    rec = (torch.from_numpy((g.normal(size=(R, 3)) * 5.0).astype(np.float32)), torch.full((R,), 6))
    xnz = _mol("coords", "n", "z")
    run_ab(lambda i: RC.receptor_overlap(rec, i["coords"], i["n"], i["z"], DEV, splits=2), xnz, "receptor_overlap(R=257, splits=2)",
           ["mcg_receptor_overlap"])
    run_ab(lambda i: RC.relieve_clashes(rec, i["coords"], i["n"], i["z"], steps=8, device=DEV, return_gradient=True), xnz,
           "relieve_clashes", ["mcg_receptor_relieve"])
    prepared = IX.prepare_receptor(IK.PDB)
    real = (torch.arange(14, device=DEV).view(1, -1) < m["n"].view(-1, 1)).unsqueeze(2)
    centre = (m["coords"] * real).sum(1, keepdim=True) / m["n"].view(-1, 1, 1)
    near = ((m["coords"] - centre + prepared.xyzr[:, :3].mean(0).to(DEV) + 1.5) * real).contiguous()     # at the pocket
    torch.cuda.synchronize()
    full = dict(coords=near, n=m["n"], z=m["z"], bonds=m["bonds"])
    run_ab(lambda i: IX.interaction_scores(prepared, i["coords"], i["n"], i["z"], i["bonds"], device=DEV), full,
           "interaction_scores", ["mcg_receptor_interactions"])
    run_ab(lambda i: IX.optimise_pose(prepared, i["coords"], i["n"], i["z"], i["bonds"], steps=4, device=DEV), full,
           "optimise_pose", ["mcg_receptor_optimise"])
    claims("test_receptor_entries_on_a_side_stream")


def test_graph_preparation_and_scores_on_a_side_stream():
    import composed_cases as CC
    import electrostatics_cases as EK
    import pharmacophore_ref as PR
    from ml_conformer_generator_amd import electrostatics as ES
    from ml_conformer_generator_amd import geometry as GE
    from ml_conformer_generator_amd import hydrogens as HY
    from ml_conformer_generator_amd import pharmacophore as PH
    from ml_conformer_generator_amd import standardize as SD
    full, graph = _mol("coords", "z", "bonds", "n"), _mol("z", "bonds", "n")
    named = [(PR.TYPE_NAMES[t], tuple(float(v) for v in p)) for t, p in CC.reference_features()]
    ref_pts = [(float(c), tuple(float(v) for v in p)) for p, c in zip(*EK.fp32_points("acetamide"))]

    def esp(i):
        ch = ES.partial_charges(i["z"], i["bonds"], i["n"], DEV)
        placed = HY.add_hydrogens(i["coords"], i["z"], i["bonds"], i["n"], DEV)
        pts, q, count = ES.charge_points(i["coords"], ch, placed)
        return [ES.electrostatic_tanimoto(ref_pts, pts, q, count), ch]
    run_ab(lambda i: GE.relax_geometry(i["coords"], i["z"], i["bonds"], i["n"], steps=3, device=DEV, return_gradient=True), full,
           "relax_geometry(steps=3)", ["mcg_geometry_relax_ex"])
    run_ab(lambda i: PH.perceive_features(i["z"], i["bonds"], i["n"], DEV), graph, "perceive_features", ["mcg_pharm_perceive"])
    run_ab(lambda i: PH.pharmacophore_tanimoto(named, i["coords"], i["z"], i["bonds"], i["n"], DEV), full,
           "pharmacophore_tanimoto", ["mcg_pharm_perceive", "mcg_pharm_score"])
    run_ab(lambda i: HY.add_hydrogens(i["coords"], i["z"], i["bonds"], i["n"], DEV, return_rotors=True), full, "add_hydrogens",
           ["mcg_hydrogens_place"])
    run_ab(lambda i: SD.standardize_graphs(i["coords"], i["z"], i["bonds"], i["n"], DEV), full, "standardize_graphs",
           ["mcg_standardize_graphs"])
    run_ab(lambda i: ES.partial_charges(i["z"], i["bonds"], i["n"], DEV), graph, "partial_charges", ["mcg_charges_peoe"])
    run_ab(esp, full, "electrostatic_tanimoto", ["mcg_charges_peoe", "mcg_hydrogens_place", "mcg_esp_overlap"])
    claims("test_graph_preparation_and_scores_on_a_side_stream")


def test_graph_identity_entries_on_a_side_stream():
    from ml_conformer_generator_amd import canonical as CA
    from ml_conformer_generator_amd import fingerprint as FP
    from ml_conformer_generator_amd import scaffold as SF
    from ml_conformer_generator_amd import stereo as SO
    from ml_conformer_generator_amd import substructure as SU
    full, graph = _mol("coords", "z", "bonds", "n"), _mol("z", "bonds", "n")
    keep = torch.tensor([(0x5555 | 1) & ((1 << n) - 1) for n in graph["n"].tolist()], dtype=torch.int64, device=DEV)
    patterns = SU.compile_patterns(["c1ccccc1", "CO", "[#7]"])

    def prints(i):
        fp, key, bits = FP.graph_fingerprints(i["z"], i["bonds"], i["n"], DEV)
        return [fp, key, bits, FP.fingerprint_tanimoto(fp, fp[1].contiguous()), FP.pairwise_fingerprint_tanimoto(fp)]
    run_ab(prints, graph, "fingerprints", ["mcg_graph_fingerprint", "mcg_fingerprint_tanimoto", "mcg_fingerprint_pair_tanimoto"])
    run_ab(lambda i: CA.canonical_order(i["z"], i["bonds"], i["n"], DEV), graph, "canonical_order", ["mcg_canonical_order"])
    run_ab(lambda i: SO.stereo_order(i["coords"], i["z"], i["bonds"], i["n"], DEV), full, "stereo_order", ["mcg_stereo_order"])
    run_ab(lambda i: SU.match_substructures(i["z"], i["bonds"], i["n"], patterns, hydrogens=False, device=DEV), graph,
           "match_substructures", ["mcg_substructure_match"])
    run_ab(lambda i: SF.ring_perception(i["z"], i["bonds"], i["n"], DEV), graph, "ring_perception", ["mcg_ring_scaffold"])
    run_ab(lambda i: SF.induced_subgraph(i["z"], i["bonds"], i["n"], i["mask"], SF.MODE_KEEP, DEV), dict(graph, mask=keep),
           "induced_subgraph", ["mcg_induced_subgraph"])
    claims("test_graph_identity_entries_on_a_side_stream")


# ---- independent handles ------------------------------------------------------------------------------------------------------
def test_two_plans_of_one_model_and_two_gcn_handles_on_two_streams(gcn_sd):
    """Two plans that share one `mcg_egnn` and two `AdjMatSeer` handles, launched alternately on S1 and S2 without a
    synchronise in between, a spin in front of S1 so that the two streams' work overlaps: every result is that of its
    serial default-stream run, and what a handle owns (the plan's h buffer, the GCN's last GraphConv output) is as its own
    last call left it."""
    from ml_conformer_generator_amd.egnn import BatchPlan
    d = _dyn("f32")
    jobs = []
    for k, sizes in enumerate(([9, 27, 20, 1], [12, 5, 27])):
        N = max(sizes)
        inp = _denoiser_inputs(sizes, N, 30 + k)
        plan = BatchPlan(torch.tensor(sizes, dtype=torch.int32), N, DEV)
        g = _gcn(gcn_sd)
        gin = _gcn_inputs([42, 15, 1][: 3 - k] + [30] * k, 40 + k)
        jobs.append(dict(plan=plan, inp=inp, out=torch.empty_like(inp["xh"]), gcn=g, gin=gin, B=len(gin["el"])))

    def one(j):
        o = d.run(j["plan"], j["inp"]["t"], j["inp"]["xh"], j["inp"]["ctx"], out=j["out"]).clone()
        return [o] + [t.clone() for t in _forward(j["gcn"])(j["gin"])]

    def owned(j):
        return [d._peek(j["plan"], 0, 432), j["gcn"]._peek(5, j["B"])]
    try:
        P.quiet_host(True)
        serial = []
        for j in jobs:
            res = one(j)
            torch.cuda.synchronize()
            serial.append((res, [t.clone() for t in owned(j)]))
        torch.cuda.synchronize()
        streams = [P.independent_stream(DEV), P.independent_stream(DEV)]
        got = [[], []]
        t0 = time.perf_counter()                                # the host time of the same launches, unsynchronised
        for rep in range(3):
            for j in jobs:
                one(j)
        t_host = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        asked = P.delay(streams[0], max(P.MIN_DELAY_MS, P.B_MARGIN * t_host), "independent handles")
        print(f"\nSTREAM independent handles: host time of the launches {t_host:.2f} ms, spin {asked:.0f} ms")
        for rep in range(3):
            for k, j in enumerate(jobs):
                with torch.cuda.stream(streams[k]):
                    got[k].append(one(j))
        assert not streams[0].query()                           # nothing synchronised on the way
        torch.cuda.synchronize()
        for k, j in enumerate(jobs):
            for rep in range(3):
                assert P.same_bits(got[k][rep], serial[k][0]), (k, rep)
            assert P.same_bits(owned(j), serial[k][1]), k
    finally:
        torch.cuda.synchronize()
        P.quiet_host(False)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_a_generation_call_wholly_on_a_side_stream(monkeypatch):
    """`generate_conformers` with relaxation, poses and shape scores on, once on the default stream and once wholly under
    `torch.cuda.stream(S)` while the default stream spins: equal records, bit-equal `last_batch` tensors.  The spin is 5 x
    the call's measured time; the call is kept small (8 samples, 10 diffusion steps: 15 - 16 ms on an MI355X, a spin of
    76 - 79 ms) so that this stays under the 250 ms cap and the "default stream still busy" assertion runs - it ran, and
    caught the device-wide synchronise `postprocess.return_records` ended with.  A host so slow that the call takes more
    than 50 ms gets the capped spin and the line printed below says so."""
    from test_geometry_gpu import _gen, _reference
    from ml_conformer_generator_amd import conformer_generator as CG
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))
    gen = _gen()
    kw = dict(reference_conformer=_reference(), n_samples=8, variance=2, optimise_geometry=False, sample_seed=SEED,
              relax_geometry=3, overlay=True, shape_scores=True)
    default = torch.cuda.default_stream(DEV)
    S = P.independent_stream(DEV)
    try:
        P.quiet_host(True)
        gen.generate_conformers(**kw)                           # plans, graphs and allocations of this request exist
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base = gen.generate_conformers(**kw)
        torch.cuda.synchronize()
        t_call = (time.perf_counter() - t0) * 1e3
        lb = {k: v.clone() for k, v in gen.last_batch.items() if torch.is_tensor(v)}
        want = max(P.MIN_DELAY_MS, P.A_MARGIN * t_call)
        asked = P.delay(default, want, "generate_conformers")
        with torch.cuda.stream(S), P.Recorder() as rec:
            got = gen.generate_conformers(**kw)
            got_lb = {k: v.clone() for k, v in gen.last_batch.items() if torch.is_tensor(v)}
            S.synchronize()
        busy = not default.query()
        print(f"\nSTREAM generate_conformers [A]: baseline {t_call:.1f} ms, spin {asked:.0f} ms of {want:.0f} wanted, default "
              f"stream {'still busy' if busy else 'idle'} behind it, {len(rec.calls)} entry calls: {sorted(rec.names())}")
        wrong = sorted({(n, s) for n, s in rec.calls if s != S.cuda_stream})
        assert not wrong, wrong
        assert {"mcg_sampler_noise_keyed", "mcg_sampler_step", "mcg_sampler_decode", "mcg_handoff_elements", "mcg_gcn_forward",
                "mcg_bond_writeback", "mcg_geometry_relax_ex", "mcg_shape_overlay"} <= rec.names(), sorted(rec.names())
        if asked == want:                                       # (a call longer than a fifth of the longest spin outlasts it)
            assert busy, "something in the call waited for the default stream"
        assert len(got) == len(base) == 8
        for a, b in zip(got, base):
            assert a == b and a.sample_id == b.sample_id
            assert (a.strain_before, a.strain_after, a.shape_tanimoto, a.overlay_tanimoto) == \
                   (b.strain_before, b.strain_after, b.shape_tanimoto, b.overlay_tanimoto)
            assert torch.equal(a.coords.view(torch.int32), b.coords.view(torch.int32))
        assert set(got_lb) == set(lb) and {"x", "h", "bond", "x_ordered", "x_relaxed"} <= set(lb)
        for k in lb:
            assert P.same_bits([got_lb[k]], [lb[k]]), k
    finally:
        torch.cuda.synchronize()
        P.quiet_host(False)
