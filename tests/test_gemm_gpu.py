"""Every node / GCN GEMM instantiation the launchers of csrc/mcg_gemm.hip can dispatch, ONE launch at a time through
`mcg_debug_gemm`, against the float64 restatement and the pass rule of tests/gemm_ref.py, at tile-edge shapes.

The shape tables below are literal.  Every table row runs with every instantiation that can take it (a gather needs a second
K segment, the LDS-staged kernel takes n_tiles % 3 == 0, at most 28 k-blocks and at most 18 of them in segment 2), once with
small-integer operands (exact tier: torch.equal, no slack) and once with Gaussian ones (rounding tier: the fp32 forward
bound).  On identical inputs all instantiations of a family must agree bit for bit (RN / MR / ring depth never change the k
order of an output element; the LDS-staged bf16 kernel equals the 32-row one).  The last test holds the set of instantiations
that were reported against the literal list of what the launchers can dispatch."""
import ctypes as C
import os
import time
from dataclasses import replace

import numpy as np
import pytest
import torch

import gemm_ref as R
from gemm_ref import ACT_NONE, ACT_RELU, ACT_SILU, BF16, F32, F32ROWS16, X6, Shape
from ml_conformer_generator_amd import _lib

pytestmark = pytest.mark.gpu

_T0 = time.time()
N_, S_, RL = ACT_NONE, ACT_SILU, ACT_RELU

# M: {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 129, 1000} (MR = 2: M % 32 in 1..16 and in 17..31 both occur);
# K1 = 16 groups + 4 tail with groups 0..9 and tails 0..3 (straddling ring depths 3, 6, 8); K2 in {0, 4, 16, 420};
# n_tiles in {1, 2, 3, 4, 5, 7, 27, 54, 128} (a last wave of 1, 2 and RN valid tiles for every RN); the four n_store kinds;
# act x bias x residual (a residual takes n_store % 4 == 0).  Rows 13 on are the real shapes: the network's W3 (420 + 420 ->
# 432, SiLU), first-layer projections (420 -> 864) and W4 (420 -> 432 + residual), the GCN's 44 -> 64, 2048 -> 2048 and 210 of
# 224 columns.
#          M    K1   K2  n_tiles store  act bias  resid
MAIN = [
    Shape(1, 4, 4, 1, "full", N_, True, True),
    Shape(15, 8, 16, 2, "m4", RL, True, True),
    Shape(16, 12, 420, 3, "m6", S_, False, False),
    Shape(17, 16, 4, 4, "p1", N_, True, False),
    Shape(31, 36, 16, 5, "full", S_, True, True),
    Shape(32, 56, 4, 7, "m4", RL, False, True),
    Shape(33, 76, 16, 27, "m6", N_, True, False),
    Shape(47, 80, 4, 54, "p1", RL, True, False),
    Shape(48, 100, 16, 128, "full", N_, False, True),
    Shape(49, 120, 4, 1, "m6", S_, True, False),
    Shape(63, 140, 16, 2, "p1", RL, False, False),
    Shape(64, 144, 4, 3, "full", N_, True, True),
    Shape(129, 16, 420, 7, "m4", S_, True, True),
    Shape(1000, 36, 16, 5, "full", RL, True, True),
    Shape(16, 28, 60, 3, "m4", N_, True, True),
    Shape(32, 64, 32, 3, "full", RL, True, False),
    Shape(65, 420, 420, 27, "full", S_, True, False),
    Shape(129, 420, 0, 54, "full", N_, True, False),
    Shape(65, 420, 0, 27, "full", N_, True, True),
    Shape(1000, 44, 0, 4, "full", N_, True, False),
    Shape(33, 2048, 0, 128, "full", RL, True, False),
    Shape(84, 64, 0, 14, "m6", RL, True, False),
]
# bf16 / x6 kernels consume K in blocks of 32: K % 32 in {0, 4, 28} and K < 32; n_tiles in {3, 27, 54} so that the LDS-staged
# kernel takes every M; 18 k-blocks in segment 2 and 28 in all are the most it parks.  The last two rows make `lds = 2` fall
# back to the 32-row kernel (29 k-blocks; 19 of them in segment 2), as does every MAIN row with n_tiles % 3 != 0.
WIDE = [
    Shape(1, 4, 0, 3, "full", N_, True, True),
    Shape(15, 28, 4, 3, "m4", RL, True, True),
    Shape(16, 32, 16, 3, "m6", S_, False, False),
    Shape(17, 36, 420, 3, "p1", N_, True, False),
    Shape(31, 60, 0, 27, "full", S_, True, True),
    Shape(32, 64, 28, 3, "m4", N_, False, True),
    Shape(33, 96, 576, 3, "full", RL, True, False),
    Shape(47, 444, 420, 3, "m6", N_, True, False),
    Shape(48, 896, 0, 3, "full", RL, True, False),
    Shape(49, 420, 420, 27, "full", S_, True, True),
    Shape(63, 12, 36, 54, "p1", RL, True, False),
    Shape(64, 100, 60, 3, "full", N_, True, True),
    Shape(129, 68, 4, 27, "m4", RL, True, True),
    Shape(1000, 36, 16, 3, "full", N_, True, True),
    Shape(33, 900, 0, 3, "full", N_, True, True),
    Shape(33, 32, 608, 3, "full", N_, True, False),
]

# (rn, mr, deep) the 16-row launcher has an instantiation for, and the ring depth each runs with
ROWS16_TILES = [(1, 1, 0), (1, 1, 1), (2, 1, 0), (2, 1, 1), (3, 1, 0), (6, 1, 0), (2, 2, 0), (3, 2, 0)]
ROWS16_RING = {(1, 1, 0): 3, (1, 1, 1): 8, (2, 1, 0): 3, (2, 1, 1): 6, (3, 1, 0): 3, (6, 1, 0): 3, (2, 2, 0): 3, (3, 2, 0): 3}

# Everything the four launchers of mcg_gemm.hip can dispatch, as mcg_debug_gemm reports it:
#   ("f32", RN)   ("rows16", RN, MR, RING, GATHER)   ("bf16", RN, GATHER)   ("lds", GATHER, RESID, SEG2)   ("x6", RN)
# (launch_lds: a gather implies SEG2, so 8 of the 12 LDS-staged combinations exist)
EXPECTED = sorted(
    [("f32", 1), ("f32", 2), ("f32", 3)]
    + [("rows16", rn, mr, ring, g) for (rn, mr, ring) in [(1, 1, 3), (1, 1, 8), (2, 1, 3), (2, 1, 6), (3, 1, 3), (6, 1, 3), (2, 2, 3), (3, 2, 3)]
       for g in (0, 2, 3, 4)]
    + [("bf16", rn, g) for rn in (1, 2, 3) for g in (0, 2, 4)]
    + [("lds", 0, 0, 0), ("lds", 0, 1, 0), ("lds", 0, 0, 1), ("lds", 0, 1, 1), ("lds", 2, 0, 1), ("lds", 2, 1, 1), ("lds", 4, 0, 1), ("lds", 4, 1, 1)]
    + [("x6", 1), ("x6", 2), ("x6", 3)])
assert len(EXPECTED) == 55

RAN = set()                       # instantiations reported so far
WORST = {}                        # (family, tier) -> worst |error| / bound over the run
TABLE_TESTS_RUN = set()
SILU_MEASURED = {}


def key_of(ran):
    k = ran.kernel
    if k == _lib.GEMM_KERNEL_F32:
        return ("f32", ran.rn)
    if k == _lib.GEMM_KERNEL_F32ROWS16:
        return ("rows16", ran.rn, ran.mr, ran.ring, ran.gather)
    if k == _lib.GEMM_KERNEL_BF16:
        return ("bf16", ran.rn, ran.gather)
    if k == _lib.GEMM_KERNEL_BF16_LDS:
        return ("lds", ran.gather, ran.resid, ran.seg2)
    assert k == _lib.GEMM_KERNEL_X6, k
    return ("x6", ran.rn)


def lds_fits(shape):
    """bf16_lds_fits() of mcg_gemm.hip."""
    b1, b2 = (shape.K1 + 31) // 32, (shape.K2 + 31) // 32
    return b1 + b2 <= 28 and b2 <= 18 and shape.n_tiles % 3 == 0


class Device:
    """The operands of one Inputs on the GPU, uploaded once and reused by every instantiation that runs on them."""

    def __init__(self, inp):
        self.inp = inp
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.host = dict(a1=inp.a1, a2=inp.a2, slots=inp.slots, bias=inp.bias, resid=inp.resid)
        self.dev = {k: up(v) for k, v in self.host.items()}

    def launch(self, family, rn=0, mr=0, deep=0, lds=0, side=None, expect_error=None):
        """One mcg_debug_gemm call.  Returns (C buffer as numpy, reported instantiation key)."""
        inp, s = self.inp, self.inp.shape
        c = torch.from_numpy(inp.c_buffer()).cuda()
        d = _lib.GemmDesc()
        t = self.dev
        d.A1, d.lda1, d.a1_floats = t["a1"].data_ptr(), inp.a1.shape[1], inp.a1.size
        if inp.a2 is not None:
            d.A2, d.lda2, d.a2_floats = t["a2"].data_ptr(), inp.a2.shape[1], inp.a2.size
        if inp.slots is not None:
            d.a2_rows, d.a2_nsum, d.a2_src_rows = t["slots"].data_ptr(), inp.nsum, inp.a2_src_rows
        if inp.bias is not None:
            d.bias = t["bias"].data_ptr()
        if inp.resid is not None:
            d.resid, d.ldr, d.resid_floats = t["resid"].data_ptr(), inp.resid.shape[1], inp.resid.size
        d.C, d.c_floats, d.c_blocked = c.data_ptr(), c.numel(), int(inp.c_blocked)
        d.ldc = 0 if inp.c_blocked else inp.ldc
        w = np.ascontiguousarray(inp.w, dtype=np.float32)
        d.w_host = w.ctypes.data
        d.M, d.K1, d.K2, d.n_out, d.n_store, d.act = s.M, s.K1, s.K2, inp.n_out, s.n_store, s.act
        d.family, d.rn, d.mr, d.deep, d.lds = family, rn, mr, deep, lds
        side_dev = None
        if side is not None:
            u, slots, x = side
            side_dev = [torch.from_numpy(v.copy()).cuda() for v in (u, slots, x)]
            d.side_u, d.side_slots, d.side_x = (v.data_ptr() for v in side_dev)
            d.side_M, d.side_u_rows = slots.shape[0], u.shape[0]
        ran = _lib.GemmRan()
        rc = _lib.lib().mcg_debug_gemm(C.byref(d), C.byref(ran), _lib.current_stream_ptr(c.device))
        if expect_error is not None:
            msg = _lib.lib().mcg_last_error()
            assert rc != 0 and expect_error in msg, (rc, msg)
            assert torch.equal(c.cpu(), torch.from_numpy(inp.c_buffer())), "a refused launch must not touch C"
            return None, None
        _lib.check(rc, "mcg_debug_gemm")
        for k, v in self.host.items():                      # guard rows, padding and the operands themselves: unchanged
            assert v is None or np.array_equal(self.dev[k].cpu().numpy(), v), f"{k} was modified by the launch"
        key = key_of(ran)
        RAN.add(key)
        out = c.cpu().numpy()
        if side is not None:
            return out, key, [v.cpu().numpy() for v in side_dev]
        return out, key


def run_group(shape, family_kind, tier, nsum, selections, **kw):
    """Every selection on the same inputs: each judged against float64, all bit-identical.  `selections` are
    (family, rn, mr, deep, lds, expected key).  Returns the common C buffer."""
    s = replace(shape, act=ACT_RELU) if (tier == "exact" and shape.act == ACT_SILU) else shape      # the exact tier has no SiLU
    inp = R.make_inputs(s, family_kind, tier, nsum, **kw)
    ref = R.reference(inp)
    dev = Device(inp)
    first = None
    for family, rn, mr, deep, lds, want in selections:
        c, key = dev.launch(family, rn, mr, deep, lds)
        assert key == want, f"asked for {want}, the launcher ran {key}"
        failures, ratio = R.judge(inp, c, ref)
        print(f"{R.FAMILY_NAME[family]:9s} {key} M={s.M} K={s.K1}+{s.K2} n_tiles={s.n_tiles} n_store={s.n_store} act={s.act} nsum={nsum} "
              f"{tier}: worst |err| / bound = {ratio:.3g}")
        WORST[(R.FAMILY_NAME[family], tier)] = max(WORST.get((R.FAMILY_NAME[family], tier), 0.0), ratio)
        assert not failures, (key, s, tier, nsum, failures)
        if first is None:
            first = (key, c)
        else:
            assert torch.equal(torch.from_numpy(c), torch.from_numpy(first[1])), f"{key} and {first[0]} differ on the same inputs ({s}, {tier})"
    return first[1]


def f32_selections():
    return [(F32, rn, 0, 0, 0, ("f32", rn)) for rn in (1, 2, 3)]


def rows16_selections(nsum):
    return [(F32ROWS16, rn, mr, deep, 0, ("rows16", rn, mr, ROWS16_RING[(rn, mr, deep)], nsum)) for rn, mr, deep in ROWS16_TILES]


def bf16_selections(shape, nsum):
    g = R.gather_width(BF16, nsum)
    sel = [(BF16, rn, 0, 0, 1, ("bf16", rn, g)) for rn in (1, 2, 3)]
    # lds = 2 means "if it fits": the LDS-staged kernel, or the 32-row kernel with the launcher's own width
    if lds_fits(shape):
        sel.append((BF16, 0, 0, 0, 2, ("lds", g, int(shape.resid), int(shape.K2 > 0))))
    return sel


def x6_selections():
    return [(X6, rn, 0, 0, 0, ("x6", rn)) for rn in (1, 2, 3)]


TIERS = ("exact", "round")
F32_CASES = [(i, t) for i in range(len(MAIN)) for t in TIERS]
ROWS16_CASES = [(i, t, n) for i in range(len(MAIN)) for t in TIERS for n in (0, 2, 3, 4) if n == 0 or MAIN[i].K2 > 0]
BOTH = MAIN + WIDE
BF16_CASES = [(i, t, n) for i in range(len(BOTH)) for t in TIERS for n in (0, 2, 3, 4) if n == 0 or BOTH[i].K2 > 0]
X6_CASES = [(i, t) for i in range(len(BOTH)) for t in TIERS]


def ids(table, cases):
    return ["-".join([f"M{table[c[0]].M}-K{table[c[0]].K1}+{table[c[0]].K2}-nt{table[c[0]].n_tiles}-{table[c[0]].store}", c[1]]
                     + [f"nsum{n}" for n in c[2:]]) for c in cases]


@pytest.mark.parametrize("i,tier", F32_CASES, ids=ids(MAIN, F32_CASES))
def test_f32_32row_kernel(i, tier):
    TABLE_TESTS_RUN.add(("f32", i, tier))
    run_group(MAIN[i], F32, tier, 0, f32_selections())


@pytest.mark.parametrize("i,tier,nsum", ROWS16_CASES, ids=ids(MAIN, ROWS16_CASES))
def test_f32_16row_kernel(i, tier, nsum):
    TABLE_TESTS_RUN.add(("rows16", i, tier, nsum))
    run_group(MAIN[i], F32ROWS16, tier, nsum, rows16_selections(nsum))


@pytest.mark.parametrize("i,tier,nsum", BF16_CASES, ids=ids(BOTH, BF16_CASES))
def test_bf16_kernels(i, tier, nsum):
    TABLE_TESTS_RUN.add(("bf16", i, tier, nsum))
    run_group(BOTH[i], BF16, tier, nsum, bf16_selections(BOTH[i], nsum))


@pytest.mark.parametrize("i,tier", X6_CASES, ids=ids(BOTH, X6_CASES))
def test_x6_kernel(i, tier):
    TABLE_TESTS_RUN.add(("x6", i, tier))
    run_group(BOTH[i], X6, tier, 0, x6_selections())


def test_lds_2_falls_back_where_the_shape_does_not_fit():
    """`lds = 2` only means "if it fits": n_tiles % 3 != 0, more than 28 k-blocks, or more than 18 of them in segment 2 run
    the 32-row kernel, and the report says so; a shape that fits runs the LDS-staged kernel.  Same bits either way."""
    for shape, fits in ((MAIN[4], False), (WIDE[14], False), (WIDE[15], False), (WIDE[6], True), (WIDE[8], True), (WIDE[7], True)):
        assert lds_fits(shape) == fits
        inp = R.make_inputs(replace(shape, act=ACT_NONE), BF16, "exact")
        dev = Device(inp)
        c2, key2 = dev.launch(BF16, 0, 0, 0, 2)
        c1, key1 = dev.launch(BF16, 0, 0, 0, 1)
        assert key1[0] == "bf16" and key2[0] == ("lds" if fits else "bf16"), (shape, key1, key2)
        assert not R.judge(inp, c2)[0] and np.array_equal(c1, c2)


def test_bf16_gather_divides_the_sum_not_the_rows():
    """Partial rows whose sum / 100 sits a few fp32 ulps from a bf16 rounding boundary (gemm_ref.adversarial_div100_pairs):
    dividing each row first would round every operand of segment 2 differently."""
    shape = Shape(33, 4, 16, 3, "full", ACT_NONE, True, False)
    run_group(shape, BF16, "round", 2, bf16_selections(shape, 2), adversarial_div100=True)


# ------------------------------------------------------------------------------------------------ side job
SIDE_SHAPE = Shape(33, 36, 16, 3, "full", ACT_RELU, True, True)
SIDE_KERNELS = [(F32, 2, 0, 0, 0), (F32ROWS16, 1, 1, 1, 0), (F32ROWS16, 3, 2, 0, 0), (F32ROWS16, 6, 1, 0, 0), (BF16, 3, 0, 0, 1), (BF16, 0, 0, 0, 2)]


@pytest.mark.parametrize("side_M", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("sel", SIDE_KERNELS, ids=lambda s: f"{R.FAMILY_NAME[s[0]]}-rn{s[1]}-mr{s[2]}-deep{s[3]}-lds{s[4]}")
def test_side_job(sel, side_M):
    """The coordinate update carried by the workgroups behind the GEMM's own: C is bit-identical with and without it, x is
    held against float64 within four fp32 roundings, component 3 and the guard rows stay as they were."""
    family = sel[0]
    nsum = 2 if family in (F32ROWS16, BF16) else 0
    inp = R.make_inputs(SIDE_SHAPE, family, "round", nsum)
    dev = Device(inp)
    c0, key0 = dev.launch(*sel)
    u, slots, x = R.side_job_inputs(side_M)
    c1, key1, (u1, slots1, x1) = dev.launch(*sel, side=(u, slots, x))
    assert key0 == key1 and not R.judge(inp, c0)[0]
    assert np.array_equal(c0, c1), "the side job changed the GEMM's output"
    assert np.array_equal(u1, u) and np.array_equal(slots1, slots)
    x64, bound = R.side_job_reference(u, slots, x, side_M)
    err = np.abs(x1.astype(np.float64) - x64)
    print(f"side job {key1} side_M={side_M}: worst |err| / bound = {(err[:side_M, :3] / bound[:side_M, :3]).max():.3g}")
    assert np.all(err[:side_M, :3] <= bound[:side_M, :3])
    assert np.array_equal(x1[:, 3], x[:, 3]) and np.array_equal(x1[side_M:], x[side_M:])


# ------------------------------------------------------------------------------------------------ blocked C
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("shape", [Shape(33, 420, 0, 54, "full", ACT_NONE, True, False), Shape(65, 36, 28, 54, "full", ACT_RELU, True, True)],
                         ids=["pab", "two-segment"])
def test_c_blocked(shape, tier):
    """The blocked layout of McgGemmArgs' comment, read back through its formula (gemm_ref.c_view): same values as the
    row-major launch, and the upper four pieces of each part's 14th block stay as the caller left them."""
    for family, selections in ((F32, f32_selections()), (BF16, bf16_selections(shape, 0))):
        row_major = run_group(shape, family, tier, 0, selections)
        blocked = run_group(shape, family, tier, 0, selections, c_blocked=True)
        inp = R.make_inputs(shape, family, tier, 0, c_blocked=True)
        c, written = R.c_view(inp, blocked)
        assert np.array_equal(c, row_major[:shape.M, :shape.n_store])
        assert written.sum() == shape.M * 864 and np.all(blocked[~written] == R.SENTINEL)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_launchers_refusals_fire_as_errors_not_as_wrong_numbers():
    """A residual on a ragged right edge and c_blocked on a kernel that ignores it used to give silently wrong output; with
    real device buffers behind the descriptor they are errors now and C is not touched."""
    ragged = Shape(17, 36, 0, 3, "m6", ACT_NONE, True, False)
    inp = R.make_inputs(ragged, F32, "exact")
    inp.resid = np.zeros((ragged.M + R.GUARD_ROWS, 48), dtype=np.float32)
    dev = Device(inp)
    for family, rn, mr in ((F32, 1, 0), (F32ROWS16, 2, 1), (BF16, 1, 0), (X6, 1, 0)):
        dev.launch(family, rn, mr, expect_error=b"n_store % 4 == 0")
    wide = Shape(17, 36, 0, 54)
    for family, rn, mr in ((F32ROWS16, 2, 1), (X6, 1, 0)):
        Device(R.make_inputs(wide, family, "exact", c_blocked=True)).launch(family, rn, mr, expect_error=b"c_blocked is implemented by")
    Device(R.make_inputs(Shape(17, 36, 0, 27), BF16, "exact", c_blocked=True)).launch(BF16, 1, 0, expect_error=b"n_tiles == 54")


def test_slot_tables_are_checked_before_the_launch():
    shape = Shape(17, 36, 16, 3)
    inp = R.make_inputs(shape, F32ROWS16, "exact", 4)
    inp.slots = inp.slots.copy()
    inp.slots[5, 3] = inp.a2_src_rows
    Device(inp).launch(F32ROWS16, 2, 1, expect_error=b"a2_rows[5][3]")


# ------------------------------------------------------------------------------------------------ SiLU
@pytest.mark.parametrize("family,rn,mr", [(F32, 1, 0), (F32ROWS16, 2, 1), (BF16, 1, 0), (X6, 1, 0)], ids=["F32", "F32Rows16", "Bf16", "X6"])
def test_silu_evaluation_error(family, rn, mr):
    """mcg_silu (v_exp_f32 / v_rcp_f32) against float64 x * sigmoid(x), through the harness: K1 = 4 and one 1 per weight row
    make the pre-activation exactly an input element; inputs on a grid over [-20, 20].  gemm_ref.EPS_SILU is twice the
    worst relative error measured here."""
    grid = np.linspace(-20.0, 20.0, 4 * 20001).astype(np.float32)
    shape = Shape(len(grid) // 4, 4, 0, 1, "full", ACT_SILU, False, False)
    inp = R.make_inputs(shape, family, "round")
    inp.a1[:shape.M, :4] = grid.reshape(-1, 4)
    inp.w = np.zeros((16, 4), dtype=np.float32)
    inp.w[:4] = np.eye(4, dtype=np.float32)
    inp.n_out = 16
    c, key = Device(inp).launch(family, rn, mr)
    v = (R.round_bf16(grid) if family == BF16 else grid).astype(np.float64)
    want = R.silu64(v)
    got = c[:shape.M, :4].reshape(-1).astype(np.float64)
    assert np.all(c[:shape.M, 4:16] == 0) and np.all(got[v == 0] == 0)
    rel = np.abs(got - want)[v != 0] / np.abs(want[v != 0])
    at = np.argmax(rel)
    SILU_MEASURED[R.FAMILY_NAME[family]] = float(rel.max())
    print(f"mcg_silu through {key}: worst relative error {rel.max():.4g} at x = {v[v != 0][at]!r}; EPS_SILU = {R.EPS_SILU:.4g}")
    assert rel.max() <= R.EPS_SILU


# ------------------------------------------------------------------------------------------------ coverage
def _launch_only(shape, family, nsum, selections):
    dev = Device(R.make_inputs(replace(shape, act=ACT_NONE), family, "exact", nsum))
    for family_, rn, mr, deep, lds, want in selections:
        assert dev.launch(family_, rn, mr, deep, lds)[1] == want


def test_zz_every_instantiation_the_launchers_can_dispatch_ran():
    """The instantiations reported over the run equal the literal list of what mcg_gemm.hip can dispatch: a new instantiation
    without a case, or a case whose instantiation disappeared, fails here.  (Run on its own, this test launches the tables
    itself without judging them.)"""
    wanted = ({("f32", i, t) for i, t in F32_CASES} | {("rows16", i, t, n) for i, t, n in ROWS16_CASES}
              | {("bf16", i, t, n) for i, t, n in BF16_CASES} | {("x6", i, t) for i, t in X6_CASES})
    if not wanted <= TABLE_TESTS_RUN:
        for i, _ in F32_CASES[::2]:
            _launch_only(MAIN[i], F32, 0, f32_selections())
        for i, t, n in ROWS16_CASES:
            if t == "exact":
                _launch_only(MAIN[i], F32ROWS16, n, rows16_selections(n))
        for i, t, n in BF16_CASES:
            if t == "exact":
                _launch_only(BOTH[i], BF16, n, bf16_selections(BOTH[i], n))
        for i, _ in X6_CASES[::2]:
            _launch_only(BOTH[i], X6, 0, x6_selections())
    assert sorted(RAN) == EXPECTED, (sorted(set(EXPECTED) - RAN), sorted(RAN - set(EXPECTED)))
    report = os.environ.get("MCG_GEMM_HARNESS_REPORT")
    if report:                                  # measurement record for profiles/gemm_harness.txt
        with open(report, "w") as f:
            f.write(f"EPS_SILU in use: {R.EPS_SILU:.4g}\n")
            for fam, worst in sorted(SILU_MEASURED.items()):
                f.write(f"mcg_silu worst relative error vs float64, {fam}: {worst:.4g}\n")
            for (fam, tier), worst in sorted(WORST.items()):
                f.write(f"worst |error| / bound, {fam} {tier}: {worst:.4g}\n")
            f.write(f"instantiations reported: {len(RAN)} of {len(EXPECTED)}\n")
            f.write(f"wall time of tests/test_gemm_gpu.py up to here: {time.time() - _T0:.1f} s\n")
