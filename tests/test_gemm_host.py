"""Host half of the node-GEMM harness (no GPU): the three weight packers against a restatement of the layout comments, every
refusal of `mcg_debug_gemm`, and the pass rule of tests/gemm_ref.py against a CPU stand-in and its mutants."""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as R
from gemm_ref import ACT_NONE, ACT_RELU, ACT_SILU, BF16, F32, F32ROWS16, X6, Shape
from ml_conformer_generator_amd import _lib


# ------------------------------------------------------------------------------------------------ packers
def pack(w, K1, K2, kind):
    L = _lib.lib()
    w = np.ascontiguousarray(w, dtype=np.float32)
    n = C.c_int64()
    args = (w.ctypes.data, w.shape[0], K1, K2, kind)
    _lib.check(L.mcg_debug_gemm_pack(*args, None, 0, C.byref(n)), "mcg_debug_gemm_pack")
    out = np.zeros(n.value, dtype=np.float32 if kind == _lib.GEMM_PACK4 else np.uint16)
    _lib.check(L.mcg_debug_gemm_pack(*args, out.ctypes.data, out.size, C.byref(n)), "mcg_debug_gemm_pack")
    assert n.value == out.size
    return out


def kperm(step, g, K):
    """mcg_common.h: k-step `step` of lane group g reads k = 16 q + 4 g + s inside full 16-groups (step = 4 q + s), and
    k = 16 Q + 4 s' + g in the tail steps behind them."""
    full = (K // 16) * 4
    return np.where(step < full, 16 * (step >> 2) + 4 * g + (step & 3), 16 * (K // 16) + 4 * (step - full) + g)


def pack4_map(K, n_tiles):
    """(n, k) read by every float of a B-pack4 segment, from the comment at the top of mcg_gemm.h:
       full 16-k groups:  Bp4[((q * n_tiles + nt) * 64 + lane) * 4 + s] = W[16 nt + (lane & 15)][16 q + 4 (lane >> 4) + s]
       then tail steps:   Bp4[tail_base + (st * n_tiles + nt) * 64 + lane] = W[16 nt + (lane & 15)][16 Q + 4 st + (lane >> 4)]"""
    Q, tail = K // 16, (K % 16) // 4
    n = np.zeros(K // 4 * n_tiles * 64, dtype=np.int64)
    k = np.zeros_like(n)
    q, nt, lane, s = np.meshgrid(np.arange(Q), np.arange(n_tiles), np.arange(64), np.arange(4), indexing="ij")
    at = (((q * n_tiles + nt) * 64 + lane) * 4 + s).ravel()
    n[at], k[at] = (16 * nt + (lane & 15)).ravel(), (16 * q + 4 * (lane >> 4) + s).ravel()
    assert np.array_equal(k[at], kperm(4 * q + s, lane >> 4, K).ravel())
    st, nt, lane = np.meshgrid(np.arange(tail), np.arange(n_tiles), np.arange(64), indexing="ij")
    at = (Q * n_tiles * 256 + (st * n_tiles + nt) * 64 + lane).ravel()
    n[at], k[at] = (16 * nt + (lane & 15)).ravel(), (16 * Q + 4 * st + (lane >> 4)).ravel()
    assert np.array_equal(k[at], kperm(4 * Q + st, lane >> 4, K).ravel())
    return n, k


def pack16_map(K, n_tiles):
    """Bp16[((kb * n_tiles + nt) * 64 + lane) * 8 + j] = bf16(W[16 nt + (lane & 15)][32 kb + 8 (lane >> 4) + j]), K padded up to
    a multiple of 32 with zero weights."""
    kb, nt, lane, j = np.meshgrid(np.arange((K + 31) // 32), np.arange(n_tiles), np.arange(64), np.arange(8), indexing="ij")
    return (16 * nt + (lane & 15)).ravel(), (32 * kb + 8 * (lane >> 4) + j).ravel()


def take(w, n, k):
    """W[n][k], zero outside the matrix (rows >= n_out, the K padding)."""
    inside = (n < w.shape[0]) & (k < w.shape[1])
    out = np.zeros(n.shape, dtype=np.float32)
    out[inside] = w[n[inside], k[inside]]
    return out


def bf16_bits(x):
    return (R.round_bf16(x).view(np.uint32) >> 16).astype(np.uint16)


def restated(w, K1, K2, kind):
    n_tiles = (w.shape[0] + 15) // 16
    parts = []
    for ws in (w[:, :K1], w[:, K1:]):
        K = ws.shape[1]
        if K == 0:
            continue
        if kind == _lib.GEMM_PACK4:
            parts.append(take(ws, *pack4_map(K, n_tiles)))
        elif kind == _lib.GEMM_PACK16:
            parts.append(bf16_bits(take(ws, *pack16_map(K, n_tiles))))
        else:
            # [k-block][part][n-tile][lane][8]; every weight the exact sum of three bf16 parts, each the rounding of what the
            # previous ones left
            left = take(ws, *pack16_map(K, n_tiles)).reshape((K + 31) // 32, 1, n_tiles * 512)
            three = []
            for _ in range(3):
                p = R.round_bf16(left)
                three.append(bf16_bits(p))
                left = (left - p).astype(np.float32)
            parts.append(np.concatenate(three, axis=1).ravel())
    return np.concatenate(parts)


PACK_K = [4, 8, 12, 16, 20, 28, 32, 36, 44, 420, 2048]


@pytest.mark.parametrize("kind", [_lib.GEMM_PACK4, _lib.GEMM_PACK16, _lib.GEMM_PACK16X3], ids=["pack4", "pack16", "pack16x3"])
@pytest.mark.parametrize("K1", PACK_K)
def test_packers_match_the_documented_layout(kind, K1):
    rng = np.random.default_rng(K1)
    for n_out, K2 in ((16, 0), (21, 0), (37, 12), (48, 420 if K1 <= 420 else 44)):
        w = rng.standard_normal((n_out, K1 + K2)).astype(np.float32)
        got = pack(w, K1, K2, kind)
        want = restated(w, K1, K2, kind)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32 if kind == _lib.GEMM_PACK4 else np.uint16),
                              want.view(np.uint32 if kind == _lib.GEMM_PACK4 else np.uint16)), (n_out, K1, K2)


@pytest.mark.parametrize("K", PACK_K)
def test_every_weight_element_is_packed_exactly_once(K):
    for n_out in (16, 21, 37):
        n_tiles = (n_out + 15) // 16
        for n, k in (pack4_map(K, n_tiles), pack16_map(K, n_tiles)):
            real = (n < n_out) & (k < K)
            count = np.zeros((n_out, K), dtype=np.int64)
            np.add.at(count, (n[real], k[real]), 1)
            assert np.all(count == 1)
        # ... and through the library: distinct values, each found once, everything else zero
        w = (np.arange(n_out * K, dtype=np.float32) + 1).reshape(n_out, K)
        got = pack(w, K, 0, _lib.GEMM_PACK4)
        assert np.array_equal(np.sort(got[got != 0]), w.ravel()) and got.size == K // 4 * n_tiles * 64
        n, k = pack4_map(K, n_tiles)
        assert np.all(got[n >= n_out] == 0)


@pytest.mark.parametrize("K", PACK_K)
def test_pack16x3_parts_sum_back_to_the_weight(K):
    rng = np.random.default_rng(K + 1)
    n_out = 21
    w = (rng.standard_normal((n_out, K)) * np.exp(rng.uniform(-6, 6, (n_out, K)))).astype(np.float32)
    got = pack(w, K, 0, _lib.GEMM_PACK16X3).reshape((K + 31) // 32, 3, -1)
    parts = (got.astype(np.uint32) << 16).view(np.float32)
    n, k = pack16_map(K, 2)
    exact = parts[:, 0].astype(np.float64) + parts[:, 1].astype(np.float64) + parts[:, 2].astype(np.float64)
    assert np.array_equal(exact.ravel(), take(w, n, k).astype(np.float64))


# ------------------------------------------------------------------------------------------------ refusals
FAKE = 0x10000          # a "device pointer" that is never dereferenced: every case below is refused on the host


def valid_desc(**over):
    """A descriptor that passes every host check (it is never launched: each test breaks one contract)."""
    w = np.zeros((48, 64), dtype=np.float32)
    d = _lib.GemmDesc()
    d.A1, d.A2, d.C, d.w_host = FAKE, FAKE, FAKE, w.ctypes.data
    d.M, d.K1, d.K2, d.n_out, d.n_store = 20, 32, 32, 48, 48
    d.lda1 = d.lda2 = 32
    d.ldc = 48
    d.a1_floats = d.a2_floats = 20 * 32
    d.c_floats = 20 * 48
    d.family, d.rn, d.mr = _lib.GEMM_F32ROWS16, 2, 1
    for k, v in over.items():
        setattr(d, k, v)
    d._keep = w
    return d


def with_gather(**over):
    return valid_desc(**{**dict(a2_rows=FAKE, a2_nsum=2, a2_src_rows=8, a2_floats=8 * 32), **over})


def with_side(**over):
    return valid_desc(**{**dict(side_x=FAKE, side_u=FAKE, side_slots=FAKE, side_M=5, side_u_rows=9), **over})


def blocked(**over):
    w = np.zeros((864, 32), dtype=np.float32)
    d = valid_desc(family=_lib.GEMM_F32, rn=1, mr=0, K2=0, A2=None, a2_floats=0, lda2=0, n_out=864, n_store=864, c_blocked=1,
                   c_floats=896 * 20, w_host=w.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    d._keep = w
    return d


REFUSALS = {
    "K1 % 4": (lambda: valid_desc(K1=30), b"K1 % 4 == 0"),
    "K2 % 4": (lambda: valid_desc(K2=30), b"K2 % 4 == 0"),
    "K1 = 0": (lambda: valid_desc(K1=0), b"K1 must be"),
    "M < 1": (lambda: valid_desc(M=0), b"M must be"),
    "n_tiles < 1": (lambda: valid_desc(n_out=0), b"n_tiles >= 1"),
    "n_store < 1": (lambda: valid_desc(n_store=0), b"n_store must be"),
    "n_store > 16 n_tiles": (lambda: valid_desc(n_store=49, ldc=52, c_floats=20 * 52), b"n_store must be"),
    "lda1 < K1": (lambda: valid_desc(lda1=28), b"A1: leading dimension"),
    "lda2 < K2": (lambda: valid_desc(lda2=28), b"A2: leading dimension"),
    "A1 buffer short (fp32)": (lambda: valid_desc(a1_floats=20 * 32 - 1), b"A1: the kernel reads"),
    "A1 buffer without the bf16 slack": (lambda: valid_desc(family=_lib.GEMM_BF16, rn=1, mr=0, K1=36, lda1=36, a1_floats=20 * 36), b"A1: the kernel reads 748"),
    "A2 buffer without the x6 slack": (lambda: valid_desc(family=_lib.GEMM_X6, rn=1, mr=0, K2=4, lda2=4, a2_floats=20 * 4), b"A2: the kernel reads 108"),
    "A2 without K2": (lambda: valid_desc(K2=0), b"A2 must be set exactly when K2 > 0"),
    "gather without K2": (lambda: with_gather(K2=0, A2=None), b"a gather (a2_rows) needs K2 > 0"),
    "gather on F32": (lambda: with_gather(family=_lib.GEMM_F32, rn=1, mr=0), b"gathering kernels"),
    "gather on X6": (lambda: with_gather(family=_lib.GEMM_X6, rn=1, mr=0), b"gathering kernels"),
    "gather width 1": (lambda: with_gather(a2_nsum=1), b"a2_nsum must be 2, 3 or 4"),
    "gather width 5": (lambda: with_gather(a2_nsum=5), b"a2_nsum must be 2, 3 or 4"),
    "gathered A2 buffer short": (lambda: with_gather(a2_floats=8 * 32 - 1), b"A2: the kernel reads"),
    "a2_nsum without a2_rows": (lambda: valid_desc(a2_nsum=2), b"without a2_rows"),
    "side job on X6": (lambda: with_side(family=_lib.GEMM_X6, rn=1, mr=0, a1_floats=10000, a2_floats=10000), b"no side job"),
    "side job without slots": (lambda: with_side(side_slots=None), b"a side job needs side_x, side_u and side_slots"),
    "side job without rows": (lambda: with_side(side_M=0), b"side_M >= 1"),
    "residual on a ragged edge": (lambda: valid_desc(resid=FAKE, n_store=46, ldr=48, resid_floats=20 * 48), b"n_store % 4 == 0"),
    "residual buffer short": (lambda: valid_desc(resid=FAKE, ldr=48, resid_floats=20 * 48 - 1), b"resid_floats"),
    "ldr < n_store": (lambda: valid_desc(resid=FAKE, ldr=44, resid_floats=20 * 48), b"ldr must be"),
    "ldc < n_store": (lambda: valid_desc(ldc=44), b"ldc must be"),
    "C buffer short": (lambda: valid_desc(c_floats=20 * 48 - 1), b"c_floats"),
    "c_blocked on F32Rows16": (lambda: blocked(family=_lib.GEMM_F32ROWS16, rn=2, mr=1), b"c_blocked is implemented by"),
    "c_blocked on X6": (lambda: blocked(family=_lib.GEMM_X6, a1_floats=10000), b"c_blocked is implemented by"),
    "c_blocked with n_tiles != 54": (lambda: valid_desc(family=_lib.GEMM_BF16, rn=1, mr=0, c_blocked=1, c_floats=10 ** 6, a1_floats=10000, a2_floats=10000), b"n_tiles == 54"),
    "c_blocked buffer short": (lambda: blocked(c_floats=896 * 20 - 1), b"896 * M"),
    "rn 4 on F32": (lambda: valid_desc(family=_lib.GEMM_F32, rn=4, mr=0), b"rn must be 0"),
    "rn 5 on F32Rows16": (lambda: valid_desc(rn=5), b"MCG_GEMM_F32ROWS16 tiles"),
    "mr 2 with rn 6": (lambda: valid_desc(rn=6, mr=2), b"MCG_GEMM_F32ROWS16 tiles"),
    "mr 3": (lambda: valid_desc(mr=3), b"MCG_GEMM_F32ROWS16 tiles"),
    "deep with rn 3": (lambda: valid_desc(rn=3, deep=1), b"deep only with"),
    "deep with mr 2": (lambda: valid_desc(mr=2, deep=1), b"deep only with"),
    "mr on Bf16": (lambda: valid_desc(family=_lib.GEMM_BF16, rn=1, mr=1, a1_floats=10000, a2_floats=10000), b"mr and deep belong to"),
    "lds on F32": (lambda: valid_desc(family=_lib.GEMM_F32, rn=1, mr=0, lds=2), b"lds must be"),
    "lds 3": (lambda: valid_desc(family=_lib.GEMM_BF16, rn=1, mr=0, lds=3, a1_floats=10000, a2_floats=10000), b"lds must be"),
    "act 3": (lambda: valid_desc(act=3), b"act must be"),
    "family 4": (lambda: valid_desc(family=4), b"family must be"),
    "no weight": (lambda: valid_desc(w_host=None), b"w_host, A1 and C are required"),
    "reserved set": (lambda: valid_desc(reserved=(C.c_int32 * 4)(0, 1, 0, 0)), b"reserved"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_out_of_contract_launches_are_refused_on_the_host(name):
    """Every contract of the kernels is checked before any device work: the call returns an error and the text names the
    contract (the pointers are fakes - a check that let one of these through would be seen at once, here without a GPU as a
    HIP error with another text)."""
    make, text = REFUSALS[name]
    L = _lib.lib()
    ran = _lib.GemmRan()
    d = make()
    rc = L.mcg_debug_gemm(C.byref(d), C.byref(ran), None)
    msg = L.mcg_last_error()
    assert rc == 1 and msg.startswith(b"mcg_debug_gemm: ") and text in msg, (name, rc, msg)
    assert ran.kernel == 0


def test_null_arguments_and_the_pack_entry_refuse():
    L = _lib.lib()
    ran = _lib.GemmRan()
    assert L.mcg_debug_gemm(None, C.byref(ran), None) == 1 and b"mcg_debug_gemm" in L.mcg_last_error()
    d = valid_desc()
    assert L.mcg_debug_gemm(C.byref(d), None, None) == 1
    w = np.zeros((16, 8), dtype=np.float32)
    n = C.c_int64()
    assert L.mcg_debug_gemm_pack(None, 16, 8, 0, 0, None, 0, C.byref(n)) == 1 and b"mcg_debug_gemm_pack" in L.mcg_last_error()
    assert L.mcg_debug_gemm_pack(w.ctypes.data, 16, 6, 0, 0, None, 0, C.byref(n)) == 1
    assert L.mcg_debug_gemm_pack(w.ctypes.data, 16, 8, 0, 3, None, 0, C.byref(n)) == 1
    out = np.zeros(8, dtype=np.float32)
    assert L.mcg_debug_gemm_pack(w.ctypes.data, 16, 8, 0, 0, out.ctypes.data, out.size, C.byref(n)) == 1 and b"holds 8" in L.mcg_last_error()


# ------------------------------------------------------------------------------------------------ the pass rule
# (shape, family, a2_nsum) the stand-in is judged on: tails, two segments, gathers of every width, ragged edges, both epilogues
RULE_CASES = [
    (Shape(33, 44, 0, 4, "full", ACT_RELU, True, True), F32, 0),
    (Shape(17, 420, 420, 27, "full", ACT_SILU, True, True), F32ROWS16, 4),
    (Shape(49, 36, 28, 5, "m6", ACT_RELU, True, False), F32ROWS16, 3),
    (Shape(65, 420, 420, 27, "full", ACT_SILU, True, True), BF16, 4),
    (Shape(31, 60, 16, 3, "m4", ACT_RELU, True, True), BF16, 2),
    (Shape(129, 2048, 0, 8, "p1", ACT_NONE, True, False), X6, 0),
    (Shape(16, 4, 4, 1, "full", ACT_SILU, True, True), X6, 0),
]


@pytest.mark.parametrize("shape,family,nsum", RULE_CASES)
def test_honest_stand_in_passes_both_tiers(shape, family, nsum):
    from dataclasses import replace
    for tier in ("exact", "round"):
        s = replace(shape, act=ACT_RELU) if (tier == "exact" and shape.act == ACT_SILU) else shape
        inp = R.make_inputs(s, family, tier, nsum)
        failures, ratio = R.judge(inp, R.standin(inp))
        assert not failures, (tier, failures)
        assert tier == "exact" or ratio < 0.5, ratio          # an honest fp32 GEMM sits well inside the bound


def mutant_case(mutant):
    """(inputs, tier) on which the mutant must be caught."""
    gather4 = Shape(33, 36, 44, 5, "full", ACT_RELU, True, True)
    picks = {
        "drop_last_k_step": (Shape(33, 420, 420, 27, "full", ACT_NONE, True, True), F32ROWS16, 0),
        "tail_wrong_lane_group": (Shape(33, 44, 0, 4, "full", ACT_NONE, True, False), F32, 0),
        "seg2_plain_rows": (gather4, F32ROWS16, 4),
        "ignore_fourth_slot": (gather4, BF16, 4),
        "bias_of_next_tile": (Shape(17, 36, 0, 3, "m4", ACT_RELU, True, False), X6, 0),
        "resid_missing_on_last_piece": (Shape(17, 36, 0, 3, "m4", ACT_NONE, True, True), F32, 0),
        "relu_silu_swapped": (Shape(17, 36, 0, 3, "full", ACT_RELU, True, False), F32ROWS16, 0),
        "bf16_by_truncation": (Shape(65, 420, 420, 27, "full", ACT_NONE, True, True), BF16, 0),
        "write_column_past_n_store": (Shape(17, 36, 0, 3, "m6", ACT_NONE, True, False), F32, 0),
        "write_row_past_M": (Shape(17, 36, 0, 3, "full", ACT_NONE, True, False), F32, 0),
    }
    return picks[mutant]


@pytest.mark.parametrize("mutant", [m for m in R.MUTANTS if m != "div100_before_sum"])
def test_the_pass_rule_catches_the_mutant(mutant):
    """The project's mutation-check habit (tools/parity_sensitivity.py) applied to the new yardstick: a planted error of the kind
    GEMM kernels make must fail the rule in BOTH tiers (bf16 truncation: in the rounding tier - small integers are exact in
    bf16 however they are rounded; swapped activations: SiLU only exists in the rounding tier)."""
    from dataclasses import replace
    shape, family, nsum = mutant_case(mutant)
    tiers = ("round",) if mutant in ("bf16_by_truncation", "relu_silu_swapped") else ("exact", "round")
    for tier in tiers:
        inp = R.make_inputs(shape, family, tier, nsum)
        assert not R.judge(inp, R.standin(inp))[0]                     # the honest stand-in passes on the very same inputs
        failures, ratio = R.judge(inp, R.standin(inp, mutant))
        assert failures, (mutant, tier, ratio)
        if tier == "round" and not mutant.startswith("write_"):
            assert ratio > 5, (mutant, ratio)                          # ... and not by a hair
    if mutant == "relu_silu_swapped":
        inp = R.make_inputs(replace(shape, act=ACT_SILU), family, "round", nsum)
        assert R.judge(inp, R.standin(inp, mutant))[0]


def test_the_pass_rule_catches_division_before_the_sum():
    """`/ 100` per partial row instead of once on the sum changes a gathered bf16 operand only where the sum sits within a few
    fp32 ulps of a bf16 rounding boundary: on Gaussian data that is one element in ~10^4, and exact-tier rows (multiples of
    100) divide exactly either way.  So the gather is judged on rows built to sit there (adversarial_div100_pairs): every
    operand of segment 2 then rounds differently."""
    shape = Shape(33, 4, 16, 2, "full", ACT_NONE, True, False)
    inp = R.make_inputs(shape, BF16, "round", 2, adversarial_div100=True)
    assert not R.judge(inp, R.standin(inp))[0]
    failures, ratio = R.judge(inp, R.standin(inp, "div100_before_sum"))
    assert failures and ratio > 5, ratio


def test_c_view_reads_the_blocked_layout_of_the_comment():
    """column = 432 part + 32 k-block + 4 piece + (0..3) at C[part][k-block][piece][row][4]; the upper four pieces of each
    part's 14th block belong to nobody."""
    shape = Shape(5, 4, 0, 54)
    inp = R.make_inputs(shape, F32, "exact", c_blocked=True)
    buf = inp.c_buffer()
    M = shape.M
    c5 = buf[:896 * M].reshape(2, 14, 8, M, 4)
    for part in range(2):
        for kb in range(14):
            for piece in range(8):
                if kb == 13 and piece >= 4:
                    continue
                for e in range(4):
                    c5[part, kb, piece, :, e] = 1000 * (432 * part + 32 * kb + 4 * piece + e) + np.arange(M)
    c, written = R.c_view(inp, buf)
    assert np.array_equal(c, 1000 * np.arange(864)[None, :] + np.arange(M)[:, None])
    assert written.sum() == 864 * M and not written.reshape(-1)[:896 * M].reshape(2, 14, 8, M, 4)[:, 13, 4:].any()
    assert np.all(buf[~written] == R.SENTINEL)
