"""High-precision restatement of ONE node / GCN GEMM launch (csrc/mcg_gemm.hip) and the rule a kernel's output passes by.
Plain numpy / torch on the CPU; tests/test_gemm_host.py holds it against mutants, tests/test_gemm_gpu.py holds the kernels
against it through `mcg_debug_gemm`.

The operation, in float64:

    C = act(A1 W1^T + G(A2) W2^T + bias) + resid        rows >= M and columns >= n_store untouched

G is the identity or the gather: the sum of rows a2_rows[r][0 ..] of A2 in slot order, accumulated in fp32 exactly as the
kernels do, ((a + b) + c) + d, followed in the Bf16 family only by an fp32 division by 100 (mcg_div100 is bit-identical to
x / 100.0f).  The fp32 16-row kernel sums a2_nsum rows (2, 3 or 4), the bf16 kernels 2, or 4 for a2_nsum 3 and 4.  For the Bf16
family the operands of the contraction (A after gather and division, and W) are first rounded to bf16, round to nearest even
(mcg_f32_to_bf16_bits); for X6 they stay fp32.  The contraction itself is float64.

The pass rule has two tiers, neither with a tuned tolerance for the linear part:

* exact: small-integer operands (|A|, |W| <= 8, integer bias / residual, gather partial rows integers - multiples of 100 for
  the bf16 gather -, K <= 2048 + 420): every product and partial sum is an integer below 2^24, exact in fp32 in any order, in
  bf16 and in the three-part split, so with act none / ReLU the output must be torch.equal to the float64 result cast to fp32.
* rounding: Gaussian operands, W scaled by K^-1/2; componentwise |C - C64| <= gamma (|A||W|^T + |bias| + |resid|) with
  gamma = (K1 + K2 + n_gather + 3) 2^-24 (an fp32 dot product summed in any order, plus one rounding each for bias, residual
  and division); X6 adds 3 * 2^-23 |A||W|^T for its three dropped partial products (include/mlconfgen_hip.h,
  mcg_egnn_set_precision).  SiLU: 1.1 x that (max |silu'| = 1.1) + EPS_SILU |silu(v)|.

Canaries are part of the rule: C is pre-filled with SENTINEL (leading-dimension padding, columns >= n_store, 64 rows past M)
and all of it must survive; the input buffers carry guard rows and must come back unchanged.  The floats of every A row
between K and the next multiple of 32 (which the bf16 / x6 kernels read and zero weights cancel) hold the finite POISON."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

F32, F32ROWS16, BF16, X6 = 0, 1, 2, 3                       # mcg_gemm_desc.family
FAMILY_NAME = {F32: "F32", F32ROWS16: "F32Rows16", BF16: "Bf16", X6: "X6"}
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2
SENTINEL = np.float32(-725000.0)
POISON = np.float32(1e30)
GUARD_ROWS = 2
C_GUARD_ROWS = 64
U24 = 2.0 ** -24

# Evaluation error of mcg_silu (v_exp_f32 / v_rcp_f32) against float64 x * sigmoid(x): TWICE the worst relative error measured
# through the harness itself on a grid over [-20, 20] (tests/test_gemm_gpu.py::test_silu_evaluation_error, K1 = 4, one 1 per
# weight row).  Measured on an MI355X: 1.012e-06 for the three fp32-operand families, 8.749e-07 for Bf16, worst near x = -18
# where the error of the exponent's fp32 argument dominates (profiles/gemm_harness.txt).  The factor 2: a grid samples, it does
# not enumerate.
EPS_SILU = 2 * 1.0122e-6


def store_columns(n_tiles: int, kind: str) -> int:
    return {"full": 16 * n_tiles, "m4": 16 * n_tiles - 4, "m6": 16 * n_tiles - 6, "p1": 16 * (n_tiles - 1) + 1}[kind]


@dataclass(frozen=True)
class Shape:
    """One row of a test's literal shape table."""
    M: int
    K1: int
    K2: int
    n_tiles: int
    store: str = "full"          # n_store: "full" 16 n, "m4" 16 n - 4, "m6" 16 n - 6 (the GCN's 210 of 224), "p1" 16 (n - 1) + 1
    act: int = ACT_NONE
    bias: bool = True
    resid: bool = False

    @property
    def n_store(self) -> int:
        return store_columns(self.n_tiles, self.store)

    def __post_init__(self):
        assert self.K1 >= 4 and self.K1 % 4 == 0 and self.K2 % 4 == 0
        assert not (self.resid and self.n_store % 4), "a residual takes n_store % 4 == 0"


def round_bf16(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 -> fp32, round to nearest even: the rule of mcg_f32_to_bf16_bits (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (u.astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def truncate_bf16(x: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(x))


def silu64(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return v / (1.0 + np.exp(-v))


def pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def kpad32(k: int) -> int:
    return (k + 31) // 32 * 32


def gather_width(family: int, nsum: int) -> int:
    """Rows of A2 a kernel of `family` sums per output row (0: plain rows): gather_rows() / the 16-row launcher."""
    if nsum == 0:
        return 0
    return (4 if nsum > 2 else 2) if family == BF16 else nsum


@dataclass
class Inputs:
    shape: Shape
    family: int
    tier: str                    # "exact" | "round"
    nsum: int                    # a2_nsum (0: no gather)
    a1: np.ndarray               # [M + GUARD_ROWS][lda1], pad columns and guard rows POISON
    a2: Optional[np.ndarray]     # [rows + GUARD_ROWS][lda2]
    a2_src_rows: int
    slots: Optional[np.ndarray]  # int32 [M][4]
    w: np.ndarray                # [n_out][K1 + K2]
    bias: Optional[np.ndarray]   # [n_out]
    resid: Optional[np.ndarray]  # [M + GUARD_ROWS][ldr]
    n_out: int
    ldc: int
    c_blocked: bool = False

    def c_buffer(self) -> np.ndarray:
        """C as the caller hands it over: SENTINEL everywhere."""
        if self.c_blocked:
            return np.full(896 * self.shape.M + 256, SENTINEL, dtype=np.float32)
        return np.full((self.shape.M + C_GUARD_ROWS, self.ldc), SENTINEL, dtype=np.float32)


def adversarial_div100_pairs(rng: np.random.Generator, n: int) -> np.ndarray:
    """fp32 pairs (a, b) for which summing then dividing, bf16(fl(fl(a + b) / 100)), and dividing then summing,
    bf16(fl(fl(a / 100) + fl(b / 100))), round to DIFFERENT bf16 values: the sum / 100 sits a few fp32 ulps from a bf16
    rounding boundary.  Returns [n][2]."""
    out = np.zeros((0, 2), dtype=np.float32)
    hundred = np.float32(100)
    while len(out) < n:
        m = 8 * n + 4096
        lo = round_bf16(rng.uniform(0.25, 4.0, m).astype(np.float32) * rng.choice([-1.0, 1.0], m).astype(np.float32))
        mid = lo.astype(np.float64) * (1 + 2.0 ** -8)                       # half-way to the next bf16 value (away from zero)
        s = (mid * 100).astype(np.float32)
        s = (s.view(np.int32) + rng.integers(-3, 4, m).astype(np.int32)).view(np.float32)
        a = (s * rng.uniform(0.1, 0.9, m).astype(np.float32)).astype(np.float32)
        b = (s - a).astype(np.float32)
        first = round_bf16(((a + b).astype(np.float32) / hundred).astype(np.float32))
        second = round_bf16(((a / hundred).astype(np.float32) + (b / hundred).astype(np.float32)).astype(np.float32))
        keep = first != second
        out = np.concatenate([out, np.stack([a[keep], b[keep]], axis=1)])
    return out[:n]


def make_inputs(shape: Shape, family: int, tier: str, nsum: int = 0, seed: int = 0, c_blocked: bool = False,
                adversarial_div100: bool = False) -> Inputs:
    """Deterministic operands of one launch.  The same (shape, family kind, tier, nsum, seed) gives the same data, so every
    instantiation of a family sees identical inputs."""
    assert tier in ("exact", "round") and (nsum == 0 or (shape.K2 > 0 and family in (F32ROWS16, BF16)))
    rng = np.random.default_rng([seed, shape.M, shape.K1, shape.K2, shape.n_tiles, nsum, family == BF16, tier == "exact"])
    M, K1, K2, K = shape.M, shape.K1, shape.K2, shape.K1 + shape.K2
    n_store = shape.n_store
    n_out = n_store
    wide = family in (BF16, X6)

    def values(rows, cols, scale=1.0, bound=8):
        if tier == "exact":
            return rng.integers(-bound, bound + 1, (rows, cols)).astype(np.float32)
        return (rng.standard_normal((rows, cols)) * scale).astype(np.float32)

    def operand(rows, k, data):
        # the network's 420-wide rows live in 432-wide buffers; otherwise the row covers what a kernel reads, plus 4
        ld = 432 if k == 420 else (kpad32(k) if wide else k) + 4
        buf = np.full((rows + GUARD_ROWS, ld), POISON, dtype=np.float32)
        buf[:rows, :k] = data
        return buf

    a1 = operand(M, K1, values(M, K1))
    a2 = slots = None
    src_rows = 0
    if K2 > 0 and nsum == 0:
        a2 = operand(M, K2, values(M, K2))
    elif K2 > 0:
        src_rows = M + 5
        unit = np.float32(100.0) if family == BF16 else np.float32(1.0)
        data = values(src_rows, K2, scale=0.5, bound=2) * unit
        data[0] = 0.0                                                       # the shared zero row
        width = gather_width(family, nsum)
        slots = np.zeros((M, 4), dtype=np.int32)
        for r in range(M):
            pick = rng.choice(np.arange(1, src_rows), size=4, replace=False).astype(np.int32)
            kind = r % 4
            if kind == 0:
                s = [pick[0], 0, 0, 0]                                      # unused slots name the zero row
            elif kind == 1:
                s = [pick[0], pick[0], pick[1], 0]                          # the same row twice
            elif kind == 2:
                s = sorted(pick, reverse=True)                              # descending rows
            else:
                s = list(pick)
            for q in range(4):
                if q >= width:
                    s[q] = pick[3]                                          # never read: a decoy with data in it
                elif q >= nsum:
                    s[q] = 0                                                # bf16, a2_nsum 3 taken as 4: the zero row
            slots[r] = s
        if adversarial_div100:
            assert family == BF16 and nsum == 2 and tier == "round"
            pairs = adversarial_div100_pairs(rng, M * K2).reshape(M, K2, 2)
            src_rows = 2 * M + 1
            data = np.zeros((src_rows, K2), dtype=np.float32)
            data[1:M + 1] = pairs[:, :, 0]
            data[M + 1:] = pairs[:, :, 1]
            slots = np.stack([np.arange(1, M + 1), np.arange(M + 1, 2 * M + 1), np.zeros(M), np.zeros(M)], axis=1).astype(np.int32)
        a2 = operand(src_rows, K2, data)
    w = values(n_out, K, scale=K ** -0.5)
    bias = values(1, n_out)[0] if shape.bias else None
    resid = None
    if shape.resid:
        resid = np.full((M + GUARD_ROWS, pad4(n_store) + 8), SENTINEL, dtype=np.float32)
        resid[:M, :n_store] = values(M, n_store)
    return Inputs(shape, family, tier, nsum, a1, a2, src_rows, slots, w, bias, resid, n_out, pad4(n_store) + 4, c_blocked)


def gathered_a2(inp: Inputs) -> Optional[np.ndarray]:
    """Segment 2's activation rows as the kernel forms them, in fp32: plain rows, or the slot-ordered sum (/ 100 for Bf16)."""
    s = inp.shape
    if s.K2 == 0:
        return None
    if inp.slots is None:
        return inp.a2[:s.M, :s.K2].copy()
    width = gather_width(inp.family, inp.nsum)
    acc = inp.a2[inp.slots[:, 0], :s.K2].copy()
    for q in range(1, width):
        acc = (acc + inp.a2[inp.slots[:, q], :s.K2]).astype(np.float32)
    if inp.family == BF16:
        acc = (acc / np.float32(100)).astype(np.float32)
    return acc


@dataclass
class Reference:
    c64: np.ndarray              # [M][n_store] float64
    pre: np.ndarray              # pre-activation, float64
    linear_bound: np.ndarray     # gamma (|A||W|^T + |bias| + |resid|) (+ the X6 term)
    bound: np.ndarray            # what |C - c64| must stay within in the rounding tier


def reference(inp: Inputs) -> Reference:
    s = inp.shape
    n_store = s.n_store
    a = inp.a1[:s.M, :s.K1]
    g = gathered_a2(inp)
    if g is not None:
        a = np.concatenate([a, g], axis=1)
    w = np.zeros((n_store, s.K1 + s.K2), dtype=np.float32)
    w[:min(inp.n_out, n_store)] = inp.w[:n_store]
    if inp.family == BF16:
        a, w = round_bf16(a), round_bf16(w)
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    bias = np.zeros(n_store)
    if inp.bias is not None:
        bias[:min(inp.n_out, n_store)] = inp.bias[:n_store]
    resid = inp.resid[:s.M, :n_store].astype(np.float64) if inp.resid is not None else np.zeros((s.M, n_store))
    pre = a64 @ w64.T + bias
    mag = np.abs(a64) @ np.abs(w64).T
    gamma = (s.K1 + s.K2 + gather_width(inp.family, inp.nsum) + 3) * U24
    lin = gamma * (mag + np.abs(bias) + np.abs(resid))
    if inp.family == X6:
        lin = lin + 3 * 2.0 ** -23 * mag
    if s.act == ACT_SILU:
        assert np.abs(pre).max() <= 20.0, "rounding-tier pre-activations stay within [-20, 20]"
        act = silu64(pre)
        bound = 1.1 * lin + EPS_SILU * np.abs(act)
    else:
        act = np.maximum(pre, 0.0) if s.act == ACT_RELU else pre
        bound = lin
    return Reference(act + resid, pre, lin, bound)


def c_view(inp: Inputs, c_buf: np.ndarray):
    """(C[M][n_store], mask of the buffer's elements a launch may write) read through the layout: row-major, or the blocked
    layout of McgGemmArgs' comment, C[part][k-block][piece][row][4] with column = 432 part + 32 k-block + 4 piece + (0..3)."""
    s = inp.shape
    M, n_store = s.M, s.n_store
    written = np.zeros(c_buf.shape, dtype=bool)
    if not inp.c_blocked:
        written[:M, :n_store] = True
        return c_buf[:M, :n_store], written
    col = np.arange(n_store)
    part, within = col // 432, col % 432
    base = ((part * 14 + within // 32) * 8 + (within % 32) // 4)
    idx = (base[None, :] * M + np.arange(M)[:, None]) * 4 + (col % 4)[None, :]
    written[idx] = True
    return c_buf[idx], written


def judge(inp: Inputs, c_buf: np.ndarray, ref: Optional[Reference] = None):
    """The pass rule on one launch's C buffer.  Returns (failures, worst |error| / bound): `failures` is empty when the launch
    passes.  Every one of the M x n_store outputs is judged; every other element of the buffer must still be SENTINEL."""
    ref = ref or reference(inp)
    s = inp.shape
    failures = []
    c, written = c_view(inp, c_buf)
    outside = c_buf[~written]
    if not np.array_equal(outside, np.full_like(outside, SENTINEL)):
        where = np.argwhere((c_buf != SENTINEL) & ~written)
        failures.append(f"{len(where)} element(s) outside C[:M, :n_store] were written, first at {tuple(where[0])}")
    if not np.all(np.isfinite(c)):
        failures.append("non-finite output")
        return failures, float("inf")
    err = np.abs(c.astype(np.float64) - ref.c64)
    ratio = float((err / np.maximum(ref.bound, np.finfo(np.float64).tiny)).max())
    if inp.tier == "exact":
        assert s.act != ACT_SILU, "the exact tier takes act none / ReLU"
        if not torch.equal(torch.from_numpy(np.ascontiguousarray(c)), torch.from_numpy(ref.c64.astype(np.float32))):
            bad = np.argwhere(c != ref.c64.astype(np.float32))
            r, q = bad[0]
            failures.append(f"exact tier: {len(bad)} of {c.size} outputs differ, first C[{r}][{q}] = {c[r, q]!r}, expected {ref.c64[r, q]!r}")
    else:
        bad = np.argwhere(err > ref.bound)
        if len(bad):
            r, q = bad[np.argmax((err / np.maximum(ref.bound, 1e-300))[tuple(bad.T)])]
            failures.append(f"rounding tier: {len(bad)} of {c.size} outputs exceed the bound, worst C[{r}][{q}] = {c[r, q]!r} vs {ref.c64[r, q]!r}: "
                            f"|err| {err[r, q]:.3e} = {err[r, q] / ref.bound[r, q]:.3g} x bound")
    return failures, ratio


# ---------------------------------------------------------------------------------------------- side job
def side_job_inputs(side_M: int, seed: int = 0):
    """u[rows][4], slots[side_M][4], x[side_M + GUARD_ROWS][4] of the coordinate-update side job."""
    rng = np.random.default_rng([seed, side_M, 77])
    rows = side_M + 5
    u = (rng.standard_normal((rows, 4)) * 30).astype(np.float32)
    u[0] = 0.0
    slots = rng.integers(0, rows, (side_M, 4)).astype(np.int32)
    slots[::3, 2:] = 0
    x = rng.standard_normal((side_M + GUARD_ROWS, 4)).astype(np.float32)
    return u, slots, x


def side_job_reference(u, slots, x, side_M):
    """x[v][0..2] += (((u[s.x] + u[s.y]) + u[s.z]) + u[s.w]) / 100 in float64, component 3 untouched; the bound is four fp32
    roundings of the magnitudes involved."""
    u64 = u.astype(np.float64)
    terms = u64[slots]                                      # [side_M][4 slots][4 components]
    x64 = x.astype(np.float64).copy()
    x64[:side_M, :3] += terms.sum(axis=1)[:, :3] / 100.0
    bound = np.zeros_like(x64)
    bound[:side_M, :3] = 4 * U24 * (np.abs(x.astype(np.float64))[:side_M, :3] + np.abs(terms).sum(axis=1)[:, :3] / 100.0)
    return x64, bound


# ---------------------------------------------------------------------------------------------- CPU stand-in and its mutants
MUTANTS = ("drop_last_k_step", "tail_wrong_lane_group", "seg2_plain_rows", "ignore_fourth_slot", "div100_before_sum",
           "bias_of_next_tile", "resid_missing_on_last_piece", "relu_silu_swapped", "bf16_by_truncation",
           "write_column_past_n_store", "write_row_past_M")


def standin(inp: Inputs, mutant: Optional[str] = None) -> np.ndarray:
    """A CPU stand-in for the kernels: fp32 torch matmul with the gather and the epilogue restated; `mutant` plants one of
    the errors GEMM kernels actually make.  Returns the C buffer (row-major)."""
    assert mutant is None or mutant in MUTANTS
    s = inp.shape
    M, K1, K2, n_store = s.M, s.K1, s.K2, s.n_store
    a1 = inp.a1[:M, :K1].copy()
    if K2 > 0 and inp.slots is not None:
        width = gather_width(inp.family, inp.nsum)
        if mutant == "seg2_plain_rows":
            g = inp.a2[:M, :K2].copy()
            if inp.family == BF16:
                g = (g / np.float32(100)).astype(np.float32)
        else:
            if mutant == "ignore_fourth_slot":
                assert width == 4
                width = 3
            rows = [inp.a2[inp.slots[:, q], :K2] for q in range(width)]
            if mutant == "div100_before_sum":
                assert inp.family == BF16
                rows = [(r / np.float32(100)).astype(np.float32) for r in rows]
            g = rows[0].copy()
            for r in rows[1:]:
                g = (g + r).astype(np.float32)
            if inp.family == BF16 and mutant != "div100_before_sum":
                g = (g / np.float32(100)).astype(np.float32)
    else:
        assert mutant not in ("seg2_plain_rows", "ignore_fourth_slot", "div100_before_sum")
        g = inp.a2[:M, :K2].copy() if K2 > 0 else None
    w = np.zeros((n_store, K1 + K2), dtype=np.float32)
    w[:min(inp.n_out, n_store)] = inp.w[:n_store]
    segs = [(a1, w[:, :K1])] + ([(g, w[:, K1:])] if g is not None else [])
    if mutant == "drop_last_k_step":
        a, ws = segs[-1]
        segs[-1] = (a[:, :-4], ws[:, :-4])
    if mutant == "tail_wrong_lane_group":
        # a tail step holds k = 16 Q + 4 st + g for lane group g: the activation taken from the neighbouring group
        a, ws = segs[0]
        full = K1 // 16 * 16
        assert full < K1, "needs a K tail"
        a = a.copy()
        for st in range((K1 - full) // 4):
            a[:, full + 4 * st:full + 4 * st + 4] = np.roll(a[:, full + 4 * st:full + 4 * st + 4], 1, axis=1)
        segs[0] = (a, ws)
    if inp.family == BF16:
        rnd = truncate_bf16 if mutant == "bf16_by_truncation" else round_bf16
        segs = [(rnd(a), rnd(ws)) for a, ws in segs]
    else:
        assert mutant != "bf16_by_truncation"
    acc = torch.zeros((M, n_store), dtype=torch.float32)
    for a, ws in segs:
        acc = acc + torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(ws)).T
    if inp.bias is not None:
        b = np.zeros(16 * s.n_tiles + 16, dtype=np.float32)
        b[:inp.n_out] = inp.bias
        if mutant == "bias_of_next_tile":
            b = np.roll(b, -16)
        acc = acc + torch.from_numpy(b[:n_store])
    else:
        assert mutant != "bias_of_next_tile"
    act = s.act
    if mutant == "relu_silu_swapped":
        assert act != ACT_NONE
        act = ACT_RELU if act == ACT_SILU else ACT_SILU
    if act == ACT_SILU:
        acc = acc * torch.sigmoid(acc)
    elif act == ACT_RELU:
        acc = torch.relu(acc)
    if inp.resid is not None:
        r = inp.resid[:M, :n_store].copy()
        if mutant == "resid_missing_on_last_piece":
            r[:, n_store - 4:] = 0.0
        acc = acc + torch.from_numpy(r)
    else:
        assert mutant != "resid_missing_on_last_piece"
    c = inp.c_buffer()
    c[:M, :n_store] = acc.numpy()
    if mutant == "write_column_past_n_store":
        c[M // 2, n_store] = 1.0
    if mutant == "write_row_past_M":
        c[M, 0] = 1.0
    return c
