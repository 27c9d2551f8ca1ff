"""The K seams of the fp32 node GEMMs (csrc/mcg_gemm_kernels.h, mcg_gemm_f32_tile), crossed densely on BOTH sides.

Those kernels run one operand pipeline per launch: the K % 16 tail steps of both segments are requested at the head of the
kernel, segment 1 is front-padded to whole ring trips and its last trip refills the ring with the first groups of segment 2.
tests/test_gemm_gpu.py crosses the K1 seams densely and hardly the segment seam; here the literal table below puts
groups = K / 16 in {0, 1, 2, 3, 4} on both sides of it, with and without tail steps (K % 16 in {0, 4, 12}), i.e. fewer groups
than the ring is deep, exactly as many, one more, a segment that is a tail only, against ring depths 3, 6 and 8.  Same harness
(`mcg_debug_gemm`, one launch at a time), same float64 restatement and pass rule (tests/gemm_ref.py), both tiers, and on
identical inputs every instantiation of a family must agree bit for bit: neither the tile shape nor the ring depth changes
the k order of an output element."""
import pytest

from gemm_ref import ACT_NONE, ACT_RELU, ACT_SILU, F32, F32ROWS16, Shape
from test_gemm_gpu import TIERS, f32_selections, rows16_selections, run_group

pytestmark = pytest.mark.gpu

MS = (17, 33)
K1S = (4, 12, 16, 20, 36, 52, 68)
K2S = (4, 12, 20, 36, 52, 68)
ACTS = (ACT_NONE, ACT_RELU, ACT_SILU)
# bias on, a residual on every second row of the table, the three activations in turn (the exact tier runs SiLU rows as ReLU)
SEAMS = [Shape(m, k1, k2, 3, "full", ACTS[i % 3], True, i % 2 == 1)
         for i, (m, k1, k2) in enumerate((m, k1, k2) for m in MS for k1 in K1S for k2 in K2S)]
assert len(SEAMS) == 84 and sum(s.resid for s in SEAMS) == 42
assert {(s.K1 // 16, s.K2 // 16) for s in SEAMS} >= {(a, b) for a in range(5) for b in range(5)}

# ring depths behind rows16_selections: 3 for every tile shape, 8 and 6 for the deep narrow tiles (rn 1 and 2, mr 1)
assert sorted({sel[5][3] for sel in rows16_selections(0)}) == [3, 6, 8]

F32_CASES = [(i, t) for i in range(len(SEAMS)) for t in TIERS]
ROWS16_CASES = [(i, t, n) for i in range(len(SEAMS)) for t in TIERS for n in (0, 2, 3, 4)]


def _id(case):
    s = SEAMS[case[0]]
    return "-".join([f"M{s.M}-K{s.K1}+{s.K2}", case[1]] + [f"nsum{n}" for n in case[2:]])


@pytest.mark.parametrize("case", F32_CASES, ids=_id)
def test_seams_32row_kernel(case):
    """Both segments through the 32-row kernel (plain rows on either side of the seam), RN 1, 2, 3."""
    i, tier = case
    run_group(SEAMS[i], F32, tier, 0, f32_selections())


@pytest.mark.parametrize("case", ROWS16_CASES, ids=_id)
def test_seams_16row_kernel(case):
    """The 16-row kernel, segment 2 as plain rows and as the sum of 2, 3 and 4 gathered rows, every tile shape, ring 3 / 6 / 8."""
    i, tier, nsum = case
    run_group(SEAMS[i], F32ROWS16, tier, nsum, rows16_selections(nsum))
