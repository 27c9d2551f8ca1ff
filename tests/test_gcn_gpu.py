"""GPU pins of the bond-prediction GCN (AdjMatSeer, csrc/mcg_gcn.hip) stage by stage against the fp64 restatement
`tests/gcn_ref.py`, through `mcg_gcn_peek`.  Every numeric comparison is against fp64; B <= 16 everywhere.

Stage tolerances (gcn_ref.STAGE_TOL): `parity_tolerance.violation` with S = the stage's own maximum and the project's
rtol 1e-4 / atol 1e-5 scaled per stage by  min(1, 16 x the fp32 CPU restatement's own worst deviation from fp64) - the 16
for a different summation order over K = 2048.  Measured on the CPU over the four input sets at B = 16 and both weight sets
(seed 4321 at gain 1.0 and at weight_gain 2.45), in units of the project tolerance, and the fraction of it chosen:

    stage        fp32 vs fp64    tolerance (x rtol 1e-4 / atol 1e-5)
    L_dm            0.0026          0.0416
    L_adj           0.0012          0.0192
    bottleneck      0.018           0.288
    scale           0.045           0.72
    e0              0.040           0.64
    xb              0.053           0.848
    res             0.050           0.8
    logits          0.049           0.784

None of these comes from a kernel's output.  (For the record, the kernels' worst on an MI355X, in units of the stage's
tolerance: L_dm 0.071, L_adj 0.050, bottleneck 0.051, scale 0.076, e0 0.078, xb 0.114, res 0.125, logits 0.106; every test
prints its own.)  tests/test_gcn_host.py shows on the CPU that every planted mistake of
gcn_ref.MUTATIONS reaches >= 10 x one of these tolerances on one of these input sets
(profiles/gcn_parity_sensitivity.txt)."""
import ctypes as C

import pytest
import torch

import gcn_ref as R
from ml_conformer_generator_amd import _lib
from parity_tolerance import violation

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PEEK = {q: k for k, q in enumerate(R.STAGES)}


def new_model(sd):
    from ml_conformer_generator_amd.adj_mat_seer import AdjMatSeer
    m = AdjMatSeer(device=DEV)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def weights():
    return {wn: R.weight_set(wn) for wn in R.WEIGHT_SETS}


@pytest.fixture(scope="module")
def models(weights):
    return {wn: new_model(sd) for wn, sd in weights.items()}


@pytest.fixture(scope="module")
def sets():
    s = R.input_sets(16)
    s["control"] = R.junk_inputs(junk=False)
    return s


@pytest.fixture(scope="module")
def ref64(weights, sets):
    """fp64 restatement, computed once per (weights, input set) on first use and left unchanged."""
    cache = {}

    def get(wn, sn):
        if (wn, sn) not in cache:
            el, dm, am, _ = sets[sn]
            with torch.no_grad():
                cache[(wn, sn)] = R.gcn_forward(weights[wn], el, dm, am, torch.float64)
        return cache[(wn, sn)]
    return get


def rows_of(ref, q, lo, hi):
    """molecules lo..hi-1 of a reference stage (xb is stored [B*42, 2048])."""
    t = ref[q]
    if q == "xb":
        return t.reshape(-1, R.D, R.HID)[lo:hi].reshape(-1, R.HID)
    return t[lo:hi]


def stage_violations(m, B, logits, ref, lo=0):
    """{quantity: violation in units of its stage tolerance} of the last forward (B molecules = rows lo.. of ref)."""
    out = {}
    for q in R.STAGES:
        out[q] = R.stage_violation(m._peek(PEEK[q], B).cpu(), rows_of(ref, q, lo, lo + B), q)
    out["logits"] = R.stage_violation(logits.cpu(), rows_of(ref, "logits", lo, lo + B), "logits")
    return out


def assert_stages(v, what):
    print(f"{what}: worst violation per stage (x stage tolerance): " + "  ".join(f"{q} {v[q]:.3f}" for q in R.QUANTITIES))
    bad = {q: round(x, 3) for q, x in v.items() if not x <= 1.0}
    assert not bad, f"{what}: outside the stage tolerance: {bad}"


@pytest.mark.parametrize("wn", list(R.WEIGHT_SETS))
@pytest.mark.parametrize("sn", ["sym", "asym", "elements", "junk"])
def test_stage_pins_vs_fp64(models, sets, ref64, wn, sn):
    """All seven peeks and the logits against fp64: the edge sizes [1, 2, 15, 27, 41, 42] plus ten ragged rows (sym); independent
    upper and lower triangles, where L^T and column degrees show (asym); every element id 0..35 in a real position (elements);
    junk in the padded rows and columns, which the reference reads (junk)."""
    el, dm, am, sizes = sets[sn]
    m, B = models[wn], len(sizes)
    bond, logits = m.bond_orders(el, dm, am, with_logits=True)
    assert_stages(stage_violations(m, B, logits, ref64(wn, sn)), f"{wn} / {sn}")
    logits = logits.cpu()
    assert torch.equal(logits, logits.transpose(1, 2))                                   # exactly symmetric, asymmetric inputs too
    assert torch.equal(torch.argmax(logits, -1).to(torch.int8), bond.cpu())
    res = m._peek(PEEK["res"], B).cpu()
    assert torch.equal(logits, res.transpose(1, 2) + res)                                # k_symm is exact on what res holds
    m.check_inputs_seen()                                                                # ids 0 and 35 are in range


def test_out_of_range_element_ids_are_flagged_and_stay_in_their_molecule(models, weights, sets):
    """Ids 36 and -1 (nn.Embedding would raise): the kernel reads table row 0 instead of out of bounds and sets a sticky
    flag; the other molecules of the batch are bit-identical to a clean run."""
    el, dm, am, sizes = sets["elements"]
    clean = models["gain1"](el, dm, am).cpu()
    models["gain1"].check_inputs_seen()
    dirty = new_model(weights["gain1"])
    dirty.check_inputs_seen()
    bad = el.clone()
    bad[1, 3], bad[2, 0] = 36, -1
    got = dirty(bad, dm, am).cpu()
    with pytest.raises(IndexError):
        dirty.check_inputs_seen()
    assert torch.equal(got[0], clean[0]) and torch.equal(got[3], clean[3])
    assert not torch.equal(got[1], clean[1]) and not torch.equal(got[2], clean[2])
    as_zero = el.clone()
    as_zero[1, 3], as_zero[2, 0] = 0, 0                                                  # the documented clamp: row 0
    assert torch.equal(got, models["gain1"](as_zero, dm, am).cpu())
    dirty(el, dm, am)
    with pytest.raises(IndexError):                                                      # sticky
        dirty.check_inputs_seen()


def test_argmax_and_layout_exact_on_ties(weights, sets):
    """resize.weight = 0: res[b, i, j, c] = bias[j*5 + c] whatever the network computed, so the logits are
    bias[j*5 + c] + bias[i*5 + c] bit for bit (multiples of 0.25: every sum exact) and `bond` is the lowest tied class."""
    sd = dict(weights["gain1"])
    g = torch.Generator().manual_seed(23)
    bias = torch.randint(0, 3, (R.D, R.NB), generator=g).float() * 0.25
    bias[0], bias[7] = 0.25, 0.5                                                        # pairs among {0, 7}: five-way ties
    sd["resize.weight"] = torch.zeros_like(sd["resize.weight"])
    sd["resize.bias"] = bias.reshape(-1).clone()
    m = new_model(sd)
    el, dm, am, _ = sets["sym"]
    el, dm, am = el[3:6], dm[3:6], am[3:6]
    want = (bias.unsqueeze(0) + bias.unsqueeze(1)).unsqueeze(0).expand(3, -1, -1, -1)    # [b, i, j, c]
    n_max = (want == want.max(-1, keepdim=True).values).sum(-1)
    assert int((n_max == 2).sum()) > 100 and int((n_max == 5).sum()) >= 4 * 3 and int((n_max == 1).sum()) > 100
    first = torch.argmax(want, -1)
    assert int((first[n_max == 5] != 0).sum()) == 0                                      # torch.argmax: the first maximum
    bond, logits = m.bond_orders(el, dm, am, with_logits=True)
    assert torch.equal(logits.cpu(), want)
    assert torch.equal(bond.cpu(), first.to(torch.int8))
    assert torch.equal(m.bond_orders(el, dm, am).cpu(), first.to(torch.int8))


def test_workspace_regrow_shrink_and_padding_junk(weights, sets, ref64):
    """B = 2, then 9, then 3 on one instance: each row bit-identical to that row run alone, each peek still within its
    tolerance after the regrow and after the shrink; then junk beyond n on the same workspace against fp64 on the same junk."""
    m, solo = new_model(weights["gain1"]), new_model(weights["gain1"])
    el, dm, am, sizes = sets["control"]
    alone = [solo.bond_orders(el[b:b + 1], dm[b:b + 1], am[b:b + 1], with_logits=True) for b in range(len(sizes))]
    alone = [(bd[0].cpu(), lg[0].cpu()) for bd, lg in alone]
    L, buf = _lib.lib(), torch.empty(9 * R.D * R.D * R.NB, device=DEV)
    assert L.mcg_gcn_peek(m._h, 0, 1, _lib.dptr(buf), None) != 0                         # nothing sized yet
    ref = ref64("gain1", "control")
    for lo, hi in ((0, 2), (0, 9), (4, 7)):
        bond, logits = m.bond_orders(el[lo:hi], dm[lo:hi], am[lo:hi], with_logits=True)
        for k in range(hi - lo):
            assert torch.equal(bond[k].cpu(), alone[lo + k][0]) and torch.equal(logits[k].cpu(), alone[lo + k][1]), (lo, hi, k)
        assert_stages(stage_violations(m, hi - lo, logits, ref, lo), f"control rows {lo}..{hi - 1}")
    for which, B in ((7, 1), (-1, 1), (0, 0), (0, 10)):                                  # unknown buffer, B outside 1..9
        assert L.mcg_gcn_peek(m._h, which, B, _lib.dptr(buf), None) != 0
        assert b"mcg_gcn_peek" in L.mcg_last_error()
    assert L.mcg_gcn_peek(m._h, 6, 9, None, None) != 0
    with pytest.raises(ValueError):
        m._peek(7, 1)
    jel, jdm, jam, _ = sets["junk"]
    jref = ref64("gain1", "junk")
    assert violation(jref["logits"][:5], ref["logits"][:5]) > 100                        # the junk matters to the reference
    assert torch.equal(jref["logits"][5], ref["logits"][5])                              # n = 42: no padding, no junk
    bond, logits = m.bond_orders(jel, jdm, jam, with_logits=True)
    assert_stages(stage_violations(m, 9, logits, jref), "junk beyond n")
    assert torch.equal(logits[5].cpu(), alone[5][1]) and not torch.equal(logits[3].cpu(), alone[3][1])


def test_output_guards_and_optional_outputs(models, sets):
    """Sentinels on either side of `logits` and `bond`: no call writes outside its buffer, a NULL output is honoured, and the
    logits-only, bond-only and combined calls agree bit for bit."""
    el, dm, am, _ = sets["asym"]
    B, G = 5, 64
    el, dm, am = el[:B].to(DEV).contiguous(), dm[:B].to(DEV).contiguous(), am[:B].to(DEV).contiguous()
    n = B * R.D * R.D
    m, L = models["gain1"], _lib.lib()
    st = _lib.current_stream_ptr(DEV)
    SF, SB = 12345.678, 90

    def run(want_logits, want_bond):
        fl = torch.full((G + n * R.NB + G,), SF, device=DEV, dtype=torch.float32)
        bd = torch.full((G + n + G,), SB, device=DEV, dtype=torch.int8)
        lp, bp = fl[G:G + n * R.NB], bd[G:G + n]
        _lib.check(L.mcg_gcn_forward(m._h, _lib.dptr(el), _lib.dptr(dm), _lib.dptr(am), _lib.dptr(lp) if want_logits else None,
                                     _lib.dptr(bp) if want_bond else None, B, st), "mcg_gcn_forward")
        torch.cuda.synchronize()
        fl, bd = fl.cpu(), bd.cpu()
        assert bool((fl[:G] == SF).all()) and bool((fl[G + n * R.NB:] == SF).all())
        assert bool((bd[:G] == SB).all()) and bool((bd[G + n:] == SB).all())
        return fl[G:G + n * R.NB], bd[G:G + n]

    both_l, both_b = run(True, True)
    only_l, untouched_b = run(True, False)
    untouched_l, only_b = run(False, True)
    assert bool((untouched_b == SB).all()) and bool((untouched_l == SF).all())
    assert not bool((both_l == SF).any()) and int(both_b.max()) < R.NB and int(both_b.min()) >= 0
    assert torch.equal(only_l, both_l) and torch.equal(only_b, both_b)
    assert torch.equal(torch.argmax(both_l.reshape(n, R.NB), -1).to(torch.int8), both_b)
    assert L.mcg_gcn_forward(m._h, _lib.dptr(el), _lib.dptr(dm), _lib.dptr(am), None, None, B, st) != 0
