"""CPU checks of the GCN stage pins (no GPU): the restatement `tests/gcn_ref.py` IS the pinned oracle in fp32, every
planted mistake is visible to something `tests/test_gcn_gpu.py` asserts, and the inputs keep plain fp32 arithmetic well
inside the stage tolerances (a condition on the inputs: the tolerances themselves are fixed in gcn_ref.STAGE_TOL).
The same table at B = 16 is committed as profiles/gcn_parity_sensitivity.txt (tools/parity_sensitivity.py --gcn)."""
import ctypes as C

import pytest
import torch

import gcn_ref as R
from ml_conformer_generator_amd import _lib
from oracle import gcn_oracle as GO

MIN_RATIO = 10.0      # as tools/parity_sensitivity.py
HOST_B = 8


@pytest.fixture(scope="module")
def sets():
    return R.input_sets(HOST_B)


@pytest.fixture(scope="module")
def tab(sets):
    return R.table(sets)


def test_restatement_is_the_oracle_in_fp32(sets, gcn_sd):
    """fp32, unmutated: bit for bit the pinned oracle (which tests/test_oracle_golden.py ties to the reference), on the
    classic B = 64 input of the existing GCN tests and on every set of the new ones, with both weight sets."""
    from ml_conformer_generator_amd.synthetic import synth_gcn_inputs
    el, dm, am = synth_gcn_inputs(16, [15 + (i * 7) % 25 for i in range(16)], seed=3)
    with torch.no_grad():
        assert torch.equal(R.gcn_forward(gcn_sd, el, dm, am)["logits"], GO.adj_mat_seer(gcn_sd, el, dm, am))
        for wn in R.WEIGHT_SETS:
            sd = R.weight_set(wn)
            for name, (el, dm, am, _) in sets.items():
                out = R.gcn_forward(sd, el, dm, am)
                assert torch.equal(out["logits"], GO.adj_mat_seer(sd, el, dm, am)), (wn, name)
                assert [tuple(out[q].shape[1:]) for q in R.STAGES] == [(42, 42), (42, 42), (42,), (42 * 64,), (42, 64), (2048,),
                                                                       (42, 42, 5)]


def test_input_sets_are_what_the_gpu_test_needs(sets):
    el, dm, am, sizes = sets["sym"]
    assert sizes[:6] == R.EDGE_SIZES and torch.equal(dm, dm.transpose(1, 2)) and torch.equal(am, am.transpose(1, 2))
    assert len(R.sym_inputs(16)[3]) == 16 and R.sym_inputs(16)[3][:6] == R.EDGE_SIZES      # + ten ragged rows on the GPU
    el, dm, am, sizes = sets["asym"]
    assert not torch.equal(dm, dm.transpose(1, 2)) and not torch.equal(am, am.transpose(1, 2))
    one_way = ((am != am.transpose(1, 2)).sum().item() / 2) / sum(n * n for n in sizes)
    assert 0.01 < one_way < 0.05, one_way                      # ~3 % extra one-way bonds
    assert set(am.unique().tolist()) == {0.0, 1.0}
    el, dm, am, sizes = sets["elements"]
    real = torch.cat([el[b, :n] for b, n in enumerate(sizes)])
    assert sorted(set(real.tolist())) == list(range(36))      # every table row, 0 and 35 included
    el, dm, am, sizes = sets["junk"]
    ce, cd, ca, _ = R.junk_inputs(junk=False)
    for b, n in enumerate(sizes):
        assert torch.equal(dm[b, :n, :n], cd[b, :n, :n]) and torch.equal(am[b, :n, :n], ca[b, :n, :n])
        if n < 42:
            assert float(dm[b, n:, :].min()) > 0 and float(dm[b, :, n:].min()) > 0 and float(am[b, n:].sum()) > 42 - n
            assert torch.equal(cd[b, n:, n:], torch.eye(42 - n)) and float(cd[b, :n, n:].abs().max()) == 0


def test_stage_tolerances_follow_the_stated_rule():
    for q in R.QUANTITIES:
        assert R.STAGE_TOL[q] == min(1.0, 16.0 * R.MEASURED_FP32[q]) and 0 < R.STAGE_TOL[q] <= 1.0


def test_unmutated_fp32_sits_inside_every_stage_tolerance(tab):
    """A condition on the inputs and weights: plain fp32 on the CPU stays within 0.25 x every asserted tolerance."""
    for key, rows in tab.items():
        for q in R.QUANTITIES:
            v = rows["base"][q] / R.STAGE_TOL[q]
            assert v <= 0.25, f"{key} {q}: fp32 restatement at {v:.3f} x its stage tolerance"


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_is_visible_to_an_asserted_quantity(tab, mutation):
    best, where = 0.0, None
    for key, rows in tab.items():
        for q in R.QUANTITIES:
            v = rows[mutation][q] / R.STAGE_TOL[q]
            if v > best:
                best, where = v, (key, q)
    print(f"{mutation}: {best:.3g} x tolerance at {where}")
    assert best >= MIN_RATIO, f"{mutation} reaches only {best:.3g} x a stage tolerance (at {where})"


def test_index_order_mutations_need_the_asymmetric_set(tab):
    """Why the asymmetric set exists: on symmetric matrices L^T and column degrees are invisible everywhere, on the
    asymmetric ones they show in both branches."""
    for m in ("Lt:dm", "Lt:main", "coldeg:dm", "coldeg:main"):
        for wn in R.WEIGHT_SETS:
            sym = max(tab[(wn, "sym")][m][q] / R.STAGE_TOL[q] for q in R.QUANTITIES)
            asym = max(tab[(wn, "asym")][m][q] / R.STAGE_TOL[q] for q in R.QUANTITIES)
            assert sym <= 0.25 and asym >= MIN_RATIO, (m, wn, sym, asym)


def test_gcn_peek_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (C.c_float * 4)()
    assert L.mcg_gcn_peek(None, 0, 1, buf, None) != 0
    assert b"mcg_gcn_peek" in L.mcg_last_error()
