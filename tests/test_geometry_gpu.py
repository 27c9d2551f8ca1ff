"""`mcg_geometry_relax` on the MI355X against the fp64 restatement of tests/geometry_ref.py: energy and gradient under the
forward-error rule (a), the relaxed coordinates under rule (b), recovery of perturbed rings, determinism over batch, row
and padded widths, sentinels around every output, and the `relax_geometry` option of the generator on synthetic weights.
The force field is the package's own (not MMFF94); every molecule here is built analytically with seeded noise."""
import ctypes

import numpy as np
import pytest
import torch

import geometry_ref as R
from ml_conformer_generator_amd import _lib, geometry

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run(cases, steps, N=None, W=None, restraint=False, gradient=True):
    """The cases as one batch through `geometry.relax_geometry`; numpy outputs.  Every row of every test passes through
    here: the energy never rises."""
    x, x0, z, bonds, n = R.pad_cases(cases, N, W)
    out = geometry.relax_geometry(torch.from_numpy(x), torch.from_numpy(z), torch.from_numpy(bonds), torch.from_numpy(n),
                                  steps=steps, device=DEV, return_gradient=gradient,
                                  restraint_coords=torch.from_numpy(x0) if restraint else None)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert (out["energy_after"] <= out["energy_before"]).all(), (out["energy_before"], out["energy_after"])
    assert np.isfinite(out["coords"]).all()
    for b, nb in enumerate(n):
        assert not out["coords"][b, nb:].any()                      # padded atoms are written as zero
        if gradient:
            assert not out["gradient"][b, nb:].any()
    return out


_REFS = {}


def _ref(case):
    """`evaluate` of a case at its own coordinates, computed once."""
    if case["name"] not in _REFS:
        _REFS[case["name"]] = R.evaluate(case["x"], case["x0"], R.topology(case["z"], case["bonds"]))
    return _REFS[case["name"]]


def test_energy_and_gradient_meet_the_forward_error_rule():
    cases = list(R.rule_a_cases().values())
    out = _run(cases, 0, N=64, W=64, restraint=True)
    worst_e = worst_g = 0.0
    failed = []
    for b, c in enumerate(cases):
        n = len(c["z"])
        ok, re_, rg = R.rule_a(out["energy_before"][b], out["gradient"][b, :n], _ref(c))
        print(f"GEOMETRY-RULE-A {c['name']:>16} n={n:2d} E={_ref(c)['E']:.6g} ratio_E={re_:.3f} ratio_g={rg:.3f}")
        worst_e, worst_g = max(worst_e, re_), max(worst_g, rg)
        if not ok:
            failed.append(c["name"])
        assert out["energy_after"][b] == out["energy_before"][b] and out["accepted_steps"][b] == 0
    print(f"GEOMETRY-RULE-A worst ratio: energy {worst_e:.3f} gradient {worst_g:.3f} (C_A = {R.C_A})")
    assert not failed, failed
    assert out["energy_before"][0] == 0.0                           # n = 1: exactly nothing


def test_the_restraint_gradient_through_a_one_step_call():
    c = R.rule_a_cases()["displaced"]
    out = _run([c], 1, restraint=True)
    ok, re_, rg = R.rule_a(out["energy_before"][0], out["gradient"][0], _ref(c))
    print(f"GEOMETRY-RULE-A displaced, one step: ratio_E={re_:.3f} ratio_g={rg:.3f}")
    assert ok
    assert out["accepted_steps"][0] == 1 and out["energy_after"][0] < out["energy_before"][0]
    assert out["max_displacement"][0] == pytest.approx(0.02, rel=1e-5)     # the atom with the largest gradient moves s
    # the displaced atom is pulled back towards where the restraint holds it
    before = np.linalg.norm(c["x"][2] - c["x0"][2])
    assert np.linalg.norm(out["coords"][0, 2] - c["x0"][2]) < before


def test_zero_steps_return_the_input_bit_for_bit():
    cases = list(R.rule_a_cases().values())
    x = R.pad_cases(cases, 64, 64)[0]
    out = _run(cases, 0, N=64, W=64, gradient=False)
    assert np.array_equal(out["coords"].view(np.uint32), x.view(np.uint32))
    assert not out["max_displacement"].any() and not out["accepted_steps"].any()
    assert np.array_equal(out["energy_before"], out["energy_after"])


def test_empty_rows_and_unknown_elements():
    c = R.rule_a_cases()["benzene"]
    x, _, z, bonds, n = R.pad_cases([c, c, c])
    n[1] = 0
    z[2, 3] = 1                                                     # hydrogen: no covalent radius
    args = (torch.from_numpy(x), torch.from_numpy(z), torch.from_numpy(bonds), torch.from_numpy(n))
    with pytest.raises(ValueError, match="covalent radius"):
        geometry.relax_geometry(*args, steps=5, device=DEV)
    out = geometry.relax_geometry(*args, steps=5, device=DEV, check=False)
    e0, e1, xo = out["energy_before"].cpu(), out["energy_after"].cpu(), out["coords"].cpu().numpy()
    assert float(e0[1]) == 0.0 and float(e1[1]) == 0.0 and not xo[1].any()
    assert torch.isnan(e0[2]) and torch.isnan(e1[2]) and np.array_equal(xo[2], x[2])     # not relaxed, and it says so
    assert float(e1[0]) < float(e0[0])
    empty = geometry.relax_geometry(torch.zeros(0, 6, 3), torch.zeros(0, 6, dtype=torch.int32),
                                    torch.zeros(0, 6, 6, dtype=torch.int8), torch.zeros(0, dtype=torch.int32), device=DEV)
    assert empty["coords"].shape == (0, 6, 3) and empty["energy_after"].shape == (0,)


def test_perturbed_rings_recover_and_agree_with_the_fp64_minimiser():
    rec = R.recovery_cases()
    cases = [c for _, _, c in rec]
    out = _run(cases, 200, gradient=False)
    worst_x = worst_e = 0.0
    problems = []
    for b, (name, sigma, c) in enumerate(rec):
        n = len(c["z"])
        topo = R.topology(c["z"], c["bonds"])
        ref = R.minimise(c["x"], c["x0"], topo, 200)
        got = out["coords"][b, :n].astype(np.float64)
        rms0, rms1 = R.bonded_rms(c["x"], topo), R.bonded_rms(got, topo)
        dev_x = float(np.sqrt(((got - ref["x"]) ** 2).sum(-1)).max())
        dev_e = abs(float(out["energy_after"][b]) - ref["E"])
        moved = float(np.sqrt(((got - c["x"]) ** 2).sum(-1)).max())
        print(f"GEOMETRY-RULE-B {name} sigma={sigma}: bonded rms {rms0:.4f} -> {rms1:.2e} (fp64 {R.bonded_rms(ref['x'], topo):.2e})"
              f"  E {out['energy_before'][b]:.4g} -> {out['energy_after'][b]:.4g} (fp64 {ref['E']:.4g})  accepted "
              f"{out['accepted_steps'][b]} (fp64 {ref['accepted']})  |x - x64| {dev_x:.3e}  |E - E64| {dev_e:.3e}  moved {moved:.3f}")
        worst_x, worst_e = max(worst_x, dev_x), max(worst_e, dev_e)
        if not rms1 < 0.1 * rms0:
            problems.append((name, sigma, "rms", rms0, rms1))
        if not moved <= 0.2 + 0.1:
            problems.append((name, sigma, "moved", moved))
        assert out["max_displacement"][b] == pytest.approx(moved, abs=1e-5)
        if dev_x > R.TOL_B_COORD or dev_e > R.TOL_B_ENERGY:
            problems.append((name, sigma, "rule b", dev_x, dev_e))
    print(f"GEOMETRY-RULE-B worst: coordinates {worst_x:.3e} A, energy {worst_e:.3e} (tolerances {R.TOL_B_COORD}, {R.TOL_B_ENERGY})")
    assert not problems, problems


def test_a_clash_is_pushed_apart():
    c = R.rule_a_cases()["clash"]
    topo = R.topology(c["z"], c["bonds"])
    out = _run([c], 200)
    assert out["energy_after"][0] < 0.5 * out["energy_before"][0]
    assert R.min_nonbonded_distance(out["coords"][0].astype(np.float64), topo) > R.min_nonbonded_distance(c["x"], topo) + 0.1


def test_a_molecule_gives_the_same_bits_in_every_arrangement():
    cases = R.rule_a_cases()
    others = [cases[k] for k in ("polyphenyl64", "clash", "ring5", "single")]
    for name, widths in (("fused56", (9, 42, 64)), ("tri_nitrile", (3, 42, 64)), ("polyphenyl63", (63, 64))):
        c = cases[name]
        n = len(c["z"])
        alone = _run([c], 60, N=n, W=n)
        keys = ("energy_before", "energy_after", "accepted_steps", "max_displacement")
        for row in range(5):
            batch = others[:row] + [c] + others[row:]
            got = _run(batch, 60, N=64, W=64)
            assert np.array_equal(got["coords"][row, :n], alone["coords"][0]), (name, row)
            assert np.array_equal(got["gradient"][row, :n], alone["gradient"][0]), (name, row)
            for k in keys:
                assert got[k][row] == alone[k][0], (name, row, k)
        for W in widths:
            for N in (n, 64):
                got = _run([c], 60, N=N, W=W)
                assert np.array_equal(got["coords"][0, :n], alone["coords"][0]), (name, N, W)
                assert np.array_equal(got["gradient"][0, :n], alone["gradient"][0]), (name, N, W)
                for k in keys:
                    assert got[k][0] == alone[k][0], (name, N, W, k)
        assert alone["accepted_steps"][0] > 10                       # the run did move


def test_sentinels_around_the_outputs_stay_intact():
    cases = [R.rule_a_cases()[k] for k in ("polyphenyl64", "fused56", "single", "chain64")]
    x, _, z, bonds, n = R.pad_cases(cases, 64, 64)
    B, N, G, S = len(cases), 64, 256, -7.25
    dev = lambda a: torch.from_numpy(a).to(DEV).contiguous()          # noqa: E731
    xd, zd, bd, nd = dev(x), dev(z), dev(bonds), dev(n)
    sizes = dict(coords=B * N * 3, energy=B * 2, grad=B * N * 3, stats=B * 2)
    bufs = {k: torch.full((G + v + G,), S, device=DEV) for k, v in sizes.items()}
    ptr = lambda k: bufs[k].data_ptr() + 4 * G                        # noqa: E731
    for with_optional in (True, False):
        for t in bufs.values():
            t.fill_(S)
        _lib.check(_lib.lib().mcg_geometry_relax(_lib.dptr(xd), _lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nd), B, N, 64, 25,
                                                 ctypes.c_void_p(ptr("coords")), ctypes.c_void_p(ptr("energy")),
                                                 ctypes.c_void_p(ptr("grad")) if with_optional else None,
                                                 ctypes.c_void_p(ptr("stats")) if with_optional else None,
                                                 _lib.current_stream_ptr(DEV)), "mcg_geometry_relax")
        torch.cuda.synchronize()
        for k, t in bufs.items():
            h = t.cpu().numpy()
            assert (h[:G] == S).all() and (h[G + sizes[k]:] == S).all(), k
            inner = h[G:G + sizes[k]]
            assert (inner != S).all() if (k in ("coords", "energy") or with_optional) else (inner == S).all(), k
        assert torch.equal(xd.cpu(), torch.from_numpy(x))             # the inputs are only read


# ----------------------------------------------------------------------------------------------- the generator
SEED = 20240607
_GEN = []


def _gen():
    if not _GEN:
        from ml_conformer_generator_amd import MLConformerGenerator
        from ml_conformer_generator_amd import weights as W
        _GEN.append(MLConformerGenerator(diffusion_steps=10, device=DEV,
                                         edm_weights=W.synth_edm_state_dict(1234, weight_gain=0.3),
                                         adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321),
                                         atom_order_provider=None, finisher=None))
    return _GEN[0]


def _reference(n=20):
    rng = np.random.RandomState(3)
    return torch.from_numpy((rng.normal(size=(n, 3)) * np.array([3.0, 2.0, 1.0])).astype(np.float32))


@pytest.fixture()
def keep_all(monkeypatch):
    """Every record is returned, valid or not (synthetic weights make few valid graphs)."""
    from ml_conformer_generator_amd import conformer_generator as CG
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))


def test_generator_off_is_the_parent_and_on_relaxes_every_record(keep_all):
    from ml_conformer_generator_amd.handoff import bond_writeback_hip
    gen = _gen()
    kw = dict(reference_conformer=_reference(), n_samples=8, variance=2, optimise_geometry=False, sample_seed=SEED)
    absent = gen.generate_conformers(**kw)
    lb = dict(gen.last_batch)
    off = gen.generate_conformers(relax_geometry=False, **kw)
    assert "x_relaxed" not in gen.last_batch and len(absent) == len(off) == 8
    for a, b in zip(absent, off):
        assert a == b and a.sample_id == b.sample_id and a.strain_before is None and b.strain_after is None
    assert torch.equal(gen.last_batch["x_ordered"], lb["x_ordered"])

    on = gen.generate_conformers(relax_geometry=True, **kw)
    lb_on = gen.last_batch
    assert torch.equal(lb_on["x_ordered"], lb["x_ordered"])          # still the unrelaxed coordinates
    sym, _ = bond_writeback_hip(lb["bond"], lb["elements"], lb["n_nodes"])
    want = geometry.relax_geometry(lb["x_ordered"], lb["elements"], sym, lb["n_nodes"], steps=200)
    assert torch.equal(lb_on["x_relaxed"], want["coords"])
    e0, e1, xw = want["energy_before"].cpu(), want["energy_after"].cpu(), want["coords"].cpu()
    assert len(on) == 8
    for m, ref in zip(on, absent):
        b, n = m.sample_id, m.GetNumAtoms()
        assert m.atomic_numbers == ref.atomic_numbers and torch.equal(m.bond_orders, ref.bond_orders)
        assert torch.equal(m.coords, xw[b, :n])                      # bit for bit
        assert m.strain_before == float(e0[b]) and m.strain_after == float(e1[b])
        assert np.isfinite(m.strain_before) and np.isfinite(m.strain_after) and m.strain_after <= m.strain_before
    assert any(m.strain_after < m.strain_before for m in on)
    few = gen.generate_conformers(relax_geometry=3, **kw)
    assert all(m.strain_before == r.strain_before and m.strain_after >= r.strain_after for m, r in zip(few, on))


def test_generator_scores_the_relaxed_coordinates_and_the_sharded_entry_relaxes_too(keep_all):
    gen = _gen()
    ref = _reference()
    kw = dict(reference_conformer=ref, n_samples=6, variance=2, optimise_geometry=False, sample_seed=SEED)
    scored = gen.generate_conformers(relax_geometry=True, shape_scores=True, **kw)
    lb = gen.last_batch
    want = gen._score(ref, lb["x_relaxed"], lb["n_nodes"]).cpu()
    raw = gen._score(ref, lb["x_ordered"], lb["n_nodes"]).cpu()
    assert [m.shape_tanimoto for m in scored] == [float(v) for v in want]
    assert not torch.equal(want, raw)
    # one pass through the sharded entry (no process group: one rank, the same code up to the collectives)
    sharded = gen.generate_conformers_sharded(relax_geometry=True, shape_scores=True, **kw)
    assert len(sharded) == len(scored)
    for a, b in zip(sharded, scored):
        assert a == b and (a.strain_before, a.strain_after, a.shape_tanimoto) == (b.strain_before, b.strain_after,
                                                                                 b.shape_tanimoto)


def test_generator_refuses_bad_values_before_any_launch(monkeypatch):
    gen = _gen()

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(gen, "_generate_shard", no_launch)
    for bad in (0, 4097, 2.5, None, "on"):
        with pytest.raises(ValueError, match="relax_geometry"):
            gen.generate_conformers(reference_conformer=_reference(), n_samples=4, relax_geometry=bad)
        with pytest.raises(ValueError, match="relax_geometry"):
            gen.generate_conformers_sharded(reference_conformer=_reference(), n_samples=4, relax_geometry=bad)
