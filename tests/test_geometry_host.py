"""Relaxed geometry without a GPU: the fp64 restatement of the force field (tests/geometry_ref.py) on hand cases, its
gradient against finite differences, that rule (a) can fail (a 1 % change of any constant), the option parsing and the
generator's refusals, the record plumbing and the C entry's argument errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import geometry_ref as R
from conftest import REPO


def _case(z, pairs):
    return R._mol("hand", z, pairs, np.zeros((len(z), 3)))


def _classes(case):
    return R.topology(case["z"], case["bonds"])


# ----------------------------------------------------------------------------------------------- topology
def test_chain_classes_and_d0():
    c = _case([6, 6, 8, 6, 6], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)])
    cls, d0 = _classes(c)
    assert cls[0, 1] == R.BOND and cls[0, 2] == R.ANGLE and cls[0, 3] == R.NONBONDED and cls[0, 4] == R.NONBONDED
    assert (cls == cls.T).all() and (np.diag(cls) == R.NONE).all() and np.allclose(d0, d0.T)
    assert d0[0, 1] == pytest.approx(1.52) and d0[1, 2] == pytest.approx(0.76 + 0.66)
    theta = np.radians(109.47)
    assert d0[0, 2] == pytest.approx(np.sqrt(1.52 ** 2 + 1.42 ** 2 - 2 * 1.52 * 1.42 * np.cos(theta)))
    assert d0[0, 3] == pytest.approx(0.76 + 0.76 + 0.9) and d0[2, 4] == pytest.approx(np.sqrt(
        1.42 ** 2 + 1.52 ** 2 - 2 * 1.42 * 1.52 * np.cos(theta)))


def test_bond_orders_shorten_the_carbon_carbon_bond_to_the_fitted_lengths():
    for code, want in ((1, 1.52), (4, 1.39), (2, 1.34), (3, 1.20)):
        assert _classes(_case([6, 6], [(0, 1, code)]))[1][0, 1] == pytest.approx(want)


@pytest.mark.parametrize("n, theta", [(3, None), (4, 90.0), (5, 108.0), (6, 109.47)])
def test_ring_angle_classes(n, theta):
    cls, d0 = _classes(R.regular_ring(n, 1))
    if n == 3:
        assert (cls[np.triu_indices(3, 1)] == R.BOND).all()          # nothing but bonds: no angle term at all
        return
    assert cls[0, 2] == R.ANGLE
    assert d0[0, 2] == pytest.approx(np.sqrt(2 * 1.52 ** 2 * (1 - np.cos(np.radians(theta)))))
    if n == 6:
        assert cls[0, 3] == R.NONBONDED
    # an aromatic six-ring keeps 120 degrees; an aromatic five-ring is pulled to 108
    if n in (5, 6):
        _, d0a = _classes(R.regular_ring(n, 4))
        want = 108.0 if n == 5 else 120.0
        assert d0a[0, 2] == pytest.approx(np.sqrt(2 * 1.39 ** 2 * (1 - np.cos(np.radians(want)))))


def test_fused_five_six_system():
    c = R.fused56()
    cls, d0 = _classes(c)
    # 0 and 1 are the shared atoms; 5-0-1 lies in the six-ring only (120), 8-0-1 in the five-ring (108), and 5-0-8 spans
    # both rings: no ring correction, the aromatic centre's 120
    ar, si = 1.39, 1.52
    assert d0[5, 1] == pytest.approx(np.sqrt(2 * ar * ar * (1 - np.cos(np.radians(120.0)))))
    assert d0[8, 1] == pytest.approx(np.sqrt(si * si + ar * ar - 2 * si * ar * np.cos(np.radians(108.0))))
    assert d0[5, 8] == pytest.approx(np.sqrt(si * si + ar * ar - 2 * si * ar * np.cos(np.radians(120.0))))
    assert d0[6, 8] == pytest.approx(np.sqrt(2 * si * si * (1 - np.cos(np.radians(108.0)))))     # centre 7, sp3, in the five-ring
    assert cls[2, 7] == R.NONBONDED and cls[0, 6] == R.ANGLE


def test_linear_centres_and_an_angle_pair_with_two_centres():
    _, d0 = _classes(_case([6, 6, 6], [(0, 1, 2), (1, 2, 2)]))                  # allene
    assert d0[0, 2] == pytest.approx(2 * 1.34)
    _, d0 = _classes(_case([6, 6, 7], [(0, 1, 1), (1, 2, 3)]))                  # nitrile
    assert d0[0, 2] == pytest.approx(1.52 + (0.76 + 0.71 - 0.32))
    _, d0 = _classes(_case([6, 6, 6], [(0, 1, 2), (1, 2, 1)]))                  # one double bond: trigonal
    assert d0[0, 2] == pytest.approx(np.sqrt(1.34 ** 2 + 1.52 ** 2 + 1.34 * 1.52))
    # 0 and 2 share the centres 1 (carbon) and 3 (sulfur): a four-ring, 90 degrees at both, the smaller d0 counts
    cls, d0 = _classes(_case([6, 6, 6, 16], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1)]))
    assert cls[0, 2] == R.ANGLE and d0[0, 2] == pytest.approx(np.sqrt(2) * 1.52)
    assert d0[1, 3] == pytest.approx(np.sqrt(1.52 ** 2 + 1.81 ** 2))
    with pytest.raises(ValueError):
        R.topology([6, 1], np.zeros((2, 2)))                                    # hydrogen: no radius


# ----------------------------------------------------------------------------------------------- energy
def test_regular_rings_are_minima_and_planar_cyclohexane_is_strained():
    h = R.hand_cases()
    for name in ("single", "ring3", "ring4", "ring5", "benzene"):
        c = h[name]
        ev = R.evaluate(c["x"], c["x0"], _classes(c))
        assert ev["E"] < 1e-10, (name, ev["E"])        # the coordinates are rounded to fp32: 1e-7 A off, E ~ 1e-12
    c = h["cyclohexane"]
    assert R.evaluate(c["x"], c["x0"], _classes(c))["E"] == pytest.approx(10.2, abs=0.05)


def test_gradient_matches_finite_differences():
    for name in ("fused56", "clash", "displaced", "tri_nitrile", "ring4"):
        c = R.rule_a_cases()[name]
        topo = _classes(c)
        g = R.evaluate(c["x"], c["x0"], topo)["grad"]
        h = 1e-6
        for i in range(len(c["z"])):
            for a in range(3):
                xp, xm = c["x"].copy(), c["x"].copy()
                xp[i, a] += h
                xm[i, a] -= h
                fd = (R.evaluate(xp, c["x0"], topo)["E"] - R.evaluate(xm, c["x0"], topo)["E"]) / (2 * h)
                assert fd == pytest.approx(g[i, a], abs=2e-5 * max(1.0, abs(g[i, a]))), (name, i, a)


def test_the_minimiser_never_goes_uphill_and_recovers_benzene():
    for name, sigma, c in R.recovery_cases():
        topo = _classes(c)
        m = R.minimise(c["x"], c["x0"], topo, 200)
        assert m["E"] <= m["E_start"]
        assert R.bonded_rms(m["x"], topo) < 0.1 * R.bonded_rms(c["x"], topo), (name, sigma)
        assert np.sqrt(((m["x"] - c["x"]) ** 2).sum(-1)).max() <= 0.3
    c = R.hand_cases()["benzene"]
    m0 = R.minimise(c["x"], c["x0"], _classes(c), 0)
    assert np.array_equal(m0["x"], c["x"]) and m0["accepted"] == 0


@pytest.mark.parametrize("key", R.MUTABLE)
def test_rule_a_fails_when_a_constant_is_off_by_one_per_cent(key):
    """The rule must be able to fail: the restatement with one constant changed by 1 % stands in for a wrong kernel."""
    assert R.C_A < 100.0
    wrong = dict(R.PARAMS, **{key: R.PARAMS[key] * 1.01})
    failed = []
    for name, c in R.rule_a_cases().items():
        ref = R.evaluate(c["x"], c["x0"], _classes(c))
        bad = R.evaluate(c["x"], c["x0"], R.topology(c["z"], c["bonds"], wrong), wrong)
        ok_true, _, _ = R.rule_a(ref["E"], ref["grad"], ref)
        assert ok_true
        if not R.rule_a(bad["E"], bad["grad"], ref)[0]:
            failed.append(name)
    assert failed, key


def test_every_rule_a_case_has_its_size_and_terms():
    cases = R.rule_a_cases()
    sizes = {name: len(c["z"]) for name, c in cases.items()}
    assert sizes["single"] == 1 and sizes["pair_triple"] == 2 and sizes["polyphenyl63"] == 63
    assert sizes["polyphenyl64"] == 64 and sizes["chain64"] == 64
    c = cases["clash"]
    ev = R.evaluate(c["x"], c["x0"], _classes(c))
    assert R.min_nonbonded_distance(c["x"], _classes(c)) == pytest.approx(1.5) and ev["E"] > 50.0
    c = cases["displaced"]
    assert np.sqrt(((c["x"] - c["x0"]) ** 2).sum(-1)).max() == pytest.approx(0.5)


# ----------------------------------------------------------------------------------------------- options
def test_check_steps():
    from ml_conformer_generator_amd.geometry import check_steps
    assert check_steps(False) == 0 and check_steps(True) == 200
    assert check_steps(1) == 1 and check_steps(4096) == 4096 and check_steps(np.int32(7)) == 7
    for bad in (0, -1, 4097, 2.0, "3", None, np.float32(4.0), [5]):
        with pytest.raises(ValueError, match="relax_geometry"):
            check_steps(bad)


def _shell_generator():
    from ml_conformer_generator_amd.conformer_generator import MLConformerGenerator
    gen = MLConformerGenerator.__new__(MLConformerGenerator)
    torch.nn.Module.__init__(gen)
    gen.device = torch.device("cpu")
    gen.dimension = 42
    gen.min_n_nodes, gen.max_n_nodes = 15, 39
    gen.last_batch = gen.last_valid_fraction = gen._timing = gen.last_noise_seed = gen.last_host_assembly_ms = None
    gen.atom_order_provider = None
    gen.finisher = None
    gen.n_host_workers = 0
    return gen


def _no_device(*args, **kwargs):
    raise AssertionError("device work started before the arguments were checked")


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_bad_values_are_refused_before_any_device_work(entry):
    gen = _shell_generator()
    gen._generate_shard = gen._relax_coords = _no_device
    ctx = torch.tensor([50.0, 100.0, 130.0])
    for bad in (0, -3, 4097, 1.5, "yes", None):
        with pytest.raises(ValueError, match="relax_geometry"):
            getattr(gen, entry)(reference_context=ctx, n_atoms=17, n_samples=4, relax_geometry=bad)


def test_the_option_reaches_the_shard_and_is_absent_when_off():
    from ml_conformer_generator_amd import postprocess
    gen = _shell_generator()
    assert postprocess.parse_request(gen, None).relax_steps == 0
    assert postprocess.parse_request(gen, None, relax_geometry=True).relax_steps == 200
    assert postprocess.parse_request(gen, None, relax_geometry=17).relax_steps == 17
    assert postprocess.parse_request(gen, None, relax_geometry=False) == postprocess.Request()
    seen = []

    class Stop(Exception):
        pass

    def shard(*args, **kwargs):
        seen.append(kwargs)
        raise Stop

    gen._generate_shard = shard
    ctx = torch.tensor([50.0, 100.0, 130.0])
    for kw, want in ((dict(), {}), (dict(relax_geometry=False), {}), (dict(relax_geometry=True), {"relax_steps": 200}),
                     (dict(relax_geometry=9), {"relax_steps": 9})):
        with pytest.raises(Stop):
            gen.generate_conformers(reference_context=ctx, n_atoms=17, n_samples=4, **kw)
        assert seen[-1] == want            # off: the parent's call, argument for argument


def test_records_carry_the_strain_or_none():
    from ml_conformer_generator_amd.handoff import GeneratedMolecule, molecules_from_tensors
    hand = GeneratedMolecule([6, 6], torch.zeros(2, 3), torch.zeros(2, 2, dtype=torch.int8))
    assert hand.strain_before is None and hand.strain_after is None
    x = torch.zeros(2, 3, 3)
    el = torch.full((2, 3), 6, dtype=torch.int8)
    bo = torch.zeros(2, 3, 3, dtype=torch.int8)
    n, valid = torch.tensor([3, 2], dtype=torch.int32), torch.ones(2, dtype=torch.uint8)
    plain = molecules_from_tensors(x, el, bo, n, valid)
    assert all(m.strain_before is None and m.strain_after is None for m in plain)
    rel = molecules_from_tensors(x, el, bo, n, valid, strain_before=torch.tensor([3.5, 1.25]),
                                 strain_after=torch.tensor([0.5, 0.25]))
    assert [(m.strain_before, m.strain_after) for m in rel] == [(3.5, 0.5), (1.25, 0.25)]
    assert [m.sample_id for m in rel] == [0, 1] and rel[0] == plain[0]


def test_finished_samples_carry_the_strain_across_the_gather():
    from ml_conformer_generator_amd import postprocess
    gen = _shell_generator()
    req = postprocess.Request(relax_steps=5)
    res = dict(strain_before=torch.tensor([2.0, 4.0]), strain_after=torch.tensor([1.0, 0.5]))
    out = postprocess.measure_finished(gen, req, ["a", None], res)
    assert [(s.measured.strain_before, s.measured.strain_after) for s in out] == [(2.0, 1.0), (4.0, 0.5)]
    assert out[1].mol is None
    assert all(s.measured.strain_before is None and s.measured.strain_after is None
               for s in postprocess.measure_finished(gen, postprocess.Request(), ["a", None]))


# ----------------------------------------------------------------------------------------------- python checks
def test_relax_geometry_refuses_bad_inputs_before_the_kernel(monkeypatch):
    from ml_conformer_generator_amd import _lib, geometry
    monkeypatch.setattr(_lib, "lib", _no_device)
    x, z = torch.zeros(2, 5, 3), torch.full((2, 5), 6)
    bo, n = torch.zeros(2, 5, 5, dtype=torch.int8), torch.tensor([5, 3])
    for kw in (dict(coords=torch.zeros(2, 5, 2)), dict(coords=torch.zeros(2, 5, 3, dtype=torch.int32)),
               dict(bond_orders=torch.zeros(2, 5, 4, dtype=torch.int8)), dict(bond_orders=torch.zeros(3, 5, 5, dtype=torch.int8)),
               dict(bond_orders=torch.zeros(2, 65, 65, dtype=torch.int8), atomic_numbers=torch.full((2, 65), 6)),
               dict(atomic_numbers=torch.full((2, 4), 6)), dict(atomic_numbers=torch.full((2, 5), 6.0)),
               dict(steps=-1), dict(steps=4097), dict(steps=True), dict(steps=2.0),
               dict(n_nodes=torch.tensor([6, 3])), dict(n_nodes=torch.tensor([5])), dict(n_nodes=torch.tensor([-1, 3])),
               dict(coords=torch.zeros(2, 4, 3)),                                   # n = 5 atoms do not fit N = 4
               dict(restraint_coords=torch.zeros(2, 4, 3))):
        args = dict(coords=x, atomic_numbers=z, bond_orders=bo, n_nodes=n, steps=3, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError):
            geometry.relax_geometry(**args)


def test_unknown_elements_and_bad_graphs_are_refused_by_the_check():
    from ml_conformer_generator_amd import geometry
    z = torch.tensor([[6, 7, 1]], dtype=torch.int32)
    bo = torch.zeros(1, 3, 3, dtype=torch.int8)
    with pytest.raises(ValueError, match="covalent radius"):
        geometry._check_molecules(z, bo, torch.tensor([3], dtype=torch.int32), 3)          # hydrogen
    geometry._check_molecules(z, bo, torch.tensor([2], dtype=torch.int32), 3)              # ... on a padded atom: ignored
    with pytest.raises(ValueError, match="covalent radius"):
        geometry._check_molecules(torch.tensor([[6, 99, 6]], dtype=torch.int32), bo, torch.tensor([3], dtype=torch.int32), 3)
    bo2 = bo.clone()
    bo2[0, 0, 1] = 1
    with pytest.raises(ValueError, match="symmetric"):
        geometry._check_molecules(torch.tensor([[6, 6, 6]], dtype=torch.int32), bo2, torch.tensor([3], dtype=torch.int32), 3)


# ----------------------------------------------------------------------------------------------- C entry
def test_the_c_entry_refuses_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check
    ok = dict(coords=p, z=p, bonds=p, n=p, B=2, N=42, W=42, steps=10, out=p, energy=p)

    def relax(**kw):
        a = dict(ok, **kw)
        return h.mcg_geometry_relax(a["coords"], a["z"], a["bonds"], a["n"], a["B"], a["N"], a["W"], a["steps"], a["out"],
                                    a["energy"], None, None, None)

    def relax_ex(**kw):
        a = dict(ok, **kw)
        return h.mcg_geometry_relax_ex(a["coords"], None, a["z"], a["bonds"], a["n"], a["B"], a["N"], a["W"], a["steps"],
                                       a["out"], a["energy"], None, None, None)

    for f in (relax, relax_ex):
        for bad in (dict(coords=None), dict(z=None), dict(bonds=None), dict(n=None), dict(out=None), dict(energy=None),
                    dict(B=-1), dict(W=65), dict(W=0), dict(N=0), dict(steps=-1), dict(steps=4097)):
            assert f(**bad) == 1, bad
            assert b"mcg_geometry_relax" in h.mcg_last_error(), bad
        assert f(B=0) == 0                        # an empty batch launches nothing
    text = open(os.path.join(REPO, "include", "mlconfgen_hip.h")).read()
    assert "#define MCG_RELAX_MAX_ATOMS 64" in text and "#define MCG_RELAX_MAX_STEPS 4096" in text
    assert "mcg_geometry_relax" in _lib.SIGNATURES and h.mcg_abi_version() == 4


def test_optimise_geometry_still_warns_as_before(monkeypatch):
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd.handoff import GeneratedMolecule
    monkeypatch.setattr(CG, "_WARNED_NO_MMFF", [False])
    rec = GeneratedMolecule([6, 6], torch.zeros(2, 3), torch.zeros(2, 2, dtype=torch.int8))
    with pytest.warns(RuntimeWarning, match=r"optimise_geometry=True \(MMFF94\) is NOT applied"):
        kept, share = CG._finish([rec], True, use_rdkit=False)
    assert kept == [rec] and share == 1.0


def test_every_element_the_generator_can_emit_has_a_radius_on_the_device():
    """The generator relaxes unchecked (no host read): every Z a decoder may name must have a covalent radius in the
    device table, else a generated row would come back with a NaN strain."""
    import re
    from ml_conformer_generator_amd.config import ELEMENTS
    from ml_conformer_generator_amd.elements import SYMBOL_TO_Z, class_z_from_decoder
    text = open(os.path.join(REPO, "ml_conformer_generator_amd", "csrc", "mcg_elements.h")).read()
    body = re.sub(r"//[^\n]*", "", text[text.index("MCG_ELEMENTS = {"):])
    rcov = [float(v) for v in re.findall(r"[0-9]+\.[0-9]+", body[:body.index("},")])]
    assert len(rcov) == 36
    for z, (sym, r, _) in ELEMENTS.items():
        assert r > 0.0 and rcov[z] == r and R.RCOV[z] == r, sym
    assert sorted(SYMBOL_TO_Z.values()) == sorted(ELEMENTS)           # a decoder can name nothing else
    assert set(class_z_from_decoder({k: s for k, s in enumerate(["B", "Si", "As", "Se", "Br", "P", "S", "Cl"])})) <= set(ELEMENTS)
    with pytest.raises(ValueError):
        class_z_from_decoder({k: "Fe" for k in range(8)})


class _StubMol:
    """What `rdkit_finish.tag_measured` needs of a Mol."""

    def __init__(self):
        self.props = {}

    def SetDoubleProp(self, k, v):
        self.props[k] = v

    def SetIntProp(self, k, v):
        self.props[k] = v


def test_finished_mols_are_tagged_with_their_strain_behind_the_gather():
    from ml_conformer_generator_amd import postprocess
    gen = _shell_generator()
    res = dict(strain_before=torch.tensor([2.0, 4.0, 8.0]), strain_after=torch.tensor([1.0, 0.5, 0.25]))
    mols = [_StubMol(), None, _StubMol()]
    req = postprocess.Request(relax_steps=5)
    samples = postprocess.measure_finished(gen, req, mols, res)
    out = postprocess.return_finished(gen, req, samples, None, sample_seed=3)
    assert out == [mols[0], mols[2]] and gen.last_valid_fraction == pytest.approx(2 / 3)
    assert mols[0].props == {"sample_id": 0, "strain_before": 2.0, "strain_after": 1.0}
    assert mols[2].props == {"sample_id": 2, "strain_before": 8.0, "strain_after": 0.25}
    # a call that did not relax tags nothing
    plain = [_StubMol()]
    postprocess.return_finished(gen, postprocess.Request(), postprocess.measure_finished(gen, postprocess.Request(), plain),
                                None, None)
    assert plain[0].props == {}
