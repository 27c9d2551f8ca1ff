"""Receptor interactions, host side (DESIGN.md section 6 "Receptor interactions"): the restatement on hand-computable
pairs, the typing rules on named molecules and a synthetic PDB string, the pass rule against mutations of the definition,
the options against stub seams, and the C entry's argument checks.  No GPU."""
import ctypes
import math
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import interactions_cases as K
import interactions_ref as R
from conftest import REPO
from ml_conformer_generator_amd import interactions as IX
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import receptor as RC
from ml_conformer_generator_amd.handoff import GeneratedMolecule, Measured, measured_from_tensors
from test_shape_overlay_host import _no_device, _ref, _shell_generator, _stub_overlay


# ----------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", list(K.HAND))
def test_hand_pairs(name):
    pair, want = K.HAND[name]
    got = R.score(*K.hand_args(pair))
    terms = dict(zip(R.TERMS, got["terms"]))
    for k, v in want.items():
        if k == "hbonds":
            assert got["hbonds"] == v
        elif k == "counted":
            assert bool(R.surface_distances(pair["x"], R.radii(pair["z"]), pair["y"], R.radii(pair["zr"]))[0][0, 0]) is v
            assert bool(terms["g1"] > 0 and terms["g2"] > 0) is v
        else:
            assert terms[k] == pytest.approx(v, abs=1e-6), (name, k)
    w = R.DEFINITION.w
    assert got["score"] == pytest.approx(sum(w[k] * terms[k] for k in R.TERMS), rel=1e-12, abs=1e-300)
    assert got["atom_scores"].sum() == pytest.approx(got["weighted"], rel=1e-12, abs=1e-300)


def test_score_divides_by_the_rotor_term_and_empty_molecule_scores_zero():
    c = R.cases()[2]
    free, bound = R.score(*c.args()[:6], 0), R.score(*c.args()[:6], 5)
    assert bound["score"] == pytest.approx(free["score"] / (1 + float(np.float32(0.0585)) * 5), rel=1e-12)
    assert free["weighted"] == bound["weighted"] and free["score"] < 0
    empty = R.score(np.zeros((0, 3)), [], [], c.rec, R.radii(c.rec_z), c.rec_t, 3)
    assert empty["score"] == 0.0 and empty["hbonds"] == 0 and not empty["terms"].any()
    far = R.Case("far", 31, 27, far=True)
    out = R.score(*far.args())
    assert out["score"] == 0.0 and not out["terms"].any() and not out["atom_terms"].any()


def test_radii_tables_agree():
    for z in list(R.RADII) + [1, 5, 11, 33, 34, 47, 79, 92, 118]:
        assert IX.interaction_radius(z) == R.radius(z), z
        assert float(IX.interaction_radii(torch.tensor([z]))[0]) == float(np.float32(R.radius(z)))
    assert R.radius(6) == 1.9 and R.radius(30) == 1.2 and R.radius(5) == RC.VDW_RADII[5] and R.radius(118) == RC.DEFAULT_RADIUS
    assert IX.WEIGHTS == dict(g1=-0.0356, g2=-0.00516, rep=0.840, hyd=-0.0351, hb=-0.587) and IX.ROTOR_WEIGHT == 0.0585
    assert {k: float(np.float32(v)) for k, v in IX.WEIGHTS.items()} == R.DEFINITION.w


# ----------------------------------------------------------------------------------------------- the pass rule
MUTANTS = ([(f"weight {k} + 1 %", {k: R.DEFINITION.w[k] * 1.01}) for k in R.TERMS] +
           [("rotor weight + 1 %", dict(rotor=R.DEFINITION.rotor * 1.01)),
            ("first Gaussian width + 1 %", dict(width1=0.505)), ("second Gaussian width + 1 %", dict(width2=2.02)),
            ("hyd ramp start + 0.05", dict(hyd_full=0.55)), ("hyd ramp end + 0.05", dict(hyd_zero=1.55)),
            ("hb ramp start + 0.05", dict(hb_full=R.DEFINITION.hb_full + 0.05)), ("hb ramp end + 0.05", dict(hb_zero=0.05)),
            ("cut-off at 7.5 A", dict(cutoff2=56.25)), ("no n_rot divisor", dict(divide=False))])


def _as_fp32(out):
    return {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if k != "hbonds" else v) for k, v in out.items()}


def test_rule_passes_the_restatement_rounded_to_fp32():
    for c in R.cases():
        assert c.n_rot >= 0
        assert R.passes(_as_fp32(R.score(*c.args())), *c.args()), c


@pytest.mark.parametrize("what, change", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_rule_sees_a_mutation(what, change):
    seen = 0
    for c in R.cases():
        args = c.args()[:6] + (max(c.n_rot, 1),)
        mutant = _as_fp32(R.score(*args, defn=R.Definition(**change)))
        seen += not R.passes(mutant, *args)
    assert seen >= 5, (what, seen)                # nine cases; one with a single receptor atom may not show every term


# ----------------------------------------------------------------------------------------------- ligand typing
@pytest.mark.parametrize("name", list(K.MOLECULES))
def test_named_molecules_under_renumbering(name):
    mol, hydrophobic, n_rot = K.MOLECULES[name]
    for (z, adj, n), p in K.renumberings(mol):
        pharm = K.pharm_types((z, adj, n))
        types = R.ligand_types(z, adj, n, pharm)
        assert [bool(t & R.HYDROPHOBIC) for t in types] == [hydrophobic[a] for a in p], name
        assert [t & 3 for t in types] == [q & 3 for q in pharm]
        assert R.rotatable_bonds(z, adj, n) == n_rot, name


def test_the_hydrophobic_type_is_wider_than_the_pharmacophores_hydrophobe():
    import pharmacophore_ref as PR
    z, adj, n = K.TOLUENE
    pharm = K.pharm_types(K.TOLUENE)
    assert sum(1 for t in pharm if t & PR.H) == 1                                 # the methyl group alone
    assert all(t & R.HYDROPHOBIC for t in R.ligand_types(z, adj, n, pharm))       # every carbon, aromatic ones too
    z, adj, n = K.ACETAMIDE
    types = R.ligand_types(z, adj, n, K.pharm_types(K.ACETAMIDE))
    assert types[1] & R.HYDROPHOBIC == 0 and types[2] & R.ACCEPTOR and types[3] & R.DONOR


def test_rotatable_bond_pattern():
    p = IX.ROTATABLE_BOND
    assert len(p.atoms) == 2 and all((q.dmin, q.dmax) == (2, 8) for q in p.atoms)
    assert len(p.bonds) == 1 and p.bonds[0].codes == (1,) and p.bonds[0].ring is False
    # amide C-N: counted, by the package's rule
    z, adj, n = R_mol([6, 6, 8, 7, 6], [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1)])
    assert R.rotatable_bonds(z, adj, n) == 1


def R_mol(z, bonds):
    import canonical_ref
    return canonical_ref.mol(z, bonds)


# ----------------------------------------------------------------------------------------------- receptor typing
def test_pdb_string_is_typed_atom_by_atom():
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        xyz, z, types = RC.load_typed_receptor(K.PDB)
    assert types.dtype == torch.uint8 and types.tolist() == [a[6] for a in K.PDB_ATOMS]
    plain = RC.load_receptor(K.PDB)
    assert torch.equal(xyz, plain[0]) and torch.equal(z, plain[1])
    assert len(seen) == 1 and f"{K.PDB_UNTEMPLATED} N, O or metal" in str(seen[0].message)
    names = RC.parse_pdb_names(K.PDB)
    assert names[0] == ("GLY", "N") and names[-1] == ("ZN", "ZN") and len(names) == len(K.PDB_ATOMS)
    want, count = R.receptor_types(xyz.numpy(), z.tolist(), names)
    assert want == types.tolist() and count == K.PDB_UNTEMPLATED


def test_proline_hetatm_fallback_and_the_warning():
    atoms = [a for a in K.PDB_ATOMS + K.EXTRA_ATOMS if a[6] is not None]          # the hydrogen is dropped
    with pytest.warns(UserWarning, match=f"{K.EXTRA_UNTEMPLATED} N, O or metal"):
        xyz, z, types = RC.load_typed_receptor(K.PDB_EXTRA)
    assert types.tolist() == [a[6] for a in atoms] and len(z) == len(atoms)
    by_name = {(a[2], a[1]): t for a, t in zip(atoms, types.tolist())}
    assert by_name[("PRO", "N")] == 0 and by_name[("GLY", "N")] == RC.TYPE_DONOR
    assert by_name[("LIG", "N1")] == by_name[("LIG", "O1")] == RC.TYPE_DONOR | RC.TYPE_ACCEPTOR
    assert by_name[("LIG", "S1")] == 0 and by_name[("LIG", "CL1")] == RC.TYPE_HYDROPHOBIC
    assert RC.typed_receptor(K.PDB_EXTRA)[3] == K.EXTRA_UNTEMPLATED
    want, count = R.receptor_types(xyz.numpy(), z.tolist(), RC.parse_pdb_names(K.PDB_EXTRA))
    assert want == types.tolist() and count == K.EXTRA_UNTEMPLATED
    assert RC.template_type("HIS", "NE2", 7) == 3 and RC.template_type("TRP", "NE1", 7) == 1
    assert RC.template_type("LYS", "NZ", 7) == 1 and RC.template_type("GLU", "OE2", 8) == 2
    assert RC.template_type("MSE", "N", 7) is None and RC.template_type("HOH", "O", 8) == 3


def test_pairs_without_names_and_explicit_types():
    xyz, z, _, _ = RC.typed_receptor(K.PDB)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                            # no names, no template, no warning
        _, z2, types = RC.load_typed_receptor((xyz, z))
    want, count = R.receptor_types(xyz.numpy(), z.tolist(), None)
    assert types.tolist() == want and count == 0 and torch.equal(z, z2)
    assert all(t == 3 for t, k in zip(types.tolist(), z.tolist()) if k in (7, 8))
    given = torch.arange(len(z)) % 8
    _, _, kept = RC.load_typed_receptor((xyz, z, given))
    assert kept.dtype == torch.uint8 and kept.tolist() == given.tolist()                      # verbatim
    zh = z.clone()
    zh[3] = 1                                                                     # a hydrogen goes, and its type with it
    _, z3, kept = RC.load_typed_receptor((xyz, zh, given))
    assert len(z3) == len(z) - 1 and kept.tolist() == [int(t) for k, t in enumerate(given.tolist()) if k != 3]
    for bad in (given + 1, -given, given[:-1], given.float(), given > 2):
        with pytest.raises(ValueError, match="types"):
            RC.load_typed_receptor((xyz, z, bad))
    with pytest.raises(ValueError):
        RC.load_typed_receptor((xyz, z, given, given))


def test_polar_carbons_cell_sort_equals_brute_force():
    g = torch.Generator().manual_seed(4)
    xyz = torch.rand(3000, 3, generator=g) * 24.0
    z = torch.tensor([6, 6, 7, 8, 16])[torch.randint(0, 5, (3000,), generator=g)]
    got = RC.polar_carbons(xyz, z)
    d = torch.cdist(xyz.double(), xyz[(z == 7) | (z == 8)].double()).min(dim=1).values
    assert torch.equal(got, (z == 6) & (d <= RC.POLAR_CARBON_DISTANCE)) and 50 < int(got.sum()) < 1500
    spread = xyz.clone()
    spread[0] = torch.tensor([5.0e7, 0.0, 0.0])                                   # too spread out for cells: chunks
    assert torch.equal(RC.polar_carbons(spread, z)[1:], RC.polar_carbons(spread[1:], z[1:]))
    assert not RC.polar_carbons(xyz, torch.full((3000,), 6)).any()


def test_sort_typed_receptor_is_independent_of_input_order():
    c = R.cases()[-1]
    xyz, z, t = c.receptor
    r = IX.interaction_radii(z)
    a_xyzr, a_t = RC.sort_typed_receptor(xyz, r, t)
    assert torch.equal(a_xyzr, RC.sort_receptor(xyz, r)) and a_t.dtype == torch.uint8          # the same geometry order
    for seed in range(4):
        p = torch.randperm(len(z), generator=torch.Generator().manual_seed(seed))
        b_xyzr, b_t = RC.sort_typed_receptor(xyz[p], r[p], t[p])
        assert torch.equal(a_xyzr, b_xyzr) and torch.equal(a_t, b_t)
    # two atoms at one place with one radius: the type breaks the tie
    twin = torch.cat([xyz, xyz[:1]]), torch.cat([r, r[:1]]), torch.cat([t, (t[:1] + 1) % 8])
    one = RC.sort_typed_receptor(*twin)
    two = RC.sort_typed_receptor(*(v.flip(0) for v in twin))
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    prepared = IX.prepare_receptor(c.receptor)
    assert torch.equal(prepared.xyzr, a_xyzr) and torch.equal(prepared.types, a_t)
    assert tuple(prepared.spheres.shape) == (17, 4) and IX.prepare_receptor(prepared) is prepared


# ----------------------------------------------------------------------------------------------- options
def _receptor():
    g = torch.Generator().manual_seed(1)
    return torch.rand(40, 3, generator=g) * 10 + 100.0, torch.tensor([6, 7, 8, 6] * 10)


def test_parse_request_implications_and_defaults():
    gen = _shell_generator()
    parse = postprocess.parse_request
    assert parse(gen, _ref(), interaction_scores=False, max_interaction_score=None) == postprocess.Request()
    rec = _receptor()
    plain = parse(gen, _ref(), overlay=True, receptor=rec)
    assert not plain.scores_interactions and plain.typed_receptor is None and plain.max_interaction_score is None
    req = parse(gen, _ref(), overlay=True, receptor=rec, interaction_scores=True)
    assert req.scores_interactions and not req.removes and req.rank_by == "shape" and not req.scores_shape
    assert isinstance(req.typed_receptor, IX.PreparedReceptor) and tuple(req.typed_receptor.xyzr.shape) == (40, 4)
    assert torch.equal(req.receptor[0], plain.receptor[0])
    req = parse(gen, _ref(), overlay=True, receptor=rec, max_interaction_score=-2.5)
    assert req.scores_interactions and req.max_interaction_score == -2.5 and req.removes
    req = parse(gen, _ref(), overlay=True, receptor=rec, interaction_scores=True, rank_by="interaction", top_k=3)
    assert req.rank_by == "interaction" and req.scores_shape and req.top_k == 3
    types = torch.arange(40) % 8
    req = parse(gen, _ref(), overlay=True, receptor=(rec[0], rec[1], types), interaction_scores=True)
    assert sorted(req.typed_receptor.types.tolist()) == sorted(types.tolist()) and len(req.receptor) == 2
    req = parse(gen, _ref(), overlay=True, receptor=(rec[0], rec[1], types))      # the types ride along unread
    assert req.typed_receptor is None and torch.equal(req.receptor[0], plain.receptor[0])
    assert IX.check_threshold("t", -3) == -3.0 and IX.check_rank_by("interaction") == "interaction"
    assert math.isnan(IX.select_score(None)) and IX.select_score(-2.0) == 2.0 and math.isnan(IX.select_score(math.nan))


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_interaction_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._interaction_scores = gen._receptor_coords = gen._score = gen._pose = gen._pharm_perceive = _no_device
    gen._match_substructures = _no_device
    call = getattr(gen, entry)
    rec = _receptor()
    nan, inf = float("nan"), float("inf")
    cases = [dict(interaction_scores=True),                                                   # no receptor
             dict(overlay=True, interaction_scores=True),
             dict(overlay=True, max_interaction_score=-1.0),
             dict(interaction_scores=True, receptor=rec),                                     # no overlay
             dict(overlay=True, receptor=rec, interaction_scores=1),
             dict(overlay=True, receptor=rec, interaction_scores="yes"),
             dict(overlay=True, receptor=rec, interaction_scores=None),
             dict(overlay=True, receptor=rec, rank_by="interaction"),                         # no score to rank by
             dict(rank_by="interaction"), dict(rank_by="interactions"),
             dict(overlay=True, receptor=(rec[0], rec[1], torch.full((40,), 8)), interaction_scores=True),
             dict(overlay=True, receptor=(rec[0], rec[1], torch.zeros(39, dtype=torch.long)), interaction_scores=True),
             dict(overlay=True, receptor=(rec[0], rec[1], torch.zeros(40)), interaction_scores=True)]
    for bad in (nan, inf, -inf, True, False, "1", [1.0]):
        cases.append(dict(overlay=True, receptor=rec, max_interaction_score=bad))
    for kw in cases:
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    for finisher in ("rdkit", HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                                         "finish_tag_chunk")):
        gen.finisher = finisher
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, overlay=True, receptor=rec, interaction_scores=True)
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, overlay=True, receptor=rec, max_interaction_score=0.0)


def _rows(shape, esp, score):
    n = len(shape)
    measured = [Measured(shape_tanimoto=s, electrostatic_tanimoto=e, interaction_score=v, chemical_tanimoto=0.1)
                for s, e, v in zip(shape, esp, score)]
    return postprocess.Rows(list(range(n)), list(range(n)), measured, list(range(n)),
                            sub=[([1], [0])] * n)


def test_select_filters_behind_the_electrostatic_filter_and_ranks_by_minus_the_score():
    nan = float("nan")
    Req = postprocess.Request
    shape = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4]
    esp = [0.1, 0.5, 0.6, 0.7, 0.9, 0.3]
    score = [-1.0, -5.0, nan, None, -3.0, 2.0]
    none = lambda rows: (_ for _ in ()).throw(AssertionError("no pair matrix was asked for"))        # noqa: E731
    sel = lambda req: postprocess.select(_rows(shape, esp, score), req, none, none)                  # noqa: E731
    # E <= t passes; NaN and None never do; the input's order stays
    assert sel(Req(scores_interactions=True, max_interaction_score=-1.0)) == [0, 1, 4]
    assert sel(Req(scores_interactions=True, max_interaction_score=-3.0)) == [1, 4]
    assert sel(Req(scores_interactions=True, max_interaction_score=1e30)) == [0, 1, 4, 5]
    both = Req(scores_electrostatics=True, min_electrostatic_tanimoto=0.4, scores_interactions=True, max_interaction_score=0.0)
    assert sel(both) == [1, 4]
    # its place: behind the electrostatic filter, in front of the substructure filters (source order of `select`)
    import inspect
    src = inspect.getsource(postprocess.select)
    assert src.index("req.min_electrostatic_tanimoto is not None") < src.index("req.max_interaction_score is not None") \
        < src.index("req.n_required or req.n_excluded")
    # rank_by="interaction": the most negative first, NaN and None last (ties to the lower sample id)
    ranked = Req(scores_shape=True, scores_interactions=True, rank_by="interaction", top_k=6)
    assert sel(ranked) == [1, 4, 0, 5, 2, 3]
    assert sel(Req(scores_shape=True, scores_interactions=True, rank_by="interaction", top_k=2)) == [1, 4]
    assert sel(Req(scores_shape=True, scores_interactions=True, top_k=2)) == [0, 1]                   # by shape, as before
    # `min_shape_tanimoto` keeps reading the shape score
    assert sel(Req(scores_shape=True, scores_interactions=True, rank_by="interaction", min_shape_tanimoto=0.55)) == [1, 0, 2, 3]
    req = Req(rank_by="interaction")
    assert req.ranking_score(Measured(interaction_score=-2.5)) == 2.5 and math.isnan(req.ranking_score(Measured()))


# ----------------------------------------------------------------------------------------------- the record path
SHARD = ["toluene", "acetamide", "butane", "pyridine", "ethanol", "biphenyl", "decalin", "chlorobenzene"]


def _shard_coords(name, n):
    g = np.random.default_rng(len(name) * 131 + n)
    return R.walk(n, g).astype(np.float32) + np.float32(3.0)


def _graph_shard(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
    ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
    el = torch.full((n_samples, 42), 9, dtype=torch.int8)                         # junk beyond the atoms
    bond = torch.full((n_samples, 42, 42), 3, dtype=torch.int8)
    x = torch.zeros(n_samples, 12, 3)
    n = torch.zeros(n_samples, dtype=torch.int32)
    for b, sid in enumerate(ids):
        z, adj, k = K.MOLECULES[SHARD[sid]][0]
        el[b, :k] = torch.tensor(z, dtype=torch.int8)
        bond[b, :k, :k] = torch.tensor(adj, dtype=torch.int8)
        n[b] = k
        x[b, :k] = torch.from_numpy(_shard_coords(SHARD[sid], k))
        if sid == 6:
            x[b, 0, 0] = float("nan")                                             # its pose fails
    valid = torch.tensor([0 if sid == 4 else 1 for sid in ids], dtype=torch.uint8)
    return dict(x=x, elements=el, bond=bond, n_nodes=n, valid=valid)


def _own(m, prepared):
    """The restatement's values of a record's own coordinates and graph against the prepared receptor."""
    z, adj = m.atomic_numbers, m.bond_orders.tolist()
    n = len(z)
    t = R.ligand_types(z, adj, n, K.pharm_types((z, adj, n)))
    return R.score(m.coords.numpy(), R.radii(z), t, prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(),
                   prepared.types.numpy(), R.rotatable_bonds(z, adj, n))


def _seam_interactions(calls):
    """`_interaction_scores` by the restatement, on the host."""
    def run(prepared, coords, n_nodes, atomic_numbers, bond_orders):
        assert isinstance(prepared, IX.PreparedReceptor)
        B, N = int(coords.shape[0]), int(coords.shape[1])
        calls.append(("interactions", B))
        out = dict(score=torch.zeros(B), terms=torch.zeros(B, 6), hbonds=torch.zeros(B, dtype=torch.int32),
                   atom_scores=torch.zeros(B, N), n_rot=torch.zeros(B, dtype=torch.int32))
        for b in range(B):
            k = int(n_nodes[b])
            z, adj = atomic_numbers[b, :k].tolist(), bond_orders[b, :k, :k].tolist()
            if not bool(torch.isfinite(coords[b, :k]).all()):
                out["score"][b], out["terms"][b], out["hbonds"][b], out["atom_scores"][b, :k] = math.nan, math.nan, -1, math.nan
                continue
            t = R.ligand_types(z, adj, k, K.pharm_types((z, adj, k)))
            rot = R.rotatable_bonds(z, adj, k)
            s = R.score(coords[b, :k].numpy(), R.radii(z), t, prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(),
                        prepared.types.numpy(), rot)
            out["score"][b], out["hbonds"][b], out["n_rot"][b] = s["score"], s["hbonds"], rot
            out["terms"][b, :5], out["terms"][b, 5] = torch.from_numpy(s["terms"]).float(), s["weighted"]
            out["atom_scores"][b, :k] = torch.from_numpy(s["atom_scores"]).float()
        return out
    return run


def _record_receptor():
    """A typed shell round where the stub pose puts the shard's molecules."""
    g = np.random.default_rng(9)
    pts = g.uniform(-9.0, 9.0, size=(400, 3))
    pts = pts[np.linalg.norm(pts, axis=1) > 4.5] + np.array([-3.0, 3.5, 3.0])
    return (torch.from_numpy(pts.astype(np.float32)), torch.from_numpy(g.choice([6, 7, 8], size=len(pts))),
            torch.from_numpy(g.integers(0, 8, size=len(pts))))


def test_record_path_carries_the_values_and_launches_nothing_unasked():
    calls = []
    gen = _shell_generator()
    gen._interaction_scores = _seam_interactions(calls)
    gen._generate_shard = _graph_shard
    gen._pose = _stub_overlay(lambda k: k * 0.0 + 0.5)
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    gen._receptor_coords = lambda rec, coords, n, z: torch.full(tuple(coords.shape[:2]), -1.0)
    rec = _record_receptor()
    kw = dict(reference_conformer=_ref(), n_samples=8, overlay=True, receptor=rec, optimise_geometry=False)
    fields = ("interaction_score", "interaction_terms", "receptor_hbonds", "interaction_atom_scores")

    plain = gen.generate_conformers(**kw)
    assert calls == [] and [m.sample_id for m in plain] == [0, 1, 2, 3, 5, 6, 7]             # 4: invalid
    assert all(getattr(m, f) is None for m in plain for f in fields)
    off = gen.generate_conformers(interaction_scores=False, max_interaction_score=None, **kw)
    keep = lambda mols: [m for m in mols if m.sample_id != 6]                     # noqa: E731 (6 holds a NaN: never equal)
    assert calls == [] and keep(off) == keep(plain) and [m.sample_id for m in off] == [m.sample_id for m in plain]
    flat = lambda m: {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in vars(m._measured).items()}   # noqa: E731
    assert [flat(m) for m in keep(off)] == [flat(m) for m in keep(plain)]
    got = gen.generate_conformers(interaction_scores=True, **kw)
    assert calls == [("interactions", 8)]                                         # one call over the rows
    assert [m.sample_id for m in got] == [0, 1, 2, 3, 5, 6, 7]
    prepared = IX.prepare_receptor(rec)
    scored = {}
    for a, m in zip(plain, got):
        if m.sample_id == 6:                                                      # its pose failed: None throughout
            assert all(getattr(m, f) is None for f in fields) and m.pose is None
            continue
        assert a == m and a.receptor_clashes == m.receptor_clashes == 0
        own = _own(m, prepared)
        assert np.float32(m.interaction_score) == np.float32(own["score"]) and m.receptor_hbonds == own["hbonds"]
        assert set(m.interaction_terms) == {"g1", "g2", "rep", "hyd", "hb", "n_rot"}
        assert m.interaction_terms["n_rot"] == K.MOLECULES[SHARD[m.sample_id]][2]
        assert [np.float32(m.interaction_terms[k]) for k in R.TERMS] == [np.float32(v) for v in own["terms"]]
        assert m.interaction_atom_scores.dtype == torch.float32
        assert m.interaction_atom_scores.tolist() == [float(np.float32(v)) for v in own["atom_scores"]]
        scored[m.sample_id] = m.interaction_score
    assert len(set(scored.values())) == 6 and min(scored.values()) < 0

    def ids(entry="generate_conformers", **more):
        return [m.sample_id for m in getattr(gen, entry)(**dict(kw, **more))]
    values = sorted(scored.values())
    t = (values[2] + values[3]) / 2
    assert ids(max_interaction_score=t) == [i for i in sorted(scored) if scored[i] <= t] and len(ids(max_interaction_score=t)) == 3
    assert ids(max_interaction_score=1e30) == sorted(scored)                      # a failed pose never passes
    order = sorted(scored, key=lambda i: (scored[i], i))
    assert ids(interaction_scores=True, rank_by="interaction", top_k=3) == order[:3]
    assert ids("generate_conformers_sharded", interaction_scores=True, rank_by="interaction", top_k=3) == order[:3]
    by_shape = {m.sample_id: m.shape_tanimoto for m in gen.generate_conformers(shape_scores=True, **kw)}
    assert ids(interaction_scores=True, top_k=3) == sorted(
        by_shape, key=lambda i: (-by_shape[i] if by_shape[i] == by_shape[i] else math.inf, i))[:3]
    assert [repr(m.interaction_score) for m in gen.forward(interaction_scores=True, **kw)] == \
        [repr(m.interaction_score) for m in got]
    assert isinstance(got[0], GeneratedMolecule)


def test_measured_from_tensors_reads_the_interaction_spellings():
    inf, nan = float("inf"), float("nan")
    atoms = torch.tensor([[0.1, -0.2, inf], [nan, inf, inf], [inf, inf, inf]])
    terms = torch.tensor([[1.0, 2.0, 0.5, 3.0, 1.0, 4.0], [nan] * 6, [0.0] * 6])
    rec = measured_from_tensors(dict(interaction_score=torch.tensor([-1.5, nan, 0.0]), interaction_terms=terms,
                                     receptor_hbonds=torch.tensor([2, -1, 0], dtype=torch.int32),
                                     interaction_atom_scores=atoms), 3)
    assert rec[0].interaction_score == -1.5 and rec[0].receptor_hbonds == 2
    assert rec[0].interaction_terms == dict(g1=1.0, g2=2.0, rep=0.5, hyd=3.0, hb=1.0, n_rot=4)
    assert rec[0].interaction_atom_scores[2] == 2 and rec[2].interaction_atom_scores[2] == 0
    assert all(getattr(rec[1], k) is None for k in ("interaction_score", "interaction_terms", "receptor_hbonds",
                                                    "interaction_atom_scores"))
    assert rec[2].interaction_score == 0.0 and rec[2].receptor_hbonds == 0
    assert all(getattr(Measured(), k) is None for k in ("interaction_score", "interaction_terms", "receptor_hbonds",
                                                        "interaction_atom_scores"))


# ----------------------------------------------------------------------------------------------- the C entry
def test_c_entry_refuses_bad_arguments_without_a_device():
    from ml_conformer_generator_amd import _lib
    assert "mcg_receptor_interactions" in _lib.SIGNATURES
    h = _lib.lib()
    assert h.mcg_abi_version() == 4
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    good = [p, p, p, p, p, 2, 27, p, p, 100, None, p, p, p, None]
    for k in (0, 1, 2, 3, 4, 7, 8, 11, 12, 13):                                   # each required buffer
        bad = list(good)
        bad[k] = None
        assert h.mcg_receptor_interactions(*bad) == 1 and b"mcg_receptor_interactions" in h.mcg_last_error(), k
    for B, N, Rn in ((0, 27, 100), (-1, 27, 100), (16385, 27, 100), (2, 0, 100), (2, 65, 100), (2, 27, 0), (2, 27, -5),
                     (2, 27, (1 << 17) + 1)):
        bad = list(good)
        bad[5], bad[6], bad[9] = B, N, Rn
        assert h.mcg_receptor_interactions(*bad) == 1, (B, N, Rn)


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_interactions`: the entry's argument checks in a stand-alone program under host-side ASan + UBSan, on the
    CPU."""
    exe = str(tmp_path / "interactions_arg_check")
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_interactions", f"INTERACTIONS_CHECK={exe}"], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 not refused" in ran.stdout, ran.stdout + ran.stderr


def test_header_compiles_with_the_new_declaration(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mlconfgen_hip.h"\n'
                   "int main(void) {\n"
                   "  int (*a)(const float*, const float*, const uint8_t*, const int32_t*, const int32_t*, int, int,\n"
                   "           const float*, const uint8_t*, int, const float*, float*, float*, int32_t*, void*)\n"
                   "      = mcg_receptor_interactions;\n"
                   "  return a == 0;\n}\n")
    inc = os.path.join(REPO, "include")
    assert shutil.which("gcc") or shutil.which("g++") or shutil.which("cc")
    for cc, flags in (("gcc", ["-std=c99", "-Wall", "-Wextra", "-Werror"]), ("g++", ["-std=c++11", "-Wall", "-Werror", "-x", "c++"]),
                      ("cc", ["-std=c99", "-Wall", "-Werror"])):
        if shutil.which(cc):
            r = subprocess.run([cc, *flags, "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
