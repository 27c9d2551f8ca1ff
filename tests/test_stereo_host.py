"""Stereo identity, host side (no GPU): the fp64 restatement of the definition and of the pruned search against the
brute force over all n! numberings, the named cases, the mutation checks, the isomeric SMILES writer through the
test-side reader, the options of the generation entries against stub seams backed by the restatement, and the C entry's
argument checks."""
import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import canonical_ref as R
import stereo_cases as SC
import stereo_ref as SR
from ml_conformer_generator_amd import canonical as CN
from ml_conformer_generator_amd import smiles as S
from ml_conformer_generator_amd import stereo as ST
from ml_conformer_generator_amd.handoff import molecules_from_tensors
from test_shape_overlay_host import _no_device, _ref, _shell_generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _agrees_with_brute_force(mol):
    out = SR.stereo(*mol)
    assert out["status"] == 0
    assert out["certificate"] == R.canonical(*mol[:3])["certificate"]           # the graph search's minimal certificate
    assert SR.brute_force(*mol, out["certificate"]) == out["stereo"], mol
    return out


# ----------------------------------------------------------------------------------------------- the restatement
def _small_embedded(rng, n):
    z = [rng.choice((6, 6, 6, 9, 17)) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a):
            adj[a][b] = adj[b][a] = rng.choice((0, 0, 1, 1, 1, 2))
    return z, adj, n, [tuple(rng.uniform(-2, 2) for _ in range(3)) for _ in range(n)]


def test_pruned_search_equals_brute_force_on_a_seeded_sample():
    """Graphs of at most 6 atoms, Z in {6, 9, 17}, codes {0, 1, 2}, random coordinates - and symmetric ones on purpose
    (rings and stars of one element, where non-terminal twins occur): the pruned search's stereo vector is the smallest
    over ALL numberings with the minimal certificate, every descriptor there read from the geometry."""
    rng = random.Random(20261020)
    seen = [0, 0, 0]
    mols = [_small_embedded(rng, rng.randint(1, 6)) for _ in range(220)]
    for n in (4, 5, 6):                                     # rings with and without a chord, stars
        for _ in range(6):
            xyz = [tuple(rng.uniform(-2, 2) for _ in range(3)) for _ in range(n)]
            ring = [(k, (k + 1) % n, 1) for k in range(n)]
            mols.append(R.mol([6] * n, ring) + (xyz,))
            mols.append(R.mol([6] * n, ring + [(0, 2, 1)]) + (xyz,))
            mols.append(R.mol([6] + [9] * (n - 1), [(0, k, 1) for k in range(1, min(n, 5))]) + (xyz,))
    for k in range(24):                                     # substituted ethenes: one to two substituents per end
        bonds = [(0, 1, 1), (1, 2, 2), (2, 3, 1)] + [(1, 4, 1)] * (k % 2) + [(2, 4 + k % 2, 1)] * (k // 2 % 2)
        n = 4 + k % 2 + k // 2 % 2
        mols.append(R.mol([rng.choice((6, 9, 17)) if a not in (1, 2) else 6 for a in range(n)], bonds) +
                    ([tuple(rng.uniform(-2, 2) for _ in range(3)) for _ in range(n)],))
    for mol in mols:
        out = _agrees_with_brute_force(mol)
        seen = [s + c for s, c in zip(seen, out["counts"])]
    assert min(seen) > 10, seen                              # the sample holds centres, double bonds and undefined ones


@pytest.mark.parametrize("name", sorted(SC.NAMED))
def test_named_case(name):
    """The counts and leaves derived by hand (`stereo_cases`), the brute force (all have at most 8 atoms), the mirror
    image, and 8 renumberings under random proper rigid motions."""
    mol, counts, leaves, achiral = SC.NAMED[name]
    rng = random.Random(sum(map(ord, name)))
    first = _agrees_with_brute_force(mol)
    assert (first["counts"], first["leaves"]) == (counts, leaves)
    ident = SR.identity_bytes(*mol)
    if achiral is not None:
        assert (SR.identity_bytes(*SC.mirror(mol)) == ident) == achiral
        assert SR.same_stereoisomer(mol, SC.mirror(mol)) == achiral
    key = SR.stereo_key(*mol[:3], first["order"], first["stereo"])
    for _ in range(8):
        other = SC.moved(rng, SC.renumbered(rng, mol))
        out = SR.stereo(*other)
        assert (out["status"], out["leaves"], out["certificate"], out["stereo"], out["counts"]) == \
            (0, leaves, first["certificate"], first["stereo"], counts)
        assert SR.identity_bytes(*other) == ident and SR.stereo_key(*other[:3], out["order"], out["stereo"]) == key
        assert R.key(*other[:3], out["order"]) == R.key(*mol[:3], R.canonical(*mol[:3])["order"])   # the graph key


def test_named_pairs():
    ids = [SR.identity_bytes(*m) for m in SC.DICHLOROBUTANES]
    assert len(set(ids)) == 3                                # four sign combinations, three stereoisomers
    meso = [m for m in SC.DICHLOROBUTANES if ids.count(SR.identity_bytes(*m)) == 2]
    assert len(meso) == 2 and all(SR.identity_bytes(*SC.mirror(m)) == SR.identity_bytes(*m) for m in meso)
    pair = [m for m in SC.DICHLOROBUTANES if m not in meso]
    assert SR.identity_bytes(*SC.mirror(pair[0])) == SR.identity_bytes(*pair[1])
    for a, b in itertools.combinations(SC.DICHLOROBUTANES, 2):
        assert SR.same_stereoisomer(a, b) == (SR.identity_bytes(*a) == SR.identity_bytes(*b))
    for cis, trans in ((SC.CIS_DCE, SC.TRANS_DCE), (SC.CIS_DMCB, SC.TRANS_DMCB), (SC.CIS_DMCH, SC.TRANS_DMCH),
                       (SC.HEXADIENE, SC.HEXADIENE_CIS_TRANS)):
        assert SR.identity_bytes(*cis) != SR.identity_bytes(*trans)
        assert R.identity_bytes(*cis[:3]) == R.identity_bytes(*trans[:3])         # one constitution
        if cis[2] <= 6:
            assert not SR.same_stereoisomer(cis, trans)
    assert SR.stereo(*SC.CYCLOHEXENE)["stereo"] == (0, 0, 0, 0, 0, 1)             # cis: the constant of a small ring
    assert SR.identity_bytes(*SC.CHFCLBR) != SR.identity_bytes(*SC.swapped(SC.CHFCLBR, 1, 2))
    assert SR.identity_bytes(*SC.mirror(SC.CHFCLBR)) == SR.identity_bytes(*SC.swapped(SC.CHFCLBR, 1, 2))
    big = SR.stereo(*SC.sixty_four())
    assert (big["counts"], big["status"], big["leaves"]) == ((1, 0, 0), 0, 1)
    assert big["stereo"] != SR.stereo(*SC.mirror(SC.sixty_four()))["stereo"]
    assert SR.stereo(*SC.over_degree())["status"] == R.DEGREE and SR.stereo([], [], 0, [])["status"] == R.EMPTY
    assert SR.identity_bytes(*SC.over_degree()) is None


def test_mutations_of_the_definition():
    """First leaf wins ties: the meso identity depends on the numbering.  The full twin rule: a cyclobutane's does."""
    rng = random.Random(4)
    meso = [m for m in SC.DICHLOROBUTANES if SR.identity_bytes(*SC.mirror(m)) == SR.identity_bytes(*m)][0]
    for mol, mutation in ((meso, dict(first_leaf_wins=True)), (SC.TRANS_DMCB, dict(full_twin_rule=True))):
        renumberings = [SC.renumbered(rng, mol) for _ in range(16)]
        assert len({SR.stereo(*m)["stereo"] for m in renumberings}) == 1
        assert len({SR.stereo(*m, **mutation)["stereo"] for m in renumberings}) == 2
    graph, full = R.canonical(*SC.TRANS_DMCB[:3]), SR.stereo(*SC.TRANS_DMCB, full_twin_rule=True)
    assert (graph["leaves"], full["leaves"], SR.stereo(*SC.TRANS_DMCB)["leaves"]) == (2, 2, 4)
    # terminal twins stay skipped: sixteen isolated atoms are one leaf, neopentane's methyls one
    assert SR.stereo([6] * 16, [[0] * 16] * 16, 16, [(float(k), 0.0, 0.0) for k in range(16)])["leaves"] == 1
    assert SR.stereo(*SC.GEM_DIMETHYL)["leaves"] == 1


# ----------------------------------------------------------------------------------------------- the writer
def _isomeric(mol, canonical=True):
    """(the string, unmarked double bonds) of an embedded molecule: in canonical order with v as it is, or in its own
    order through `stereo.own_order_descriptors`."""
    out = SR.stereo(*mol)
    z, adj, n, _ = mol
    if canonical:
        zc, ac, _ = R.permute(z, adj, n, out["order"])
        return S.write_smiles_counted(zc, torch.tensor(ac, dtype=torch.int8).reshape(n, n), out["stereo"])
    own = ST.own_order_descriptors(out["order"], out["stereo"], torch.tensor(adj, dtype=torch.int8).reshape(n, n))
    return S.write_smiles_counted(z, torch.tensor(adj, dtype=torch.int8).reshape(n, n), own)


def _read_identity(text):
    z, adj, n, tet, dbs = SR.read_isomeric(text)
    out = SR.stereo(z, adj, n, None, perceived=(tet, dbs))
    return R.identity_bytes(z, adj, n) + bytes(out["stereo"])


def test_own_order_descriptors_are_the_restatement_at_the_identity_labelling():
    rng = random.Random(12)
    for mol in [m for m, _, _, _ in SC.NAMED.values()] + [SC.TRANS_CYCLOOCTENE, SC.sixty_four()]:
        for m in (mol, SC.renumbered(rng, mol)):
            out = SR.stereo(*m)
            n = m[2]
            own = ST.own_order_descriptors(out["order"], out["stereo"], torch.tensor(m[1], dtype=torch.int8).reshape(n, n))
            tet, dbs = SR.tetrahedral(*m), SR.double_bonds(*m)
            assert own == SR.descriptors(tet, dbs, n, list(range(n)))


def test_smiles_anchors_by_the_opensmiles_text():
    """Explicit coordinates.  The viewer sits on the first neighbour, +z, and looks down at the centre: x to the right and
    y up, so growing angles run anticlockwise.  The other three at 0, 120 and 240 degrees are anticlockwise in that order:
    "@".  trans-1,2-difluoroethene is F/C=C/F."""
    ring = [(math_cos, math_sin, -0.5) for math_cos, math_sin in ((1.4, 0.0), (-0.7, 1.2124), (-0.7, -1.2124))]
    z, adj, n = R.mol([9, 6, 17, 35, 53], [(1, 0, 1), (1, 2, 1), (1, 3, 1), (1, 4, 1)])      # F first, then C, Cl, Br, I
    xyz = [(0.0, 0.0, 1.5), (0.0, 0.0, 0.0)] + ring
    tet = SR.tetrahedral(z, adj, n, xyz)
    own = SR.descriptors(tet, {}, n, list(range(n)))
    assert S.write_smiles(z, adj, own) == "F[C@](Cl)(Br)I"
    assert S.write_smiles(z, adj, SR.descriptors(SR.tetrahedral(*SC.mirror((z, adj, n, xyz))), {}, n, list(range(n)))) \
        == "F[C@@](Cl)(Br)I"
    # the implicit hydrogen: the same picture with I taken away is [C@H] seen from F with H, Cl, Br... H takes I's place
    # in the written order directly behind F, which is two transpositions away from (Cl, Br, H): the same mark
    z3, adj3, _ = R.mol([9, 6, 17, 35], [(1, 0, 1), (1, 2, 1), (1, 3, 1)])
    own3 = SR.descriptors(SR.tetrahedral(z3, adj3, 4, xyz[:4]), {}, 4, list(range(4)))
    assert S.write_smiles(z3, adj3, own3) == "F[C@H](Cl)Br"
    zf, adjf, _ = R.mol([9, 6, 6, 9], [(0, 1, 1), (1, 2, 2), (2, 3, 1)])
    for side, text in ((-1, "F/C=C/F"), (1, "F/C=C\\F")):
        xyz = [(-0.7, 1.2, 0.0), (0.0, 0.0, 0.0), (1.34, 0.0, 0.0), (2.04, 1.2 * side, 0.0)]
        own = SR.descriptors([None] * 4, SR.double_bonds(zf, adjf, 4, xyz), 4, list(range(4)))
        assert own == [0, 0, 2 if side < 0 else 1, 0] and S.write_smiles(zf, adjf, own) == text
    assert S.write_smiles(zf, adjf) == S.write_smiles(zf, adjf, [0] * 4) == "FC=CF"
    with pytest.raises(ValueError, match="one descriptor per atom"):
        S.write_smiles(zf, adjf, [0] * 3)


def test_isomeric_strings_round_trip_through_the_reader():
    """write -> read -> the restated identity from the read parities equals the original's: the named cases in canonical
    and in their own order, a conjugated diene that shares a single bond, an end with ring-closure bonds only."""
    rng = random.Random(6)
    mols = [m for m, _, _, _ in SC.NAMED.values()] + [SC.HEXADIENE_CIS_TRANS, SC.TRANS_CYCLOOCTENE, SC.CFCLBRI,
                                                      SC.mirror(SC.CHFCLBR)] + SC.DICHLOROBUTANES
    mols += [SC.renumbered(rng, m) for m in mols]
    for mol in mols:
        ident = SR.identity_bytes(*mol)
        canon, unmarked = _isomeric(mol)
        assert unmarked == 0 and _read_identity(canon) == ident, canon
        own, unmarked = _isomeric(mol, canonical=False)
        assert unmarked == 0 and _read_identity(own) == ident, own
        assert _isomeric(SC.moved(rng, SC.renumbered(rng, mol)))[0] == canon           # one string per stereoisomer
    assert _isomeric(SC.HEXADIENE)[0] != _isomeric(SC.HEXADIENE_CIS_TRANS)[0]
    assert _isomeric(SC.HEXADIENE)[0].count("/") + _isomeric(SC.HEXADIENE)[0].count("\\") == 3    # the shared bond once
    # the ring-closure-only end: atom 0 of trans-cyclooctene written first has one tree edge - its double bond
    z, adj, n, xyz = SC.TRANS_CYCLOOCTENE
    own = SR.descriptors(SR.tetrahedral(*SC.TRANS_CYCLOOCTENE), SR.double_bonds(*SC.TRANS_CYCLOOCTENE), n, list(range(n)))
    text = S.write_smiles(z, adj, own)
    assert text in ("C/1=C/CCCCCC1", "C/1=C\\CCCCCC1") and _read_identity(text) == SR.identity_bytes(*SC.TRANS_CYCLOOCTENE)
    # marks may sit on centres a reader does not call stereogenic: 3-pentanol's C3 carries one, in both mirror images
    assert "@" in _isomeric(SC.PENTAN_3_OL)[0] and _isomeric(SC.PENTAN_3_OL)[0] == _isomeric(SC.mirror(SC.PENTAN_3_OL))[0]
    assert _isomeric(SC.CHFCLBR)[0] != _isomeric(SC.mirror(SC.CHFCLBR))[0]
    assert "@" not in _isomeric(SC.PLANAR_CENTRE)[0] and "@" not in _isomeric(SC.GEM_DIMETHYL)[0]


# ----------------------------------------------------------------------------------------------- options
_SCORES = [0.3, 0.9, 0.5, 0.8, 0.2, 0.6, 0.4, 0.7]


def _planted():
    """sample id -> embedded molecule: 1 is the mirror image of 0, 2 is 0 renumbered and moved; 4 / 5 are cis / trans; 6 and
    7 have an atom with nine neighbours (no order of either kind)."""
    rng = random.Random(21)
    return [SC.CHFCLBR, SC.mirror(SC.CHFCLBR), SC.moved(rng, SC.renumbered(rng, SC.CHFCLBR)), SC.BUTAN_2_OL, SC.CIS_DCE,
            SC.TRANS_DCE, SC.over_degree(), SC.moved(rng, SC.over_degree())]


def _seam_stereo(calls):
    """`_stereo_order` by the restatement, on the host; NaN beyond a row's atoms must not matter."""
    def run(coords, z, bonds, n):
        coords, z, bonds = torch.as_tensor(coords), torch.as_tensor(z), torch.as_tensor(bonds)
        n = torch.as_tensor(n).reshape(-1).tolist()
        calls.append(len(n))
        W = int(bonds.shape[1])
        order = torch.full((len(n), W), -1, dtype=torch.int32)
        stereo = torch.zeros(len(n), W, dtype=torch.int8)
        status, leaves, keys, skeys, counts = [], [], [], [], []
        for b, k in enumerate(n):
            mol = (z[b, :k].tolist(), bonds[b, :k, :k].tolist(), k, [tuple(p) for p in coords[b, :k].double().tolist()])
            out = SR.stereo(*mol)
            status.append(out["status"])
            leaves.append(out["leaves"])
            counts.append(list(out["counts"]))
            keys.append(R.key(*mol[:3], out["order"]) if out["status"] == 0 else 0)
            skeys.append(SR.stereo_key(*mol[:3], out["order"], out["stereo"]) if out["status"] == 0 else 0)
            if out["status"] == 0:
                order[b, :k] = torch.tensor(out["order"], dtype=torch.int32)
                stereo[b, :k] = torch.tensor(out["stereo"], dtype=torch.int8)
        as64 = lambda v: torch.from_numpy(np.array(v, dtype=np.uint64).view(np.int64))
        return dict(order=order, status=torch.tensor(status, dtype=torch.int32), leaves=torch.tensor(leaves, dtype=torch.int32),
                    key=as64(keys), stereo=stereo, stereo_key=as64(skeys), counts=torch.tensor(counts, dtype=torch.int32))
    return run


def _embedded_shard(mols):
    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
        el = torch.full((n_samples, 42), 9, dtype=torch.int8)                     # junk beyond the atoms
        bond = torch.full((n_samples, 42, 42), 3, dtype=torch.int8)
        x = torch.full((n_samples, 42, 3), float("nan"))
        n = torch.zeros(n_samples, dtype=torch.int32)
        for b, sid in enumerate(ids):
            z, adj, k, xyz = mols[sid]
            el[b, :k] = torch.tensor(z, dtype=torch.int8)
            bond[b, :k, :k] = torch.tensor(adj, dtype=torch.int8)
            n[b] = k
            x[b, :k] = torch.tensor(xyz, dtype=torch.float64).float()
            x[b, 41, 0] = _SCORES[sid]                                            # the stub shape score, in the padding
        return dict(x=x, elements=el, bond=bond, n_nodes=n, valid=torch.ones(n_samples, dtype=torch.uint8))
    return run


def _generator(calls, stereo_calls, finisher=None):
    from test_canonical_host import _seam_canonical
    from test_fingerprint_host import _seam_fingerprints
    gen = _shell_generator(finisher=finisher)
    gen._canonical_order = _seam_canonical(calls)
    gen._stereo_order = _seam_stereo(stereo_calls)
    gen._graph_fingerprints = _seam_fingerprints([])
    gen._score = lambda ref, coords, n: coords[:, 41, 0].clone()
    return gen


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_stereo_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._canonical_order = gen._stereo_order = gen._graph_fingerprints = gen._score = _no_device
    call = getattr(gen, entry)
    for kw in (dict(smiles="Isomeric"), dict(smiles="iso"), dict(smiles=b"isomeric"), dict(smiles="stereo"), dict(smiles=2),
               dict(unique="Stereo"), dict(unique="stereoo"), dict(unique=b"stereo"), dict(unique="isomeric"),
               dict(unique="stereo", top_k=0)):
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    custom = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"), "finish_tag_chunk")
    for finisher in ("rdkit", custom):
        gen.finisher = finisher
        with pytest.raises(ValueError) as e:
            call(reference_conformer=_ref(), n_samples=4, smiles="isomeric")
        assert str(e.value) == CN.REFUSAL_WITH_FINISHER
        with pytest.raises(ValueError) as e:
            call(reference_conformer=_ref(), n_samples=4, unique="stereo")
        assert str(e.value) == ST.REFUSAL_UNIQUE_WITH_FINISHER and "finisher" in str(e.value)


def test_unique_stereo_keeps_both_enantiomers_where_exact_keeps_one():
    mols = _planted()
    calls, stereo_calls = [], []
    gen = _generator(calls, stereo_calls)
    gen._generate_shard = _embedded_shard(mols)
    kw = dict(reference_conformer=_ref(), n_samples=8)

    def ids(**more):
        return [m.sample_id for m in gen.generate_conformers(**dict(kw, **more))]
    assert ids() == list(range(8)) and calls == [] and stereo_calls == []          # no option: neither seam is touched
    assert ids(unique="exact") == [0, 3, 4, 6, 7] and stereo_calls == []           # one per constitution; no order: stays
    assert ids(unique="stereo") == [0, 1, 3, 4, 5, 6, 7] and stereo_calls == [8] and calls == [8]   # "exact" made the 8
    assert ids(unique="stereo", shape_scores=True) == [1, 2, 3, 4, 5, 6, 7]         # the better-ranked copy: 2 (0.5) over 0
    assert ids(unique="stereo", top_k=3) == [1, 3, 7]
    assert [m.sample_id for m in gen.generate_conformers_sharded(unique="stereo", **kw)] == [0, 1, 3, 4, 5, 6, 7]
    assert [m.sample_id for m in gen.forward(unique="stereo", **kw)] == [0, 1, 3, 4, 5, 6, 7]
    assert ids(unique="stereo", exclude_graphs=[mols[4][:2]]) == [0, 1, 3, 6, 7]    # exclusion stays at constitution level
    assert all(m.stereo_status is None and m.smiles is None for m in gen.generate_conformers(unique="stereo", **kw))


def test_smiles_isomeric_adds_to_what_smiles_true_gives():
    mols = _planted()
    calls, stereo_calls = [], []
    gen = _generator(calls, stereo_calls)
    gen._generate_shard = _embedded_shard(mols)
    kw = dict(reference_conformer=_ref(), n_samples=8)
    plain = gen.generate_conformers(smiles=True, **kw)
    got = gen.generate_conformers(smiles="isomeric", **kw)
    assert calls == [8, 8] and stereo_calls == [8]                                  # one more launch
    assert [m.sample_id for m in got] == list(range(8))
    for a, m in zip(plain, got):
        sid = m.sample_id
        assert a == m and (a.canonical_order, a.canonical_status) == (m.canonical_order, m.canonical_status)
        assert a.stereo_status is None and a.stereo_order is None and a.stereo_descriptors is None
        assert a.n_stereo_defined is None and a.n_stereo_unmarked is None
        ref = SR.stereo(*mols[sid])
        assert m.stereo_status == ref["status"]
        assert (m.n_stereo_defined, m.n_stereo_undefined) == (ref["counts"][0] + ref["counts"][1], ref["counts"][2])
        if sid in (6, 7):
            assert m.stereo_order is None and m.stereo_descriptors is None and m.smiles is None and a.smiles is None
            with pytest.raises(ValueError, match="DEGREE"):
                m.to_smiles(isomeric=True)
            continue
        assert m.to_smiles(isomeric=False) == a.smiles == a.to_smiles()             # the non-isomeric string, bit for bit
        assert m.stereo_order == ref["order"]
        n = mols[sid][2]
        assert m.stereo_descriptors == SR.descriptors(SR.tetrahedral(*mols[sid]), SR.double_bonds(*mols[sid]), n,
                                                      list(range(n)))
        assert m.smiles == m.to_smiles() == _isomeric(mols[sid])[0] and m.n_stereo_unmarked == 0
        assert _read_identity(m.smiles) == _read_identity(m.to_smiles(canonical=False)) == SR.identity_bytes(*mols[sid])
    assert got[0].smiles == got[2].smiles != got[1].smiles and plain[0].smiles == plain[1].smiles == plain[2].smiles
    assert {got[0].smiles, got[1].smiles} == {"[C@H](F)(Cl)Br", "[C@@H](F)(Cl)Br"}
    assert (got[4].smiles, got[5].smiles) == ("C(=C/Cl)/Cl", "C(=C\\Cl)/Cl")      # cis: both Cl up
    with pytest.raises(ValueError, match='smiles="isomeric"'):
        plain[0].to_smiles(isomeric=True)
    both = gen.generate_conformers(smiles="isomeric", unique="stereo", **kw)
    assert [m.sample_id for m in both] == [0, 1, 3, 4, 5, 6, 7] and stereo_calls == [8, 8]     # one launch serves both
    assert both[1].smiles == got[1].smiles


def test_stereo_record_fields_from_tensors():
    z, adj, n, xyz = SC.CHFCLBR
    ref = SR.stereo(*SC.CHFCLBR)
    order = torch.tensor([ref["order"] + [-1], [-1] * 5], dtype=torch.int32)
    v = torch.tensor([list(ref["stereo"]) + [0], [0] * 5], dtype=torch.int8)
    bonds = torch.zeros(2, 5, 5, dtype=torch.int8)
    bonds[0, :4, :4] = torch.tensor(adj, dtype=torch.int8)
    x = torch.zeros(2, 5, 3)
    x[0, :4] = torch.tensor(xyz)
    mols = molecules_from_tensors(x, torch.tensor([z + [0], [6, 0, 0, 0, 0]]), bonds, torch.tensor([4, 1]), torch.ones(2),
                                  canonical_order=order, canonical_status=torch.tensor([0, 0], dtype=torch.int32),
                                  stereo_order=order, stereo_status=torch.tensor([0, 4], dtype=torch.int32),
                                  stereo_descriptors=v, n_stereo_defined=torch.tensor([1, 0]),
                                  n_stereo_undefined=torch.tensor([0, 0]))
    assert mols[0].stereo_order == ref["order"] and mols[0].stereo_descriptors == [4, 0, 0, 0]
    assert mols[0].smiles == _isomeric(SC.CHFCLBR)[0] and "@" in mols[0].smiles
    assert mols[1].stereo_order is None and mols[1].stereo_descriptors is None and mols[1].stereo_status == 4
    with pytest.raises(ValueError, match="BUDGET"):
        mols[1].to_smiles(isomeric=True)


# ----------------------------------------------------------------------------------------------- C ABI
def test_stereo_entry_refuses_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check

    def order(coords=p, z=p, bonds=p, n=p, B=3, W=42, out=p, status=p, leaves=p, key=p, stereo=p, skey=p, counts=p):
        return h.mcg_stereo_order(coords, z, bonds, n, B, W, out, status, leaves, key, stereo, skey, counts, None)

    for bad in (dict(coords=None), dict(z=None), dict(bonds=None), dict(n=None), dict(out=None), dict(status=None),
                dict(leaves=None), dict(key=None), dict(stereo=None), dict(skey=None), dict(counts=None), dict(B=-1),
                dict(B=16385), dict(W=0), dict(W=65), dict(W=-3)):
        assert order(**bad) == 1, bad
        assert b"mcg_stereo_order" in h.mcg_last_error(), bad
    assert order(B=0) == 0                        # nothing to do, nothing launched
    assert h.mcg_abi_version() == 4 and "mcg_stereo_order" in _lib.SIGNATURES
    good = (torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8), torch.tensor([3, 2]))
    for coords in (torch.zeros(2, 5, 2), torch.zeros(3, 5, 3), torch.zeros(2, 5, 3, dtype=torch.int32), torch.zeros(2, 15)):
        with pytest.raises(ValueError, match="coords"):
            ST.stereo_order(coords, *good)
    with pytest.raises(ValueError, match="n_nodes"):
        ST.stereo_order(torch.zeros(2, 2, 3), *good)          # narrower than the graphs: fine up to the largest molecule
    with pytest.raises(ValueError):
        ST.stereo_order(torch.zeros(1, 65, 3), torch.zeros(1, 65, dtype=torch.int32),
                        torch.zeros(1, 65, 65, dtype=torch.int8), torch.tensor([3]))
    with pytest.raises(ValueError):
        ST.stereo_order(torch.zeros(2, 5, 3), good[0], good[1], torch.tensor([3, 6]))


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_stereo`: the entry's argument checks in a stand-alone program under host-side ASan + UBSan, on the CPU."""
    exe = str(tmp_path / "stereo_arg_check")
    csrc = os.path.join(ROOT, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_stereo", f"STEREO_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 wrong" in ran.stdout, ran.stdout + ran.stderr
