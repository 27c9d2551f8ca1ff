"""Standardised graphs without a GPU ("Standardised graphs"): the plain-Python restatement against the
hand-derived answers of `standardize_cases`, against an independent brute-force matching checker, and against deliberate
mis-readings of the definition; the argument refusals of `standardize_graphs` that need no device; the record's new
fields and the `ValueError`s of `to_molblock(kekulize=True)`."""
import types

import pytest
import torch

import standardize_cases as C
import standardize_ref as SR


def test_restatement_reproduces_the_hand_derived_answers():
    cases, ref = C.cases(), C.references()
    assert {"benzene", "pyridine", "pyrrole", "furan", "imidazole", "pyrazine", "2-pyridone", "naphthalene", "indole",
            "benzimidazole", "azulene", "cyclopentadienyl", "N-methylpyridine", "aromatic biphenyl", "benzene and water",
            "propane and ethanol", "two ethanes", "benzene and a bad fragment", "five-bonded carbon", "no atoms",
            "one atom", "interleaved 64", "decacene", "triangular 46 shuffled"} <= set(cases)
    for name, c in cases.items():
        r, (z, codes, n) = ref[name], c["mol"]
        assert r["status"] == c["status"], (name, r["status"])
        assert r["atom_map"] == c["atom_map"] and r["n_out"] == len(c["atom_map"]), name
        assert r["n_fragments"] == c["n_fragments"] and r["atoms_removed"] == n - len(c["atom_map"]), name
        assert r["atomic_numbers"] == [z[a] for a in c["atom_map"]], name
        m = r["n_out"]
        if c["status"]:
            assert r["kekule_orders"] == [[0] * m for _ in range(m)], name
            continue
        if c["doubles"] is not None:
            assert r["doubles"] == c["doubles"], (name, r["doubles"])
        for i in range(m):                            # a Kekule form: no code 4 left, symmetric, nobody above v0
            for j in range(m):
                code, k = r["bond_orders"][i][j], r["kekule_orders"][i][j]
                assert k == r["kekule_orders"][j][i] and (k == code if code != 4 else k in (1, 2)), name
            if 4 in r["bond_orders"][i]:
                assert sum(r["kekule_orders"][i]) <= SR.V0.get(r["atomic_numbers"][i], 0), (name, i)
            assert sum(1 for j in range(m) if r["bond_orders"][i][j] == 4 and r["kekule_orders"][i][j] == 2) <= 1, name
    assert cases["pyrrole"]["xyz"][2, 1] != cases["pyrrole"]["xyz"][2, 1]          # the NaN is there, and is copied
    assert ref["interleaved 64"]["atom_map"] == list(range(1, 64, 2))


def test_budget_cases_sit_where_they_were_chosen():
    ref = C.references()
    assert C.cases()["decacene"]["mol"][2] == 42 and ref["decacene"]["status"] == 0
    assert max(ref["decacene"]["steps"]) <= 64                                    # far inside the budget
    assert ref["triangular 46 shuffled"]["status"] == SR.SEARCH_BUDGET
    assert ref["triangular 46 shuffled"]["steps"] == [SR.KEKULE_BUDGET + 1]
    assert ref["triangular 46"]["status"] == SR.NOT_KEKULIZABLE                   # the same graph, numbered geometrically
    assert max(ref["triangular 46"]["steps"]) < SR.KEKULE_BUDGET


def test_verdict_equals_the_brute_force_checker():
    seen = {True: 0, False: 0}
    for name, c in C.cases().items():
        r = C.references()[name]
        if r["status"] & (SR.EMPTY | SR.OVER_VALENCE | SR.AROMATIC_BRIDGE | SR.SEARCH_BUDGET):
            continue                                  # the search did not run, or did not finish
        if C.eligible_count(c["mol"]) > 14:
            continue
        exists = SR.matching_exists(*c["mol"], keep=c["atom_map"])
        assert exists == (r["status"] == 0), name
        seen[exists] += 1
    assert seen[True] >= 12 and seen[False] >= 2


def test_mutations_change_a_listed_answer():
    """Each deliberate mis-reading of the definition must show on the hand-derived answers, or they pin nothing."""
    cases = C.cases()
    small = {k: c for k, c in cases.items() if c["mol"][2] <= 12}

    def differs(mutation):
        out = []
        for name, c in small.items():
            r = SR.standardize(*c["mol"], mutate=mutation)
            if (r["status"], r["atom_map"], r["doubles"] if c["doubles"] is not None else None) != \
                    (c["status"], c["atom_map"], c["doubles"]):
                out.append(name)
        return out
    assert differs(None) == []
    assert "imidazole" in differs("lowest_first")     # the unmatched N moves from N0 to N2
    assert {"pyrrole", "indole"} <= set(differs("no_optional"))
    assert differs("no_tie_break") == ["propane and ethanol"]


def test_status_names():
    from ml_conformer_generator_amd import standardize as S
    assert (S.EMPTY, S.OVER_VALENCE, S.AROMATIC_BRIDGE, S.NOT_KEKULIZABLE, S.SEARCH_BUDGET) == \
        (SR.EMPTY, SR.OVER_VALENCE, SR.AROMATIC_BRIDGE, SR.NOT_KEKULIZABLE, SR.SEARCH_BUDGET)
    assert S.KEKULE_BUDGET == SR.KEKULE_BUDGET and S.MAX_ATOMS == 64 and S.MAX_BATCH == 16384
    assert S.describe_status(0) == [] and S.describe_status(12) == ["AROMATIC_BRIDGE", "NOT_KEKULIZABLE"]
    assert S.describe_status(31) == list(S.STATUS_NAMES.values())
    for bad in (-1, 32):
        with pytest.raises(ValueError):
            S.describe_status(bad)
    from ml_conformer_generator_amd import hydrogens as HY
    from ml_conformer_generator_amd.config import ELEMENTS
    assert HY.VALENCE == SR.V0                        # the restatement wrote the two tables out again
    assert {z: v for z, v in SR.MAX_VALENCE.items()} == {z: ELEMENTS[z][2] for z in SR.MAX_VALENCE if z in ELEMENTS}


def test_refusals_that_need_no_device():
    from ml_conformer_generator_amd import standardize as S
    x, z, b, n = torch.zeros(2, 5, 3), torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8), \
        torch.tensor([5, 3])
    for args in ((x[:, :, :2], z, b, n),                                          # coords not [B,N,3]
                 (x.to(torch.int32), z, b, n),                                    # integer coordinates
                 (x, z, b[:, :, :4], n),                                          # bonds not square
                 (x, z[:, :4], b, n),                                             # too few atomic numbers
                 (x, z.float(), b, n), (x, z, b.float(), n),                      # float graph tensors
                 (x[:1], z, b, n),                                                # another batch
                 (x, z, b, n[:1]),                                                # another count of counts
                 (x, z, b, torch.tensor([6, 3])), (x, z, b, torch.tensor([5, -1])),      # counts outside [0, min(N, W)]
                 (x[:, :4], z, b, n),                                             # n = 5 > N = 4
                 (torch.zeros(1, 65, 3), torch.ones(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8),
                  torch.tensor([65]))):                                           # W > 64
        with pytest.raises(ValueError):
            S.standardize_graphs(*args)
    from ml_conformer_generator_amd import postprocess
    with pytest.raises(ValueError, match="finisher"):
        postprocess.parse_request(types.SimpleNamespace(finisher="rdkit"), None, standardize=True)
    with pytest.raises(ValueError):
        postprocess.parse_request(types.SimpleNamespace(finisher=None), None, standardize=1)
    assert postprocess.parse_request(types.SimpleNamespace(finisher=None), None, standardize=True).standardize is True
    assert postprocess.parse_request(types.SimpleNamespace(finisher="rdkit"), None).standardize is False


def _records(names, hydrogen_parents=None):
    """Records as a generation call with `standardize=True` builds them, from the restatement's answers (host tensors)."""
    from ml_conformer_generator_amd.handoff import molecules_from_tensors
    ref = C.references()
    B, W = len(names), 12
    x, el, bond, kek = torch.zeros(B, W, 3), torch.zeros(B, W, dtype=torch.int8), \
        torch.zeros(B, W, W, dtype=torch.int8), torch.zeros(B, W, W, dtype=torch.int8)
    amap = torch.full((B, W), -1, dtype=torch.int32)
    n, removed, frags = (torch.zeros(B, dtype=torch.int32) for _ in range(3))
    for r, name in enumerate(names):
        a = ref[name]
        m = a["n_out"]
        n[r], removed[r], frags[r] = m, a["atoms_removed"], a["n_fragments"]
        x[r, :m] = torch.arange(3 * m, dtype=torch.float32).reshape(m, 3)
        el[r, :m] = torch.tensor(a["atomic_numbers"], dtype=torch.int8)
        bond[r, :m, :m] = torch.tensor(a["bond_orders"], dtype=torch.int8).reshape(m, m)
        kek[r, :m, :m] = torch.tensor(a["kekule_orders"], dtype=torch.int8).reshape(m, m)
        amap[r, :m] = torch.tensor(a["atom_map"], dtype=torch.int32)
    hyd = {}
    if hydrogen_parents is not None:
        H = max(len(p) for p in hydrogen_parents)
        parents = torch.full((B, H), -1, dtype=torch.int32)
        for r, p in enumerate(hydrogen_parents):
            parents[r, :len(p)] = torch.tensor(p, dtype=torch.int32)
        hyd = dict(hydrogen_coords=torch.ones(B, H, 3), hydrogen_parents=parents,
                   hydrogens_unplaced=torch.zeros(B, dtype=torch.int32))
    valid = torch.tensor([ref[k]["status"] == 0 for k in names])
    return molecules_from_tensors(x, el, bond, n, valid, atoms_removed=removed, n_fragments=frags, atom_map=amap,
                                  kekule_bond_orders=kek, **hyd)


def _bond_lines(block):
    lines = block.split("\n")
    n_atoms, n_bonds = int(lines[3][:3]), int(lines[3][3:6])
    return [(int(ln[:3]), int(ln[3:6]), int(ln[6:9])) for ln in lines[4 + n_atoms: 4 + n_atoms + n_bonds]]


def test_record_fields_and_molblock():
    from ml_conformer_generator_amd.handoff import GeneratedMolecule, molecules_from_tensors
    ref = C.references()
    pyridine, water, dead = _records(["pyridine", "benzene and water", "cyclopentadienyl"])
    assert water.atoms_removed == 1 and water.n_fragments == 2 and water.atom_map == list(range(6))
    assert pyridine.atoms_removed == 0 and pyridine.n_fragments == 1
    assert pyridine.kekule_bond_orders.dtype == torch.int8 and tuple(pyridine.kekule_bond_orders.shape) == (6, 6)
    assert pyridine.kekule_bond_orders.tolist() == ref["pyridine"]["kekule_orders"]
    plain = _bond_lines(pyridine.to_molblock())
    assert sorted(o for _, _, o in plain) == [4] * 6                              # the default output: the aromatic codes
    kek = _bond_lines(pyridine.to_molblock(kekulize=True))
    assert [(i, j) for i, j, _ in kek] == [(i, j) for i, j, _ in plain]
    assert sorted(o for _, _, o in kek) == [1, 1, 1, 2, 2, 2]
    assert {(j - 1, i - 1) for i, j, o in kek if o == 2} == {(0, 1), (2, 3), (4, 5)}
    with pytest.raises(ValueError, match="no Kekule form"):
        dead.to_molblock(kekulize=True)               # all zero: the standardisation found it invalid
    by_hand = GeneratedMolecule([6, 6], torch.zeros(2, 3), torch.tensor([[0, 1], [1, 0]], dtype=torch.int8))
    assert by_hand.atoms_removed is None and by_hand.n_fragments is None and by_hand.atom_map is None \
        and by_hand.kekule_bond_orders is None
    with pytest.raises(ValueError, match="standardize=True"):
        by_hand.to_molblock(kekulize=True)
    unset = molecules_from_tensors(torch.zeros(1, 2, 3), torch.full((1, 2), 6, dtype=torch.int8),
                                   torch.zeros(1, 2, 2, dtype=torch.int8), torch.tensor([2]), torch.tensor([True]))[0]
    assert unset.atoms_removed is None and unset.kekule_bond_orders is None
    assert _bond_lines(unset.to_molblock()) == [] and _bond_lines(by_hand.to_molblock()) == [(2, 1, 1)]


def test_molblock_with_hydrogens_names_the_atom_that_disagrees():
    # pyridine: every carbon has Kekule valence 3 and room for one hydrogen, N0 has valence 3 and room for none
    good, bad = _records(["pyridine", "pyridine"], hydrogen_parents=[[1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]])
    block = good.to_molblock(kekulize=True, hydrogens=True)
    assert block.count(" H  ") == 5 and sorted(o for _, _, o in _bond_lines(block)) == [1] * 8 + [2] * 3
    with pytest.raises(ValueError, match=r"atom 0 \(N\)"):
        bad.to_molblock(kekulize=True, hydrogens=True)
    assert bad.to_molblock(hydrogens=True).count(" H  ") == 6                     # the aromatic writer does not judge
    no_h = _records(["pyridine"])[0]
    with pytest.raises(ValueError, match="add_hydrogens"):
        no_h.to_molblock(kekulize=True, hydrogens=True)
