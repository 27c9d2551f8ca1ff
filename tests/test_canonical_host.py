"""Canonical graphs and SMILES, host side (no GPU): the restatement of the definition against brute-force isomorphism and
its named cases, the mutation checks, the SMILES writer through the test-side reader, the options of the generation
entries against stub seams backed by the restatement, and the C entry's argument checks."""
import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import canonical_cases as C
import canonical_ref as R
from ml_conformer_generator_amd import canonical as CN
from ml_conformer_generator_amd import fingerprint as FP
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import smiles as S
from ml_conformer_generator_amd.handoff import GeneratedMolecule, measured_from_tensors, molecules_from_tensors
from test_fingerprint_host import _as_mol, _MolStage, _seam_fingerprints
from test_shape_overlay_host import _no_device, _ref, _shell_generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def canonical_string(mol):
    out = R.canonical(*mol)
    z, adj, _ = R.permute(*mol, out["order"])
    return S.write_smiles(z, torch.tensor(adj, dtype=torch.int8).reshape(mol[2], mol[2]))


# ----------------------------------------------------------------------------------------------- exact identity
def _brute_classes(n, patterns):
    """Every graph on n atoms with the Z sequences `patterns` and codes in {0, 1, 2}, grouped by brute force: the smallest
    encoding over all n! renumberings.  Yields (class, z, the members of one isomorphism class restricted to z as
    indices, index -> adjacency matrix)."""
    pairs = [(i, j) for i in range(n) for j in range(i)]
    where = {p: k for k, p in enumerate(pairs)}
    codes = np.array(list(itertools.product((0, 1, 2), repeat=len(pairs))), dtype=np.int64).reshape(3 ** len(pairs), len(pairs))
    weights = 3 ** np.arange(len(pairs), dtype=np.int64)
    for z in patterns:
        best = None
        for p in itertools.permutations(range(n)):
            zval = sum((z[p[i]] == 7) << i for i in range(n))
            idx = [where[(max(p[i], p[j]), min(p[i], p[j]))] for i, j in pairs]
            val = zval * 3 ** len(pairs) + codes[:, idx] @ weights
            best = val if best is None else np.minimum(best, val)
        groups = {}
        for g, v in enumerate(best.tolist()):
            groups.setdefault(v, []).append(g)
        def adjacency(g):
            adj = [[0] * n for _ in range(n)]
            for (i, j), c in zip(pairs, codes[g].tolist()):
                adj[i][j] = adj[j][i] = c
            return adj
        for v, members in groups.items():
            yield (tuple(sorted(z)), v), list(z), members, adjacency


def _check_every_graph(n, patterns):
    """Every labelled graph on n atoms with the Z sequences `patterns` goes through the restatement: within a brute-force
    class all identity bytes are equal, and different classes have different ones.  Returns the number of classes."""
    by_class = {}
    for cls, z, members, adjacency in _brute_classes(n, patterns):
        got = {R.identity_bytes(z, adjacency(g), n) for g in members}
        assert len(got) == 1 and None not in got, (z, adjacency(members[0]))
        by_class.setdefault(cls, set()).update(got)
    assert all(len(v) == 1 for v in by_class.values())                       # isomorphic -> equal
    every = [next(iter(v)) for v in by_class.values()]
    assert len(set(every)) == len(every)                                     # equal -> isomorphic
    return len(every)


def test_identity_equals_isomorphism_on_every_graph_up_to_4_atoms():
    """Every graph on at most 4 atoms with Z in {6, 7} and codes in {0, 1, 2} - every Z sequence, every code pattern:
    equal identity bytes if and only if isomorphic, isomorphism by brute force over all renumberings (which finds 2, 9, 56
    and 705 classes)."""
    assert [_check_every_graph(n, list(itertools.product((6, 7), repeat=n))) for n in range(1, 5)] == [2, 9, 56, 705]


@pytest.mark.parametrize("nitrogens", range(6))
def test_identity_equals_isomorphism_on_every_graph_of_5_atoms(nitrogens):
    """The same over every graph on 5 atoms: one case per number of N atoms, holding every arrangement of that Z multiset
    (1, 5, 10, 10, 5, 1 sequences) times all 59 049 code patterns - 1.9 million labelled graphs over the six cases, each
    through the restatement (about 80 s of CPU in all).  Graphs of different cases differ in their Z bytes."""
    patterns = sorted(set(itertools.permutations([7] * nitrogens + [6] * (5 - nitrogens))))
    assert len(patterns) == [1, 5, 10, 10, 5, 1][nitrogens]
    assert _check_every_graph(5, patterns) > 500


def _sample_graph(rng, n):
    z = [rng.choice((6, 7)) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a):
            adj[a][b] = adj[b][a] = rng.choice((0, 0, 1, 1, 2))
    return z, adj, n


def test_identity_equals_isomorphism_on_a_sample_of_6_and_7_atoms():
    rng = random.Random(7)
    for n in (6, 7):
        graphs = []
        for _ in range(12):
            g = _sample_graph(rng, n)
            h = [row[:] for row in g[1]]
            a, b = rng.sample(range(n), 2)
            h[a][b] = h[b][a] = (h[a][b] + 1) % 3                               # one code changed: usually another graph
            graphs += [g, C.renumbered(rng, g), C.renumbered(rng, (g[0], h, n))]
        ids = [R.identity_bytes(*g) for g in graphs]
        for i, j in itertools.combinations(range(len(graphs)), 2):
            if sorted(graphs[i][0]) == sorted(graphs[j][0]) and i // 3 == j // 3:    # brute force within a family
                assert (ids[i] == ids[j]) == R.isomorphic(graphs[i], graphs[j]), (graphs[i], graphs[j])
        assert all(ids[3 * k] == ids[3 * k + 1] for k in range(12))
        assert len({ids[3 * k] for k in range(12)}) == 12                       # twelve random graphs, twelve identities


# ----------------------------------------------------------------------------------------------- named cases
@pytest.mark.parametrize("name", sorted(C.NAMED))
def test_named_case_under_renumbering(name):
    mol, leaves, string = C.NAMED[name]
    rng = random.Random(sum(map(ord, name)))
    first = R.canonical(*mol)
    assert first["status"] == 0 and first["leaves"] == leaves
    text = canonical_string(mol)
    assert string is None or text == string
    back = R.read_smiles(text)
    assert R.identity_bytes(*back[:3]) == R.identity_bytes(*mol)
    key = R.key(*mol, first["order"])
    for _ in range(8):
        other = C.renumbered(rng, mol)
        out = R.canonical(*other)
        assert (out["status"], out["leaves"], out["certificate"]) == (0, leaves, first["certificate"])
        assert canonical_string(other) == text and R.key(*other, out["order"]) == key


def test_cube_and_wagner_graph_differ_where_the_graph_key_does_not():
    import fingerprint_ref
    assert fingerprint_ref.key(*C.CUBE) == fingerprint_ref.key(*C.WAGNER) == 0xb8f57617ecefa100
    cube, wagner = R.canonical(*C.CUBE), R.canonical(*C.WAGNER)
    assert cube["certificate"] != wagner["certificate"] and R.identity_bytes(*C.CUBE) != R.identity_bytes(*C.WAGNER)
    assert R.key(*C.CUBE, cube["order"]) != R.key(*C.WAGNER, wagner["order"])


def test_budget_and_refusals_of_the_restatement():
    """Seven disjoint propanes have 7! = 5 040 leaves: BUDGET, under 8 seeded renumberings like the other named cases."""
    rng = random.Random(3)
    for mol in [C.OVER_BUDGET] + [C.renumbered(rng, C.OVER_BUDGET) for _ in range(8)]:
        out = R.canonical(*mol)
        assert (out["status"], out["leaves"], out["order"]) == (R.BUDGET, R.LEAF_BUDGET, [])
    assert R.identity_bytes(*R.mol([6] * 9, [])[:2], 9, ) is not None and R.identity_bytes([6] * 9, [[1] * 9] * 9, 0) is None
    assert R.canonical(*C.EDGES["no atoms"])["status"] == R.EMPTY
    assert R.canonical(*C.over_degree(rng))["status"] == R.DEGREE
    assert [R.canonical(*C.EDGES[k])["leaves"] for k in ("one atom", "two atoms", "64-atom chain", "64 isolated atoms")] \
        == [1, 1, 2, 1]
    assert (R.MAX_DEGREE, R.LEAF_BUDGET, R.EMPTY, R.DEGREE, R.BUDGET) == \
        (CN.MAX_DEGREE, CN.LEAF_BUDGET, CN.STATUS_EMPTY, CN.STATUS_DEGREE, CN.STATUS_BUDGET)
    assert CN.describe_status(0) == "ok" and CN.describe_status(4) == "BUDGET" and CN.describe_status(3) == "EMPTY|DEGREE"
    assert CN.MAX_ATOMS == 64 and CN.MAX_BATCH == 16384 and set(CN.STATUS_NAMES.values()) == {"EMPTY", "DEGREE", "BUDGET"}


def test_mutations_of_the_definition():
    """The twin rule prunes and changes no certificate; the bond code in the refinement key matters - named pair:
    1,3,5-cyclohexatriene against benzene."""
    for name, more in (("neopentane", 24), ("16 isolated C", None)):
        mol = C.NAMED[name][0]
        if more is None:                                  # 16! leaves without the rule: cut off, still more than one
            mol, more = R.mol([6] * 6, []), 720
        with_rule, without = R.canonical(*mol), R.canonical(*mol, twins=False)
        assert with_rule["leaves"] == 1 and without["leaves"] == more
        assert with_rule["certificate"] == without["certificate"]
    sixteen = R.canonical(*C.NAMED["16 isolated C"][0], twins=False, budget=50)
    assert sixteen["status"] == R.BUDGET and sixteen["leaves"] == 50          # more leaves than the one with the rule
    triene, benzene = R.canonical(*C.CYCLOHEXATRIENE), R.canonical(*C.BENZENE)
    assert (triene["leaves"], benzene["leaves"]) == (6, 12)
    blind = R.canonical(*C.CYCLOHEXATRIENE, codes=False)
    assert blind["leaves"] == 12 and blind["certificate"] == triene["certificate"]
    assert R.canonical(*C.BENZENE, codes=False)["leaves"] == 12


# ----------------------------------------------------------------------------------------------- the writer
def test_writer_pins():
    assert canonical_string(C.PYRROLE) == "c1cc[nH]c1"
    assert canonical_string(C.METHYLSILANE) == "C[SiH3]"
    assert S.write_smiles([], torch.zeros(0, 0, dtype=torch.int8)) == ""
    assert S.write_smiles([6, 8], [[0, 2], [2, 0]]) == "C=O" and S.write_smiles([6, 7], [[0, 3], [3, 0]]) == "C#N"
    assert S.write_smiles([6, 6, 8], [[0, 4, 0], [4, 0, 1], [0, 1, 0]]) == "ccO"
    assert S.write_smiles([6, 9], [[0, 4], [4, 0]]) == "c:F"                    # code 4 to an atom that stays uppercase
    assert S.write_smiles([34, 6], [[0, 4], [4, 0]]) == "[se]c" and S.write_smiles([34, 6], [[0, 1], [1, 0]]) == "[SeH]C"
    assert S.write_smiles([14], [[0]]) == "[SiH4]" and S.write_smiles([6, 6], [[0, 0], [0, 0]]) == "C.C"
    for bad in (([6, 6], [[0, 5], [5, 0]]), ([6, 6], [[0, 1], [2, 0]]), ([6, 0], [[0, 1], [1, 0]]), ([6, 6], [[0, 1.0], [1.0, 0]]),
                ([6, 99], [[0, 1], [1, 0]]), ([6, 6, 6], [[0, 1], [1, 0]])):
        with pytest.raises(ValueError):
            S.write_smiles(*bad)


def test_imidazole_string_does_not_follow_the_input_numbering():
    from ml_conformer_generator_amd.hydrogens import implicit_counts
    rng = random.Random(11)
    mol = C.IMIDAZOLE_4_METHYL
    strings, carriers = set(), set()
    for _ in range(12):
        z, adj, n = C.renumbered(rng, mol)
        strings.add(canonical_string((z, adj, n)))
        nh = implicit_counts(torch.tensor([z]), torch.tensor([adj], dtype=torch.int8), torch.tensor([n]))[0].tolist()
        (a,) = [k for k in range(n) if z[k] == 7 and nh[k] == 1]
        carriers.add(sum(1 for j in range(n) if adj[a][j] and sum(1 for k in range(n) if adj[j][k]) == 3))
    assert strings == {"Cc1c[nH]cn1"}
    assert carriers == {0, 1}          # on the graph as numbered the hydrogen sits on either N: next to the methyl's C or not


def test_round_trip_through_the_reader():
    rng = random.Random(5)
    mols = [m for m, _, _ in C.NAMED.values()] + [C.PYRROLE, C.IMIDAZOLE_4_METHYL, C.METHYLSILANE, C.CYCLOHEXATRIENE]
    mols += [g for g in C.fuzz_set(96) if R.canonical(*g)["status"] == 0]
    z, adj, n = R.mol([6, 6, 34, 6, 6, 17, 35, 15, 5, 16], [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 4, 4), (4, 0, 4), (0, 5, 1),
                                                           (1, 6, 1), (3, 7, 1), (7, 8, 2), (4, 9, 1)])
    mols.append((z, adj, n))
    for mol in mols:
        for text in (canonical_string(mol), S.write_smiles(mol[0], mol[1])):       # canonical, and the order as given
            back = R.read_smiles(text)
            assert R.identity_bytes(*back[:3]) == R.identity_bytes(*mol), text
        assert canonical_string(C.renumbered(rng, mol)) == canonical_string(mol)


def test_closure_numbers():
    assert canonical_string(C.NAMED["K5"][0]) == "C123C45C11C24C351"             # 1 is free again at the third atom
    z, adj, n = C.nested_rings(26)
    text = S.write_smiles(z, adj)
    assert text == "C1C2C3C4C5C6C7C8C9C%10C%11C%12CCC%12C%11C%10C9C8C7C6C5C4C3C2C1"
    assert R.identity_bytes(*R.read_smiles(text)[:3]) == R.identity_bytes(z, adj, n)
    z, adj, n = C.nested_rings(200)                                             # 99 closures open at once: the last number
    text = S.write_smiles(z, adj)
    assert "%99" in text and R.read_smiles(text)[1] == adj
    z, adj, n = C.nested_rings(202)                                             # 100
    with pytest.raises(ValueError, match="99"):
        S.write_smiles(z, adj)


# ----------------------------------------------------------------------------------------------- options
_SCORES = [0.3, 0.9, 0.5, 0.8, 0.2, 0.6, 0.4, 0.7]


def _shard_molecules():
    """sample id -> molecule: 3 repeats the cube 0, 7 the Wagner graph 1 (renumbered); 4 and 5 are one graph over budget."""
    rng = random.Random(8)
    return [C.CUBE, C.WAGNER, C.BENZENE, C.renumbered(rng, C.CUBE), C.OVER_BUDGET, C.renumbered(rng, C.OVER_BUDGET),
            C.NAMED["K5"][0], C.renumbered(rng, C.WAGNER)]


_BUDGET_ROWS = {}      # the restatement's verdict on the over-budget rows, computed once (a second each)


def _seam_canonical(calls):
    """`_canonical_order` by the restatement, on the host."""
    def run(z, bonds, n):
        z, bonds, n = torch.as_tensor(z), torch.as_tensor(bonds), torch.as_tensor(n).reshape(-1).tolist()
        calls.append(len(n))
        W = int(bonds.shape[1])
        order = torch.full((len(n), W), -1, dtype=torch.int32)
        status, leaves, keys = [], [], []
        for b, k in enumerate(n):
            zs, adj = z[b, :k].tolist(), bonds[b, :k, :k].tolist()
            memo = (tuple(zs), tuple(map(tuple, adj)))
            if k == 21 and memo not in _BUDGET_ROWS:
                _BUDGET_ROWS[memo] = R.canonical(zs, adj, k)
            out = _BUDGET_ROWS[memo] if k == 21 else R.canonical(zs, adj, k)
            status.append(out["status"])
            leaves.append(out["leaves"])
            keys.append(R.key(zs, adj, k, out["order"]) if out["status"] == 0 else 0)
            if out["status"] == 0:
                order[b, :k] = torch.tensor(out["order"], dtype=torch.int32)
        return dict(order=order, status=torch.tensor(status, dtype=torch.int32), leaves=torch.tensor(leaves, dtype=torch.int32),
                    key=torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64)))
    return run


def _graph_shard(mols):
    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
        el = torch.full((n_samples, 42), 9, dtype=torch.int8)                     # junk beyond the atoms
        bond = torch.full((n_samples, 42, 42), 3, dtype=torch.int8)
        x = torch.zeros(n_samples, 42, 3)
        n = torch.zeros(n_samples, dtype=torch.int32)
        for b, sid in enumerate(ids):
            z, adj, k = mols[sid]
            el[b, :k] = torch.tensor(z, dtype=torch.int8)
            bond[b, :k, :k] = torch.tensor(adj, dtype=torch.int8)
            n[b] = k
            x[b, :k, 0] = torch.arange(k) * 1.5
            x[b, 0, 1] = _SCORES[sid]                                             # the stub shape score
        return dict(x=x, elements=el, bond=bond, n_nodes=n, valid=torch.ones(n_samples, dtype=torch.uint8))
    return run


def _generator(calls, finisher=None):
    gen = _shell_generator(finisher=finisher)
    gen._canonical_order = _seam_canonical(calls)
    gen._graph_fingerprints = _seam_fingerprints([])
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    return gen


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_canonical_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._canonical_order = gen._graph_fingerprints = gen._chem_tanimoto = gen._chem_pair = gen._score = _no_device
    call = getattr(gen, entry)
    big = ([6] * 65, [[0] * 65] * 65)
    cases = [dict(unique=1), dict(unique="yes"), dict(unique=None), dict(unique=0.0), dict(unique="Exact"),
             dict(unique="exactly"), dict(unique=b"exact"),
             dict(smiles=1), dict(smiles="yes"), dict(smiles=None), dict(smiles=0.0),
             dict(exclude_graphs=3.5), dict(exclude_graphs="CCO"), dict(exclude_graphs=[3.5]),
             dict(exclude_graphs=[C.CUBE[:2], ([6, 6], [[0, 1], [2, 0]])]), dict(exclude_graphs=[C.CUBE[:2], big]),
             dict(exclude_graphs=[C.CUBE[:2]], unique="exactly"), dict(exclude_graphs=[C.CUBE[:2]], top_k=0)]
    for kw in cases:
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    with pytest.raises(ValueError, match=r"exclude_graphs\[1\]"):
        call(reference_conformer=_ref(), n_samples=4, exclude_graphs=[C.CUBE[:2], big])
    with pytest.raises(ValueError, match="unique must be True or False"):
        call(reference_conformer=_ref(), n_samples=4, unique="yes")
    gen.finisher = "rdkit"
    with pytest.raises(ValueError) as e:
        call(reference_conformer=_ref(), n_samples=4, smiles=True)
    assert str(e.value) == CN.REFUSAL_WITH_FINISHER
    gen.finisher = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                              "finish_tag_chunk")
    for kw in (dict(unique="exact"), dict(exclude_graphs=[C.CUBE[:2]]), dict(smiles=True)):
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, **kw)


def test_exclude_graphs_that_cannot_be_labelled_are_refused_before_the_generation():
    calls = []
    gen = _generator(calls)
    gen._generate_shard = _no_device
    kw = dict(reference_conformer=_ref(), n_samples=8)
    with pytest.raises(ValueError, match=r"exclude_graphs\[2\].*BUDGET"):
        gen.generate_conformers(exclude_graphs=[C.CUBE[:2], C.WAGNER[:2], C.OVER_BUDGET[:2]], **kw)
    with pytest.raises(ValueError, match=r"exclude_graphs\[0\].*EMPTY"):
        gen.generate_conformers(exclude_graphs=[([1], [[0]])], **kw)               # no heavy atom
    assert calls == [3, 1]
    # a refusal of the entry itself, behind parse_request, costs no launch: the graphs are labelled last
    with pytest.raises(ValueError):
        gen.generate_conformers(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_samples=8,
                                exclude_graphs=[C.CUBE[:2]])                       # no n_atoms
    with pytest.raises(ValueError):
        gen.generate_conformers_sharded(gather="some", exclude_graphs=[C.CUBE[:2]], **kw)
    assert calls == [3, 1]
    req = postprocess.parse_request(gen, None, exclude_graphs=[C.CUBE[:2]])
    assert calls == [3, 1] and req.exclude is None and len(req.excluded_graphs) == 1      # read, not labelled
    assert postprocess.label_excluded(gen, req).exclude == {(R.key(*C.CUBE, R.canonical(*C.CUBE)["order"]),
                                                             R.identity_bytes(*C.CUBE))} and calls == [3, 1, 1]
    assert postprocess.label_excluded(gen, postprocess.Request()) == postprocess.Request()


def test_proxy_path_exact_uniqueness_exclusion_and_strings():
    mols = _shard_molecules()
    calls = []
    gen = _generator(calls)
    gen._generate_shard = _graph_shard(mols)
    kw = dict(reference_conformer=_ref(), n_samples=8)

    plain = gen.generate_conformers(**kw)
    assert calls == [] and [m.sample_id for m in plain] == list(range(8))         # no option: the seam is not touched
    assert all(m.smiles is None and m.canonical_order is None and m.canonical_status is None for m in plain)

    def ids(**more):
        return [m.sample_id for m in gen.generate_conformers(**dict(kw, **more))]
    # the graph key cannot tell the cube from the Wagner graph; the exact identity can.  Rows over budget always stay.
    assert ids(unique=True) == [0, 2, 4, 6]
    assert calls == []
    assert ids(unique="exact") == [0, 1, 2, 4, 5, 6] and calls == [8]
    assert ids(unique="exact", shape_scores=True) == [1, 2, 3, 4, 5, 6]            # the better-ranked copy: 3 (0.8), 1 (0.9)
    assert ids(unique="exact", top_k=3) == [1, 3, 5]
    del calls[:]
    cube_record = GeneratedMolecule(C.CUBE[0], torch.zeros(8, 3), torch.tensor(C.CUBE[1], dtype=torch.int8))
    for cube in (C.CUBE[:2], cube_record, _as_mol(C.CUBE, hydrogens=2), C.renumbered(random.Random(1), C.CUBE)[:2]):
        assert ids(exclude_graphs=[cube]) == [1, 2, 4, 5, 6, 7]
    assert calls == [1, 8] * 4                                                     # the excluded set first, then the rows
    assert ids(exclude_graphs=[C.CUBE[:2]], unique="exact") == [1, 2, 4, 5, 6]
    assert ids(exclude_graphs=iter([C.CUBE[:2], C.WAGNER[:2], C.NAMED["K5"][0][:2]]), unique="exact") == [2, 4, 5]
    assert ids(exclude_graphs=[]) == list(range(8))
    assert [m.sample_id for m in gen.generate_conformers_sharded(unique="exact", **kw)] == [0, 1, 2, 4, 5, 6]
    assert [m.sample_id for m in gen.forward(unique="exact", exclude_graphs=[C.WAGNER[:2]], **kw)] == [0, 2, 4, 5, 6]

    got = gen.generate_conformers(smiles=True, **kw)
    assert [m.sample_id for m in got] == list(range(8))
    assert isinstance(got[7]._measured.canonical_order, tuple)                    # sliced on first read
    for a, m in zip(plain, got):
        assert a == m
        ref = R.canonical(*mols[m.sample_id]) if m.sample_id not in (4, 5) else dict(status=R.BUDGET, order=None)
        assert m.canonical_status == ref["status"] and m.canonical_order == ref["order"]
    assert isinstance(got[7]._measured.canonical_order, list)
    assert got[0].smiles == got[3].smiles == "C12C3C4C1C1C2C3C41" == got[3].to_smiles()
    assert got[1].smiles == got[7].smiles == canonical_string(C.WAGNER) != got[0].smiles
    assert got[2].smiles == "c1ccccc1" and got[6].smiles == "C123C45C11C24C351"
    assert got[4].smiles is None and got[4].canonical_order is None and got[4].canonical_status == 4
    with pytest.raises(ValueError, match="BUDGET"):
        got[4].to_smiles()
    assert got[4].to_smiles(canonical=False) == "CCC.CCC.CCC.CCC.CCC.CCC.CCC"
    with pytest.raises(ValueError, match="smiles=True"):
        plain[0].to_smiles()
    assert R.identity_bytes(*R.read_smiles(plain[3].to_smiles(canonical=False))[:3]) == R.identity_bytes(*C.CUBE)
    both = gen.generate_conformers(smiles=True, unique="exact", **kw)
    assert [m.sample_id for m in both] == [0, 1, 2, 4, 5, 6] and both[1].smiles == got[1].smiles


def test_object_path_exact_uniqueness_reads_the_mols_own_graphs():
    mols = _shard_molecules()
    calls = []
    gen = _generator(calls, finisher="rdkit")
    gen._generate_shard = _MolStage(gen, mols)                                   # sample 2 is dropped by the finish
    kw = dict(reference_conformer=_ref(), n_samples=8, sample_seed=5)

    def ids(**more):
        return [m.props["sample_id"] for m in gen.generate_conformers(**dict(kw, **more))]
    assert ids() == [0, 1, 3, 4, 5, 6, 7] and calls == []
    assert ids(unique=True) == [0, 4, 6]
    assert ids(unique="exact") == [0, 1, 4, 5, 6] and calls == [7]               # the live Mols in ONE batched call
    assert ids(unique="exact", exclude_graphs=[C.CUBE[:2]]) == [1, 4, 5, 6]


def test_select_exact_and_lazy_record_fields():
    a, b = (5, b"x"), (5, b"y")                                                   # one key, two identities: both stay
    assert postprocess.select_exact([a, b, a, None, None, b], [0, 1, 2, 3, 4, 5]) == [0, 1, 3, 4]
    assert postprocess.select_exact([a, b, a, None, None, b], [5, 4, 3, 2, 1, 0]) == [2, 3, 4, 5]
    assert postprocess.select_exact([], []) == []
    order = torch.tensor([[2, 0, 1, -1], [-1, -1, -1, -1], [0, 1, -1, -1]], dtype=torch.int32)
    status = torch.tensor([0, 2, 0], dtype=torch.int32)
    recs = measured_from_tensors(dict(canonical_order=order, canonical_status=status), 3)
    assert [r.canonical_status for r in recs] == [0, 2, 0]
    assert recs[0].canonical_order[1:] == (0, 3) and recs[2].canonical_order[1:] == (2, 2)      # (batch, row, n): unsliced
    z = torch.tensor([[6, 6, 8, 0], [6, 0, 0, 0], [6, 7, 0, 0]])
    bonds = torch.zeros(3, 4, 4, dtype=torch.int8)
    bonds[0, 0, 1] = bonds[0, 1, 0] = bonds[0, 1, 2] = bonds[0, 2, 1] = 1         # C-C-O, canonical order O? no: 2, 0, 1
    bonds[2, 0, 1] = bonds[2, 1, 0] = 3
    mols = molecules_from_tensors(torch.zeros(3, 4, 3), z, bonds, torch.tensor([3, 1, 2]), torch.ones(3),
                                  canonical_order=order, canonical_status=status)
    assert mols[0].canonical_order == [2, 0, 1] and mols[0].smiles == "OCC" and mols[0]._smiles == "OCC"
    assert mols[1].canonical_order is None and mols[1].smiles is None and mols[1].to_smiles(canonical=False) == "C"
    assert mols[2].smiles == "C#N"
    with pytest.raises(ValueError, match="DEGREE"):
        mols[1].to_smiles()


def test_identity_bytes_and_relabel_on_the_host():
    mols = [C.CUBE, C.WAGNER, C.renumbered(random.Random(2), C.CUBE), C.EDGES["no atoms"], C.PYRROLE]
    z, bonds, n = C.pad_batch(mols, 9, junk=random.Random(4))
    ordered = _seam_canonical([])(z, bonds, n)
    got = CN.identity_bytes(z, bonds, n, ordered=ordered)
    assert got == [R.identity_bytes(*m) for m in mols] and got[0] == got[2] != got[1] and got[3] is None
    zc, bc = CN.canonical_graphs(z, bonds, n, ordered=ordered)
    assert torch.equal(zc[0], zc[2]) and torch.equal(bc[0], bc[2]) and not torch.equal(bc[0], bc[1])
    assert int(zc[3].abs().sum()) == 0 and int(bc[3].abs().sum()) == 0 and zc.dtype == torch.int32 and bc.dtype == torch.int8
    back = R.permute(*C.PYRROLE, ordered["order"][4, :5].tolist())
    assert zc[4, :5].tolist() == back[0] and bc[4, :5, :5].tolist() == back[1] and int(bc[4, 5:].abs().sum()) == 0


# ----------------------------------------------------------------------------------------------- C ABI
def test_canonical_entry_refuses_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check

    def order(z=p, bonds=p, n=p, B=3, W=42, out=p, status=p, leaves=p, key=p):
        return h.mcg_canonical_order(z, bonds, n, B, W, out, status, leaves, key, None)

    for bad in (dict(z=None), dict(bonds=None), dict(n=None), dict(out=None), dict(status=None), dict(leaves=None),
                dict(key=None), dict(B=-1), dict(B=16385), dict(W=0), dict(W=65), dict(W=-3)):
        assert order(**bad) == 1, bad
        assert b"mcg_canonical_order" in h.mcg_last_error(), bad
    assert order(B=0) == 0                        # nothing to do, nothing launched
    assert h.mcg_abi_version() == 4 and "mcg_canonical_order" in _lib.SIGNATURES
    with pytest.raises(ValueError):
        CN.canonical_order(torch.zeros(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8), torch.tensor([3]))
    with pytest.raises(ValueError):
        CN.canonical_order(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8), torch.tensor([3, 6]))
    with pytest.raises(ValueError):
        CN.canonical_order(torch.zeros(2, 5), torch.zeros(2, 5, 5, dtype=torch.int8), torch.tensor([3, 2]))


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_canonical`: the entry's argument checks in a stand-alone program under host-side ASan + UBSan, on the CPU."""
    exe = str(tmp_path / "canonical_arg_check")
    csrc = os.path.join(ROOT, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_canonical", f"CANONICAL_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 wrong" in ran.stdout, ran.stdout + ran.stderr
