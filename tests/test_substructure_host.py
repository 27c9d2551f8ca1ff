"""Host-side tests of the substructure patterns: the restatement (`substructure_ref`) against brute force over every
injective map, the named table under renumbering, the budget pair, mutation checks, the parser and the compiler, the
catalogue, the options against stub seams and the C entry's argument checks.  No GPU."""
import ctypes
import itertools
import os
import random
import subprocess
import warnings

import pytest
import torch

import canonical_cases as C
import canonical_ref as CR
import substructure_cases as SC
import substructure_ref as R
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import substructure as S
from ml_conformer_generator_amd.handoff import Measured, measured_from_tensors, molecules_from_tensors
from test_canonical_host import _graph_shard
from test_fingerprint_host import _MolStage, _seam_fingerprints
from test_shape_overlay_host import _no_device, _ref, _shell_generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- the definition
def _ring_bonds_by_union(adj, n):
    """{(i, j)} of the ring bonds, another way than the restatement's: a bond is a chain bond iff the components of the
    graph without it - by union-find - separate its ends."""
    edges = [(i, j) for i in range(n) for j in range(i) if adj[i][j]]
    rings = set()
    for gone in edges:
        root = list(range(n))

        def find(a):
            while root[a] != a:
                a = root[a]
            return a
        for e in edges:
            if e != gone:
                root[find(e[0])] = find(e[1])
        if find(gone[0]) == find(gone[1]):
            rings |= {gone, gone[::-1]}
    return rings


def _brute(mol, pattern, nh):
    """count, covered and the smallest embedding in matching order, over EVERY injective map of the pattern's atoms."""
    z, adj, n = mol
    rings = _ring_bonds_by_union(adj, n)
    deg = [sum(1 for c in row if c) for row in adj]
    if nh is None:
        nh = [max(0, (2 * R.V0.get(z[a], 0) - sum(R.V2[c] for c in adj[a])) // 2) for a in range(n)]

    def atom_ok(q, a):
        ring, arom = any((a, j) in rings for j in range(n)), 4 in adj[a]
        return (q.elements is None or z[a] in q.elements) and q.dmin <= deg[a] <= q.dmax and q.hmin <= nh[a] <= q.hmax \
            and (q.ring is None or q.ring == ring) and (q.aromatic is None or q.aromatic == arom)

    order = S.matching_order(len(pattern.atoms), [(q.a, q.b) for q in pattern.bonds])
    count, covered, best = 0, set(), None
    for image in itertools.permutations(range(n), len(pattern.atoms)):
        if all(atom_ok(q, a) for q, a in zip(pattern.atoms, image)) and all(
                adj[image[q.a]][image[q.b]] in q.codes and (q.ring is None or q.ring == ((image[q.a], image[q.b]) in rings))
                for q in pattern.bonds):
            count += 1
            covered |= set(image)
            key = [image[a] for a in order]
            if best is None or key < best[0]:
                best = (key, list(image))
    return count, covered, None if best is None else best[1]


def _small_graph(rng, n):
    z = [rng.choice([6, 6, 7, 8]) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i):
            if rng.random() < 0.35:
                adj[i][j] = adj[j][i] = rng.choice([1, 1, 2, 4])
    return z, adj, n


def test_restatement_equals_brute_force_over_every_injective_map():
    rng = random.Random(20261019)
    found = disconnected = constrained = 0
    for trial in range(240):
        mol = _small_graph(rng, rng.randint(1, 7))
        nh = None if trial % 3 == 0 else [rng.randint(0, 3) for _ in range(mol[2])]
        for _ in range(4):
            pattern = SC.random_pattern(rng, rng.randint(1, 4))
            got = SC.reference(mol, pattern, nh=nh)
            count, covered, first = _brute(mol, pattern, nh)
            assert (got["count"], got["covered"], got["first"], got["status"]) == (count, covered, first, 0), (mol, pattern)
            found += count > 0
            disconnected += len(set(SC.to_ref(pattern)[2])) > 1 + len(pattern.bonds)
            constrained += pattern.needs_hydrogens
    assert found > 150 and disconnected > 50 and constrained > 100


@pytest.mark.parametrize("row", range(len(SC.TABLE)))
def test_named_table_under_renumbering(row):
    text, name, count, cov = SC.TABLE[row]
    mol = SC.molecule(name)
    out = SC.reference(mol, text)
    assert (out["count"], out["status"], len(out["covered"])) == (count, 0, cov)
    assert out["first"] is None if count == 0 else SC.is_embedding(mol, text, out["first"])
    assert max(out["nodes"] or [0]) <= R.NODE_BUDGET
    rng = random.Random(row)
    for _ in range(8):
        again = SC.reference(C.renumbered(rng, mol), text)
        assert (again["count"], again["status"], len(again["covered"])) == (count, 0, cov)
        assert sorted(again["nodes"]) == sorted(out["nodes"])    # a root's tree is a function of the graph alone


def test_one_pattern_tells_cubane_from_the_wagner_graph():
    import fingerprint_ref as FR
    assert FR.fingerprint_and_key(*C.CUBE) == FR.fingerprint_and_key(*C.WAGNER)      # one key, one fingerprint
    assert SC.reference(C.CUBE, SC.ANY5)["count"] == 0 and SC.reference(C.WAGNER, SC.ANY5)["count"] == 80


def test_budget_pair():
    fits = SC.reference(SC.K12, SC.PATH6)
    assert fits["status"] == 0 and fits["count"] == SC.K12_PATH6_COUNT and set(fits["nodes"]) == {SC.K12_PATH6_NODES}
    over = SC.reference(SC.K12, SC.PATH7)
    assert over["status"] == R.BUDGET and set(over["nodes"]) == {R.NODE_BUDGET} and over["count"] == SC.K12_PATH7_COUNT
    assert over["first"] == list(range(7)) and len(over["covered"]) == 12
    small = SC.reference(C.NAMED["K5"][0], SC.path_smarts(5), budget=100)            # the budget is per root
    assert small["status"] == 0 and small["nodes"] == [65] * 5 and small["count"] == 120
    assert SC.reference(C.NAMED["K5"][0], SC.path_smarts(5), budget=64)["status"] == R.BUDGET


def test_mutations_of_the_definition():
    toluene, decalin = C.NAMED["toluene"][0], C.NAMED["decalin"][0]
    assert SC.reference(toluene, "[#6]~!@[#6]")["count"] == 2
    assert SC.reference(toluene, "[#6]~!@[#6]", ring_test=False)["count"] == 14     # without the ring test
    assert SC.reference(SC.ETHANE, "CCC")["count"] == 0
    assert SC.reference(SC.ETHANE, "CCC", injective=False)["count"] == 2            # without injectivity
    assert SC.reference(decalin, SC.AROM6.replace("c", "[#6]"))["count"] == 0
    assert SC.reference(decalin, SC.AROM6.replace("c", "[#6]"), code_mask=False)["count"] == 24     # without the code mask


# ----------------------------------------------------------------------------------------------- parser and compiler
def test_every_accepted_construct_parses_to_the_pattern_built_by_hand():
    A, Bd, P = S.atom, S.bond, S.Pattern
    single_or_arom = (1, 4)
    cases = {
        "C": P((A(6, aromatic=False),)),
        "c": P((A(6, aromatic=True),)),
        "*": P((A(),)), "a": P((A(aromatic=True),)), "A": P((A(aromatic=False),)),
        "ClBr": P((A(17, aromatic=False), A(35, aromatic=False)), (Bd(0, 1, single_or_arom),)),
        "BNOFPSI": P(tuple(A(z, aromatic=False) for z in (5, 7, 8, 9, 15, 16, 53)),
                     tuple(Bd(i, i + 1, single_or_arom) for i in range(6))),
        "bnops": P(tuple(A(z, aromatic=True) for z in (5, 7, 8, 15, 16)), tuple(Bd(i, i + 1, single_or_arom) for i in range(4))),
        "[Si,Se,As]": P((A([14, 34, 33], aromatic=False),)),
        "[se,as]": P((A([34, 33], aromatic=True),)),
        "[#6,#7]": P((A([6, 7]),)),
        "[#53]": P((A(53),)),
        "[C,N;D2;H1;R]": P((A([6, 7], degree=2, hydrogens=1, ring=True, aromatic=False),)),
        "[nH]": P((A(7, hydrogens=1, aromatic=True),)),
        "[CH3]": P((A(6, hydrogens=3, aromatic=False),)),
        "[OD1&H0]": P((A(8, degree=1, hydrogens=0, aromatic=False),)),
        "[*R0]": P((A(ring=False),)), "[*;!R]": P((A(ring=False),)), "[a;R]": P((A(ring=True, aromatic=True),)),
        "C-C=C#C:C~C@C!@C": P(tuple(A(6, aromatic=False) for _ in range(8)),
                              (Bd(0, 1, 1), Bd(1, 2, 2), Bd(2, 3, 3), Bd(3, 4, 4), Bd(4, 5), Bd(5, 6, ring=True),
                               Bd(6, 7, ring=False))),
        "C-@C=!@C": P(tuple(A(6, aromatic=False) for _ in range(3)), (Bd(0, 1, 1, ring=True), Bd(1, 2, 2, ring=False))),
        "C(=O)(N)Cl": P((A(6, aromatic=False), A(8, aromatic=False), A(7, aromatic=False), A(17, aromatic=False)),
                        (Bd(0, 1, 2), Bd(0, 2, single_or_arom), Bd(0, 3, single_or_arom))),
        "C1OC1": P((A(6, aromatic=False), A(8, aromatic=False), A(6, aromatic=False)),
                   (Bd(0, 1, single_or_arom), Bd(1, 2, single_or_arom), Bd(0, 2, single_or_arom))),
        "C=1CC=1": P(tuple(A(6, aromatic=False) for _ in range(3)), (Bd(0, 1, single_or_arom), Bd(1, 2, single_or_arom), Bd(0, 2, 2))),
        "C%12CC%12.O": P((A(6, aromatic=False), A(6, aromatic=False), A(6, aromatic=False), A(8, aromatic=False)),
                         (Bd(0, 1, single_or_arom), Bd(1, 2, single_or_arom), Bd(0, 2, single_or_arom))),
        "C(C)(C).N": P((A(6, aromatic=False),) * 3 + (A(7, aromatic=False),), (Bd(0, 1, single_or_arom), Bd(0, 2, single_or_arom))),
    }
    for text, want in cases.items():
        got = S.parse(text)
        assert (got.atoms, got.bonds) == (want.atoms, want.bonds), text
        assert got.name == text and hash(got) == hash(S.parse(text)) and got == S.parse(text)
        assert "Pattern(" in repr(got)
    assert S.parse("C", name="methyl").name == "methyl"
    with pytest.raises(Exception):
        S.parse("C").atoms = ()                                                    # frozen


def test_every_refusal_names_its_position():
    cases = {"C[N+]": 3, "[O-]": 2, "C$(C)": 1, "C!=C": 1, "[!C]": 1, "[CX4]": 2, "[Cv4]": 2, "[13C]": 1, "[C@H]": 2,
             "[C@@]": 2, "[C:1]": 2, "[C,c]": 3, "[CR2]": 2, "[Cr5]": 2, "C/C": 1, "C1CC": 1, "C(C": 3, "C)": 1, "(C)": 0,
             "C..C": 2, ".C": 0, "C=": 1, "=C": 0, "C==C": 2, "C%1C": 1, "[C": 2, "[]": 1, "Q": 0, "[Xe]": 1, "[#54]": 1,
             "[#0]": 1, "C1C1": 3, "C11": 2, "[CD2D3]": 4, "[CH1H2]": 4, "[*,C]": 3, "": 0, "C=1CC#1": 6}
    for text, position in cases.items():
        with pytest.raises(ValueError, match=rf"position {position} \(") as e:
            S.parse(text)
        assert repr(text) in str(e.value), text
    for text in ("C[N+]", "[O-]", "[NH3+]"):
        with pytest.raises(ValueError, match="no charges in this package"):
            S.parse(text)
    with pytest.raises(ValueError, match="at most 32"):
        S.parse("C" * 33)
    assert len(S.parse("C" * 32).atoms) == 32
    with pytest.raises(ValueError):
        S.parse(None)
    for bad in (dict(elements=0), dict(elements=54), dict(elements=[]), dict(elements=True), dict(degree=-1),
                dict(degree=256), dict(hydrogens=(3, 1)), dict(ring=1), dict(aromatic="yes")):
        with pytest.raises(ValueError):
            S.atom(**bad)
    for bad in ((0, 0), (0, 1, 5), (0, 1, []), (-1, 2), (0, 1, 1, 1)):
        with pytest.raises(ValueError):
            S.bond(*bad)
    with pytest.raises(ValueError):
        S.Pattern((S.atom(),), (S.bond(0, 1),))                                    # a bond to an atom that is not there
    with pytest.raises(ValueError):
        S.Pattern((S.atom(), S.atom()), (S.bond(0, 1), S.bond(1, 0, 2)))           # two bonds on one pair
    with pytest.raises(ValueError):
        S.Pattern(())


def test_matching_order_rule_and_the_mapping_of_first():
    # breadth-first from the lowest atom of each component, neighbours ascending, components by their lowest atom
    assert S.matching_order(6, [(0, 5), (0, 2), (2, 1), (5, 4), (4, 3)]) == [0, 2, 5, 1, 4, 3]
    assert S.matching_order(5, [(3, 1), (4, 0)]) == [0, 4, 1, 3, 2]
    assert S.matching_order(3, []) == [0, 1, 2]
    ring = [(i, (i + 1) % 6) for i in range(6)]
    assert S.matching_order(6, ring) == [0, 1, 5, 2, 4, 3] == R.matching_order(6, set(ring))
    rng = random.Random(4)
    for _ in range(50):
        pat = SC.random_pattern(rng, rng.randint(1, 8))
        pairs = [(q.a, q.b) for q in pat.bonds]
        assert S.matching_order(len(pat.atoms), pairs) == R.matching_order(len(pat.atoms), set(pairs))
    # `first` comes back from the kernel in matching order and is returned in the caller's
    compiled = S.compile_patterns(["C(N)(=O)Cl", "O", "CC"])
    assert compiled.order[0] == (0, 1, 2, 3) and compiled.max_atoms == 4
    odd = S.compile_patterns([S.Pattern((S.atom(6), S.atom(7), S.atom(8)), (S.bond(0, 2), S.bond(2, 1)))])
    assert odd.order[0] == (0, 2, 1) and odd.inverse[0] == (0, 2, 1)
    raw = torch.full((1, 1, 32), -1, dtype=torch.int32)
    raw[0, 0, :3] = torch.tensor([10, 11, 12])                                     # positions: atoms 0, 2, 1
    assert S.first_in_caller_order(raw, odd).tolist() == [[[10, 12, 11]]]
    raw3 = torch.full((2, 3, 32), -1, dtype=torch.int32)
    raw3[1, 0, :4], raw3[1, 1, :1] = torch.tensor([5, 6, 7, 8]), torch.tensor([9])
    assert S.first_in_caller_order(raw3, compiled).tolist() == [[[-1] * 4] * 3, [[5, 6, 7, 8], [9, -1, -1, -1], [-1] * 4]]


def test_compile_patterns_round_trips_through_the_unpacker():
    rng = random.Random(6)
    patterns = list(SC.TABLE_PATTERNS) + [SC.random_pattern(rng, rng.randint(1, 9)) for _ in range(40)] + \
        list(S.CATALOGUE.values()) + [C.NAMED["naphthalene"][0][:2]]
    compiled = S.compile_patterns(patterns)
    assert compiled.pat_n.dtype == torch.int32 and tuple(compiled.pat_atoms.shape) == (len(patterns), 32, 2)
    assert compiled.pat_atoms.dtype == torch.int64 and compiled.pat_bonds.dtype == torch.uint8
    assert tuple(compiled.pat_bonds.shape) == (len(patterns), 32, 32)
    for p, pat in enumerate(compiled.patterns):
        atoms, bonds, order = SC.to_ref(pat)
        assert SC.unpack(compiled, p) == (atoms, bonds) and list(compiled.order[p]) == order
        assert [compiled.inverse[p][a] for a in order] == list(range(len(order)))
    assert compiled.needs_hydrogens and not S.compile_patterns(["CC", "c1ccccc1"]).needs_hydrogens
    assert S.compile_patterns(compiled) is compiled
    assert S.compile_patterns(iter(["CC"])).patterns == (S.parse("CC"),)
    # a graph source: exact elements and codes, nothing else
    naph = compiled.patterns[-1]
    assert len(naph.atoms) == 10 and len(naph.bonds) == 11 and {q.codes for q in naph.bonds} == {(4,)}
    assert all(q == S.atom(6) for q in naph.atoms)
    loose = S.from_graph(C.NAMED["naphthalene"][0][:2], bonds="any", elements=False)
    assert {q.codes for q in loose.bonds} == {S.ANY_CODES} and all(q == S.atom() for q in loose.atoms)
    for bad, where in ((["CC", "C[N+]"], r"patterns\[1\].*position 3"), ("CC", "iterable"), (3.5, "iterable"),
                       ([3.5], r"patterns\[0\]"), ([([6] * 33, [[0] * 33] * 33)], r"patterns\[0\].*32"),
                       ([([6, 0], [[0, 1], [1, 0]])], r"patterns\[0\]"), ([([], torch.zeros(0, 0, dtype=torch.int8))], "1 to 32")):
        with pytest.raises(ValueError, match=where):
            S.compile_patterns(bad)
    with pytest.raises(ValueError, match="codes"):
        S.from_graph(C.BENZENE[:2], bonds="exact")
    assert S.describe_status(0) == "ok" and S.describe_status(1) == "BUDGET" and S.describe_status(3) == "BUDGET|0x2"


_CATALOGUE_CASES = {                                       # name -> (a molecule that has the group, one that has not)
    "peroxide": (([6, 8, 8, 6], [(0, 1, 1), (1, 2, 1), (2, 3, 1)]), ([6, 8, 6], [(0, 1, 1), (1, 2, 1)])),
    "acyl halide": (([6, 6, 8, 17], [(0, 1, 1), (1, 2, 2), (1, 3, 1)]), ([6, 6, 17], [(0, 1, 1), (1, 2, 1)])),
    "aldehyde": (([6, 6, 8], [(0, 1, 1), (1, 2, 2)]), ([6, 6, 8, 6], [(0, 1, 1), (1, 2, 2), (1, 3, 1)])),
    "azo": (([6, 7, 7, 6], [(0, 1, 1), (1, 2, 2), (2, 3, 1)]), ([6, 7, 7, 6], [(0, 1, 1), (1, 2, 1), (2, 3, 1)])),
    "thiol": (([6, 16], [(0, 1, 1)]), ([6, 16, 6], [(0, 1, 1), (1, 2, 1)])),
    "isocyanate": (([6, 7, 6, 8], [(0, 1, 1), (1, 2, 2), (2, 3, 2)]), ([6, 6, 8, 7], [(0, 1, 1), (1, 2, 2), (1, 3, 1)])),
    "isothiocyanate": (([6, 7, 6, 16], [(0, 1, 1), (1, 2, 2), (2, 3, 2)]), ([6, 7, 6, 8], [(0, 1, 1), (1, 2, 2), (2, 3, 2)])),
    "Michael-acceptor enone": (([6, 6, 6, 8, 6], [(0, 1, 2), (1, 2, 1), (2, 3, 2), (2, 4, 1)]),
                               ([6, 6, 6, 8, 6], [(0, 1, 1), (1, 2, 1), (2, 3, 2), (2, 4, 1)])),
    "alkyl halide": (([6, 35], [(0, 1, 1)]), ([6] * 6 + [17], [(i, (i + 1) % 6, 4) for i in range(6)] + [(0, 6, 1)])),
    "epoxide": (([6, 8, 6], [(0, 1, 1), (1, 2, 1), (0, 2, 1)]), ([6, 8, 6], [(0, 1, 1), (1, 2, 1)])),
    "aziridine": (([6, 7, 6], [(0, 1, 1), (1, 2, 1), (0, 2, 1)]), ([6, 8, 6], [(0, 1, 1), (1, 2, 1), (0, 2, 1)])),
    "sulfonyl halide": (([6, 16, 8, 8, 17], [(0, 1, 1), (1, 2, 2), (1, 3, 2), (1, 4, 1)]),
                        ([6, 16, 8, 8, 6], [(0, 1, 1), (1, 2, 2), (1, 3, 2), (1, 4, 1)])),
    "disulfide": (([6, 16, 16, 6], [(0, 1, 1), (1, 2, 1), (2, 3, 1)]), ([6, 16, 6], [(0, 1, 1), (1, 2, 1)])),
    "nitroso": (([6, 7, 8], [(0, 1, 1), (1, 2, 2)]), ([6, 7, 8], [(0, 1, 2), (1, 2, 1)])),
    "ring larger than 8": (([6] * 9, [(i, (i + 1) % 9, 1) for i in range(9)]), ([6] * 8, [(i, (i + 1) % 8, 1) for i in range(8)])),
}


def test_every_catalogue_entry_matches_its_positive_and_misses_its_negative():
    assert set(S.CATALOGUE) == set(_CATALOGUE_CASES) and len(S.CATALOGUE) >= 12
    for name, pattern in S.CATALOGUE.items():
        assert pattern.name == name and pattern == S.parse({n: t for n, t in S._CATALOGUE_SOURCE}[name], name)
        has, has_not = (CR.mol(*m) for m in _CATALOGUE_CASES[name])
        assert SC.reference(has, pattern)["count"] >= 1, name
        assert SC.reference(has_not, pattern)["count"] == 0, name
    # the chain of nine ring bonds also fires on a fused system of ten ring atoms: the docstring says so
    assert SC.reference(C.NAMED["naphthalene"][0], S.CATALOGUE["ring larger than 8"])["count"] > 0
    assert SC.reference(C.BENZENE, S.CATALOGUE["ring larger than 8"])["count"] == 0


# ----------------------------------------------------------------------------------------------- options
UNDETERMINED = SC.path_smarts(7) + "~[#7]"     # on K12 (no nitrogen): every root hits the budget before any embedding
_SEAM_MEMO = {}


def _shard_molecules():
    """sample id -> molecule; 4 is K12, whose search for `UNDETERMINED` is stopped by the budget with nothing found."""
    return [C.CUBE, C.WAGNER, C.BENZENE, C.NAMED["toluene"][0], SC.K12, C.NAMED["decalin"][0],
            C.NAMED["naphthalene"][0], C.NAMED["biphenyl"][0]]


def _seam(calls):
    """`_match_substructures` by the restatement, each (molecule, pattern) computed once in the session."""
    inner = SC.seam_by_restatement(calls)

    def run(z, bonds, n, compiled):
        z, bonds = torch.as_tensor(z), torch.as_tensor(bonds)
        out = None
        counts = torch.as_tensor(n).reshape(-1).tolist()
        keys = [(tuple(z[b, :k].tolist()), tuple(map(tuple, bonds[b, :k, :k].tolist()))) for b, k in enumerate(counts)]
        todo = [p for p, pat in enumerate(compiled.patterns) if any((key, pat) not in _SEAM_MEMO for key in keys)]
        if todo:
            out = inner(z, bonds, n, S.compile_patterns([compiled.patterns[p] for p in todo]))
            calls.pop()
            for j, p in enumerate(todo):
                for b, key in enumerate(keys):
                    _SEAM_MEMO[(key, compiled.patterns[p])] = (int(out["count"][b, j]), int(out["status"][b, j]),
                                                              out["first"][b, j].tolist(), int(out["covered"][b, j]))
        calls.append((len(counts), len(compiled.patterns)))
        P, M = len(compiled.patterns), compiled.max_atoms
        res = dict(count=torch.zeros(len(counts), P, dtype=torch.int32), status=torch.zeros(len(counts), P, dtype=torch.int32),
                   first=torch.full((len(counts), P, M), -1, dtype=torch.int32),
                   covered=torch.zeros(len(counts), P, dtype=torch.int64))
        for b, key in enumerate(keys):
            for p, pat in enumerate(compiled.patterns):
                c, st, first, cov = _SEAM_MEMO[(key, pat)]
                res["count"][b, p], res["status"][b, p], res["covered"][b, p] = c, st, cov
                res["first"][b, p, : len(pat.atoms)] = torch.tensor(first[: len(pat.atoms)], dtype=torch.int32)
        return res
    return run


def _generator(calls, finisher=None):
    gen = _shell_generator(finisher=finisher)
    gen._match_substructures = _seam(calls)
    gen._graph_fingerprints = _seam_fingerprints([])
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    return gen


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_substructure_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._match_substructures = gen._canonical_order = gen._graph_fingerprints = gen._score = _no_device
    call = getattr(gen, entry)
    big = ([6] * 33, [[0] * 33] * 33)
    for option in ("require_substructures", "exclude_substructures", "substructure_counts"):
        for bad in ("c1ccccc1", 3.5, [3.5], ["C[N+]"], [big], ["C" * 33], [None], [C.CUBE], ["CC", ""]):
            with pytest.raises(ValueError, match=option):
                call(reference_conformer=_ref(), n_samples=4, **{option: bad})
    with pytest.raises(ValueError, match=r"exclude_substructures\[1\].*position 3 .*no charges"):
        call(reference_conformer=_ref(), n_samples=4, require_substructures=["CC"], exclude_substructures=["CC", "C[N+]"])
    with pytest.raises(ValueError, match=r"substructure_counts\[0\].*32"):
        call(reference_conformer=_ref(), n_samples=4, substructure_counts=[big])
    with pytest.raises(ValueError):
        call(reference_conformer=_ref(), n_samples=4, require_substructures=["CC"], top_k=0)
    gen.finisher = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                              "finish_tag_chunk")
    for option in ("require_substructures", "exclude_substructures", "substructure_counts"):
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, **{option: ["CC"]})


def test_parse_request_compiles_the_three_lists_together():
    gen = _shell_generator()
    gen._match_substructures = _no_device
    req = postprocess.parse_request(gen, None, require_substructures=["c1ccccc1", C.CUBE[:2]],
                                    exclude_substructures=[S.CATALOGUE["peroxide"]], substructure_counts=iter(["[nH]"]))
    assert (req.n_required, req.n_excluded, len(req.substructures.patterns)) == (2, 1, 4)
    assert req.substructures.patterns[1] == S.from_graph(C.CUBE[:2]) and req.substructures.needs_hydrogens
    assert req.measures and req.removes
    only = postprocess.parse_request(gen, None, substructure_counts=["CC"])
    assert only.measures and not only.removes and (only.n_required, only.n_excluded) == (0, 0)
    none = postprocess.parse_request(gen, None, require_substructures=[], exclude_substructures=None)
    assert none.substructures is None and not none.measures and none == postprocess.Request()


def test_proxy_path_filters_counts_and_the_undetermined_rows():
    mols = _shard_molecules()
    calls = []
    gen = _generator(calls)
    gen._generate_shard = _graph_shard(mols)
    kw = dict(reference_conformer=_ref(), n_samples=8)

    plain = gen.generate_conformers(**kw)
    assert calls == [] and [m.sample_id for m in plain] == list(range(8))         # no option: the seam is not touched
    assert all(m.substructure_counts is None and m.substructure_status is None and m.substructure_first is None
               and m.substructure_patterns is None for m in plain)

    def ids(**more):
        with warnings.catch_warnings():
            warnings.simplefilter("error")                                        # no warning without an undetermined row
            return [m.sample_id for m in gen.generate_conformers(**dict(kw, **more))]
    assert ids(require_substructures=[SC.ANY5]) == [1, 4] and calls == [(8, 1)]   # the Wagner graph (and K12), not the cube
    assert ids(exclude_substructures=[SC.ANY5]) == [0, 2, 3, 5, 6, 7]
    assert ids(require_substructures=[SC.AROM6]) == [2, 3, 6, 7]
    assert ids(require_substructures=[SC.AROM6, "Cc"]) == [3]                     # every required pattern
    assert ids(exclude_substructures=["Cc", SC.ANY4]) == [2, 5, 6, 7]             # any excluded pattern
    assert ids(require_substructures=[SC.AROM6], exclude_substructures=["c-c"], substructure_counts=["C"]) == [2, 3, 6]
    assert calls[-1] == (8, 3)                                                    # ONE call, every pattern in it
    assert ids(require_substructures=[C.BENZENE[:2]]) == [2, 3, 6, 7]             # a graph as the pattern
    assert ids(require_substructures=[]) == list(range(8))
    # in front of `unique`: the cube (sample 0) and the Wagner graph share a graph key, and `unique` keeps sample 0
    assert ids(unique=True) == [0, 2, 3, 4, 5, 6, 7]
    assert ids(unique=True, require_substructures=[SC.ANY5]) == [1, 4]
    assert ids(unique=True, exclude_substructures=[SC.ANY4 + ".*"]) == [2, 3, 5, 6, 7]
    # a budget row WITH an embedding is proven to contain the pattern: K12 has a 7-path (only benzene has none)
    assert ids(require_substructures=[SC.PATH7]) == [0, 1, 3, 4, 5, 6, 7] and ids(exclude_substructures=[SC.PATH7]) == [2]
    # a budget row without one is undetermined: `require` drops it, `exclude` keeps it, one warning says how many
    with pytest.warns(UserWarning, match="1 molecule") as seen:
        got = gen.generate_conformers(exclude_substructures=[UNDETERMINED, "Cc"], **kw)
    assert [m.sample_id for m in got] == [0, 1, 2, 4, 5, 6, 7] and len([w for w in seen if "BUDGET" in str(w.message)]) == 1
    assert got[3].substructure_status == [S.STATUS_BUDGET, 0] and got[3].substructure_counts == [0, 0]
    with pytest.warns(UserWarning, match="1 molecule"):
        assert gen.generate_conformers(require_substructures=[UNDETERMINED], **kw) == []
    with pytest.warns(UserWarning, match="1 molecule"):
        kept = gen.generate_conformers(require_substructures=["*"], exclude_substructures=[UNDETERMINED], **kw)
    assert [m.sample_id for m in kept] == list(range(8))
    assert ids(substructure_counts=[UNDETERMINED]) == list(range(8))              # only measured: nothing to warn about

    patterns = [SC.ANY5, "Cc", SC.AROM6, "[#6]~!@[#6]"]
    got = gen.generate_conformers(substructure_counts=patterns, **kw)
    assert [m.sample_id for m in got] == list(range(8)) and all(a == m for a, m in zip(plain, got))
    assert isinstance(got[7]._measured.substructure_counts, tuple)                # sliced on first read
    for m in got:
        want = [SC.reference(mols[m.sample_id], p) for p in patterns]
        assert m.substructure_counts == [w["count"] for w in want] and m.substructure_status == [0] * 4
        assert m.substructure_first == [w["first"] for w in want]
        assert m.substructure_patterns == tuple(S.parse(p) for p in patterns)
    assert isinstance(got[7]._measured.substructure_counts, list)
    assert got[3].substructure_first[1] == [6, 0] and got[0].substructure_first == [None] * 4
    assert [m.sample_id for m in gen.generate_conformers_sharded(require_substructures=[SC.ANY5], **kw)] == [1, 4]
    assert [m.sample_id for m in gen.forward(exclude_substructures=[SC.AROM6], **kw)] == [0, 1, 4, 5]
    both = gen.generate_conformers(require_substructures=[SC.AROM6], substructure_counts=["Cc"], top_k=2, **kw)
    assert [m.sample_id for m in both] == [3, 7] and [m.substructure_counts for m in both] == [[12, 1], [24, 0]]


def test_object_path_reads_the_mols_own_graphs():
    mols = _shard_molecules()
    calls = []
    gen = _generator(calls, finisher="rdkit")
    gen._generate_shard = _MolStage(gen, mols)                                   # sample 2 is dropped by the finish
    kw = dict(reference_conformer=_ref(), n_samples=8, sample_seed=5)

    def ids(**more):
        return [m.props["sample_id"] for m in gen.generate_conformers(**dict(kw, **more))]
    assert ids() == [0, 1, 3, 4, 5, 6, 7] and calls == []
    assert ids(require_substructures=[SC.ANY5]) == [1, 4] and calls == [(7, 1)]  # the live Mols in ONE batched call
    assert ids(exclude_substructures=[SC.AROM6]) == [0, 1, 4, 5]
    got = gen.generate_conformers(substructure_counts=[SC.ANY4, SC.AROM6], **kw)
    assert [m.props["substructure_counts"] for m in got] == ["48 0", "32 0", "0 12", "11880 0", "0 0", "0 24", "0 24"]
    assert all(m.props["substructure_status"] == "0 0" for m in got)


def test_select_places_the_two_filters_behind_the_electrostatic_threshold():
    compiled = S.compile_patterns(["CC", "N"])
    req = postprocess.Request(min_electrostatic_tanimoto=0.5, substructures=compiled, n_required=1, n_excluded=1)
    measured = [Measured(electrostatic_tanimoto=v) for v in (0.9, 0.1, 0.8, 0.7)]
    sub = [([1, 0], [0, 0]), ([0, 0], [1, 0]), ([0, 0], [0, 0]), ([3, 2], [0, 0])]
    rows = postprocess.Rows(list("abcd"), [0, 1, 2, 3], measured, [0, 1, 2, 3], None, sub)
    with warnings.catch_warnings():
        warnings.simplefilter("error")            # the undetermined row fell to the electrostatic threshold before
        assert postprocess.select(rows, req, None, None) == ["a"]
    loose = postprocess.Request(substructures=compiled, n_required=1, n_excluded=1)
    with pytest.warns(UserWarning, match="1 molecule"):
        assert postprocess.select(rows, loose, None, None) == ["a"]
    recs = measured_from_tensors(dict(substructure_counts=torch.tensor([[2, 0]]), substructure_status=torch.tensor([[0, 1]]),
                                      substructure_first=torch.tensor([[[4, 7], [-1, -1]]]),
                                      substructure_patterns=compiled.patterns), 1)
    assert recs[0].substructure_counts[1] == 0 and recs[0].substructure_patterns == compiled.patterns      # (batch, row)
    mol = molecules_from_tensors(torch.zeros(1, 9, 3), torch.full((1, 9), 6), torch.zeros(1, 9, 9, dtype=torch.int8),
                                 torch.tensor([9]), torch.ones(1), substructure_counts=torch.tensor([[2, 0]]),
                                 substructure_status=torch.tensor([[0, 1]]), substructure_first=torch.tensor([[[4, 7], [-1, -1]]]),
                                 substructure_patterns=compiled.patterns)[0]
    assert (mol.substructure_counts, mol.substructure_status, mol.substructure_first) == ([2, 0], [0, 1], [[4, 7], None])


# ----------------------------------------------------------------------------------------------- C ABI
def test_substructure_entry_refuses_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check

    def match(z=p, bonds=p, n=p, nh=p, B=3, W=42, pat_n=p, atoms=p, pbonds=p, P=5, count=p, status=p, first=p, covered=p):
        return h.mcg_substructure_match(z, bonds, n, nh, B, W, pat_n, atoms, pbonds, P, count, status, first, covered, None)

    for bad in (dict(z=None), dict(bonds=None), dict(n=None), dict(pat_n=None), dict(atoms=None), dict(pbonds=None),
                dict(count=None), dict(status=None), dict(first=None), dict(covered=None), dict(B=-1), dict(B=16385),
                dict(W=0), dict(W=65), dict(W=-3), dict(P=0), dict(P=65), dict(P=-1), dict(B=0, P=0), dict(nh=None, z=None)):
        assert match(**bad) == 1, bad
        assert b"mcg_substructure_match" in h.mcg_last_error(), bad
    assert match(B=0) == 0 and match(B=0, nh=None) == 0                            # nothing to do, nothing launched
    assert h.mcg_abi_version() == 4 and "mcg_substructure_match" in _lib.SIGNATURES
    assert (S.MAX_ATOMS, S.MAX_PATTERN_ATOMS, S.MAX_PATTERNS, S.MAX_B, S.NODE_BUDGET, S.STATUS_BUDGET) == \
        (64, 32, 64, 16384, 65536, 1)
    header = open(os.path.join(ROOT, "include", "mlconfgen_hip.h")).read()
    for name, value in (("MAX_ATOMS", 64), ("MAX_PATTERN_ATOMS", 32), ("MAX_PATTERNS", 64), ("MAX_B", 16384),
                        ("NODE_BUDGET", 65536), ("BUDGET", 1)):
        assert f"#define MCG_SUBSTRUCTURE_{name} {value}\n" in header
    with pytest.raises(ValueError):
        S.match_substructures(torch.zeros(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8),
                              torch.tensor([3]), ["CC"])
    with pytest.raises(ValueError):
        S.match_substructures(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8),
                              torch.tensor([3, 6]), ["CC"])
    with pytest.raises(ValueError):
        S.match_substructures(torch.zeros(2, 5), torch.zeros(2, 5, 5, dtype=torch.int8), torch.tensor([3, 2]), ["CC"])
    with pytest.raises(ValueError):
        S.match_substructures(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8),
                              torch.tensor([3, 2]), [])
    with pytest.raises(ValueError, match=r"patterns\[0\]"):
        S.match_substructures(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8),
                              torch.tensor([3, 2]), ["C+"])


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_substructure`: the entry's argument checks in a stand-alone program under host-side ASan + UBSan, on the
    CPU."""
    exe = str(tmp_path / "substructure_arg_check")
    csrc = os.path.join(ROOT, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_substructure", f"SUBSTRUCTURE_CHECK={exe}"], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 wrong" in ran.stdout, ran.stdout + ran.stderr
