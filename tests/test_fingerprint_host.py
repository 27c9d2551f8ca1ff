"""Chemical fingerprints and graph keys, host side (no GPU): the plain-Python restatement against its pins, its invariance
under renumbering, the graph key against brute-force isomorphism, `mol_graph`, `select_unique`, the combined exclusion walk,
every refusal of the generation entries before any device work, the C entries' argument checks, and the records / Mol
properties and filters through the device seams replaced by the restatement, on the proxy and the object path."""
import ctypes
import itertools
import os
import random

import numpy as np
import pytest
import torch

import fingerprint_cases as C
import fingerprint_ref as R
from ml_conformer_generator_amd import fingerprint as FP
from ml_conformer_generator_amd.cheminformatics import select_diverse
from ml_conformer_generator_amd.handoff import GeneratedMolecule
from test_shape_overlay_host import PosedMol, _no_device, _ref, _shell_generator, _Stage

U64 = (1 << 64) - 1


# ----------------------------------------------------------------------------------------------- the restatement
def test_restatement_reproduces_its_pins():
    assert R.mm3([], 0) == 0 and R.mm3([0], 0) == 0x2362f9de and R.mm3([1, 2, 3], 0x6d636731) == 0x9def72fb
    assert R.SEED == 0x6d636731
    for name, (mol, bits, key) in C.PINNED.items():
        assert sorted(R.fingerprint(*mol)) == bits, name
        assert R.key(*mol) == key, name
        assert R.fingerprint_and_key(*mol) == (set(bits), key), name
    sets = {k: set(v[1]) for k, v in C.PINNED.items()}
    assert R.tanimoto(sets["ethanol"], sets["dimethyl ether"]) == np.float32(1) / np.float32(14)
    assert R.tanimoto(sets["benzene"], sets["pyridine"]) == np.float32(3) / np.float32(9)
    assert np.isnan(R.tanimoto(sets["no atoms"], sets["benzene"])) and np.isnan(R.tanimoto(set(), set()))


def test_restatement_is_invariant_under_renumbering():
    rng = random.Random(2026)
    mols = C.molecule_like_set()
    assert len(mols) >= 500 and {m[2] for m in mols} == set(range(1, 43))
    moved = 0
    for mol in mols:
        other = C.random_permutation(rng, mol)
        moved += other[:2] != mol[:2]
        assert R.fingerprint_and_key(*other) == R.fingerprint_and_key(*mol)
    assert moved >= 450


def _small_graph(rng):
    n = rng.randint(4, 6)
    z = [rng.choice([6, 6, 7, 8]) for _ in range(n)]
    adj = [[0] * n for _ in range(n)]
    for a in range(1, n):
        j = rng.randrange(a)
        adj[a][j] = adj[j][a] = rng.choice([1, 1, 2])
    if rng.random() < 0.5:
        a, j = rng.sample(range(n), 2)
        if adj[a][j] == 0:
            adj[a][j] = adj[j][a] = rng.choice([1, 1, 2])
    return z, adj, n


def _canonical(z, adj, n):
    """The smallest (elements, upper triangle) over all n! numberings."""
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return (n,) + min(tuple(z[p[i]] for i in range(n)) + tuple(adj[p[i]][p[j]] for i, j in pairs)
                      for p in itertools.permutations(range(n)))


def test_key_equality_coincides_with_isomorphism_on_small_graphs():
    rng = random.Random(31)
    graphs = [_small_graph(rng) for _ in range(600)]
    canon = [_canonical(*g) for g in graphs]
    keys = [R.key(*g) for g in graphs]
    isomorphic = wrong = 0
    for i in range(len(graphs)):
        for j in range(i):
            same = canon[i] == canon[j]
            wrong += same != (keys[i] == keys[j])
            isomorphic += same and graphs[i] != graphs[j]
    assert wrong == 0
    assert isomorphic >= 20, isomorphic


def _fluoro_chain(at):
    return R.mol([6] * 20 + [9], [(i, i + 1, 1) for i in range(19)] + [(at, 20, 1)])


def test_key_named_cases():
    assert R.key(*C.PINNED["decalin"][0]) != R.key(*C.PINNED["bicyclopentyl"][0])
    f5, f6, f14 = _fluoro_chain(5), _fluoro_chain(6), _fluoro_chain(14)
    assert R.key(*f5) != R.key(*f6)
    assert R.fingerprint(*f5) == R.fingerprint(*f6)          # radius 2 cannot see where along the chain it sits
    assert R.key(*f5) == R.key(*f14)                         # the mirror image


# ----------------------------------------------------------------------------------------------- mol_graph
class _Bond:
    def __init__(self, i, j, order):
        self.i, self.j, self.order = i, j, order

    def GetBeginAtomIdx(self):
        return self.i

    def GetEndAtomIdx(self):
        return self.j

    def GetBondTypeAsDouble(self):
        return self.order


class BondedMol(PosedMol):
    """`PosedMol` with bonds and string properties: what a finished Mol shows `mol_graph`."""

    def __init__(self, z, bonds, pos=None):
        super().__init__([[0.1 * k, 0.0, 0.0] for k in range(len(z))] if pos is None else pos, z=z)
        self.bonds = [_Bond(*b) for b in bonds]

    def GetBonds(self):
        return list(self.bonds)

    def SetProp(self, k, v):
        assert isinstance(v, str)
        self.props[k] = v


_ORDER = {1: 1.0, 2: 2.0, 3: 3.0, 4: 1.5}


def _as_mol(mol, hydrogens=0):
    """A (z, adj, n) molecule as a stand-in Mol, with `hydrogens` explicit hydrogens on atom 0."""
    z, adj, n = mol
    bonds = [(i, j, _ORDER[adj[i][j]]) for i in range(n) for j in range(i) if adj[i][j]]
    return BondedMol(list(z) + [1] * hydrogens, bonds + [(0, n + k, 1.0) for k in range(hydrogens)])


def test_mol_graph_reads_records_mols_and_pairs():
    z, adj, n = C.PINNED["pyridine"][0]
    rec = GeneratedMolecule(z, torch.zeros(n, 3), torch.tensor(adj, dtype=torch.int8))
    for obj in (rec, _as_mol((z, adj, n)), (z, torch.tensor(adj)), (torch.tensor(z), np.array(adj)), [z, adj]):
        got_z, got_b = FP.mol_graph(obj)
        assert got_z == z and got_b.dtype == torch.int8 and got_b.tolist() == adj
    # hydrogens and their bonds are dropped, wherever they sit; 1.5 -> 4
    m = BondedMol([1, 6, 1, 6, 8, 1], [(0, 1, 1.0), (1, 2, 1.0), (1, 3, 1.5), (3, 4, 2.0), (4, 5, 1.0)])
    got_z, got_b = FP.mol_graph(m)
    assert got_z == [6, 6, 8] and got_b.tolist() == [[0, 4, 0], [4, 0, 2], [0, 2, 0]]
    got_z, got_b = FP.mol_graph(([1, 6, 8], [[0, 1, 0], [1, 0, 3], [0, 3, 0]]))
    assert got_z == [6, 8] and got_b.tolist() == [[0, 3], [3, 0]]
    assert FP.mol_graph(([], torch.zeros(0, 0, dtype=torch.int8)))[0] == []
    zs, bonds, nn = FP.pad_graphs([FP.mol_graph(m), FP.mol_graph(rec)])
    assert zs.shape == (2, 6) and bonds.shape == (2, 6, 6) and nn.tolist() == [3, 6] and zs.dtype == torch.int32


def test_mol_graph_refusals():
    for bad in (3.5, "CCO", None, torch.zeros(3, 3), ([6, 6], [[0, 1], [2, 0]]), ([6, 6], [[0, 5], [5, 0]]),
                ([6, 6], [[0, -1], [-1, 0]]), ([6, 6], [[0, 1.0], [1.0, 0]]), ([6, 6], [[0, 1, 0], [1, 0, 0]]),
                ([6, 0], [[0, 1], [1, 0]]), ([6, 6, 6], [[0, 1], [1, 0]]), ([6, 6], [[False, True], [True, False]]),
                BondedMol([6, 6], [(0, 1, 2.5)]), BondedMol([6, 6], [(0, 1, 0.0)])):
        with pytest.raises(ValueError):
            FP.mol_graph(bad)


# ----------------------------------------------------------------------------------------------- host selection
def test_select_unique():
    keys = [5, 9, 5, 7, 9, 5]
    assert FP.select_unique(keys, range(6)) == [0, 1, 3]
    assert FP.select_unique(keys, [5, 4, 3, 2, 1, 0]) == [3, 4, 5]
    assert FP.select_unique(keys, [2, 0, 4, 1, 3, 5]) == [2, 3, 4]
    assert FP.select_unique(keys, [2, 4]) == [2, 4]                   # positions the order does not name are not kept
    assert FP.select_unique([], []) == []
    assert FP.select_unique([U64, 0, U64], [2, 1, 0]) == [1, 2]


def test_combined_exclusion_walk_with_two_pair_matrices():
    nan = float("nan")
    scores, ids = [0.9, 0.8, 0.7, 0.6], [0, 1, 2, 3]
    shape = [[1, .9, .1, .1], [.9, 1, .1, .1], [.1, .1, 1, .2], [.1, .1, .2, 1]]
    chem = [[1, .1, .1, .1], [.1, 1, .1, .1], [.1, .1, 1, .8], [.1, .1, .8, 1]]
    assert select_diverse(scores, ids, shape, 0.5) == [0, 2, 3]                               # as before
    assert select_diverse(scores, ids, None, None, chemical_pair=chem, max_pairwise_chemical_tanimoto=0.5) == [0, 1, 2]
    assert select_diverse(scores, ids, shape, 0.5, None, None, chem, 0.5) == [0, 2]          # either matrix excludes
    assert select_diverse(scores, ids, shape, 0.5, 1, None, chem, 0.5) == [0]
    assert select_diverse(scores, ids, shape, 0.5, None, 0.65, chem, 0.5) == [0, 2]
    assert select_diverse(scores, ids, shape, 0.95, None, None, chem, 0.8) == [0, 1, 2]      # >= excludes at the value
    assert select_diverse(scores, ids, shape, 0.95, None, None, chem, 0.81) == [0, 1, 2, 3]
    holes = [[1, nan, .1, .1], [nan, 1, .1, .1], [.1, .1, 1, nan], [.1, .1, nan, 1]]
    assert select_diverse(scores, ids, shape, 0.95, None, None, holes, 0.5) == [0, 1, 2, 3]  # NaN excludes nothing
    assert select_diverse(scores, ids, holes, 0.5, None, None, chem, 0.5) == [0, 1, 2]
    # ranking order decides who is kept: the better-scored of a chemical pair
    assert select_diverse([0.1, 0.2, 0.3, 0.9], ids, None, None, None, None, chem, 0.5) == [3, 1, 0]
    # unscored calls walk in sample order
    assert select_diverse([None] * 4, [7, 3, 5, 1], None, None, None, None, chem, 0.5) == [3, 1, 0]
    assert select_diverse([None] * 4, ids, None, None, None, None, chem, 0.5) == [0, 1, 2]
    assert select_diverse(scores, ids, None, None) == [0, 1, 2, 3]
    assert select_diverse([0.5, nan, 0.7, 0.5], [4, 1, 2, 3], None, None, 3) == [2, 3, 0]     # today's ranking


# ----------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_chemical_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._graph_fingerprints = gen._chem_tanimoto = gen._chem_pair = gen._score = _no_device
    call = getattr(gen, entry)
    graph = C.PINNED["benzene"][0][:2]
    nan = float("nan")
    cases = [dict(chemical_scores=True),                                          # coordinates carry no graph
             dict(max_chemical_tanimoto=0.5),
             dict(reference_graph=graph),                                         # a graph nobody reads
             dict(reference_graph=graph, unique=True),
             dict(chemical_scores=True, reference_graph=3.5),
             dict(chemical_scores=True, reference_graph=([], [])),
             dict(chemical_scores=True, reference_graph=([1, 1], [[0, 1], [1, 0]])),          # no heavy atoms
             dict(chemical_scores=True, reference_graph=([6, 6], [[0, 1], [2, 0]])),
             dict(chemical_scores=True, reference_graph=BondedMol([6, 6], [(0, 1, 2.5)])),
             dict(chemical_scores=True, reference_graph=([6] * 65, [[0] * 65] * 65)),
             dict(chemical_scores=1, reference_graph=graph), dict(chemical_scores="yes", reference_graph=graph),
             dict(chemical_scores=None, reference_graph=graph),
             dict(unique=1), dict(unique="yes"), dict(unique=None), dict(unique=0.0)]
    for name in ("max_chemical_tanimoto", "max_pairwise_chemical_tanimoto"):
        for bad in (0, 0.0, -0.1, 1.0001, 2, True, False, nan, "0.5", [0.5]):
            cases.append({name: bad, "reference_graph": graph, "chemical_scores": True})
    for kw in cases:
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    with pytest.raises(ValueError):
        call(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=17, n_samples=4, chemical_scores=True)
    gen.finisher = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                              "finish_tag_chunk")
    with pytest.raises(ValueError, match="custom finisher"):
        call(reference_conformer=_ref(), n_samples=4, unique=True)


def test_fingerprint_entries_refuse_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check

    def graph(z=p, bonds=p, n=p, B=3, W=42, fp=p, key=p):
        return h.mcg_graph_fingerprint(z, bonds, n, B, W, fp, key, None, None)

    for bad in (dict(z=None), dict(bonds=None), dict(n=None), dict(fp=None), dict(key=None), dict(B=-1), dict(W=0),
                dict(W=65), dict(W=-3)):
        assert graph(**bad) == 1, bad
        assert b"mcg_graph_fingerprint" in h.mcg_last_error(), bad
    for bad in ((None, p, 3, p), (p, None, 3, p), (p, p, 3, None), (p, p, -1, p)):
        assert h.mcg_fingerprint_tanimoto(*bad, None) == 1, bad
        assert b"mcg_fingerprint_tanimoto" in h.mcg_last_error(), bad
    for bad in ((None, 3, p), (p, 3, None), (p, -1, p), (p, 16385, p)):
        assert h.mcg_fingerprint_pair_tanimoto(*bad, None) == 1, bad
        assert b"mcg_fingerprint_pair_tanimoto" in h.mcg_last_error(), bad
    assert graph(B=0) == 0 and h.mcg_fingerprint_tanimoto(p, p, 0, p, None) == 0      # nothing to do, nothing launched
    assert h.mcg_fingerprint_pair_tanimoto(p, 0, p, None) == 0
    assert h.mcg_abi_version() == 4
    for name in ("mcg_graph_fingerprint", "mcg_fingerprint_tanimoto", "mcg_fingerprint_pair_tanimoto"):
        assert name in _lib.SIGNATURES
    with pytest.raises(ValueError):
        FP.graph_fingerprints(torch.zeros(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8),
                              torch.tensor([3]))
    with pytest.raises(ValueError):
        FP.graph_fingerprints(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8),
                              torch.tensor([3, 6]))
    with pytest.raises(ValueError):
        FP.pairwise_fingerprint_tanimoto(torch.zeros(16385, 64, dtype=torch.int32))
    with pytest.raises(ValueError):
        FP.fingerprint_tanimoto(torch.zeros(4, 63, dtype=torch.int32), torch.zeros(64, dtype=torch.int32))


# ----------------------------------------------------------------------------------------------- seams = restatement
def _seam_fingerprints(calls):
    """`_graph_fingerprints` by the restatement, on the host."""
    def run(z, bonds, n):
        z, bonds, n = torch.as_tensor(z), torch.as_tensor(bonds), torch.as_tensor(n).reshape(-1).tolist()
        calls.append(len(n))
        words, keys, pops = [], [], []
        for b, k in enumerate(n):
            bits, key = R.fingerprint_and_key(z[b, :k].tolist(), bonds[b, :k, :k].tolist(), k)
            words.append(R.words(bits))
            keys.append(key)
            pops.append(len(bits))
        fp = torch.from_numpy(np.array(words, dtype=np.uint32).reshape(len(n), 64).view(np.int32))
        return fp, torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64)), torch.tensor(pops, dtype=torch.int32)
    return run


def _bits(row):
    return {32 * w + k for w, v in enumerate(np.asarray(row).view(np.uint32).tolist()) for k in range(32) if v >> k & 1}


def _seam_tanimoto(fp, ref_fp):
    ref = _bits(ref_fp.numpy())
    return torch.tensor([float(R.tanimoto(_bits(r), ref)) for r in fp.numpy()], dtype=torch.float32)


def _seam_pair(calls):
    def run(fp):
        sets = [_bits(r) for r in fp.numpy()]
        calls.append(len(sets))
        return torch.tensor([[float(R.tanimoto(a, b)) for b in sets] for a in sets], dtype=torch.float32).reshape(
            len(sets), len(sets))
    return run


def _with_seams(gen, fp_calls, pair_calls):
    gen._graph_fingerprints = _seam_fingerprints(fp_calls)
    gen._chem_tanimoto = _seam_tanimoto
    gen._chem_pair = _seam_pair(pair_calls)
    return gen


# sample id -> molecule of the stub shards: 3 and 6 repeat 0 (renumbered), 7 repeats 4
def _shard_molecules():
    rng = random.Random(8)
    eth = C.PINNED["ethanol"][0]
    ben = C.PINNED["benzene"][0]
    return [eth, C.PINNED["dimethyl ether"][0], C.PINNED["n-hexane"][0], R.permute(*eth, [2, 0, 1]), ben,
            C.PINNED["pyridine"][0], R.permute(*eth, [1, 2, 0]), C.random_permutation(rng, ben)]


def _graph_shard(mols):
    def run(ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
        el = torch.full((n_samples, 42), 9, dtype=torch.int8)                     # junk beyond the atoms
        bond = torch.full((n_samples, 42, 42), 3, dtype=torch.int8)
        x = torch.zeros(n_samples, 8, 3)
        n = torch.zeros(n_samples, dtype=torch.int32)
        for b, sid in enumerate(ids):
            z, adj, k = mols[sid]
            el[b, :k] = torch.tensor(z, dtype=torch.int8)
            bond[b, :k, :k] = torch.tensor(adj, dtype=torch.int8)
            n[b] = k
            x[b, :k, 0] = torch.arange(k) * 1.5
            x[b, 0, 1] = [0.3, 0.9, 0.5, 0.8, 0.2, 0.6, 0.4, 0.7][sid]           # the stub shape score
        valid = torch.tensor([0 if sid == 2 else 1 for sid in ids], dtype=torch.uint8)
        return dict(x=x, elements=el, bond=bond, n_nodes=n, valid=valid)
    return run


def test_proxy_path_records_carry_scores_and_keys_and_pass_the_filters():
    mols = _shard_molecules()
    keys = [R.key(*m) for m in mols]
    sets = [R.fingerprint(*m) for m in mols]
    fp_calls, pair_calls = [], []
    gen = _with_seams(_shell_generator(), fp_calls, pair_calls)
    gen._generate_shard = _graph_shard(mols)
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    kw = dict(reference_conformer=_ref(), n_samples=8)
    ben = _as_mol(C.PINNED["benzene"][0], hydrogens=2)

    plain = gen.generate_conformers(**kw)
    assert fp_calls == [] and [m.sample_id for m in plain] == [0, 1, 3, 4, 5, 6, 7]          # 2: invalid
    assert all(m.chemical_tanimoto is None and m.graph_key is None for m in plain)

    got = gen.generate_conformers(chemical_scores=True, reference_graph=ben, **kw)
    assert fp_calls == [8, 1] and pair_calls == []               # one launch over the shard, one for the reference
    assert [m.sample_id for m in got] == [0, 1, 3, 4, 5, 6, 7]
    for a, m in zip(plain, got):
        assert a == m and m.graph_key == keys[m.sample_id]
        assert np.float32(m.chemical_tanimoto) == R.tanimoto(sets[m.sample_id], sets[4])
    assert got[3].chemical_tanimoto == 1.0 and got[4].chemical_tanimoto == pytest.approx(3 / 9)

    def ids(**more):
        return [m.sample_id for m in gen.generate_conformers(**dict(kw, **more))]
    assert ids(max_chemical_tanimoto=1.0, reference_graph=ben) == [0, 1, 3, 5, 6]
    assert ids(max_chemical_tanimoto=0.3, reference_graph=ben) == [0, 1, 3, 6]
    only_keys = gen.generate_conformers(unique=True, **kw)
    assert [m.sample_id for m in only_keys] == [0, 1, 4, 5]      # unscored: the lowest sample id of a graph stays
    assert all(m.graph_key == keys[m.sample_id] and m.chemical_tanimoto is None for m in only_keys)
    # scored: the best-scored copy stays (0.3 / 0.8 / 0.4 -> 3; 0.2 / 0.7 -> 7), still in sample order
    assert ids(unique=True, shape_scores=True) == [1, 3, 5, 7]
    assert ids(unique=True, top_k=2) == [1, 3]                   # then the selection, in ranking order
    assert ids(unique=True, max_chemical_tanimoto=1.0, reference_graph=ben) == [0, 1, 5]
    # chemical diversity: ethanol / ether share 1 of 14 bits, benzene / pyridine 3 of 9
    assert ids(max_pairwise_chemical_tanimoto=1.0) == [0, 1, 4, 5] and pair_calls == [7]
    assert ids(max_pairwise_chemical_tanimoto=0.3) == [0, 1, 4]
    assert ids(max_pairwise_chemical_tanimoto=0.3, shape_scores=True) == [1, 3, 7]           # ranking order
    assert ids(max_pairwise_chemical_tanimoto=1.0, unique=True, top_k=3) == [1, 3, 7]
    assert gen.last_valid_fraction == pytest.approx(7 / 8)
    assert [m.sample_id for m in gen.generate_conformers_sharded(unique=True, **kw)] == [0, 1, 4, 5]
    assert [m.sample_id for m in gen.forward(unique=True, shape_scores=True, **kw)] == [1, 3, 5, 7]


class _MolStage:
    """`_generate_shard` for the object path: finished stand-in Mols (with hydrogens) of the shard molecules; sample 2 is
    dropped by the finish."""
    def __init__(self, gen, mols):
        self.gen, self.mols = gen, mols

    def __call__(self, ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
        self.gen._finish_stage = _Stage([None if i == 2 else _as_mol(self.mols[i], hydrogens=i % 3) for i in ids])
        return dict(x=torch.zeros(n_samples, 5, 3))


def test_object_path_mols_carry_the_properties_and_pass_the_filters():
    mols = _shard_molecules()
    keys = [R.key(*m) for m in mols]
    sets = [R.fingerprint(*m) for m in mols]
    fp_calls, pair_calls = [], []
    gen = _with_seams(_shell_generator(finisher="rdkit"), fp_calls, pair_calls)
    gen._generate_shard = _MolStage(gen, mols)
    kw = dict(reference_conformer=_ref(), n_samples=8, sample_seed=5)
    ben = C.PINNED["benzene"][0][:2]

    plain = gen.generate_conformers(**kw)
    assert fp_calls == [] and [m.props["sample_id"] for m in plain] == [0, 1, 3, 4, 5, 6, 7]
    assert all("graph_key" not in m.props and "chemical_tanimoto" not in m.props for m in plain)
    got = gen.generate_conformers(chemical_scores=True, reference_graph=ben, **kw)
    assert fp_calls == [7, 1]                                    # the live Mols in ONE batched call; the reference
    assert [m.props["sample_id"] for m in got] == [0, 1, 3, 4, 5, 6, 7]
    for m in got:
        sid = m.props["sample_id"]
        assert m.props["graph_key"] == str(keys[sid]) and int(m.props["graph_key"]) == keys[sid]
        assert np.float32(m.props["chemical_tanimoto"]) == R.tanimoto(sets[sid], sets[4])

    def ids(**more):
        return [m.props["sample_id"] for m in gen.generate_conformers(**dict(kw, **more))]
    # duplicates and the reference's own graph dropped; the dropped Mol passed over
    assert ids(unique=True, max_chemical_tanimoto=1.0, reference_graph=ben) == [0, 1, 5]
    assert ids(unique=True) == [0, 1, 4, 5]
    assert ids(max_chemical_tanimoto=1.0, reference_graph=ben) == [0, 1, 3, 5, 6]
    assert ids(max_pairwise_chemical_tanimoto=0.3) == [0, 1, 4] and pair_calls == [7]
    uniq = gen.generate_conformers(unique=True, **kw)
    assert all("chemical_tanimoto" not in m.props and m.props["graph_key"] == str(keys[m.props["sample_id"]])
               for m in uniq)
    assert gen.last_valid_fraction == pytest.approx(7 / 8)
    assert [m.props["sample_id"] for m in gen.generate_conformers_sharded(unique=True, **kw)] == [0, 1, 4, 5]
