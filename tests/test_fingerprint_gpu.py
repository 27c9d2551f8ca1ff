"""Chemical fingerprints and graph keys by HIP (`mcg_graph_fingerprint`, `mcg_fingerprint_tanimoto`,
`mcg_fingerprint_pair_tanimoto`) on the MI355X: every bit against the plain-Python restatement (`fingerprint_ref`), the
same bits whatever the numbering, row, batch and padded width, the Tanimoto kernels against numpy fp32, sentinels around
the outputs, and the chemical options of the generation entries end to end."""
import random

import numpy as np
import pytest
import torch

import fingerprint_cases as C
import fingerprint_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U64 = (1 << 64) - 1


def _batch(mols, W=None, junk_seed=None):
    """(z [B,W] int32, bonds [B,W,W] int8, n [B] int32); with `junk_seed` the padding (and the diagonal) holds junk
    elements and junk, asymmetric codes."""
    W = W or max([m[2] for m in mols] + [1])
    B = len(mols)
    if junk_seed is None:
        z, bonds = np.zeros((B, W), np.int32), np.zeros((B, W, W), np.int8)
    else:
        g = np.random.default_rng(junk_seed)
        z = g.integers(-3, 90, (B, W)).astype(np.int32)
        bonds = g.integers(-128, 128, (B, W, W)).astype(np.int8)
    for b, (zs, adj, n) in enumerate(mols):
        if n:
            z[b, :n] = zs
            diag = bonds[b, np.arange(n), np.arange(n)].copy()
            bonds[b, :n, :n] = np.asarray(adj, dtype=np.int8).reshape(n, n)
            if junk_seed is not None:
                bonds[b, np.arange(n), np.arange(n)] = diag
    return torch.from_numpy(z), torch.from_numpy(bonds), torch.tensor([m[2] for m in mols], dtype=torch.int32)


def _run(mols, W=None, junk_seed=None):
    """The kernel's (words [B,64] uint32, keys [B] Python ints, popcounts [B]) of `mols`."""
    from ml_conformer_generator_amd.fingerprint import graph_fingerprints
    z, bonds, n = _batch(mols, W, junk_seed)
    fp, key, pop = graph_fingerprints(z, bonds, n, DEV, check=junk_seed is None)
    assert fp.dtype == torch.int32 and key.dtype == torch.int64 and pop.dtype == torch.int32 and fp.is_cuda
    return (fp.cpu().numpy().view(np.uint32), [int(k) & U64 for k in key.cpu().tolist()], pop.cpu().tolist())


def _expected(mols):
    ref = [R.fingerprint_and_key(*m) for m in mols]
    return (np.array([R.words(b) for b, _ in ref], dtype=np.uint32).reshape(len(mols), 64), [k for _, k in ref],
            [len(b) for b, _ in ref])


def _assert_equal(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    assert got[1] == want[1], (what, [i for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:5])
    assert got[2] == want[2], what


# ----------------------------------------------------------------------------------------------- kernel vs restatement
def test_pinned_molecules():
    mols = [m for m, _, _ in C.PINNED.values()]
    words, keys, pops = _run(mols)
    for b, (name, (_, bits, key)) in enumerate(C.PINNED.items()):
        assert sorted(k for k in range(2048) if words[b, k >> 5] >> (k & 31) & 1) == bits, name
        assert keys[b] == key, name
        assert pops[b] == len(bits), name
    _assert_equal((words, keys, pops), _expected(mols), "pinned")


def test_molecule_like_graphs_match_the_restatement_bit_for_bit():
    mols = C.molecule_like_set()
    assert len(mols) >= 500 and {m[2] for m in mols} == set(range(1, 43))
    _assert_equal(_run(mols), _expected(mols), "molecule-like")


@pytest.mark.parametrize("n", [42, 64])
def test_dense_junk_graphs_match_the_restatement(n):
    rng = random.Random(4200 + n)
    mols = [C.junk_graph(rng, n) for _ in range(50)]
    assert min(sum(1 for c in row if c) for m in mols for row in m[1]) > 4            # far denser than any molecule
    _assert_equal(_run(mols), _expected(mols), f"junk {n}")


def test_tiny_molecules_and_a_batch_of_all_sizes():
    rng = random.Random(7)
    tiny = [R.mol([], []), R.mol([8], []), R.mol([6, 7], [(0, 1, 3)]), R.mol([6, 6], [])]
    _assert_equal(_run(tiny), _expected(tiny), "tiny")
    mixed = tiny + C.molecule_like_set(90, seed=99) + [C.junk_graph(rng, 64), C.junk_graph(rng, 42), R.mol([], [])]
    rng.shuffle(mixed)
    _assert_equal(_run(mixed), _expected(mixed), "mixed")


# ----------------------------------------------------------------------------------------------- same bits, always
def test_same_bits_whatever_numbering_row_batch_and_width():
    rng = random.Random(11)
    mols = C.molecule_like_set(300, seed=5)
    base = _run(mols)
    perm = _run([C.random_permutation(rng, m) for m in mols])
    _assert_equal(perm, base, "renumbered atoms")
    order = list(range(len(mols)))
    rng.shuffle(order)
    moved = _run([mols[i] for i in order])
    _assert_equal(moved, (base[0][order], [base[1][i] for i in order], [base[2][i] for i in order]), "other rows")
    for b in (0, 17, 299):
        alone = _run([mols[b]])
        _assert_equal(alone, (base[0][b:b + 1], base[1][b:b + 1], base[2][b:b + 1]), f"alone {b}")
    for W, seed in ((42, 1), (64, 2), (43, 3), (None, 4)):
        _assert_equal(_run(mols, W, junk_seed=seed), base, f"width {W} with junk padding")


def test_checked_call_refuses_bad_graphs():
    from ml_conformer_generator_amd.fingerprint import graph_fingerprints
    z, bonds, n = _batch([C.PINNED["ethanol"][0], C.PINNED["benzene"][0]])
    graph_fingerprints(z, bonds, n, DEV)
    for which, index, value in (("bonds", (0, 0, 1), 5), ("bonds", (0, 1, 0), -1), ("bonds", (1, 2, 4), 1),
                                ("z", (0, 1), 0)):
        zz, bb = z.clone(), bonds.clone()
        (bb if which == "bonds" else zz)[index] = value
        with pytest.raises(ValueError):
            graph_fingerprints(zz, bb, n, DEV)
    bonds[0, 0, 5] = 9                                       # in the padding of ethanol: ignored
    graph_fingerprints(z, bonds, n, DEV)
    with pytest.raises(ValueError):
        graph_fingerprints(z, bonds, torch.tensor([3, 7]), DEV)
    with pytest.raises(ValueError):
        graph_fingerprints(torch.zeros(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8),
                           torch.tensor([3]), DEV)


# ----------------------------------------------------------------------------------------------- Tanimoto
def _bit_sets(mols):
    return [R.fingerprint(*m) for m in mols]


def _expected_pair(sets):
    B = len(sets)
    out = np.empty((B, B), np.float32)
    for i in range(B):
        for j in range(B):
            out[i, j] = R.tanimoto(sets[i], sets[j])
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _torch_pair(fp):
    """The matrix from a torch formulation: bits unpacked to 0/1 fp32, F @ F.T (exact: counts <= 2 048), one division."""
    shifts = torch.arange(32, device=fp.device, dtype=torch.int32)
    bits = ((fp.unsqueeze(2) >> shifts) & 1).reshape(fp.shape[0], -1).to(torch.float32)
    c = bits @ bits.t()
    p = bits.sum(1)
    t = c / (p.view(-1, 1) + p.view(1, -1) - c)
    empty = p == 0
    t[empty, :] = float("nan")
    t[:, empty] = float("nan")
    return t


def test_tanimoto_of_the_pinned_pairs():
    from ml_conformer_generator_amd.fingerprint import fingerprint_tanimoto, graph_fingerprints
    names = ["ethanol", "dimethyl ether", "benzene", "pyridine"]
    fp, _, _ = graph_fingerprints(*_batch([C.PINNED[k][0] for k in names]), DEV)
    t = fingerprint_tanimoto(fp, fp[0]).cpu().numpy()
    assert t[0] == 1.0 and t[1] == np.float32(1) / np.float32(14)
    assert fingerprint_tanimoto(fp, fp[2]).cpu().numpy()[3] == np.float32(3) / np.float32(9)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 331])
def test_tanimoto_kernels_match_numpy_fp32_bit_for_bit(B):
    from ml_conformer_generator_amd.fingerprint import (fingerprint_tanimoto, graph_fingerprints,
                                                        pairwise_fingerprint_tanimoto)
    mols = C.molecule_like_set(B, seed=1000 + B)
    if B >= 63:
        mols[5] = mols[40] = R.mol([], [])                      # two molecules without atoms
        mols[7] = mols[50]                                      # and one duplicate
    sets = _bit_sets(mols)
    want = _expected_pair(sets)
    fp, _, _ = graph_fingerprints(*_batch(mols), DEV)
    pair = pairwise_fingerprint_tanimoto(fp)
    assert pair.shape == (B, B) and pair.dtype == torch.float32
    got = pair.cpu().numpy()
    assert _same_bits(got, want)
    assert _same_bits(got, got.T)
    live = [i for i, s in enumerate(sets) if s]
    assert all(got[i, i] == 1.0 for i in live)
    if B >= 63:
        assert np.isnan(got[5]).all() and np.isnan(got[:, 40]).all() and got[7, 50] == 1.0
        assert not np.isnan(got[np.ix_(live, live)]).any()
    assert _same_bits(_torch_pair(fp).cpu().numpy(), got)
    for r in sorted({0, B // 2, B - 1}):
        assert _same_bits(fingerprint_tanimoto(fp, fp[r]).cpu().numpy(), want[r]), r


def test_sentinels_around_the_outputs_stay_intact():
    from ml_conformer_generator_amd import _lib
    mols = C.molecule_like_set(131, seed=77)
    z, bonds, n = (t.to(DEV).contiguous() for t in _batch(mols))
    B, W, G = len(mols), z.shape[1], 256
    lib, stream = _lib.lib(), _lib.current_stream_ptr(DEV)
    fp = torch.full((G + B * 64 + G,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    key = torch.full((G + B + G,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    pop = torch.full((G + B + G,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    _lib.check(lib.mcg_graph_fingerprint(_lib.dptr(z), _lib.dptr(bonds), _lib.dptr(n), B, W, fp[G:].data_ptr(),
                                         key[G:].data_ptr(), pop[G:].data_ptr(), stream), "mcg_graph_fingerprint")
    want = _expected(mols)
    assert np.array_equal(fp[G:G + B * 64].cpu().numpy().view(np.uint32).reshape(B, 64), want[0])
    assert [int(k) & U64 for k in key[G:G + B].cpu().tolist()] == want[1]
    assert pop[G:G + B].cpu().tolist() == want[2]
    for t, size, fill in ((fp, B * 64, 0x5A5A5A5A), (key, B, 0x5A5A5A5A5A5A5A5A), (pop, B, 0x5A5A5A5A)):
        assert bool((t[:G] == fill).all()) and bool((t[G + size:] == fill).all())
    words = fp[G:G + B * 64].clone()
    for entry, size, call in (
            ("pair", B * B, lambda out: lib.mcg_fingerprint_pair_tanimoto(_lib.dptr(words), B, out, stream)),
            ("one", B, lambda out: lib.mcg_fingerprint_tanimoto(_lib.dptr(words), _lib.dptr(words), B, out, stream))):
        out = torch.full((G + size + G,), -7.0, device=DEV)
        _lib.check(call(out[G:].data_ptr()), entry)
        assert bool((out[:G] == -7.0).all()) and bool((out[G + size:] == -7.0).all()), entry
        assert not bool((out[G:G + size] == -7.0).any()), entry


# ----------------------------------------------------------------------------------------------- generation entries
def _record_graph(m):
    n = len(m.atomic_numbers)
    return list(m.atomic_numbers), [[int(v) for v in row] for row in m.bond_orders.tolist()], n


def _duplicated_shards(gen, inner):
    """`inner` (a `_generate_shard`) with the graphs of sample ids 3 and 7 overwritten by atom-permuted copies of sample
    1's: elements, bonds and atom count."""
    def run(*args):
        res = inner(*args)
        ids = torch.as_tensor(args[12] if len(args) > 12 and args[12] is not None else torch.arange(args[4])).tolist()
        if 1 not in ids:
            return res
        el, bond, n = res["elements"].clone(), res["bond"].clone(), res["n_nodes"].clone()
        src = ids.index(1)
        k = int(n[src])
        for sid in (3, 7):
            if sid in ids:
                b = ids.index(sid)
                p = torch.randperm(k, generator=torch.Generator().manual_seed(sid)).to(el.device)
                el[b], bond[b], n[b] = 0, 0, k
                el[b, :k] = el[src, :k][p]
                bond[b, :k, :k] = bond[src, :k, :k][p][:, p]
        return dict(res, elements=el, bond=bond, n_nodes=n)
    return run


def _fields(m):
    return (m.sample_id, m.atomic_numbers, m.coords.tolist(), m.bond_orders.tolist(), m.valid, m.shape_tanimoto)


def test_generation_chemical_scores_uniqueness_and_diversity(monkeypatch):
    from conftest import load_golden
    from test_shape_frames_gpu import SEED, _gen, _molecule_like_shards
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd.cheminformatics import select_diverse
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _duplicated_shards(gen, gen._generate_shard))
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen))      # coordinates follow the new atom counts
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"])
    kw = dict(reference_conformer=ref, n_samples=12, variance=2, optimise_geometry=False, sample_seed=SEED)

    plain = gen.generate_conformers(**kw)
    assert [m.sample_id for m in plain] == list(range(12))
    assert all(m.chemical_tanimoto is None and m.graph_key is None for m in plain)
    graphs = [_record_graph(m) for m in plain]
    assert R.key(*graphs[3]) == R.key(*graphs[1]) == R.key(*graphs[7]) and graphs[3][2] == graphs[1][2]
    keys = [R.key(*g) for g in graphs]
    sets = [R.fingerprint(*g) for g in graphs]
    dup = {i for i in range(12) if keys[i] in keys[:i]}
    assert {3, 7} <= dup

    # unique: the plain call minus the repeated graphs, nothing else changed
    uniq = gen.generate_conformers(unique=True, **kw)
    assert [m.sample_id for m in uniq] == [i for i in range(12) if i not in dup]
    for m in uniq:
        assert _fields(m) == _fields(plain[m.sample_id])
        assert m.graph_key == keys[m.sample_id] and m.chemical_tanimoto is None
    assert gen.generate_conformers_sharded(unique=True, **kw) == uniq
    assert [m.sample_id for m in gen.forward(unique=True, **kw)] == [m.sample_id for m in uniq]

    # with shape scores the best-scored copy survives
    scored = gen.generate_conformers(shape_scores=True, **kw)
    both = gen.generate_conformers(shape_scores=True, unique=True, **kw)
    by_id = {m.sample_id: m.shape_tanimoto for m in scored}
    best = min((1, 3, 7), key=lambda i: (-by_id[i] if by_id[i] == by_id[i] else float("inf"), i))
    assert [i for i in (1, 3, 7) if i in {m.sample_id for m in both}] == [best]
    assert [m.sample_id for m in both] == sorted(m.sample_id for m in both)      # a filter: sample order stays

    # chemical scores against record 5's graph
    chem = gen.generate_conformers(chemical_scores=True, reference_graph=plain[5], **kw)
    assert [m.sample_id for m in chem] == list(range(12))
    for m in chem:
        want = R.tanimoto(sets[m.sample_id], sets[5])
        assert np.float32(m.chemical_tanimoto).view(np.uint32) == want.view(np.uint32), m.sample_id
        assert m.graph_key == keys[m.sample_id]
        assert _fields(m) == _fields(plain[m.sample_id])
    assert chem[5].chemical_tanimoto == 1.0
    pair_ref = gen.generate_conformers(chemical_scores=True,
                                       reference_graph=(plain[5].atomic_numbers, plain[5].bond_orders), **kw)
    assert [m.chemical_tanimoto for m in pair_ref] == [m.chemical_tanimoto for m in chem]
    drop = gen.generate_conformers(max_chemical_tanimoto=1.0, reference_graph=plain[5], **kw)
    assert [m.sample_id for m in drop] == [i for i in range(12) if sets[i] != sets[5]]
    assert 5 not in [m.sample_id for m in drop]
    positive = sorted(m.chemical_tanimoto for m in chem if m.chemical_tanimoto > 0)
    t = positive[len(positive) // 2]
    some = gen.generate_conformers(max_chemical_tanimoto=t, reference_graph=plain[5], **kw)
    assert [m.sample_id for m in some] == [m.sample_id for m in chem if m.chemical_tanimoto < t]

    # chemical diversity: a host replay of the walk on the restatement's matrix
    matrix = _expected_pair(sets)
    off = np.sort(matrix[np.triu_indices(12, 1)])
    off = off[off > 0]
    for t in (1.0, float(off[len(off) // 2]), float(off[len(off) // 4])):
        div = gen.generate_conformers(max_pairwise_chemical_tanimoto=t, **kw)
        want = select_diverse([None] * 12, list(range(12)), None, None, chemical_pair=matrix,
                              max_pairwise_chemical_tanimoto=t)
        assert [m.sample_id for m in div] == want, t
        assert all(m.graph_key is None for m in div)
    assert 3 not in want and 7 not in want and len(want) < 12
    ranked = gen.generate_conformers(shape_scores=True, max_pairwise_chemical_tanimoto=t, top_k=4, **kw)
    order = [m.sample_id for m in scored]
    want = select_diverse([m.shape_tanimoto for m in scored], order, None, None, 4, None, matrix, t)
    assert [m.sample_id for m in ranked] == [order[i] for i in want]
    assert gen.generate_conformers_sharded(shape_scores=True, max_pairwise_chemical_tanimoto=t, top_k=4, **kw) == ranked

    # a call with none of the new arguments returns what it returned
    again = gen.generate_conformers(**kw)
    assert again == plain and [_fields(m) for m in again] == [_fields(m) for m in plain]
