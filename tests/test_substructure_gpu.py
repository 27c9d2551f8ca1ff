"""`mcg_substructure_match` on the device against the restatement (`substructure_ref`): the named table and the kernel's
edge sizes in one launch and row by row, P = 1 / 64 / 65, renumberings, a seeded fuzz, the hydrogen input and the NULL
rule, the budget pair, and the options through `postprocess.return_records` and the generation entries.  Integers only:
equal means equal."""
import random

import pytest
import torch

import canonical_cases as C
import substructure_cases as SC
import substructure_ref as R
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import hydrogens as HY
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import substructure as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                        # sentinel elements on either side of an output buffer
_MASK = 2 ** 64 - 1
_REF = {}


def _ref(mol, pattern, nh=None):
    """The restatement's verdict on (molecule, pattern), computed once: (count, status, first or None, covered mask)."""
    pattern = S.as_pattern(pattern)
    key = (tuple(mol[0]), tuple(map(tuple, mol[1])), pattern, None if nh is None else tuple(nh))
    if key not in _REF:
        out = SC.reference(mol, pattern, nh=nh)
        _REF[key] = (out["count"], out["status"], out["first"], R.covered_mask(out["covered"]))
    return _REF[key]


def _cases():
    return dict({k: v[0] for k, v in C.NAMED.items()}, **C.EDGES)


def _patterns():
    """The table's patterns (m = 32 among them) and patterns of one and two atoms."""
    return SC.TABLE_PATTERNS + ["[#6]", "O", "[#6;D3]", "C=C", "c:c", "*.*"]


def _launch(z, bonds, n, compiled, nh=None):
    """One `mcg_substructure_match` launch into buffers with sentinels on both sides: (count [B,P], status [B,P], first
    [B,P,M] in the caller's order, covered [B,P] unsigned) as host lists; the sentinels are checked here."""
    B, W, P = int(bonds.shape[0]), int(bonds.shape[1]), len(compiled.patterns)
    dev = torch.device(DEV)
    zd, bd, nd = z.to(dev, torch.int32).contiguous(), bonds.to(dev, torch.int8).contiguous(), n.to(dev, torch.int32)
    nhd = None if nh is None else nh.to(dev, torch.int32).contiguous()
    pn, pa, pb = compiled.pat_n.to(dev), compiled.pat_atoms.to(dev), compiled.pat_bonds.to(dev)
    bufs = [torch.full((B * P + 2 * GUARD,), -77, dtype=torch.int32, device=dev),
            torch.full((B * P + 2 * GUARD,), -77, dtype=torch.int32, device=dev),
            torch.full((B * P * 32 + 2 * GUARD,), -77, dtype=torch.int32, device=dev),
            torch.full((B * P + 2 * GUARD,), -77, dtype=torch.int64, device=dev)]
    views = [b[GUARD: b.numel() - GUARD] for b in bufs]
    _lib.check(_lib.lib().mcg_substructure_match(_lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nd), _lib.dptr(nhd), B, W,
                                                 _lib.dptr(pn), _lib.dptr(pa), _lib.dptr(pb), P,
                                                 *[_lib.dptr(v) for v in views], _lib.current_stream_ptr(dev)),
               "mcg_substructure_match")
    torch.cuda.synchronize()
    for b in bufs:
        host = b.cpu()
        assert bool((host[:GUARD] == -77).all()) and bool((host[-GUARD:] == -77).all())
    count, status, first, covered = views
    raw = first.reshape(B, P, 32).cpu()
    for p, pat in enumerate(compiled.patterns):                  # -1 beyond the pattern's atoms, in matching order too
        assert bool((raw[:, p, len(pat.atoms):] == -1).all())
    first = S.first_in_caller_order(first.reshape(B, P, 32), compiled).cpu()
    return (count.reshape(B, P).cpu().tolist(), status.reshape(B, P).cpu().tolist(), first.tolist(),
            [[v & _MASK for v in row] for row in covered.reshape(B, P).cpu().tolist()])


def _row(out, b):
    return tuple(part[b] for part in out)


def _expect(mol, compiled, nh=None):
    """One molecule's row of `_launch`'s result, by the restatement."""
    M = compiled.max_atoms
    refs = [_ref(mol, pat, nh) for pat in compiled.patterns]
    return ([r[0] for r in refs], [r[1] for r in refs],
            [([-1] * M if r[2] is None else r[2] + [-1] * (M - len(r[2]))) for r in refs], [r[3] for r in refs])


def test_named_cases_in_one_launch_and_row_by_row():
    cases = _cases()
    names, mols = list(cases), list(cases.values())
    compiled = S.compile_patterns(_patterns())
    assert {len(p.atoms) for p in compiled.patterns} >= {1, 2, 32}
    junk = random.Random(99)
    z, bonds, n = SC.pad_batch(mols, 64, junk=junk)              # junk on the diagonal and in the padding
    out = _launch(z, bonds, n, compiled)
    assert out == _launch(*SC.pad_batch(mols, 64), compiled)
    for b, mol in enumerate(mols):
        assert _row(out, b) == _expect(mol, compiled), names[b]
    for text, name, count, cov in SC.TABLE:                      # the numbers the definition pins
        b, p = names.index(name), compiled.patterns.index(S.parse(text))
        assert (out[0][b][p], out[1][b][p], bin(out[3][b][p]).count("1")) == (count, 0, cov), (text, name)
    empty = names.index("no atoms")
    assert set(out[0][empty]) == {0} and set(out[1][empty]) == {0} and set(out[3][empty]) == {0}
    # one row at a time, at W = n and at W = 64, and at another batch row: every bit is the same
    for b, mol in enumerate(mols):
        for width in sorted({max(mol[2], 1), 64}):
            assert _row(_launch(*SC.pad_batch([mol], width, junk=junk), compiled), 0) == _row(out, b), names[b]
        moved = _launch(*SC.pad_batch([C.CUBE, C.WAGNER, mol], 64, junk=junk), compiled)
        assert _row(moved, 2) == _row(out, b), names[b]


def test_public_entry_matches_the_raw_launch():
    mols = list(_cases().values())
    compiled = S.compile_patterns(_patterns())
    z, bonds, n = SC.pad_batch(mols, 64)
    got = S.match_substructures(z, bonds, n, _patterns(), device=DEV)
    assert got["count"].dtype == got["status"].dtype == got["first"].dtype == torch.int32 and got["count"].is_cuda
    assert got["covered"].dtype == torch.int64 and tuple(got["first"].shape) == (len(mols), len(_patterns()), 32)
    raw = _launch(z, bonds, n, compiled)
    assert (got["count"].tolist(), got["status"].tolist(), got["first"].tolist(),
            [[v & _MASK for v in row] for row in got["covered"].tolist()]) == raw
    again = S.match_substructures(z.to(DEV), bonds.to(DEV), n.to(DEV), compiled)
    assert all(torch.equal(got[k], again[k]) for k in got)
    with pytest.raises(ValueError):
        S.match_substructures(z, torch.full_like(bonds, 5), n, compiled, device=DEV)     # check=True: a code outside 0..4
    none = S.match_substructures(torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0, 4, 4, dtype=torch.int8),
                                 torch.zeros(0, dtype=torch.int32), ["CC"], device=DEV)
    assert tuple(none["count"].shape) == (0, 1) and tuple(none["first"].shape) == (0, 1, 2)
    bare = S.match_substructures(torch.zeros(2, 0, dtype=torch.int32), torch.zeros(2, 0, 0, dtype=torch.int8),
                                 torch.zeros(2, dtype=torch.int32), ["CC"], device=DEV)
    assert bare["count"].tolist() == [[0], [0]] and bare["status"].tolist() == [[0], [0]]


def test_one_pattern_64_patterns_and_65_through_the_chunking():
    rng = random.Random(5)
    patterns = SC.TABLE_PATTERNS[:4] + [SC.random_pattern(rng, 1 + k % 5) for k in range(61)]
    assert len(patterns) == 65
    mols = [C.NAMED[k][0] for k in ("naphthalene", "cube", "Wagner graph", "toluene")] + C.fuzz_set(28, seed=77)
    z, bonds, n = SC.pad_batch(mols)
    nh = HY.implicit_counts(z, bonds, n)
    all65 = S.match_substructures(z, bonds, n, patterns, hydrogens=nh, device=DEV)
    assert tuple(all65["count"].shape) == (32, 65) and tuple(all65["first"].shape) == (32, 65, 6)     # the largest: 6 atoms
    first64 = S.match_substructures(z, bonds, n, patterns[:64], hydrogens=nh, device=DEV)
    for key in all65:
        assert torch.equal(all65[key][:, :64], first64[key]), key
    for p in (0, 3, 17, 63, 64):                                # a pattern's results do not depend on the others
        one = S.match_substructures(z, bonds, n, [patterns[p]], hydrogens=nh, device=DEV)
        m = len(S.as_pattern(patterns[p]).atoms)
        assert torch.equal(one["count"][:, 0], all65["count"][:, p]) and torch.equal(one["status"][:, 0], all65["status"][:, p])
        assert torch.equal(one["covered"][:, 0], all65["covered"][:, p])
        assert torch.equal(one["first"][:, 0], all65["first"][:, p, :m]) and bool((all65["first"][:, p, m:] == -1).all())
    raw = _launch(z, bonds, n, S.compile_patterns(patterns[64:]), nh)             # the chunk of one
    assert raw[0] == all65["count"][:, 64:].tolist()
    for b, mol in enumerate(mols):                               # and against the restatement
        want = _ref(mol, patterns[64], nh[b, : mol[2]].tolist())
        assert (raw[0][b][0], raw[1][b][0], raw[3][b][0]) == (want[0], want[1], want[3])


def test_every_named_molecule_under_renumbering():
    rng = random.Random(31)
    compiled = S.compile_patterns(SC.TABLE_PATTERNS)
    base, mols = [], []
    for name in SC.TABLE_MOLECULES:
        base.append(SC.molecule(name))
        mols += [C.renumbered(rng, SC.molecule(name)) for _ in range(8)]
    out = _launch(*SC.pad_batch(base + mols, 64, junk=rng), compiled)
    for b, mol in enumerate(base + mols):
        origin = b if b < len(base) else (b - len(base)) // 8
        for p, pat in enumerate(compiled.patterns):
            want = _ref(mol, pat)
            assert (out[0][b][p], out[1][b][p]) == (out[0][origin][p], out[1][origin][p]) and out[1][b][p] == 0
            assert bin(out[3][b][p]).count("1") == bin(out[3][origin][p]).count("1")
            image = out[2][b][p][: len(pat.atoms)]
            if out[0][b][p] == 0:
                assert set(out[2][b][p]) == {-1}
            else:
                assert SC.is_embedding(mol, pat, image) and set(out[2][b][p][len(pat.atoms):]) <= {-1}
            assert (out[0][b][p], out[1][b][p], out[3][b][p]) == (want[0], want[1], want[3])
            assert want[2] is None or image == want[2]


def test_fuzz_against_the_restatement():
    mols = C.fuzz_set(256)
    patterns = SC.fuzz_patterns(16)
    compiled = S.compile_patterns(patterns)
    z, bonds, n = SC.pad_batch(mols, junk=random.Random(3))
    nh = HY.implicit_counts(z, bonds, n)
    out = _launch(z, bonds, n, compiled, nh)
    assert max(map(max, out[0])) > 0
    for b, mol in enumerate(mols):
        assert _row(out, b) == _expect(mol, compiled, nh[b, : mol[2]].tolist()), b
    public = S.match_substructures(z, bonds, n, compiled, device=DEV, check=False)    # `implicit_counts` inside; junk: unchecked
    assert public["count"].tolist() == out[0] and public["first"][:, :, : compiled.max_atoms].tolist() == out[2]
    null = _launch(z, bonds, n, compiled)                                     # the NULL rule
    for b, mol in enumerate(mols):
        assert _row(null, b) == _expect(mol, compiled), b


def test_hydrogen_input_and_the_null_rule():
    mols = [C.PYRROLE, SC.PYRIDINE, C.IMIDAZOLE_4_METHYL, C.NAMED["toluene"][0]]
    z, bonds, n = SC.pad_batch(mols, 9)
    nh = HY.implicit_counts(z, bonds, n)
    assert nh[0, 0] == 1 and nh[1, 0] == 0 and sorted(nh[2, [0, 2]].tolist()) == [0, 1]
    patterns = ["[nH]", "[nH0]", "[CH3]", "[cH]", "[#6;H0]"]
    got = S.match_substructures(z, bonds, n, patterns, device=DEV)            # `implicit_counts` is passed: a pattern asks
    given = S.match_substructures(z, bonds, n, patterns, hydrogens=nh, device=DEV)
    assert all(torch.equal(got[k], given[k]) for k in got)
    assert got["count"][:, 0].tolist() == [1, 0, 1, 0]                        # pyrrole yes, pyridine no, one N of the two
    assert got["count"][:, 1].tolist() == [0, 1, 1, 0] and got["count"][:, 2].tolist() == [0, 0, 1, 1]
    for b, mol in enumerate(mols):
        for p, pat in enumerate(patterns):
            want = _ref(mol, pat, nh[b, : mol[2]].tolist())
            assert (int(got["count"][b, p]), int(got["covered"][b, p]) & _MASK) == (want[0], want[3])
    null = S.match_substructures(z, bonds, n, patterns, hydrogens=False, device=DEV)
    assert null["count"][:, 0].tolist() == [0, 0, 0, 0]                       # no aromatic N-H without the ring rule
    for b, mol in enumerate(mols):
        for p, pat in enumerate(patterns):
            assert int(null["count"][b, p]) == _ref(mol, pat)[0]
    odd = nh.clone()
    odd[3, 6] = 250                                                           # any value is compared as it is
    assert S.match_substructures(z, bonds, n, ["[CH3]", "[#6;H250]"], hydrogens=odd, device=DEV)["count"][3].tolist() == [0, 1]
    with pytest.raises(ValueError):
        S.match_substructures(z, bonds, n, patterns, hydrogens=nh[:2], device=DEV)


def test_budget_pair():
    mols = [C.BENZENE, SC.K12, C.renumbered(random.Random(2), SC.K12), C.CUBE]
    z, bonds, n = SC.pad_batch(mols)
    out = S.match_substructures(z, bonds, n, [SC.PATH6, SC.PATH7, SC.AROM6], device=DEV)
    assert out["status"].tolist() == [[0, 0, 0], [0, S.STATUS_BUDGET, 0], [0, S.STATUS_BUDGET, 0], [0, 0, 0]]
    assert out["count"][:, 0].tolist() == [12, SC.K12_PATH6_COUNT, SC.K12_PATH6_COUNT, _ref(C.CUBE, SC.PATH6)[0]]
    assert out["count"][1:3, 1].tolist() == [SC.K12_PATH7_COUNT] * 2          # the lower bound, by the restatement
    assert out["covered"][1:3].tolist() == [[4095, 4095, 0]] * 2 and out["count"][:, 2].tolist() == [12, 0, 0, 0]
    assert out["first"][1, 1, :7].tolist() == list(range(7)) and S.describe_status(out["status"][1, 1]) == "BUDGET"


# ----------------------------------------------------------------------------------------------- the options
def _crafted(mols):
    B = len(mols)
    z, bonds, n = C.pad_batch(mols, 42)
    x = torch.zeros(B, 42, 3)
    for b, m in enumerate(mols):
        x[b, : m[2], 0] = torch.arange(m[2]) * 1.5
    return dict(x=x.to(DEV), elements=z.to(DEV, torch.int64), bond=bonds.to(DEV), n_nodes=n.to(DEV),
                valid=torch.ones(B, dtype=torch.bool, device=DEV))


def test_cubane_and_the_wagner_graph_through_return_records(monkeypatch):
    """The feature's reason: one graph key, one fingerprint - and one pattern that tells them apart."""
    from test_shape_overlay_host import _shell_generator
    from ml_conformer_generator_amd import conformer_generator as CG
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    gen = _shell_generator()
    gen.device = torch.device(DEV)
    mols = [C.CUBE, C.WAGNER, C.NAMED["toluene"][0], C.NAMED["decalin"][0]]
    res = _crafted(mols)

    def rows(**kw):
        return postprocess.return_records(gen, postprocess.parse_request(gen, None, **kw), res, None, False)
    assert [m.sample_id for m in rows(require_substructures=[SC.ANY5])] == [1]
    assert [m.sample_id for m in rows(exclude_substructures=[SC.ANY5])] == [0, 2, 3]
    assert [m.sample_id for m in rows(require_substructures=[SC.ANY6], exclude_substructures=["c"])] == [0, 1, 3]
    got = rows(substructure_counts=[SC.ANY5, SC.ANY4, "Cc", S.from_graph(C.BENZENE[:2])])
    assert [m.sample_id for m in got] == [0, 1, 2, 3]
    assert [m.substructure_counts for m in got] == [[0, 48, 0, 0], [80, 32, 0, 0], [0, 0, 1, 12], [0, 0, 0, 0]]
    assert all(m.substructure_status == [0, 0, 0, 0] and len(m.substructure_patterns) == 4 for m in got)
    assert got[2].substructure_first[2] == [6, 0] and got[2].substructure_first[0] is None
    assert SC.is_embedding(mols[1], SC.ANY5, got[1].substructure_first[0])


def test_generation_entries_agree_with_a_direct_call(monkeypatch):
    """The three options through the three entries on the shared synthetic-weight generator, each sample's chemistry
    replaced by a grown, molecule-like graph (`test_hydrogens_gpu._grown_shards`): every record's counts equal a direct
    `match_substructures` call on its own returned graph, and the filters keep exactly the rows those counts name."""
    from conftest import load_golden
    from test_hydrogens_gpu import _grown_shards
    from test_shape_frames_gpu import SEED, _gen
    from ml_conformer_generator_amd import conformer_generator as CG
    gen = _gen()
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    monkeypatch.setattr(gen, "_generate_shard", _grown_shards(gen))
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"])
    kw = dict(reference_conformer=ref, n_samples=8, variance=2, optimise_geometry=False, sample_seed=SEED)
    patterns = ["[#6]~@[#6]", "[#6]~!@[#7,#8]", "[CH3]", SC.ANY6]
    plain = gen.generate_conformers(**kw)
    assert all(m.substructure_counts is None and m.substructure_patterns is None for m in plain)
    got = gen.generate_conformers(substructure_counts=patterns, **kw)
    assert [m.sample_id for m in got] == list(range(8)) and all(a == m for a, m in zip(plain, got))
    for m in got:
        z, bonds = m.atomic_numbers, m.bond_orders
        own = S.match_substructures(torch.tensor([z], dtype=torch.int32), bonds.unsqueeze(0), torch.tensor([len(z)]),
                                    patterns, device=DEV)
        assert m.substructure_counts == own["count"][0].tolist() and m.substructure_status == own["status"][0].tolist()
        for p, image in enumerate(m.substructure_first):
            assert (image is None) == (m.substructure_counts[p] == 0)
            assert image is None or SC.is_embedding((z, bonds.tolist(), len(z)), patterns[p], image,
                                                    HY.implicit_counts(torch.tensor([z]), bonds.unsqueeze(0),
                                                                       torch.tensor([len(z)]))[0].tolist())
    counts = {m.sample_id: m.substructure_counts for m in got}

    def fields(mols):
        return [(m.sample_id, m.substructure_counts, m.substructure_status, m.substructure_first) for m in mols]
    assert fields(gen.generate_conformers_sharded(substructure_counts=patterns, **kw)) == fields(got)
    assert fields(gen.forward(substructure_counts=patterns, **kw)) == fields(got)
    for p in range(len(patterns)):
        kept = [m.sample_id for m in gen.generate_conformers(require_substructures=[patterns[p]], **kw)]
        assert kept == [s for s in range(8) if counts[s][p] >= 1]
        left = [m.sample_id for m in gen.generate_conformers(exclude_substructures=[patterns[p]], **kw)]
        assert left == [s for s in range(8) if counts[s][p] == 0]
