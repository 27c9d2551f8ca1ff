"""`mcg_stereo_order` on the device against the fp64 restatement (`stereo_ref`): the named cases and the kernel's edge
sizes in one launch and row by row with sentinels and junk - NaN in the coordinates' padding -, renumberings under proper
rigid motions, a seeded fuzz whose coordinates stay away from the 0.1 threshold, and the feature's reason - an
enantiomer pair through the generation entries.  Integers, signs and strings only: equal means equal."""
import random

import pytest
import torch

import canonical_ref as R
import stereo_cases as SC
import stereo_ref as SR
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import canonical as CN
from ml_conformer_generator_amd import stereo as ST

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                        # sentinel elements on either side of an output buffer
_MASK = 2 ** 64 - 1
_REF = {}


def _ref(name, mol):
    """The restatement's verdict on a named molecule, computed once."""
    if name not in _REF:
        out = SR.stereo(*mol)
        ok = out["status"] == 0
        out["key"] = R.key(*mol[:3], out["order"]) if ok else 0
        out["stereo_key"] = SR.stereo_key(*mol[:3], out["order"], out["stereo"]) if ok else 0
        _REF[name] = out
    return _REF[name]


def _cases():
    named = {k: v[0] for k, v in SC.NAMED.items()}
    edges = {"no atoms": ([], [], 0, []), "one atom": ([8], [[0]], 1, [(0.5, 0.25, -1.0)]),
             "two atoms": R.mol([6, 7], [(0, 1, 3)]) + ([(0.0, 0.0, 0.0), (1.2, 0.0, 0.0)],),
             "64 atoms, lane 63 a neighbour of the centre": SC.sixty_four(), "its mirror image": SC.mirror(SC.sixty_four()),
             "nine neighbours": SC.over_degree(), "mirror CHFClBr": SC.mirror(SC.CHFCLBR),
             "trans-cyclooctene": SC.TRANS_CYCLOOCTENE, "2,3-dichlorobutane c": SC.DICHLOROBUTANES[2],
             "2,3-dichlorobutane d": SC.DICHLOROBUTANES[3]}
    return dict(named, **edges)


def _launch(x, z, bonds, n):
    """One `mcg_stereo_order` launch into buffers with sentinels on both sides: (order [B,W], status, leaves, key, stereo
    [B,W], stereo_key, counts [B,3]) as host lists; the sentinels are checked here."""
    B, W = int(bonds.shape[0]), int(bonds.shape[1])
    xd = x.to(DEV, torch.float32).contiguous()
    zd, bd, nd = z.to(DEV, torch.int32).contiguous(), bonds.to(DEV, torch.int8).contiguous(), n.to(DEV, torch.int32)
    shapes = [(B * W, torch.int32), (B, torch.int32), (B, torch.int32), (B, torch.int64), (B * W, torch.int8),
              (B, torch.int64), (B * 3, torch.int32)]
    bufs = [torch.full((size + 2 * GUARD,), -77, dtype=dtype, device=DEV) for size, dtype in shapes]
    views = [b[GUARD: b.numel() - GUARD] for b in bufs]
    _lib.check(_lib.lib().mcg_stereo_order(_lib.dptr(xd), _lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nd), B, W,
                                           *[_lib.dptr(v) for v in views], _lib.current_stream_ptr(torch.device(DEV))),
               "mcg_stereo_order")
    torch.cuda.synchronize()
    for b in bufs:
        host = b.cpu()
        assert bool((host[:GUARD] == -77).all()) and bool((host[-GUARD:] == -77).all())
    order, status, leaves, key, stereo, skey, counts = (v.cpu() for v in views)
    return (order.reshape(B, W).tolist(), status.tolist(), leaves.tolist(), [k & _MASK for k in key.tolist()],
            stereo.reshape(B, W).tolist(), [k & _MASK for k in skey.tolist()], counts.reshape(B, 3).tolist())


def _row(out, b):
    return tuple(part[b] for part in out)


def _expected(ref, W):
    k = len(ref["order"])
    return (ref["order"] + [-1] * (W - k), ref["status"], ref["leaves"], ref["key"],
            list(ref["stereo"] or ()) + [0] * (W - k), ref["stereo_key"], list(ref["counts"]))


def test_named_cases_in_one_launch_and_row_by_row():
    cases = _cases()
    names, mols = list(cases), list(cases.values())
    junk = random.Random(99)
    out = _launch(*SC.pad_batch(mols, 64, junk=junk))          # junk on the diagonal and in the padding, NaN coordinates
    assert out == _launch(*SC.pad_batch(mols, 64))
    graph = CN.canonical_order(*SC.pad_batch(mols, 64)[1:], DEV)
    for b, (name, mol) in enumerate(zip(names, mols)):
        ref = _ref(name, mol)
        assert _row(out, b) == _expected(ref, 64), name
        if name in SC.NAMED:
            assert (out[6][b], out[2][b]) == (list(SC.NAMED[name][1]), SC.NAMED[name][2]), name
        if ref["status"] == 0 and int(graph["status"][b]) == 0:
            assert out[3][b] == int(graph["key"][b]) & _MASK, name                # the graph key: the same certificate
    status = dict(zip(names, out[1]))
    assert status["no atoms"] == CN.STATUS_EMPTY and status["nine neighbours"] == CN.STATUS_DEGREE
    at = names.index("64 atoms, lane 63 a neighbour of the centre")
    assert out[6][at] == [1, 0, 0] and out[0][at] == out[0][at + 1]            # one graph, one order, the other hand:
    assert sorted(set(out[4][at]) | set(out[4][at + 1])) == [0, 4, 8] and len(set(out[4][at])) == 2
    # one row at a time, at W = n and at W = 64, and at another batch row: every bit is the same
    for b, mol in enumerate(mols):
        k = mol[2]
        for width in sorted({max(k, 1), 64}):
            one = _launch(*SC.pad_batch([mol], width, junk=junk))
            assert _row(one, 0) == _expected(_ref(names[b], mol), width), (names[b], width)
        moved = _launch(*SC.pad_batch([SC.CIS_DMCB, SC.CHFCLBR, mol], 64, junk=junk))
        assert _row(moved, 2) == _row(out, b), names[b]


def test_public_entry_matches_the_raw_launch():
    cases = _cases()
    mols = list(cases.values())
    x, z, bonds, n = SC.pad_batch(mols, 64)
    out = ST.stereo_order(x, z, bonds, n, DEV)
    raw = _launch(x, z, bonds, n)
    assert out["stereo"].dtype == torch.int8 and out["stereo_key"].dtype == torch.int64 and out["counts"].shape == (len(mols), 3)
    assert (out["order"].tolist(), out["status"].tolist(), out["leaves"].tolist(), [k & _MASK for k in out["key"].tolist()],
            out["stereo"].tolist(), [k & _MASK for k in out["stereo_key"].tolist()], out["counts"].tolist()) == raw
    ids = ST.stereo_identity_bytes(x, z, bonds, n, DEV, ordered=out)
    assert ids == [SR.identity_bytes(*m) for m in mols]
    for b, (name, mol) in enumerate(cases.items()):
        if ids[b] is not None:
            k = mol[2]
            own = ST.own_order_descriptors(out["order"][b, :k].tolist(), out["stereo"][b, :k].tolist(), bonds[b, :k, :k])
            assert own == SR.descriptors(SR.tetrahedral(*mol), SR.double_bonds(*mol), k, list(range(k))), name
    small = [SC.CHFCLBR, SC.BUTAN_2_OL, SC.TRANS_DCE]           # coordinates only as wide as the largest molecule
    xs, zs, bs, ns = SC.pad_batch(small, 42)
    narrow, wide = ST.stereo_order(xs[:, :5], zs, bs, ns, DEV), ST.stereo_order(xs, zs, bs, ns, DEV)
    assert all(torch.equal(narrow[k], wide[k]) for k in wide) and wide["counts"].tolist() == [[1, 0, 0], [1, 0, 0], [0, 1, 0]]
    with pytest.raises(ValueError):
        ST.stereo_order(x, z, torch.full_like(bonds, 5), n, DEV)                   # check=True: a code outside 0..4
    empty = ST.stereo_order(torch.zeros(0, 4, 3), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0, 4, 4, dtype=torch.int8),
                            torch.zeros(0, dtype=torch.int32), DEV)
    assert empty["stereo"].shape == (0, 4) and empty["counts"].shape == (0, 3)
    none = ST.stereo_order(torch.zeros(2, 0, 3), torch.zeros(2, 0, dtype=torch.int32), torch.zeros(2, 0, 0, dtype=torch.int8),
                           torch.zeros(2, dtype=torch.int32), DEV)
    assert none["status"].tolist() == [CN.STATUS_EMPTY] * 2 and none["stereo"].shape == (2, 0)


def test_every_case_under_renumbering_and_rigid_motion_in_one_batch():
    cases = _cases()
    rng = random.Random(41)
    mols, owner = [], []
    for k, mol in enumerate(cases.values()):
        mols += [mol] + [SC.moved(rng, SC.renumbered(rng, mol)) for _ in range(8)]
        owner += [k] * 9
    x, z, bonds, n = SC.pad_batch(mols, 64)
    out = ST.stereo_order(x, z, bonds, n, DEV)
    ids = ST.stereo_identity_bytes(x, z, bonds, n, DEV, ordered=out)
    cols = [out[k].tolist() for k in ("stereo", "stereo_key", "leaves", "status", "key", "counts")]
    for b, k in enumerate(owner):
        first = 9 * k
        assert ids[b] == ids[first] and all(c[b] == c[first] for c in cols), b
    good = {name: ids[9 * k] for k, name in enumerate(cases) if ids[9 * k] is not None}
    assert len(good) == len(cases) - 2                                          # no atoms and nine neighbours have none
    same = [{"2,3-dichlorobutane a", "2,3-dichlorobutane d"}]                   # the meso form, drawn twice
    for a in good:
        for b in good:
            if a < b:
                assert (good[a] == good[b]) == ({a, b} in same), (a, b)
    assert good["CHFClBr"] != good["mirror CHFClBr"] and good["2,3-dichlorobutane b"] != good["2,3-dichlorobutane c"]


def test_fuzz_against_the_restatement():
    mols = SC.fuzz_set()
    assert len(mols) == 256 and max(m[2] for m in mols) == 42 and min(m[2] for m in mols) == 1
    assert all(not (0.05 <= v <= 0.2) for m in mols for v in SR.margins(*m))    # no case skipped: all 256 qualify
    refs = [SR.stereo(*m) for m in mols]
    seen = [sum(r["counts"][k] for r in refs) for k in range(3)]
    assert min(seen) >= 32 and sum(1 for r in refs if r["leaves"] >= 2) >= 16, seen   # centres, double bonds, undefined
    junk = random.Random(8)
    out = _launch(*SC.pad_batch(mols, 42, junk=junk))
    for b, (m, ref) in enumerate(zip(mols, refs)):
        ok = ref["status"] == 0
        ref = dict(ref, key=R.key(*m[:3], ref["order"]) if ok else 0,
                   stereo_key=SR.stereo_key(*m[:3], ref["order"], ref["stereo"]) if ok else 0)
        assert _row(out, b) == _expected(ref, 42), b


def test_leaf_budget_is_the_graph_search_s():
    """Seven disjoint propanes: their ends are terminal twins, skipped here too, so the 7! = 5 040 orders of the propanes
    exceed the 4 096 leaves as in the graph search: BUDGET, nothing returned.  Six: 720 leaves, no candidate."""
    import canonical_cases as C
    rng = random.Random(3)
    mols = [m + ([tuple(rng.uniform(-4, 4) for _ in range(3)) for _ in range(m[2])],)
            for m in (C.NAMED["6 disjoint propanes"][0], C.OVER_BUDGET)]
    out = _launch(*SC.pad_batch(mols, 21, junk=rng))
    assert _row(out, 0)[1:3] == (0, 720) and out[6][0] == [0, 0, 0] and set(out[4][0]) == {0} and out[5][0] != 0
    assert _row(out, 1) == ([-1] * 21, CN.STATUS_BUDGET, CN.LEAF_BUDGET, 0, [0] * 21, 0, [0, 0, 0])


# ----------------------------------------------------------------------------------------------- the reason for the feature
def _planted_shards(gen, mols):
    """The generator's real `_generate_shard` with each sample's molecule replaced by the planted one of its sample id."""
    real = gen._generate_shard

    def run(*args):
        res = real(*args)
        ids = args[12] if len(args) > 12 and args[12] is not None else torch.arange(args[4])
        x, el = torch.zeros(res["x"].shape), torch.zeros(res["elements"].shape, dtype=res["elements"].dtype)
        bond, n = torch.zeros(res["bond"].shape, dtype=torch.int8), torch.zeros(res["n_nodes"].shape, dtype=res["n_nodes"].dtype)
        for b, sid in enumerate(torch.as_tensor(ids).tolist()):
            z, adj, k, xyz = mols[sid]
            x[b, :k] = torch.tensor(xyz, dtype=torch.float64).float()
            el[b, :k] = torch.tensor(z, dtype=el.dtype)
            bond[b, :k, :k] = torch.tensor(adj, dtype=torch.int8)
            n[b] = k
        dev = res["x"].device
        return dict(res, x=x.to(dev), elements=el.to(dev), bond=bond.to(dev), n_nodes=n.to(dev))
    return run


def test_an_enantiomer_pair_through_the_generation_entries(monkeypatch):
    from conftest import load_golden
    from test_shape_frames_gpu import SEED, _gen
    from ml_conformer_generator_amd import conformer_generator as CG
    rng = random.Random(21)
    mols = [SC.CHFCLBR, SC.mirror(SC.CHFCLBR), SC.moved(rng, SC.renumbered(rng, SC.CHFCLBR)), SC.BUTAN_2_OL, SC.CIS_DCE,
            SC.TRANS_DCE, SC.CIS_DMCB, SC.TRANS_DMCB]
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _planted_shards(gen, mols))
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"])
    kw = dict(reference_conformer=ref, n_samples=8, variance=2, optimise_geometry=False, sample_seed=SEED)

    def ids(got):
        return [m.sample_id for m in got]
    plain = gen.generate_conformers(smiles=True, **kw)
    got = gen.generate_conformers(smiles="isomeric", **kw)
    assert ids(got) == list(range(8))
    for a, m, mol in zip(plain, got, mols):
        assert a == m and (a.canonical_order, a.canonical_status, a.smiles) == \
            (m.canonical_order, m.canonical_status, m.to_smiles(isomeric=False))
        want = SR.stereo(*mol)
        n = mol[2]
        assert (m.stereo_status, m.stereo_order) == (0, want["order"])
        assert (m.n_stereo_defined, m.n_stereo_undefined) == (want["counts"][0] + want["counts"][1], want["counts"][2])
        assert m.stereo_descriptors == SR.descriptors(SR.tetrahedral(*mol), SR.double_bonds(*mol), n, list(range(n)))
        z, adj, _, tet, dbs = SR.read_isomeric(m.smiles)
        back = SR.stereo(z, adj, len(z), None, perceived=(tet, dbs))
        assert R.identity_bytes(z, adj, len(z)) + bytes(back["stereo"]) == SR.identity_bytes(*mol) and m.n_stereo_unmarked == 0
    assert got[0].smiles == got[2].smiles != got[1].smiles and plain[0].smiles == plain[1].smiles
    assert got[4].smiles != got[5].smiles and got[6].smiles != got[7].smiles

    def fields(rows):
        return [(m.sample_id, m.stereo_status, m.stereo_order, m.stereo_descriptors, m.smiles) for m in rows]
    assert fields(gen.generate_conformers_sharded(smiles="isomeric", **kw)) == fields(got)
    assert ids(gen.generate_conformers(unique="exact", **kw)) == [0, 3, 4, 6]
    assert ids(gen.generate_conformers(unique="stereo", **kw)) == [0, 1, 3, 4, 5, 6, 7]
    assert ids(gen.generate_conformers_sharded(unique="stereo", **kw)) == [0, 1, 3, 4, 5, 6, 7]
    both = gen.generate_conformers(unique="stereo", smiles="isomeric", **kw)
    assert len({m.smiles for m in both}) == len(both) == 7
