"""`mcg_canonical_order` on the device against the restatement (`canonical_ref`): the named cases and the kernel's edge
sizes in one launch and row by row, renumberings, a seeded fuzz, the leaf budget, and the feature's reason - cubane and
the Wagner graph through `postprocess.return_records` and the generation entries.  Integers and strings only: equal means
equal."""
import random
import time

import numpy as np
import pytest
import torch

import canonical_cases as C
import canonical_ref as R
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import canonical as CN
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import smiles as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                        # sentinel elements on either side of an output buffer
_MASK = 2 ** 64 - 1
_REF = {}


def _ref(name, mol):
    """The restatement's verdict on a named molecule, computed once."""
    if name not in _REF:
        out = R.canonical(*mol)
        out["key"] = R.key(*mol, out["order"]) if out["status"] == 0 else 0
        _REF[name] = out
    return _REF[name]


def _cases():
    named = {k: v[0] for k, v in C.NAMED.items()}
    return dict(named, **{"7 disjoint propanes": C.OVER_BUDGET}, **C.EDGES)


def _launch(z, bonds, n):
    """One `mcg_canonical_order` launch into buffers with sentinels on both sides: (order [B,W], status, leaves, key) as
    host lists; the sentinels are checked here."""
    B, W = int(bonds.shape[0]), int(bonds.shape[1])
    zd, bd, nd = z.to(DEV, torch.int32).contiguous(), bonds.to(DEV, torch.int8).contiguous(), n.to(DEV, torch.int32)
    bufs = [torch.full((B * W + 2 * GUARD,), -77, dtype=torch.int32, device=DEV),
            torch.full((B + 2 * GUARD,), -77, dtype=torch.int32, device=DEV),
            torch.full((B + 2 * GUARD,), -77, dtype=torch.int32, device=DEV),
            torch.full((B + 2 * GUARD,), -77, dtype=torch.int64, device=DEV)]
    views = [b[GUARD: b.numel() - GUARD] for b in bufs]
    _lib.check(_lib.lib().mcg_canonical_order(_lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nd), B, W, *[_lib.dptr(v) for v in views],
                                              _lib.current_stream_ptr(torch.device(DEV))), "mcg_canonical_order")
    torch.cuda.synchronize()
    for b in bufs:
        host = b.cpu()
        assert bool((host[:GUARD] == -77).all()) and bool((host[-GUARD:] == -77).all())
    order, status, leaves, key = (v.cpu() for v in views)
    return order.reshape(B, W).tolist(), status.tolist(), leaves.tolist(), [k & _MASK for k in key.tolist()]


def test_named_cases_in_one_launch_and_row_by_row():
    cases = _cases()
    names, mols = list(cases), list(cases.values())
    junk = random.Random(99)
    z, bonds, n = C.pad_batch(mols, 64, junk=junk)            # junk on the diagonal and in the padding
    order, status, leaves, key = _launch(z, bonds, n)
    clean = _launch(*C.pad_batch(mols, 64))
    assert (order, status, leaves, key) == clean
    for b, (name, mol) in enumerate(zip(names, mols)):
        ref = _ref(name, mol)
        assert (status[b], leaves[b], key[b]) == (ref["status"], ref["leaves"], ref["key"]), name
        assert order[b] == ref["order"] + [-1] * (64 - len(ref["order"])), name
        if name in C.NAMED:
            assert leaves[b] == C.NAMED[name][1] and status[b] == 0, name
    assert status[names.index("7 disjoint propanes")] == CN.STATUS_BUDGET and status[names.index("no atoms")] == CN.STATUS_EMPTY
    assert leaves[names.index("64 isolated atoms")] == 1 and leaves[names.index("64-atom chain")] == 2
    # one row at a time, at W = n and at W = 64, and at another batch row: every bit is the same
    for b, mol in enumerate(mols):
        k = mol[2]
        for width in sorted({max(k, 1), 64}):
            one = _launch(*C.pad_batch([mol], width, junk=junk))
            assert one[0][0][:k] == order[b][:k] and all(v == -1 for v in one[0][0][k:])
            assert (one[1][0], one[2][0], one[3][0]) == (status[b], leaves[b], key[b]), names[b]
        moved = _launch(*C.pad_batch([C.CUBE, C.WAGNER, mol], 64, junk=junk))
        assert moved[0][2] == order[b] and (moved[1][2], moved[2][2], moved[3][2]) == (status[b], leaves[b], key[b])


def test_public_entry_matches_the_raw_launch():
    cases = _cases()
    mols = list(cases.values())
    z, bonds, n = C.pad_batch(mols, 64)
    out = CN.canonical_order(z, bonds, n, DEV)
    raw = _launch(z, bonds, n)
    assert out["order"].dtype == torch.int32 and out["key"].dtype == torch.int64 and out["order"].is_cuda
    assert (out["order"].tolist(), out["status"].tolist(), out["leaves"].tolist(),
            [k & _MASK for k in out["key"].tolist()]) == raw
    ids = CN.identity_bytes(z, bonds, n, DEV)
    assert ids == [None if _ref(k, m)["status"] else R.identity_bytes(*m) for k, m in cases.items()]
    zc, bc = CN.canonical_graphs(z, bonds, n, DEV)
    for b, (name, mol) in enumerate(cases.items()):
        ref = _ref(name, mol)
        if ref["status"] == 0:
            want = R.permute(*mol, ref["order"])
            assert zc[b, : mol[2]].tolist() == want[0] and bc[b, : mol[2], : mol[2]].tolist() == want[1], name
        else:
            assert int(zc[b].abs().sum()) == 0 and int(bc[b].abs().sum()) == 0
    with pytest.raises(ValueError):
        CN.canonical_order(z, torch.full_like(bonds, 5), n, DEV)                  # check=True: a code outside 0..4
    empty = CN.canonical_order(torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0, 4, 4, dtype=torch.int8),
                               torch.zeros(0, dtype=torch.int32), DEV)
    assert empty["order"].shape == (0, 4) and empty["status"].numel() == 0


def test_every_case_under_renumbering_in_one_batch():
    cases = _cases()
    rng = random.Random(41)
    mols, owner = [], []
    for k, mol in enumerate(cases.values()):
        mols += [mol] + [C.renumbered(rng, mol) for _ in range(8)]
        owner += [k] * 9
    z, bonds, n = C.pad_batch(mols, 64)
    out = CN.canonical_order(z, bonds, n, DEV)
    ids = CN.identity_bytes(z, bonds, n, DEV, ordered=out)
    key, leaves, status = out["key"].tolist(), out["leaves"].tolist(), out["status"].tolist()
    for b, k in enumerate(owner):
        first = 9 * k
        assert (ids[b], key[b], leaves[b], status[b]) == (ids[first], key[first], leaves[first], status[first]), b
    good = [ids[9 * k] for k in range(len(cases)) if ids[9 * k] is not None]
    assert len(set(good)) == len(good) == len(cases) - 2                       # no atoms and the budget row have none


def test_fuzz_against_the_restatement():
    mols = C.fuzz_set()
    assert len(mols) == 256 and {m[2] for m in mols} == set(range(1, 25))
    refs = [R.canonical(*m) for m in mols]
    assert sum(1 for r in refs if r["leaves"] >= 2) >= 32                      # a real search on a good share of them
    assert all(max(sum(1 for c in row if c) for row in m[1]) <= 4 for m in mols)
    rng = random.Random(6)
    dense = [C.over_degree(rng) for _ in range(4)]
    z, bonds, n = C.pad_batch(mols + dense, 24)
    order, status, leaves, key = _launch(z, bonds, n)
    for b, (m, ref) in enumerate(zip(mols, refs)):
        assert (status[b], leaves[b]) == (ref["status"], ref["leaves"]), b
        assert order[b] == ref["order"] + [-1] * (24 - len(ref["order"])), b
        assert key[b] == (R.key(*m, ref["order"]) if ref["status"] == 0 else 0), b
    for b in range(256, 260):
        assert (status[b], leaves[b], key[b]) == (CN.STATUS_DEGREE, 0, 0) and set(order[b]) == {-1}


def test_leaf_budget():
    """Six disjoint propanes: 6! = 720 leaves, status 0.  Seven: 5 040 > 4 096, BUDGET.  Measured on an MI355X: the budget
    row alone takes about 105 ms (the six-propane row 17 ms), far inside a test's few seconds."""
    z, bonds, n = C.pad_batch([C.NAMED["6 disjoint propanes"][0], C.OVER_BUDGET])
    CN.canonical_order(z[:1], bonds[:1], n[:1], DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = CN.canonical_order(z[1:], bonds[1:], n[1:], DEV)
    torch.cuda.synchronize()
    print(f"over-budget row: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    assert out["status"].tolist() == [CN.STATUS_BUDGET] and out["leaves"].tolist() == [4096] == [CN.LEAF_BUDGET]
    assert set(out["order"][0].tolist()) == {-1} and out["key"].tolist() == [0]
    both = CN.canonical_order(z, bonds, n, DEV)
    assert both["status"].tolist() == [0, CN.STATUS_BUDGET] and both["leaves"].tolist() == [720, 4096]
    assert CN.identity_bytes(z, bonds, n, DEV, ordered=both)[1] is None


# ----------------------------------------------------------------------------------------------- the reason for the feature
def _crafted(mols):
    B = len(mols)
    z, bonds, n = C.pad_batch(mols, 42)
    x = torch.zeros(B, 42, 3)
    for b, m in enumerate(mols):
        x[b, : m[2], 0] = torch.arange(m[2]) * 1.5
    return dict(x=x.to(DEV), elements=z.to(DEV, torch.int64), bond=bonds.to(DEV), n_nodes=n.to(DEV),
                valid=torch.ones(B, dtype=torch.bool, device=DEV))


def test_cubane_twice_and_the_wagner_graph_through_return_records(monkeypatch):
    from test_shape_overlay_host import _shell_generator
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd import fingerprint as FP
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    gen = _shell_generator()
    gen.device = torch.device(DEV)
    mols = [C.CUBE, C.WAGNER, C.renumbered(random.Random(12), C.CUBE)]
    res = _crafted(mols)
    keys = FP.graph_fingerprints(res["elements"], res["bond"], res["n_nodes"], DEV)[1].tolist()
    assert keys[0] == keys[1] == keys[2] and keys[0] & _MASK == 0xb8f57617ecefa100    # the graph key sees one molecule

    def rows(**kw):
        req = postprocess.label_excluded(gen, postprocess.parse_request(gen, None, **kw))
        return postprocess.return_records(gen, req, res, None, False)
    assert [m.sample_id for m in rows(unique=True)] == [0]
    assert [m.sample_id for m in rows(unique="exact")] == [0, 1]
    assert [m.sample_id for m in rows(unique="exact", exclude_graphs=[C.CUBE[:2]])] == [1]
    got = rows(smiles=True)
    assert [m.sample_id for m in got] == [0, 1, 2]
    assert got[0].smiles == got[2].smiles == "C12C3C4C1C1C2C3C41" and got[1].smiles not in (None, got[0].smiles)
    assert R.identity_bytes(*R.read_smiles(got[2].smiles)[:3]) == R.identity_bytes(*C.CUBE)
    assert R.identity_bytes(*R.read_smiles(got[1].smiles)[:3]) == R.identity_bytes(*C.WAGNER)
    for m, mol in zip(got, mols):
        assert m.canonical_status == 0 and m.canonical_order == R.canonical(*mol)["order"]


def _check_against_the_host_stage(got):
    """Every record's order equals a direct `canonical_order` call on its own returned graph, its string `write_smiles`
    of that graph relabelled by its own order; how many records carry a string."""
    for m in got:
        z, bonds = m.atomic_numbers, m.bond_orders
        n = len(z)
        own = CN.canonical_order(torch.tensor([z], dtype=torch.int32), bonds.unsqueeze(0), torch.tensor([n]), DEV)
        assert m.canonical_status == int(own["status"][0])
        if m.canonical_status != 0:
            assert m.canonical_order is None and m.smiles is None
            continue
        assert m.canonical_order == own["order"][0, :n].tolist()
        if int(own["leaves"][0]) <= 64:                 # (a wide search takes the restatement seconds)
            assert m.canonical_order == R.canonical(z, bonds.tolist(), n)["order"]
        idx = torch.tensor(m.canonical_order)
        assert m.smiles == S.write_smiles([z[a] for a in m.canonical_order], bonds.index_select(0, idx).index_select(1, idx))
        assert R.identity_bytes(*R.read_smiles(m.smiles)[:3]) == R.identity_bytes(z, bonds.tolist(), n)
    return sum(1 for m in got if m.smiles)


def test_generation_entries_agree_with_the_host_stage(monkeypatch):
    """`smiles=True` through the three entries on the shared synthetic-weight generator: first on whatever graphs those
    weights write (dense: most are refused with DEGREE, which must match the direct call too), then with each sample's
    chemistry replaced by a grown, molecule-like graph (`test_hydrogens_gpu._grown_shards`)."""
    from conftest import load_golden
    from test_hydrogens_gpu import _grown_shards
    from test_shape_frames_gpu import SEED, _gen
    from ml_conformer_generator_amd import conformer_generator as CG
    gen = _gen()
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"])
    kw = dict(reference_conformer=ref, n_samples=8, variance=2, optimise_geometry=False, sample_seed=SEED)

    def fields(mols):
        return [(m.sample_id, m.canonical_status, m.canonical_order, m.smiles) for m in mols]
    for grown in (False, True):
        if grown:
            monkeypatch.setattr(gen, "_generate_shard", _grown_shards(gen))
        plain = gen.generate_conformers(**kw)
        assert all(m.smiles is None and m.canonical_order is None and m.canonical_status is None for m in plain)
        got = gen.generate_conformers(smiles=True, **kw)
        assert [m.sample_id for m in got] == list(range(8)) and all(a == m for a, m in zip(plain, got))
        written = _check_against_the_host_stage(got)
        assert written == 8 or not grown
        assert fields(gen.generate_conformers_sharded(smiles=True, **kw)) == fields(got)
        assert fields(gen.forward(smiles=True, **kw)) == fields(got)
    exact = gen.generate_conformers(unique="exact", smiles=True, **kw)
    strings = [m.smiles for m in exact]
    assert len(set(strings)) == len(strings) and set(strings) == {m.smiles for m in got}
    known = got[2]
    left = gen.generate_conformers(exclude_graphs=[known], smiles=True, **kw)
    assert known.smiles not in {m.smiles for m in left} and len(left) == sum(1 for m in got if m.smiles != known.smiles)
