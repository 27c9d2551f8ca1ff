"""`mcg_ring_scaffold` and `mcg_induced_subgraph` on the device against the restatement (`scaffold_ref`): the named cases
in one launch and row by row, a seeded fuzz, renumberings, the sub-graph entry in both modes, the scaffold identities,
and the feature's reason - `unique="scaffold"` and the record fields through `postprocess.return_records` and a generation
entry.  Integers, bytes and strings only: equal means equal."""
import random

import pytest
import torch

import canonical_cases as C
import canonical_ref as R
import scaffold_cases as SC
import scaffold_ref as SR
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import canonical as CN
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import scaffold as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                        # sentinel elements on either side of an output buffer
_MASK = 2 ** 64 - 1
_REF = {}


def _ref(name):
    """The restatement's verdict on a named molecule, computed once and never changed."""
    if name not in _REF:
        _REF[name] = SR.perceive(*SC.NAMED[name][0])
    return _REF[name]


def _guarded(shape_numel, dtype):
    return torch.full((shape_numel + 2 * GUARD,), -77, dtype=dtype, device=DEV)


def _check_guards(bufs):
    for b in bufs:
        host = b.cpu()
        assert bool((host[:GUARD] == -77).all()) and bool((host[-GUARD:] == -77).all())


def _launch(z, bonds, n):
    """One `mcg_ring_scaffold` launch into buffers with sentinels on both sides: per row a dict in `scaffold_ref.perceive`'s
    layout over the FULL width (fill included), as host lists; the sentinels are checked here."""
    B, W = int(bonds.shape[0]), int(bonds.shape[1])
    zd, bd, nd = z.to(DEV, torch.int32).contiguous(), bonds.to(DEV, torch.int8).contiguous(), n.to(DEV, torch.int32)
    bufs = [_guarded(B * W, torch.int64), _guarded(B * W, torch.int32), _guarded(B * W, torch.int32),
            _guarded(B * 4, torch.int64), _guarded(B * 8, torch.int32)]
    views = [b[GUARD: b.numel() - GUARD] for b in bufs]
    _lib.check(_lib.lib().mcg_ring_scaffold(_lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nd), B, W, *[_lib.dptr(v) for v in views],
                                            _lib.current_stream_ptr(torch.device(DEV))), "mcg_ring_scaffold")
    torch.cuda.synchronize()
    _check_guards(bufs)
    ring_nb, size, system, masks, counts = (v.cpu() for v in views)
    ring_nb = [[v & _MASK for v in row] for row in ring_nb.reshape(B, W).tolist()]
    masks = [[v & _MASK for v in row] for row in masks.reshape(B, 4).tolist()]
    return [dict(ring_nb=ring_nb[b], ring_size=size.reshape(B, W)[b].tolist(), ring_system=system.reshape(B, W)[b].tolist(),
                 masks=masks[b], counts=counts.reshape(B, 8)[b].tolist()) for b in range(B)]


def _widened(ref, W):
    """A restatement result with the kernel's documented fill beyond the molecule's atoms."""
    k = W - len(ref["ring_nb"])
    return dict(ref, ring_nb=ref["ring_nb"] + [0] * k, ring_size=ref["ring_size"] + [0] * k,
                ring_system=ref["ring_system"] + [-1] * k)


def _induced(z, bonds, n, mask, mode):
    """One `mcg_induced_subgraph` launch into guarded buffers: (z_out [B,W], bonds_out [B,W,W], n_out [B], map_out [B,W])."""
    B, W = int(bonds.shape[0]), int(bonds.shape[1])
    zd, bd, nd = z.to(DEV, torch.int32).contiguous(), bonds.to(DEV, torch.int8).contiguous(), n.to(DEV, torch.int32)
    md = torch.tensor([m - 2 ** 64 if m >= 2 ** 63 else m for m in mask], dtype=torch.int64, device=DEV)
    bufs = [_guarded(B * W, torch.int32), _guarded(B * W * W, torch.int8), _guarded(B, torch.int32),
            _guarded(B * W, torch.int32)]
    views = [b[GUARD: b.numel() - GUARD] for b in bufs]
    _lib.check(_lib.lib().mcg_induced_subgraph(_lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nd), _lib.dptr(md), mode, B, W,
                                               *[_lib.dptr(v) for v in views],
                                               _lib.current_stream_ptr(torch.device(DEV))), "mcg_induced_subgraph")
    torch.cuda.synchronize()
    _check_guards(bufs)
    zo, bo, no, mo = (v.cpu() for v in views)
    return zo.reshape(B, W).tolist(), bo.reshape(B, W, W).tolist(), no.tolist(), mo.reshape(B, W).tolist()


def test_named_cases_in_one_launch_and_row_by_row():
    names, mols = list(SC.NAMED), list(SC.molecules().values())
    junk = random.Random(99)
    got = _launch(*C.pad_batch(mols, 64, junk=junk))          # junk on the diagonal and in the padding
    assert got == _launch(*C.pad_batch(mols, 64))
    for b, name in enumerate(names):
        assert got[b] == _widened(_ref(name), 64), name
        assert got[b] == _widened(SC.expected(name), 64), name            # and the hand-written values
    # one row at a time, at W = n and at W = 64, and at another batch row: every bit is the same
    for b, mol in enumerate(mols):
        k = mol[2]
        for width in sorted({max(k, 1), 64}):
            one = _launch(*C.pad_batch([mol], width, junk=junk))[0]
            assert one == _widened(_ref(names[b]), width), (names[b], width)
        moved = _launch(*C.pad_batch([C.CUBE, C.WAGNER, mol], 64, junk=junk))
        assert moved[2] == got[b], names[b]


def test_fuzz_against_the_restatement():
    mols = SC.fuzz_set()
    assert len(mols) == 320 and {m[2] for m in mols} == set(range(1, 65))
    assert all(max(sum(1 for c in row if c) for row in m[1]) <= 4 for m in mols)
    refs = [SR.perceive(*m) for m in mols]
    assert sum(1 for r in refs if r["counts"][5] > 0) >= 16 and sum(1 for r in refs if r["counts"][0] > 1) >= 64
    got = _launch(*C.pad_batch(mols, 64, junk=random.Random(5)))
    for b, ref in enumerate(refs):
        assert got[b] == _widened(ref, 64), b


def test_every_case_under_renumbering_in_one_batch():
    rng = random.Random(41)
    mols, want = [], []
    for name, mol in SC.molecules().items():
        for _ in range(8):
            p = list(range(mol[2]))
            rng.shuffle(p)
            mols.append(R.permute(*mol, p))
            want.append(SR.permuted(_ref(name), p))
    got = _launch(*C.pad_batch(mols, 64))
    for b, ref in enumerate(want):
        assert got[b] == _widened(ref, 64), b
        assert got[b]["counts"] == _ref(list(SC.NAMED)[b // 8])["counts"]


def test_induced_subgraph_in_both_modes():
    names, mols = list(SC.NAMED), list(SC.molecules().values())
    rows, masks = [], []
    for name, mol in zip(names, mols):
        for m in _ref(name)["masks"] + [0, _MASK]:
            rows.append(mol)
            masks.append(m)
    junk = random.Random(17)
    z, bonds, n = C.pad_batch(rows, 64, junk=junk)
    for mode in (0, 1):
        zo, bo, no, mo = _induced(z, bonds, n, masks, mode)
        for b, (mol, m) in enumerate(zip(rows, masks)):
            sz, sadj, sn, keep = SR.induced(*mol, m, mode)
            assert no[b] == sn and mo[b] == keep + [-1] * (64 - sn) and zo[b] == sz + [0] * (64 - sn), (b, mode)
            want = [[sadj[i][j] if i < sn and j < sn else 0 for j in range(64)] for i in range(64)]
            assert bo[b] == want, (b, mode)
    # at W = n too: nothing is written past the row
    mol = SC.NAMED["benzophenone"][0]
    zo, bo, no, mo = _induced(*C.pad_batch([mol], mol[2], junk=junk), [_ref("benzophenone")["masks"][3]], 0)
    sz, sadj, sn, keep = SR.scaffold(*mol)
    assert (zo[0], no[0], mo[0]) == (sz, sn, keep) and sn == mol[2] and bo[0] == sadj


def test_public_entries_match_the_raw_launches():
    names, mols = list(SC.NAMED), list(SC.molecules().values())
    z, bonds, n = C.pad_batch(mols, 64)
    out = SF.ring_perception(z, bonds, n, DEV)
    raw = _launch(z, bonds, n)
    assert out["ring_nb"].dtype == torch.int64 and out["counts"].dtype == torch.int32 and out["masks"].is_cuda
    assert [[v & _MASK for v in row] for row in out["ring_nb"].tolist()] == [r["ring_nb"] for r in raw]
    assert out["ring_size"].tolist() == [r["ring_size"] for r in raw]
    assert out["ring_system"].tolist() == [r["ring_system"] for r in raw]
    assert [[v & _MASK for v in row] for row in out["masks"].tolist()] == [r["masks"] for r in raw]
    assert out["counts"].tolist() == [r["counts"] for r in raw]
    for generic in (False, True):
        found = SF.murcko_scaffolds(z, bonds, n, DEV, generic=generic)
        strings = SF.scaffold_smiles(z, bonds, n, DEV, generic=generic)
        for b, (name, mol) in enumerate(zip(names, mols)):
            sz, sadj, sn, keep = SR.scaffold(*mol, generic=generic)
            assert int(found["n"][b]) == sn and found["atom_map"][b, :sn].tolist() == keep, name
            assert found["atomic_numbers"][b, :sn].tolist() == sz and found["bond_orders"][b, :sn, :sn].tolist() == sadj
            if sn == 0:
                assert found["identity"][b] == SF.EMPTY_IDENTITY == (0, b"") and strings[b] == "", name
            else:
                assert found["identity"][b][1] == R.identity_bytes(sz, sadj, sn), name
                assert R.identity_bytes(*R.read_smiles(strings[b])[:3]) == R.identity_bytes(sz, sadj, sn), name
    with pytest.raises(ValueError):
        SF.ring_perception(z, torch.full_like(bonds, 5), n, DEV)                  # check=True: a code outside 0..4
    empty = SF.ring_perception(torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0, 4, 4, dtype=torch.int8),
                               torch.zeros(0, dtype=torch.int32), DEV)
    assert empty["ring_size"].shape == (0, 4) and empty["counts"].shape == (0, 8)


def test_scaffold_identities():
    mols = dict(toluene=SC.NAMED["toluene"][0], ethylbenzene=SC.ETHYLBENZENE, benzene=SC.NAMED["benzene"][0],
                pyridine=SC.PYRIDINE, cyclohexanone=SC.NAMED["cyclohexanone"][0], cyclohexane=SC.CYCLOHEXANE,
                butane=SC.NAMED["butane"][0], atom=SC.NAMED["one atom"][0])
    z, bonds, n = C.pad_batch(list(mols.values()), 16, junk=random.Random(3))
    sc = dict(zip(mols, SF.murcko_scaffolds(z, bonds, n, DEV, check=False)["identity"]))     # (junk on the diagonal)
    fw = dict(zip(mols, SF.murcko_scaffolds(z, bonds, n, DEV, generic=True, check=False)["identity"]))
    assert sc["toluene"] == sc["ethylbenzene"] == sc["benzene"] and sc["benzene"] is not None
    assert sc["pyridine"] != sc["benzene"] and fw["pyridine"] == fw["benzene"]
    assert sc["cyclohexanone"] != sc["cyclohexane"] and fw["cyclohexanone"] == fw["cyclohexane"]
    assert fw["benzene"] == fw["cyclohexane"]                        # the generic framework: carbon, code 1
    assert sc["butane"] == sc["atom"] == SF.EMPTY_IDENTITY == fw["butane"]
    for name, mol in mols.items():
        assert sc[name][1] == SR.identity(*mol) and fw[name][1] == SR.identity(*mol, generic=True), name
    groups = SF.group_by_scaffold(list(sc.values()))
    assert groups == [[0, 1, 2], [3], [4], [5], [6, 7]]


# ----------------------------------------------------------------------------------------------- the reason for the feature
_BATCH = ("toluene", "benzene", "benzophenone", "butane", "cyclohexanone", "diphenylmethane", "one atom", "naphthalene")


def _crafted(mols):
    B = len(mols)
    z, bonds, n = C.pad_batch(mols, 42)
    x = torch.zeros(B, 42, 3)
    for b, m in enumerate(mols):
        x[b, : m[2], 0] = torch.arange(m[2]) * 1.5
    return dict(x=x.to(DEV), elements=z.to(DEV, torch.int64), bond=bonds.to(DEV), n_nodes=n.to(DEV),
                valid=torch.ones(B, dtype=torch.bool, device=DEV))


def _check_fields(m, mol, generic=False, smiles=False):
    ref = SR.perceive(*mol)
    sz, sadj, sn, keep = SR.scaffold(*mol, generic=generic, perceived=ref)
    assert (m.n_rings, m.n_ring_systems, m.min_ring_size, m.max_ring_size) == tuple(ref["counts"][:4])
    assert m.ring_sizes == ref["ring_size"] and m.ring_systems == ref["ring_system"] and m.scaffold_atoms == keep
    assert m.scaffold_status == (CN.STATUS_EMPTY if sn == 0 else 0)
    assert m.scaffold_key == (0 if sn == 0 else R.key(sz, sadj, sn, R.canonical(sz, sadj, sn)["order"]))
    if not smiles:
        assert m.scaffold_smiles is None
    elif sn == 0:
        assert m.scaffold_smiles == ""
    else:
        assert R.identity_bytes(*R.read_smiles(m.scaffold_smiles)[:3]) == R.identity_bytes(sz, sadj, sn)


def test_unique_scaffold_through_return_records(monkeypatch):
    from test_shape_overlay_host import _shell_generator
    from ml_conformer_generator_amd import conformer_generator as CG
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    gen = _shell_generator()
    gen.device = torch.device(DEV)
    mols = [SC.NAMED[k][0] for k in _BATCH]
    res = _crafted(mols)

    def rows(**kw):
        req = postprocess.label_excluded(gen, postprocess.parse_request(gen, None, **kw))
        return postprocess.return_records(gen, req, res, None, False)
    plain = rows()
    assert all(m.n_rings is None and m.scaffold_atoms is None and m.scaffold_key is None for m in plain)
    # toluene and benzene share benzene's scaffold; benzophenone keeps its C=O, diphenylmethane has none; butane and the
    # lone atom share the empty scaffold.  No score: the lowest sample id of each scaffold stays.
    got = rows(unique="scaffold")
    assert [m.sample_id for m in got] == [0, 2, 3, 4, 5, 7]
    for m in got:
        _check_fields(m, mols[m.sample_id])
    # at framework level benzophenone and diphenylmethane are one graph, and so are benzene and cyclohexanone's ring
    got = rows(unique="framework", smiles=True)
    assert [m.sample_id for m in got] == [0, 2, 3, 7]
    for m in got:
        _check_fields(m, mols[m.sample_id], generic=True, smiles=True)
        assert m.smiles is not None
    assert [m.sample_id for m in rows(unique="scaffold", exclude_graphs=[SC.NAMED["toluene"][0][:2]])] == [1, 2, 3, 4, 5, 7]
    annotated = SF.of_records(rows(), device=DEV)
    for m in annotated:
        _check_fields(m, mols[m.sample_id], smiles=True)


def test_composed_call_with_unique_scaffold(monkeypatch):
    """`unique="scaffold"` on top of the composed call of `test_composed_path_gpu` - every other option held fixed: the
    rows that remain are the best-ranked of each scaffold of the plain call's rows, they carry the restatement's fields
    for their own returned graph (with `standardize` the parent fragment's), and no bit of any other field changes; the
    other two entries return the same."""
    import test_composed_path_gpu as TC
    from ml_conformer_generator_amd import cheminformatics
    base = TC._call(monkeypatch, "all")
    got = TC._call(monkeypatch, "unique scaffold", unique="scaffold")
    by_id = {m.sample_id: m for m in base}
    assert all(m.n_rings is None and m.scaffold_atoms is None for m in base)
    ids = {m.sample_id: SR.identity(*TC._graph(m)) for m in base}
    seen, keep = set(), set()
    for m in sorted(base, key=lambda m: cheminformatics.ranking_key(m.shape_tanimoto, m.sample_id)):
        if ids[m.sample_id] not in seen:
            seen.add(ids[m.sample_id])
            keep.add(m.sample_id)
    assert [m.sample_id for m in got] == sorted(keep) and 2 < len(keep) < len(base)
    assert len(set(ids.values())) == len(keep) and b"" in seen               # acyclic rows collapse into one
    for m in got:
        assert TC._bits(m, without=SF._RECORD_FIELDS) == TC._bits(by_id[m.sample_id], without=SF._RECORD_FIELDS), m.sample_id
        _check_fields(m, TC._graph(m))
    for entry in ("generate_conformers_sharded", "forward"):
        again = TC._call(monkeypatch, "unique scaffold " + entry, entry=entry, unique="scaffold")
        assert [TC._bits(m) for m in again] == [TC._bits(m) for m in got], entry
