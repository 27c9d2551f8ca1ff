"""Standardised graphs on the MI355X (`mcg_standardize_graphs`, DESIGN.md section 6 "Standardised graphs"): the kernel
against the plain-Python restatement `standardize_ref` on the cases of `standardize_cases` - every output exact, the
coordinates by their bits, sentinels round every buffer, junk beyond every row's atoms and on the diagonal; bit identity
whatever the batch, row and padded widths; the Python layer and the C entry's refusals; and `standardize=True` through
the generation entries, with the cases' chemistry substituted at the sampler and write-back seams (the synthetic
weights write no chemistry).  No tolerance anywhere: every output is an integer or a copied float."""
import numpy as np
import pytest
import torch

import standardize_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 256
KEYS = ("coords", "z", "bonds", "kekule", "atom_map", "n_out", "n_fragments", "atoms_removed", "status")


def _shapes(B, N, W):
    return dict(coords=(B, N, 3), z=(B, W), bonds=(B, W, W), kekule=(B, W, W), atom_map=(B, W), n_out=(B,),
                n_fragments=(B,), atoms_removed=(B,), status=(B,))


def _dtype(key):
    return torch.int8 if key in ("bonds", "kekule") else torch.int32          # the coordinates travel as their bits


def _standardize(xyz, z, bonds, n):
    """`mcg_standardize_graphs` through the C entry point, every output between sentinels.  Host tensors by `KEYS`;
    `coords` is int32: the bit patterns."""
    from ml_conformer_generator_amd import _lib
    x, zz, bb, nn = (torch.as_tensor(t).to(DEV).contiguous() for t in (xyz, z, bonds, n))
    B, N, W = int(x.shape[0]), int(x.shape[1]), int(bb.shape[1])
    shapes = _shapes(B, N, W)
    fill = {torch.int8: 0x5A, torch.int32: 0x5A5A5A5A}
    buf = {k: torch.full((GUARD + int(np.prod(s)) + GUARD,), fill[_dtype(k)], dtype=_dtype(k), device=DEV)
           for k, s in shapes.items()}
    ptr = {k: v[GUARD:].data_ptr() for k, v in buf.items()}
    _lib.check(_lib.lib().mcg_standardize_graphs(
        _lib.dptr(x), _lib.dptr(zz), _lib.dptr(bb), _lib.dptr(nn), B, N, W, *(ptr[k] for k in KEYS),
        _lib.current_stream_ptr(DEV)), "mcg_standardize_graphs")
    torch.cuda.synchronize()
    out = {}
    for k, s in shapes.items():
        size = int(np.prod(s))
        assert bool((buf[k][:GUARD] == fill[_dtype(k)]).all()) and bool((buf[k][GUARD + size:] == fill[_dtype(k)]).all()), k
        out[k] = buf[k][GUARD: GUARD + size].cpu().reshape(s)
    return out


def _bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).view(torch.int32)


def _check_row(out, b, ref, xyz, name):
    """Row b of the kernel's outputs against a restatement result: every element of every output."""
    m = ref["n_out"]
    got = {k: int(out[k][b]) for k in ("n_out", "n_fragments", "atoms_removed", "status")}
    want = {k: ref[k] for k in got}
    assert got == want, (name, got, want)
    assert out["atom_map"][b, :m].tolist() == ref["atom_map"] and bool((out["atom_map"][b, m:] == -1).all()), name
    assert out["z"][b, :m].tolist() == ref["atomic_numbers"] and not out["z"][b, m:].any(), name
    for key, mine in (("bonds", "bond_orders"), ("kekule", "kekule_orders")):
        full = torch.zeros_like(out[key][b])
        if m:
            full[:m, :m] = torch.tensor(ref[mine], dtype=torch.int8).reshape(m, m)
        assert torch.equal(out[key][b], full), (name, key)
    want_x = torch.zeros_like(out["coords"][b])
    if m:
        want_x[:m] = _bits(xyz[ref["atom_map"]])
    assert torch.equal(out["coords"][b], want_x), name


@pytest.mark.parametrize("W,N", [(64, 66), (42, 42), (7, 9), (1, 1)])
def test_kernel_matches_the_restatement(W, N):
    cases, ref = C.cases(), C.references()
    names = [k for k in cases if cases[k]["mol"][2] <= min(W, N)]
    assert len(names) >= (len(cases) if W == 64 else 2) and len(names) <= 64
    for seed in (None, 7):                            # clean padding, then junk beyond every row's atoms and on the diagonal
        out = _standardize(*C.pad_batch([cases[k] for k in names], W, N, garbage_seed=seed))
        for b, k in enumerate(names):
            _check_row(out, b, ref[k], cases[k]["xyz"], k)
    if W == 64:
        status = {k: ref[k]["status"] for k in names}
        assert set(status.values()) == {0, 1, 2, 4, 8, 16}                        # every verdict is exercised
        print("STANDARDIZE kernel == restatement on", len(names), "graphs; Kekule steps up to",
              max(max(ref[k]["steps"], default=0) for k in names))


def test_same_bits_whatever_batch_row_and_padded_widths():
    cases = C.cases()
    probe = ["benzimidazole", "benzene and a bad fragment", "decacene", "N-methylpyridine", "aromatic biphenyl"]
    others = [cases[k] for k in ("indole", "two ethanes", "interleaved 64", "triangular 46 shuffled", "no atoms")]
    alone = {k: _standardize(*C.pad_batch([cases[k]], 42, 42)) for k in probe}
    crowd = _standardize(*C.pad_batch(others[:3] + [cases[k] for k in probe] + others[3:], 64, 66, garbage_seed=5))
    for i, k in enumerate(probe):
        a, row = alone[k], 3 + i
        for key in ("n_out", "n_fragments", "atoms_removed", "status"):
            assert int(crowd[key][row]) == int(a[key][0]), (k, key)
        for key in ("z", "atom_map"):
            assert torch.equal(crowd[key][row, :42], a[key][0]), (k, key)
        assert not crowd["z"][row, 42:].any() and bool((crowd["atom_map"][row, 42:] == -1).all())
        for key in ("bonds", "kekule"):
            assert torch.equal(crowd[key][row, :42, :42], a[key][0]), (k, key)
            assert not crowd[key][row, 42:].any() and not crowd[key][row, :, 42:].any()
        assert torch.equal(crowd["coords"][row, :42], a["coords"][0]) and not crowd["coords"][row, 42:].any()


def test_c_entry_refusals_launch_nothing():
    from ml_conformer_generator_amd import _lib
    L = _lib.lib()
    c = C.cases()["benzene"]
    x, z, b, n = (torch.from_numpy(t).to(DEV) for t in C.pad_batch([c], 7, 7))
    outs = {k: torch.full(s, 0x5A, dtype=_dtype(k), device=DEV) for k, s in _shapes(1, 7, 7).items()}
    stream = _lib.current_stream_ptr(DEV)

    def call(B=1, N=7, W=7, drop=None, inputs=(x, z, b, n)):
        ins = [None if drop == i else _lib.dptr(t) for i, t in enumerate(inputs)]
        ptrs = [None if drop == k else _lib.dptr(outs[k]) for k in KEYS]
        return L.mcg_standardize_graphs(*ins, B, N, W, *ptrs, stream)
    for kw in (dict(B=-1), dict(B=16385), dict(N=0), dict(W=0), dict(W=65), dict(drop=0), dict(drop=3),
               dict(drop="coords"), dict(drop="kekule"), dict(drop="status")):
        assert call(**kw) != 0, kw
        assert b"mcg_standardize_graphs" in L.mcg_last_error()
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in outs.values())                    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert int(outs["status"][0]) == 0 and int(outs["n_out"][0]) == 6


def test_python_layer():
    from ml_conformer_generator_amd import standardize as S
    cases = C.cases()
    names = [k for k in cases if cases[k]["mol"][2] <= 7]
    xyz, z, bonds, n = (torch.from_numpy(t) for t in C.pad_batch([cases[k] for k in names], 7, 9))
    raw = _standardize(xyz, z, bonds, n)
    out = S.standardize_graphs(xyz, z, bonds, n, DEV)
    assert set(out) == {"coords", "atomic_numbers", "bond_orders", "n_nodes", "kekule_orders", "atom_map", "n_fragments",
                        "atoms_removed", "status", "valid"}
    assert all(t.is_cuda for t in out.values()) and out["coords"].dtype == torch.float32
    assert out["bond_orders"].dtype == out["kekule_orders"].dtype == torch.int8 and out["valid"].dtype == torch.bool
    for mine, key in (("atomic_numbers", "z"), ("bond_orders", "bonds"), ("n_nodes", "n_out"), ("kekule_orders", "kekule"),
                      ("atom_map", "atom_map"), ("n_fragments", "n_fragments"), ("atoms_removed", "atoms_removed"),
                      ("status", "status")):
        assert out[mine].dtype == raw[key].dtype and torch.equal(out[mine].cpu(), raw[key]), mine
    assert torch.equal(out["coords"].cpu().view(torch.int32), raw["coords"])
    assert torch.equal(out["valid"].cpu(), raw["status"] == 0)
    wide = S.standardize_graphs(xyz, torch.cat([z, z], dim=1).long(), bonds.long(), n.long(), DEV)      # z wider than W; int64
    assert all(torch.equal(wide[k].view(torch.int32) if k == "coords" else wide[k],
                           out[k].view(torch.int32) if k == "coords" else out[k]) for k in out)      # (a NaN rides along)
    empty = S.standardize_graphs(xyz[:0], z[:0], bonds[:0], n[:0], DEV)
    assert tuple(empty["coords"].shape) == (0, 9, 3) and tuple(empty["kekule_orders"].shape) == (0, 7, 7)
    assert tuple(empty["valid"].shape) == (0,) and empty["atom_map"].dtype == torch.int32
    lopsided = bonds.clone()
    row = names.index("benzene")
    lopsided[row, 0, 1] = 1                           # [1, 0] stays 4
    with pytest.raises(ValueError, match="symmetric"):
        S.standardize_graphs(xyz, z, lopsided, n, DEV)
    unchecked = S.standardize_graphs(xyz, z, lopsided, n, DEV, check=False)       # read through the lower triangle
    assert torch.equal(unchecked["kekule_orders"], out["kekule_orders"])
    bad = bonds.clone()
    bad[row, 0, 1] = bad[row, 1, 0] = 5
    with pytest.raises(ValueError, match="codes"):
        S.standardize_graphs(xyz, z, bad, n, DEV)


# ----------------------------------------------------------------------------------------------- generation entries
ROWS = ["benzene", "pyridine", "pyrrole", "furan", "imidazole", "pyrazine", "2-pyridone", "naphthalene", "indole",
        "benzimidazole", "azulene", "cyclopentadienyl", "N-methylpyridine", "aromatic biphenyl", "benzene and water",
        "propane and ethanol", "two ethanes", "benzene and a bad fragment", "five-bonded carbon", "one atom"]
WIDTH = 16


def _substituted(monkeypatch, finish_all=False):
    """The shared generator with the cases' chemistry substituted at its seams (`composed_cases.substituted`), the rows at
    seeded Gaussian clouds: the coordinates play no part in the verdict.  Returns (generator, call keywords, the rows'
    full tensors on the host, the proxy's own flags for them)."""
    from composed_cases import substituted
    cases = C.cases()
    rng = np.random.RandomState(3)
    items = [dict(cases[k], xyz=(rng.standard_normal((cases[k]["mol"][2], 3)) * 2.5).astype(np.float32)) for k in ROWS]
    gen, full, proxy = substituted(monkeypatch, items, WIDTH, finish_all)
    kw = dict(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=20, n_samples=len(ROWS), variance=2,
              optimise_geometry=False)
    return gen, kw, full, proxy


def _handoff_kept(last_batch, full):
    """`last_batch` still holds what the hand-off wrote: every row's own atoms, unstandardised."""
    x, el = last_batch["x_ordered"].cpu(), last_batch["elements"].cpu()
    for b, n in enumerate(full["n"].tolist()):
        assert torch.equal(x[b, :n].contiguous().view(torch.int32), full["xyz"][b, :n].contiguous().view(torch.int32)), b
        assert el[b, :n].tolist() == full["z"][b, :n].tolist(), b


def _fields(m):
    k = m.kekule_bond_orders
    return (m.sample_id, m.atomic_numbers, m.coords.contiguous().view(torch.int32).tolist(), m.bond_orders.tolist(), m.valid,
            m.atoms_removed, m.n_fragments, m.atom_map, None if k is None else k.tolist())


def test_generation_with_standardize(monkeypatch):
    gen, kw, full, proxy = _substituted(monkeypatch)
    ref = {k: C.references()[k] for k in ROWS}
    want_std = [b for b, k in enumerate(ROWS) if ref[k]["status"] == 0]
    want_plain = [b for b, ok in enumerate(proxy) if ok]

    plain = gen.generate_conformers(**kw)
    assert [m.sample_id for m in plain] == want_plain                            # what the call returns today: the proxy's rows
    for m in plain:
        b, n = m.sample_id, int(full["n"][m.sample_id])
        assert m.atomic_numbers == full["z"][b, :n].tolist() and m.bond_orders.tolist() == full["bonds"][b, :n, :n].tolist()
        assert torch.equal(m.coords.view(torch.int32), full["xyz"][b, :n].view(torch.int32))
        assert m.atoms_removed is None and m.n_fragments is None and m.atom_map is None and m.kekule_bond_orders is None
        with pytest.raises(ValueError):
            m.to_molblock(kekulize=True)
    assert "standardized" not in gen.last_batch
    assert gen.last_valid_fraction == len(want_plain) / len(ROWS)

    std = gen.generate_conformers(standardize=True, **kw)
    assert [m.sample_id for m in std] == want_std                                # exactly the rows whose status is 0
    assert gen.last_valid_fraction == len(want_std) / len(ROWS)
    only_with, only_without = set(want_std) - set(want_plain), set(want_plain) - set(want_std)
    assert ROWS.index("benzene and water") in only_with and ROWS.index("naphthalene") in only_with
    assert ROWS.index("cyclopentadienyl") in only_without and ROWS.index("N-methylpyridine") in only_without
    for m in std:
        r, b = ref[ROWS[m.sample_id]], m.sample_id
        assert m.valid and m.atomic_numbers == r["atomic_numbers"] and m.bond_orders.tolist() == r["bond_orders"]
        assert m.atom_map == r["atom_map"] and m.atoms_removed == r["atoms_removed"] and m.n_fragments == r["n_fragments"]
        assert m.kekule_bond_orders.tolist() == r["kekule_orders"]
        assert torch.equal(m.coords.view(torch.int32), full["xyz"][b, r["atom_map"]].view(torch.int32))
        assert " 4  0\n" not in m.to_molblock(kekulize=True)
    lb = gen.last_batch                               # what the hand-off wrote stays; the stage's result is a key of its own
    _handoff_kept(lb, full)
    assert lb["standardized"]["status"].cpu().tolist() == [ref[k]["status"] for k in ROWS]
    assert lb["standardized"]["n_nodes"].cpu().tolist() == [ref[k]["n_out"] for k in ROWS]

    assert [_fields(m) for m in gen.generate_conformers_sharded(standardize=True, **kw)] == [_fields(m) for m in std]
    assert [_fields(m) for m in gen.forward(standardize=True, **kw)] == [_fields(m) for m in std]
    assert [_fields(m) for m in gen.generate_conformers_sharded(**kw)] == [_fields(m) for m in plain]


def test_generation_with_standardize_and_the_later_stages(monkeypatch):
    gen, kw, full, proxy = _substituted(monkeypatch)
    ref = {k: C.references()[k] for k in ROWS}
    with_h = gen.generate_conformers(standardize=True, add_hydrogens=True, **kw)
    by_name = {ROWS[m.sample_id]: m for m in with_h}
    for name in ("imidazole", "benzimidazole", "pyrrole", "indole", "benzene and water"):
        m = by_name[name]
        block = m.to_molblock(kekulize=True, hydrogens=True)                      # the two definitions agree on these
        assert block.count(" H  ") == len(m.hydrogen_parents) and " 4  0\n" not in block
        assert all(0 <= p < ref[name]["n_out"] for p in m.hydrogen_parents)       # placed on the parent fragment's atoms
    assert 0 in by_name["imidazole"].hydrogen_parents and 2 not in by_name["imidazole"].hydrogen_parents      # N0-H, not N2
    assert len(by_name["benzene and water"].hydrogen_parents) == 6                # the water went before the hydrogens came

    seen = []
    real_relax = gen._relax_coords
    monkeypatch.setattr(gen, "_relax_coords", lambda x, el, sym, ng, steps: (seen.append((ng.cpu().tolist(), el.cpu(), sym.cpu())),
                                                                            real_relax(x, el, sym, ng, steps))[1])
    relaxed = gen.generate_conformers(standardize=True, relax_geometry=8, **kw)
    assert len(seen) == 1 and seen[0][0] == [ref[k]["n_out"] for k in ROWS]       # the parent's atom counts, not the sampler's
    b = ROWS.index("propane and ethanol")
    assert seen[0][1][b, :3].tolist() == [6, 6, 8] and not seen[0][1][b, 3:].any() and not seen[0][2][b, 3:].any()
    assert [m.sample_id for m in relaxed] == [ROWS.index(k) for k in ROWS if ref[k]["status"] == 0]
    assert all(m.strain_after is not None and len(m.atomic_numbers) == ref[ROWS[m.sample_id]]["n_out"] for m in relaxed)
    _handoff_kept(gen.last_batch, full)


def test_generation_on_the_decoders_own_output(monkeypatch):
    """The unsubstituted call: whatever the synthetic weights write, the records of `standardize=True` are
    `standardize_graphs` of the tensors the hand-off and the write-back produced."""
    from test_shape_frames_gpu import SEED, _gen
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd import standardize as S
    from ml_conformer_generator_amd.handoff import bond_writeback_hip
    gen = _gen()
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    kw = dict(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=20, n_samples=6, variance=2,
              optimise_geometry=False, sample_seed=SEED)
    plain = gen.generate_conformers(**kw)
    got = gen.generate_conformers(standardize=True, **kw)
    lb = gen.last_batch
    assert len(got) == len(plain) == 6
    sym, _ = bond_writeback_hip(lb["bond"], lb["elements"], lb["n_nodes"])
    own = S.standardize_graphs(lb["x_ordered"], lb["elements"], sym, lb["n_nodes"], DEV, check=False)
    assert all(torch.equal(own[k].view(torch.int32) if k == "coords" else own[k],
                           lb["standardized"][k].view(torch.int32) if k == "coords" else lb["standardized"][k]) for k in own)
    own = {k: v.cpu() for k, v in own.items()}
    for b, (m, p) in enumerate(zip(got, plain)):
        n = int(own["n_nodes"][b])
        assert m.sample_id == b and m.valid == bool(own["valid"][b]) and len(m.atomic_numbers) == n
        assert m.atomic_numbers == own["atomic_numbers"][b, :n].tolist()
        assert torch.equal(m.coords.view(torch.int32), own["coords"][b, :n].view(torch.int32))
        assert torch.equal(m.bond_orders, own["bond_orders"][b, :n, :n])
        assert torch.equal(m.kekule_bond_orders, own["kekule_orders"][b, :n, :n])
        assert m.atom_map == own["atom_map"][b, :n].tolist() and m.atoms_removed == int(own["atoms_removed"][b])
        assert m.n_fragments == int(own["n_fragments"][b]) and m.atoms_removed == len(p.atomic_numbers) - n
        assert m.atomic_numbers == [p.atomic_numbers[a] for a in m.atom_map]       # the parent, cut out of today's record


def test_a_finisher_with_standardize_raises(monkeypatch):
    from test_shape_frames_gpu import _gen
    gen = _gen()
    kw = dict(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=20, n_samples=2, optimise_geometry=False)
    monkeypatch.setattr(gen, "finisher", "rdkit")
    with pytest.raises(ValueError, match="finisher"):
        gen.generate_conformers(standardize=True, **kw)
    with pytest.raises(ValueError, match="finisher"):
        gen.generate_conformers_sharded(standardize=True, **kw)
