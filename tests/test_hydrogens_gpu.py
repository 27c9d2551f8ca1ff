"""Explicit hydrogens on the MI355X (`mcg_hydrogens_place`, DESIGN.md section 6 "Explicit hydrogens"): the kernel against
the fp64 restatement `hydrogens_ref` on the fixtures of `hydrogens_cases` - integers exact, coordinates within a derived
1e-4 A - with the conditions under which fp32 and fp64 must decide alike asserted on the restatement; rigid motion; bit
identity whatever the batch, row and padded widths; sentinels round every output; and `add_hydrogens=True` through
`generate_conformers`.

The tolerance 1e-4 A is derived, not measured: the fixtures keep |coordinates| <= 16 A, where fp32 numbers are 1.9e-6
apart; every normalised sum has norm >= 0.2, which amplifies an error by at most 5; X-H is at most 1.5 A: a few 1e-5 A in
the worst case, and the tolerance is about 5 x that.  (Measured on the MI355X: DESIGN.md section 6.)"""
import numpy as np
import pytest
import torch

import hydrogens_cases as C
import hydrogens_ref as HR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 256
TOL = 1e-4


def _guarded(size, dtype, fill):
    return torch.full((GUARD + size + GUARD,), fill, dtype=dtype, device=DEV)


def _place(xyz, z, bonds, n, HW=None, rotors=True):
    """`mcg_pharm_perceive` + `mcg_hydrogens_place` through the C entry points, every output between sentinels.  Returns
    host tensors: coords [B,HW,3], parents [B,HW], counts [B,W], n_h [B], unplaced [B], rotor_delta [B,W]."""
    from ml_conformer_generator_amd import _lib
    x, zz, bb, nn = (torch.as_tensor(t).to(DEV).contiguous() for t in (xyz, z, bonds, n))
    B, N, W = int(x.shape[0]), int(x.shape[1]), int(bb.shape[1])
    HW = HW or max(4, 3 * W)
    types = torch.zeros(B, W, dtype=torch.uint8, device=DEV)
    rings = torch.zeros(B, 32, dtype=torch.int64, device=DEV)
    count = torch.zeros(B, dtype=torch.int32, device=DEV)
    L, stream = _lib.lib(), _lib.current_stream_ptr(DEV)
    _lib.check(L.mcg_pharm_perceive(_lib.dptr(zz), _lib.dptr(bb), _lib.dptr(nn), B, W, _lib.dptr(types), _lib.dptr(count),
                                    _lib.dptr(rings), stream), "mcg_pharm_perceive")
    F, I = float("nan"), 0x5A5A5A5A
    sizes = dict(coords=B * HW * 3, parents=B * HW, counts=B * W, n_h=B, unplaced=B, rotor_delta=B * W)
    buf = {k: _guarded(s, torch.float32 if k == "coords" else torch.int32, F if k == "coords" else I)
           for k, s in sizes.items()}
    ptr = {k: v[GUARD:].data_ptr() for k, v in buf.items()}
    _lib.check(L.mcg_hydrogens_place(_lib.dptr(x), _lib.dptr(zz), _lib.dptr(bb), _lib.dptr(nn), _lib.dptr(types),
                                     _lib.dptr(rings), _lib.dptr(count), B, N, W, HW, ptr["coords"], ptr["parents"],
                                     ptr["counts"], ptr["n_h"], ptr["unplaced"], ptr["rotor_delta"] if rotors else None,
                                     stream), "mcg_hydrogens_place")
    torch.cuda.synchronize()
    sentinel = torch.full((1,), F).view(torch.int32).item()
    for k, s in sizes.items():
        if k == "coords":
            t = buf[k].view(torch.int32)
            assert bool((t[:GUARD] == sentinel).all()) and bool((t[GUARD + s:] == sentinel).all()), k
        elif k == "rotor_delta" and not rotors:
            assert bool((buf[k] == I).all()), "an output that was not asked for was written"
        else:
            assert bool((buf[k][:GUARD] == I).all()) and bool((buf[k][GUARD + s:] == I).all()), k
    shape = dict(coords=(B, HW, 3), parents=(B, HW), counts=(B, W), n_h=(B,), unplaced=(B,), rotor_delta=(B, W))
    return {k: buf[k][GUARD: GUARD + s].cpu().reshape(shape[k]) for k, s in sizes.items()}


def _check_row(out, b, ref, n, name):
    """Row b of the kernel's outputs against a restatement result; returns the largest coordinate error."""
    h = ref["n_hydrogens"]
    assert int(out["n_h"][b]) == h, name
    assert int(out["unplaced"][b]) == ref["unplaced"], name
    assert out["counts"][b, :n].tolist() == ref["counts"] and not out["counts"][b, n:].any(), name
    assert out["rotor_delta"][b, :n].tolist() == ref["rotor_delta"] and bool((out["rotor_delta"][b, n:] == -1).all()), name
    h = max(h, 0)
    assert out["parents"][b, :h].tolist() == ref["parents"] and bool((out["parents"][b, h:] == -1).all()), name
    assert not out["coords"][b, h:].any(), name
    if h == 0:
        return 0.0
    err = float(np.abs(out["coords"][b, :h].numpy().astype(np.float64) - ref["coords"]).max())
    assert err <= TOL, (name, err)
    return err


def test_fixtures_meet_the_conditions_of_the_tolerance():
    """On the restatement alone, no case skipped: where these hold, fp32 and fp64 take every decision alike and the
    derivation of the tolerance applies."""
    f, ref = C.fixtures(), C.references()
    assert len(f) <= 31 and f["grown 64"]["mol"][2] == 64 and f["methane"]["mol"][2] == 1 and f["no atoms"]["mol"][2] == 0
    fallbacks = 0
    for name, r in ref.items():
        t = r["trace"]
        assert np.abs(f[name]["xyz"]).max(initial=0.0) <= 16.0, name
        assert all(v >= 0.2 for v in t["sums"]), (name, t["sums"])
        for v in t["tested"]:                     # no vector within a factor 10 of the 1e-3 degeneracy threshold ...
            assert v >= 1e-2 or (f[name]["degenerate"] and v < 1e-4), (name, v)      # ... but the ones written to be degenerate
            fallbacks += v < 1e-4
        assert all(g == 0.0 or g >= 1e-3 for g in t["perp_gaps"]), (name, t["perp_gaps"])
        for best, second in t["gaps"]:
            assert second - best >= 1e-3 or (best == 0.0 and second == 0.0), (name, best, second)
    assert fallbacks >= 4
    moved = [d for r in ref.values() for d in r["rotor_delta"] if d > 0]
    assert len(moved) >= 4                        # the scan decides something on these fixtures


def test_kernel_matches_the_restatement():
    f, ref = C.fixtures(), C.references()
    names = list(f)
    poisoned = dict(f["ethanol"], xyz=f["ethanol"]["xyz"].copy())
    poisoned["xyz"][1, 2] = np.nan
    items = [f[k] for k in names] + [poisoned]
    # W = 64 (every lane real in one row), N = 66 > W, junk in everything at or beyond a row's atoms
    xyz, z, bonds, n = C.pad_batch(items, 64, 66, garbage_seed=7)
    out = _place(xyz, z, bonds, n)
    worst = max(_check_row(out, b, ref[k], f[k]["mol"][2], k) for b, k in enumerate(names))
    print(f"HYDROGENS kernel vs fp64 restatement: max |dx| = {worst:.3e} A over "
          f"{sum(r['n_hydrogens'] for r in ref.values())} hydrogens of {len(names)} molecules")
    b = len(names)                                # the row with a NaN coordinate: -1, nothing else
    assert int(out["n_h"][b]) == -1 and int(out["unplaced"][b]) == 0
    assert not out["counts"][b].any() and bool((out["parents"][b] == -1).all()) and not out["coords"][b].any()
    assert bool((out["rotor_delta"][b] == -1).all())
    healthy = _place(*C.pad_batch([f[k] for k in names] + [f["ethanol"]], 64, 66, garbage_seed=7))
    for key in out:                               # the other rows do not notice it
        assert torch.equal(out[key][:b], healthy[key][:b]), key
    assert int(healthy["n_h"][b]) == 6
    # clean padding, the narrowest widths that hold the batch's largest small molecule, and no rotor output
    small = [k for k in names if f[k]["mol"][2] <= 7]
    tight = _place(*C.pad_batch([f[k] for k in small], 7, 7), rotors=False)
    for b2, k in enumerate(small):
        h = max(ref[k]["n_hydrogens"], 0)
        assert torch.equal(tight["coords"][b2, :h], out["coords"][names.index(k), :h]), k
        assert tight["parents"][b2, :h].tolist() == ref[k]["parents"], k


def test_rigid_motion_carries_the_hydrogens_along():
    """Only fixtures without a degenerate fallback: `perp` picks a coordinate axis and is deliberately not equivariant."""
    f, ref = C.fixtures(), C.references()
    names = [k for k in f if not ref[k]["trace"]["used_perp"] and not f[k]["degenerate"] and f[k]["mol"][2] > 1]
    assert "grown 64" in names and "acetamide" in names and len(names) >= 10
    rot, shift = C.MOTION
    assert abs(np.linalg.det(rot) - 1.0) < 1e-12
    moved = [dict(f[k], xyz=(f[k]["xyz"].astype(np.float64) @ rot.T + shift).astype(np.float32)) for k in names]
    a = _place(*C.pad_batch([f[k] for k in names], 64, 64))
    b = _place(*C.pad_batch(moved, 64, 64))
    for key in ("parents", "counts", "n_h", "unplaced", "rotor_delta"):
        assert torch.equal(a[key], b[key]), key
    worst = 0.0
    for r, k in enumerate(names):
        h = ref[k]["n_hydrogens"]
        want = a["coords"][r, :h].numpy().astype(np.float64) @ rot.T + shift
        worst = max(worst, float(np.abs(b["coords"][r, :h].numpy() - want).max()))
    print(f"HYDROGENS rigid motion: max |dx| = {worst:.3e} A")
    assert worst <= TOL


def test_same_bits_whatever_batch_row_and_padded_widths():
    f = C.fixtures()
    mol = C.grown(5, 20)
    others = [f[k] for k in ("phenol", "acetamide", "ethanol", "imidazole", "isobutane", "propyne", "benzene")]
    alone = _place(*C.pad_batch([mol], 20, 20))
    h = int(alone["n_h"][0])
    assert h >= 20
    crowd = _place(*C.pad_batch(others[:5] + [mol] + others[5:], 20, 20))
    wide = _place(*C.pad_batch([mol], 64, 64, garbage_seed=3))
    for got, row in ((crowd, 5), (wide, 0)):
        assert int(got["n_h"][row]) == h and int(got["unplaced"][row]) == int(alone["unplaced"][0])
        assert torch.equal(got["coords"][row, :h], alone["coords"][0, :h])
        assert torch.equal(got["parents"][row, :h], alone["parents"][0, :h])
        assert torch.equal(got["counts"][row, :20], alone["counts"][0]) and not got["counts"][row, 20:].any()
        assert torch.equal(got["rotor_delta"][row, :20], alone["rotor_delta"][0])
    assert torch.equal(wide["coords"][0, :h].view(torch.int32), alone["coords"][0, :h].view(torch.int32))


def test_python_layer():
    from ml_conformer_generator_amd import hydrogens as HY
    f, ref = C.fixtures(), C.references()
    names = [k for k in f if f[k]["mol"][2] <= 7]
    xyz, z, bonds, n = (torch.from_numpy(t) for t in C.pad_batch([f[k] for k in names], 7, 9))
    raw = _place(xyz, z, bonds, n)
    out = HY.add_hydrogens(xyz, z, bonds, n, DEV, return_rotors=True)
    hmax = max(ref[k]["n_hydrogens"] for k in names)
    assert tuple(out["coords"].shape) == (len(names), hmax, 3) and tuple(out["parents"].shape) == (len(names), hmax)
    assert out["coords"].is_cuda and out["parents"].dtype == torch.int32
    assert torch.equal(out["coords"].cpu(), raw["coords"][:, :hmax]) and torch.equal(out["parents"].cpu(), raw["parents"][:, :hmax])
    for key, mine in (("counts", "counts"), ("n_hydrogens", "n_h"), ("unplaced", "unplaced"), ("rotor_delta", "rotor_delta")):
        assert torch.equal(out[key].cpu(), raw[mine]), key
    assert "rotor_delta" not in HY.add_hydrogens(xyz, z, bonds, n, DEV)
    assert torch.equal(HY.implicit_counts(z, bonds, n).sum(1), (out["n_hydrogens"] + out["unplaced"]).cpu())
    empty = HY.add_hydrogens(xyz[:0], z[:0], bonds[:0], n[:0], DEV)
    assert tuple(empty["coords"].shape) == (0, 0, 3) and tuple(empty["counts"].shape) == (0, 7)
    bad = bonds.clone()
    bad[1, 0, 1] = bad[1, 1, 0] = 5                  # row 1: ethanol
    with pytest.raises(ValueError, match="codes"):
        HY.add_hydrogens(xyz, z, bad, n, DEV)
    iodine = z.clone()
    iodine[1, 0] = 53
    with pytest.raises(ValueError, match="covalent radius"):
        HY.add_hydrogens(xyz, iodine, bonds, n, DEV)
    assert names[1] == "ethanol"
    assert int(HY.add_hydrogens(xyz, iodine, bonds, n, DEV, check=False)["n_hydrogens"][0]) == ref[names[0]]["n_hydrogens"]


# ----------------------------------------------------------------------------------------------- generation entries
def _heavy(m):
    """The heavy-atom fields of a record, floats by their bits or their text (a NaN equals itself that way)."""
    return (m.sample_id, m.atomic_numbers, m.coords.contiguous().view(torch.int32).tolist(), m.bond_orders.tolist(), m.valid,
            repr(m.shape_tanimoto), repr(m.overlay_tanimoto),
            None if m.pose is None else (m.pose[0].tolist(), m.pose[1].tolist()),
            m.receptor_clashes, repr(m.receptor_max_overlap), m.to_molblock(), m.to_xyz_block())


def _own_hydrogens(mols):
    """`add_hydrogens` applied to each record's own returned coordinates and bonds, one molecule per call."""
    from ml_conformer_generator_amd import hydrogens as HY
    out = []
    for m in mols:
        n = len(m.atomic_numbers)
        out.append(HY.add_hydrogens(m.coords[None], torch.tensor([m.atomic_numbers], dtype=torch.int32), m.bond_orders[None],
                                    torch.tensor([n], dtype=torch.int32), DEV))
    return out


def _grown_shards(gen, nan_ids=()):
    """The generator's real `_generate_shard` (sampler, hand-off, GCN, write-back on the device) with each sample's
    coordinates, elements and bond codes replaced by a grown molecule of its own size, keyed on the sample id: the
    synthetic weights' own molecules are hundreds of angstroms wide and their bond codes leave no hydrogen to place.
    Sample ids in `nan_ids` get a non-finite coordinate."""
    real = gen._generate_shard

    def run(*args):
        res = real(*args)
        ids = args[12] if len(args) > 12 and args[12] is not None else torch.arange(args[4])
        n = res["n_nodes"].cpu().tolist()
        x, el, bond = torch.zeros(res["x"].shape), torch.zeros(res["elements"].shape, dtype=torch.int8), \
            torch.zeros(res["bond"].shape, dtype=torch.int8)
        for b, sid in enumerate(torch.as_tensor(ids).tolist()):
            fx = C.grown(1000 + sid, n[b])
            z, adj, k = fx["mol"]
            c = torch.from_numpy(fx["xyz"])
            x[b, :k] = c - c.mean(0)
            el[b, :k] = torch.tensor(z, dtype=torch.int8)
            bond[b, :k, :k] = torch.tensor(adj, dtype=torch.int8)
            if sid in nan_ids:
                x[b, 0, 0] = float("nan")
        return dict(res, x=x.to(res["x"].device), elements=el.to(res["elements"].device), bond=bond.to(res["bond"].device))
    return run


def _setup(monkeypatch):
    from conftest import load_golden
    from test_shape_frames_gpu import SEED, _gen
    from ml_conformer_generator_amd import conformer_generator as CG
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _grown_shards(gen, nan_ids=(3,)))
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"]) + torch.tensor([12.0, -5.0, 3.0])
    return gen, ref, dict(reference_conformer=ref, n_samples=8, variance=2, optimise_geometry=False, sample_seed=SEED)


def test_generation_with_add_hydrogens(monkeypatch):
    gen, ref, kw = _setup(monkeypatch)
    plain = gen.generate_conformers(**kw)
    assert all(m.hydrogen_coords is None and m.hydrogen_parents is None and m.hydrogens_unplaced is None
               and m.receptor_hydrogen_clashes is None for m in plain)
    full = gen.generate_conformers(add_hydrogens=True, **kw)
    assert [m.sample_id for m in full] == list(range(8))
    assert [_heavy(m) for m in full] == [_heavy(m) for m in plain]        # the heavy-atom fields: bit for bit
    placed = 0
    for m, own in zip(full, _own_hydrogens(full)):
        if m.sample_id == 3:                      # a non-finite coordinate: no hydrogens on the record
            assert int(own["n_hydrogens"][0]) == -1
            assert m.hydrogen_coords is None and m.hydrogen_parents is None and m.hydrogens_unplaced is None
            with pytest.raises(ValueError):
                m.to_molblock(hydrogens=True)
            continue
        h = int(own["n_hydrogens"][0])
        assert torch.equal(m.hydrogen_coords, own["coords"][0, :h].cpu()) and m.hydrogen_coords.dtype == torch.float32
        assert m.hydrogen_parents == own["parents"][0, :h].cpu().tolist() and m.hydrogens_unplaced == int(own["unplaced"][0])
        assert m.receptor_hydrogen_clashes is None
        assert m.to_molblock(hydrogens=True).count(" H  ") == h
        placed += h
    assert placed >= 40
    def everything(m):                            # (record equality would trip over the NaN of sample 3)
        h = m.hydrogen_coords
        return _heavy(m) + (None if h is None else h.contiguous().view(torch.int32).tolist(), m.hydrogen_parents,
                            m.hydrogens_unplaced, m.receptor_hydrogen_clashes)
    assert [everything(m) for m in gen.generate_conformers_sharded(add_hydrogens=True, **kw)] == [everything(m) for m in full]
    assert [everything(m) for m in gen.forward(add_hydrogens=True, **kw)] == [everything(m) for m in full]

    # posed, with a receptor: the hydrogens sit on the RETURNED (posed) coordinates and are counted against the receptor
    posed_kw = dict(kw, overlay=True)
    base = gen.generate_conformers(**posed_kw)
    pts = torch.cat([m.coords for m in base if m.pose is not None])
    lo, hi = pts.min(0).values.floor() - 1.0, pts.max(0).values.ceil() + 1.0
    axes = [torch.arange(float(lo[d]), float(hi[d]) + 0.5, 1.5) for d in range(3)]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    from ml_conformer_generator_amd import receptor as RC
    lattice = grid[torch.cdist(grid.double(), ref.double()).min(dim=1).values > RC.SELF_CONTACT + 0.5].float().contiguous()
    rec = (lattice, torch.full((lattice.shape[0],), 6))
    heavy_only = gen.generate_conformers(receptor=rec, **posed_kw)
    got = gen.generate_conformers(receptor=rec, add_hydrogens=True, **posed_kw)
    assert [_heavy(m) for m in got] == [_heavy(m) for m in heavy_only]
    y, ry = lattice.numpy(), np.float32(RC.vdw_radius(6))
    seen = 0
    for m, own in zip(got, _own_hydrogens(got)):
        if m.sample_id == 3:
            assert m.hydrogen_coords is None and m.receptor_hydrogen_clashes is None
            continue
        h = int(own["n_hydrogens"][0])
        assert torch.equal(m.hydrogen_coords, own["coords"][0, :h].cpu())
        if m.pose is None:
            assert m.receptor_hydrogen_clashes is None
            continue
        x = m.hydrogen_coords.numpy()
        count = 0
        for i in range(h):                        # the receptor kernel's own order of operations, in numpy fp32
            dx, dy, dz = x[i, 0] - y[:, 0], x[i, 1] - y[:, 1], x[i, 2] - y[:, 2]
            overlap = ((np.float32(1.20) + ry) - np.sqrt((dx * dx + dy * dy) + dz * dz)).max()
            count += bool(overlap >= np.float32(RC.CLASH_OVERLAP))
        assert m.receptor_hydrogen_clashes == count, m.sample_id
        seen += count
    assert seen >= 1
    print(f"HYDROGENS generation: {placed} hydrogens on 7 records; {seen} of the posed ones clash with the lattice")


def test_generation_on_the_decoders_own_output(monkeypatch):
    """The unsubstituted call: the synthetic weights' own coordinates, int8 elements and written-back bond codes, invalid
    rows kept.  Whatever the count rule finds there, each record carries exactly `add_hydrogens` of its own fields."""
    from test_shape_frames_gpu import SEED, _gen
    from ml_conformer_generator_amd import conformer_generator as CG
    gen = _gen()
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    kw = dict(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=20, n_samples=6, variance=2,
              optimise_geometry=False, sample_seed=SEED)
    plain = gen.generate_conformers(**kw)
    full = gen.generate_conformers(add_hydrogens=True, **kw)
    assert len(full) == 6 and [_heavy(m) for m in full] == [_heavy(m) for m in plain]
    for m, own in zip(full, _own_hydrogens(full)):
        h = int(own["n_hydrogens"][0])
        assert h >= 0 and isinstance(m.hydrogen_parents, list) and len(m.hydrogen_parents) == h
        assert m.hydrogen_parents == own["parents"][0, :h].cpu().tolist()
        assert tuple(m.hydrogen_coords.shape) == (h, 3) and torch.equal(m.hydrogen_coords, own["coords"][0, :h].cpu())
        assert m.hydrogens_unplaced == int(own["unplaced"][0])
        assert m.to_xyz_block(hydrogens=True).split("\n")[0] == str(len(m.atomic_numbers) + h)


def test_receptor_hydrogen_clashes_beyond_one_chunk_of_columns():
    """`postprocess.hydrogens` on a batch whose largest row has more than 64 hydrogens: the receptor kernel then runs over
    two chunks of hydrogen columns, the second one partly filled for one row and empty for the other."""
    from test_shape_frames_gpu import _gen
    from ml_conformer_generator_amd import postprocess
    from ml_conformer_generator_amd import receptor as RC
    f, ref = C.fixtures(), C.references()
    names = ["grown 64", "phenol", "ethanol"]
    xyz, z, bonds, n = (torch.from_numpy(t).to(DEV) for t in C.pad_batch([f[k] for k in names], 64, 64))
    assert ref["grown 64"]["n_hydrogens"] > 64
    pts = torch.from_numpy(f["grown 64"]["xyz"])
    lo, hi = pts.min(0).values.floor() - 2.0, pts.max(0).values.ceil() + 2.0
    axes = [torch.arange(float(lo[d]), float(hi[d]) + 0.5, 2.0) for d in range(3)]
    lattice = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).float().contiguous()
    rec = (lattice, torch.full((lattice.shape[0],), 6))
    pose = torch.zeros(3, 12)
    pose[2, 4] = float("nan")                     # the third row's pose failed
    req = postprocess.Request(add_hydrogens=True, overlay=True, receptor=rec)
    out = postprocess.hydrogens(_gen(), req, dict(x=xyz, elements=z.to(torch.int8), bond=bonds, n_nodes=n, pose=pose.to(DEV)))
    assert int(out["hydrogen_coords"].shape[1]) == ref["grown 64"]["n_hydrogens"] > 64
    y, ry = lattice.numpy(), np.float32(RC.vdw_radius(6))
    want = []
    for b, k in enumerate(names):
        x = out["hydrogen_coords"][b, : ref[k]["n_hydrogens"]].cpu().numpy()
        count = 0
        for i in range(x.shape[0]):
            dx, dy, dz = x[i, 0] - y[:, 0], x[i, 1] - y[:, 1], x[i, 2] - y[:, 2]
            count += bool(((np.float32(1.20) + ry) - np.sqrt((dx * dx + dy * dy) + dz * dz)).max() >= np.float32(RC.CLASH_OVERLAP))
        want.append(count)
    beyond = out["hydrogen_coords"][0, 64:].cpu().numpy()                    # clashes in the second chunk are counted too
    assert want[0] >= 8 and want[1] >= 1 and beyond.shape[0] >= 1
    assert out["receptor_hydrogen_clashes"].cpu().tolist() == [want[0], want[1], -1]
    assert out["hydrogens_unplaced"].cpu().tolist() == [ref[k]["unplaced"] for k in names]
