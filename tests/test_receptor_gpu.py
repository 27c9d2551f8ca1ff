"""Receptor contacts on the MI355X (`mcg_receptor_overlap`, DESIGN.md section 6 "Receptor clashes"): the per-atom
overlap bit for bit against a numpy fp32 restatement in the same operation order across the kernel's tile and split
boundaries, bit identity whatever the batch, row, padded width, receptor order and split, padded and non-finite atoms,
and `receptor` / `max_receptor_clashes` through `generate_conformers` with synthetic receptors built around the posed
molecules of the same seeded call."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from ml_conformer_generator_amd import receptor as RC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x5EED_0000_2026_1016
ELEMENTS = (6, 7, 8, 9, 15, 16, 17, 35, 5, 26)          # incl. boron and an element off Bondi's table


def _restate(x, z, n, rec_xyz, rec_z):
    """The definition in numpy fp32, in the kernel's order: d = x_i - y_j, (dx*dx + dy*dy) + dz*dz, correctly rounded
    sqrt, (r_i + r_j) - sqrt; the maximum over the receptor.  -inf on padded atoms, NaN on a non-finite atom."""
    x = np.asarray(x, dtype=np.float32)
    ri = RC.vdw_radii(torch.as_tensor(z)).numpy()
    y = np.asarray(rec_xyz, dtype=np.float32)
    rj = RC.vdw_radii(torch.as_tensor(rec_z)).numpy()
    B, N = x.shape[0], x.shape[1]
    out = np.full((B, N), -np.inf, dtype=np.float32)
    for b in range(B):
        for i in range(int(n[b])):
            if not np.isfinite(x[b, i]).all():
                out[b, i] = np.nan
                continue
            dx, dy, dz = x[b, i, 0] - y[:, 0], x[b, i, 1] - y[:, 1], x[b, i, 2] - y[:, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            out[b, i] = ((ri[b, i] + rj) - np.sqrt(d2)).max()
    return out


def _cloud(R, B, N, seed):
    """A receptor of R atoms in a 12 A box with duplicated atoms (exact ties), and B ligands of up to N atoms placed on,
    next to and between receptor atoms (near contacts, zero distances) as well as at random."""
    g = np.random.default_rng(seed)
    rec = (g.random((R, 3)) * 12.0).astype(np.float32)
    if R > 4:
        rec[g.integers(0, R, R // 4)] = rec[g.integers(0, R, R // 4)]          # exact duplicates: ties
    rec_z = g.choice(ELEMENTS, R)
    n = g.integers(1, N + 1, B)
    n[0] = N
    x = (g.random((B, N, 3)) * 14.0 - 1.0).astype(np.float32)
    pick = g.integers(0, R, (B, N))
    near = g.random((B, N)) < 0.5
    x[near] = rec[pick[near]] + (g.normal(size=(int(near.sum()), 3)) * 0.05).astype(np.float32)
    on = g.random((B, N)) < 0.1
    x[on] = rec[pick[on]]                                                    # d = 0
    z = g.choice(ELEMENTS, (B, N))
    return x, z, n, rec, rec_z


def _run(x, z, n, rec, rec_z, splits=None):
    return RC.receptor_overlap((torch.as_tensor(rec), torch.as_tensor(rec_z)), torch.as_tensor(x),
                               torch.as_tensor(n, dtype=torch.int32), torch.as_tensor(z), DEV, splits=splits).cpu()


def _bits(t):
    return np.asarray(t, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("R", [1, 255, 256, 257, 4097])
def test_overlap_matches_the_fp32_restatement_bit_for_bit(R):
    x, z, n, rec, rec_z = _cloud(R, 9, 40, seed=R)
    want = _restate(x, z, n, rec, rec_z)
    for splits in (None, 1, 2, 3, 7, 256):
        got = _run(x, z, n, rec, rec_z, splits).numpy()
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"R={R} splits={splits}")
    real = np.arange(40)[None, :] < n[:, None]
    assert np.isneginf(want[~real]).all() and np.isfinite(want[real]).all()
    print(f"RECEPTOR R={R}: {int(real.sum())} atoms, {int((want[real] >= RC.CLASH_OVERLAP).sum())} clashing, "
          f"max overlap {float(want[real].max()):.3f}")


def test_overlap_bits_do_not_depend_on_batch_row_width_or_receptor_order():
    x, z, n, rec, rec_z = _cloud(1500, 12, 30, seed=7)
    base = _run(x, z, n, rec, rec_z).numpy()
    g = np.random.default_rng(3)
    perm = g.permutation(len(rec))
    np.testing.assert_array_equal(_bits(_run(x, z, n, rec[perm], rec_z[perm]).numpy()), _bits(base))
    for W in (41, 64):                                                       # wider padding, junk in the padded rows
        xw = np.full((12, W, 3), 5.0, dtype=np.float32)
        xw[:, :30] = x
        zw = np.full((12, W), 8)
        zw[:, :30] = z
        got = _run(xw, zw, n, rec, rec_z).numpy()
        np.testing.assert_array_equal(_bits(got[:, :30]), _bits(base))
        assert np.isneginf(got[:, 30:]).all()
    for b in (0, 5, 11):                                                     # alone, at the row it had and at another
        k = int(n[b])
        alone = _run(x[b:b + 1, :k], z[b:b + 1, :k], [k], rec, rec_z).numpy()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(base[b, :k]))
        rows = [(b + 1) % 12, b, (b + 7) % 12]                               # row b moved to row 1
        moved = _run(x[rows], z[rows], n[rows], rec, rec_z).numpy()
        np.testing.assert_array_equal(_bits(moved[1]), _bits(base[b]))
    big = np.concatenate([x] * 30)                                           # a batch that needs no split
    got = _run(big, np.concatenate([z] * 30), np.concatenate([n] * 30), rec, rec_z).numpy()
    np.testing.assert_array_equal(_bits(got), _bits(np.concatenate([base] * 30)))


def test_padded_and_non_finite_atoms():
    x, z, n, rec, rec_z = _cloud(700, 4, 20, seed=11)
    n = np.array([20, 7, 0, 13])
    base = _run(x, z, n, rec, rec_z).numpy()
    assert np.isneginf(base[1, 7:]).all() and np.isneginf(base[2]).all() and np.isfinite(base[0]).all()
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[3, 4, 1] = bad
        got = _run(xb, z, n, rec, rec_z).numpy()
        assert np.isnan(got[3, 4])
        keep = np.ones_like(got, dtype=bool)
        keep[3, 4] = False
        np.testing.assert_array_equal(_bits(got[keep]), _bits(base[keep]))
        np.testing.assert_array_equal(_bits(got), _bits(_restate(xb, z, n, rec, rec_z)))


# ----------------------------------------------------------------------------------------------- generation entries
def _posed_setup(monkeypatch):
    from ml_conformer_generator_amd import conformer_generator as CG
    from test_shape_frames_gpu import _gen, _molecule_like_shards
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen))
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"]) + torch.tensor([12.0, -5.0, 3.0])
    kw = dict(reference_conformer=ref, variance=2, optimise_geometry=False, sample_seed=SEED, n_samples=12, overlay=True)
    base = gen.generate_conformers(**kw)
    assert base and all(m.receptor_clashes is None for m in base)
    return gen, ref, kw, base


def _same(a, b):
    assert a.sample_id == b.sample_id and torch.equal(a.coords, b.coords)
    assert a.atomic_numbers == b.atomic_numbers and torch.equal(a.bond_orders, b.bond_orders)
    assert (a.overlay_tanimoto == b.overlay_tanimoto or (math.isnan(a.overlay_tanimoto)
                                                         and math.isnan(b.overlay_tanimoto)))
    assert (a.pose is None) == (b.pose is None)
    if a.pose is not None:
        assert torch.equal(a.pose[0], b.pose[0]) and torch.equal(a.pose[1], b.pose[1])


def test_generation_with_a_distant_shell_has_no_clashes(monkeypatch):
    gen, ref, kw, base = _posed_setup(monkeypatch)
    pts = torch.cat([ref.float()] + [m.coords for m in base if m.pose is not None]).double()
    c = pts.mean(0)
    radius = float((pts - c).norm(dim=1).max()) + 5.5
    k = torch.arange(2000, dtype=torch.float64) + 0.5                        # a Fibonacci sphere of 2 000 atoms
    phi, theta = torch.acos(1 - 2 * k / 2000), math.pi * (1 + 5 ** 0.5) * k
    shell = c + radius * torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi),
                                      torch.cos(phi)], dim=1)
    rec = (shell.float(), torch.full((2000,), 16))
    got = gen.generate_conformers(receptor=rec, **kw)
    assert len(got) == len(base)
    for a, b in zip(base, got):
        _same(a, b)
        if a.pose is None:
            assert b.receptor_clashes is None and b.receptor_max_overlap is None
        else:
            assert b.receptor_clashes == 0 and b.receptor_max_overlap < -1.0
    kept = gen.generate_conformers(receptor=rec, max_receptor_clashes=0, **kw)
    assert [m.sample_id for m in kept] == [m.sample_id for m in base if m.pose is not None]
    print(f"RECEPTOR shell: {len(got)} molecules, max overlap "
          f"{max(m.receptor_max_overlap for m in got if m.receptor_max_overlap is not None):.3f}")


def test_generation_inside_a_lattice_clashes_everywhere(monkeypatch):
    gen, ref, kw, base = _posed_setup(monkeypatch)
    posed = [m for m in base if m.pose is not None]
    pts = torch.cat([m.coords for m in posed])
    lo, hi = pts.min(0).values.floor(), pts.max(0).values.ceil()
    axes = [torch.arange(float(lo[d]), float(hi[d]) + 0.5, 1.0) for d in range(3)]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    clear = torch.cdist(grid.double(), ref.double()).min(dim=1).values > RC.SELF_CONTACT
    lattice = grid[clear].float().contiguous()
    assert 0 < lattice.shape[0] <= RC.MAX_RECEPTOR_ATOMS
    rec = (lattice, torch.full((lattice.shape[0],), 6))
    got = gen.generate_conformers(receptor=rec, **kw)
    assert [m.sample_id for m in got] == [m.sample_id for m in base]
    for a, b in zip(base, got):
        _same(a, b)
        if b.pose is None:
            assert b.receptor_clashes is None
            continue
        assert b.receptor_clashes >= 1
        want = _restate(b.coords[None].numpy(), np.array([b.atomic_numbers]), [len(b.atomic_numbers)],
                        lattice.numpy(), rec[1].numpy())[0]
        assert b.receptor_clashes == int((want >= np.float32(RC.CLASH_OVERLAP)).sum())
        assert b.receptor_max_overlap == float(want.max())
    assert gen.generate_conformers(receptor=rec, max_receptor_clashes=0, **kw) == []
    print(f"RECEPTOR lattice of {lattice.shape[0]} atoms: clashes per molecule "
          f"{[m.receptor_clashes for m in got]}")


def test_generation_refuses_a_receptor_holding_the_reference(monkeypatch):
    gen, ref, kw, base = _posed_setup(monkeypatch)
    xyz = torch.cat([ref.float() + torch.tensor([0.0, 0.0, 40.0]), ref.float()])    # a complex: the ligand included

    def no_device(*a, **k):
        raise AssertionError("device work started before the receptor was checked")
    monkeypatch.setattr(gen, "_generate_shard", no_device)
    for rec in ((xyz, torch.full((xyz.shape[0],), 6)), (xyz[:-1] + 0.0, torch.full((xyz.shape[0] - 1,), 7))):
        with pytest.raises(ValueError, match="contains the reference"):
            gen.generate_conformers(receptor=rec, **kw)
        with pytest.raises(ValueError, match="contains the reference"):
            gen.generate_conformers_sharded(receptor=rec, max_receptor_clashes=0, **kw)
