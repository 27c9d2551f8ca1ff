"""Pairwise shape Tanimoto on the MI355X (`mcg_shape_pair_tanimoto`): agreement with a CPU restatement on the same grid,
exact symmetry and diagonal, bit-identity whatever the batch, posed copies and the reference row against `shape_overlay`,
failing rows, and `max_pairwise_tanimoto` through `generate_conformers`.

These tests reach the kernel through `pairwise_shape_tanimoto` on the 40-point grid only, whose border is empty: n^3 = 64 000
is already a multiple of the kernel's k alignment (no padded column exists), and with a 9.6 A margin round the reference the
first and the last 32-point k-block of every wave's range add exactly 0 to every Gram entry.  The stages (densities, Gram
matrix, Tanimoto map) are pinned one by one on small full grids, at every tile-edge batch size and with guard words, in
`tests/test_shape_pair_stages_gpu.py`."""
import math

import pytest
import torch

from conftest import load_golden
from oracle.shape_oracle import density_on_grid

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x5EED_0000_2026_1016

# Tolerance against the fp64 restatement.  The device evaluates each density in fp32 with the hardware exponential
# (a few ulp per point) and sums 64 000 products per pair in fp32 (four k-ordered chains of 16 000, then a tree of
# two adds); the restatement maps the atoms and evaluates and sums everything in fp64.  A Tanimoto in [0, 1] carries
# that as an absolute error of a few 1e-6 in practice; the bound leaves two decades.
PAIR_ATOL = 2e-4
# The reference row against `overlay_tanimoto`: the same densities evaluated from the reference frame (overlay) or from
# the posed coordinates mapped back into it (here: y = (x - t_r) @ M_r, a few 1e-6 A apart), summed in another order.
REF_ROW_ATOL = 2e-4


def _pad(coord_list, N=None):
    N = N or max(int(c.shape[0]) for c in coord_list)
    x = torch.zeros(len(coord_list), N, 3)
    for b, c in enumerate(coord_list):
        x[b, : c.shape[0]] = torch.as_tensor(c, dtype=torch.float32)
    return x, torch.tensor([int(c.shape[0]) for c in coord_list], dtype=torch.int32)


def _walk(n, g, step=1.5, clearance=1.4):
    pts = [torch.zeros(3, dtype=torch.float64)]
    while len(pts) < n:
        d = torch.randn(3, generator=g, dtype=torch.float64)
        p = pts[-1] + d / d.norm() * step
        if min(float((p - q).norm()) for q in pts) >= clearance - 1e-9:
            pts.append(p)
    return torch.stack(pts).to(torch.float32)


def _reference():
    return load_golden("shape_quadrupole.npz")["xyz_ceyyag"].to(torch.float32)


def _molecules(ref, n_walks=10, seed=7):
    """The golden molecules and self-avoiding walks of 10..64 atoms, centred on the reference (so that they overlap its
    grid), each slightly moved so that no two are copies."""
    g = load_golden("shape_quadrupole.npz")
    gen = torch.Generator().manual_seed(seed)
    mols = [g[f"xyz_{k}"].to(torch.float32) for k in ("ceyyag", "yibfeu", "paba", "crown_6", "walk12", "walk27")]
    mols += [_walk(int(torch.randint(10, 65, (1,), generator=gen)), gen) for _ in range(n_walks)]
    centre = ref.mean(0)
    out = []
    for m in mols:
        shift = (torch.rand(3, generator=gen) - 0.5) * 1.0
        out.append(m - m.mean(0) + centre + shift)
    return out


def _restated(ref, coord_list):
    """T [B,B] in fp64 on the grid of the reference's frame, from `density_on_grid`."""
    from ml_conformer_generator_amd.cheminformatics import ALPHA, AMPLITUDE, _grid_axes, shape_frames_hip
    xform = torch.empty(1, 12, device=DEV)
    _, frames = shape_frames_hip(ref.to(DEV).unsqueeze(0), torch.tensor([ref.shape[0]], dtype=torch.int32, device=DEV),
                                 DEV, centre_atoms=True, xform_out=xform)
    axes = _grid_axes(frames[0].cpu(), 40).double()
    xg, yg, zg = torch.meshgrid(axes[0], axes[1], axes[2], indexing="ij")
    pts = torch.stack([xg.flatten(), yg.flatten(), zg.flatten()], dim=-1)
    M, t = xform[0, :9].cpu().double().reshape(3, 3), xform[0, 9:].cpu().double()
    F = torch.stack([density_on_grid((c.double() - t) @ M, pts, ALPHA, AMPLITUDE) for c in coord_list])
    G = F @ F.T
    d = G.diagonal()
    return G / (d.view(-1, 1) + d.view(1, -1) - G)


def test_pair_matrix_matches_the_restatement():
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto
    ref = _reference()
    mols = _molecules(ref)
    want = _restated(ref, mols)
    assert float((want - torch.eye(len(mols), dtype=want.dtype)).max()) > 0.3    # real overlaps, not a matrix of zeros
    for N in (None, 64):                                          # ragged counts, tight and widest padding
        x, n = _pad(mols, N)
        got = pairwise_shape_tanimoto(ref, x, n, DEV).cpu().double()
        err = float((got - want).abs().max())
        print(f"SHAPE-DIVERSITY restatement B={len(mols)} N={x.shape[1]} max |err| {err:.2e}")
        assert err < PAIR_ATOL


def test_pair_matrix_is_symmetric_with_a_unit_diagonal():
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto
    ref = _reference()
    mols = _molecules(ref, n_walks=60, seed=11)                   # 66 molecules: tiles across and on the diagonal
    x, n = _pad(mols)
    T = pairwise_shape_tanimoto(ref, x, n, DEV).cpu()
    assert torch.equal(T, T.T)
    assert torch.equal(T.diagonal(), torch.ones(len(mols)))
    assert bool(((T >= 0) & (T <= 1)).all())


def test_every_entry_is_bit_identical_whatever_the_batch(monkeypatch):
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto
    ref = _reference()
    mols = _molecules(ref, n_walks=30, seed=3)
    x, n = _pad(mols)
    T = pairwise_shape_tanimoto(ref, x, n, DEV).cpu()
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(len(mols), generator=g)
    xp, np_ = _pad([mols[int(i)] for i in perm], 64)              # permuted and padded wider
    Tp = pairwise_shape_tanimoto(ref, xp, np_, DEV).cpu()
    assert torch.equal(Tp, T[perm][:, perm])
    others = _molecules(ref, n_walks=100, seed=99)                # extended: 106 + 36 rows, the block off the tile grid
    xe, ne = _pad(others[:50] + mols + others[50:])
    k = len(mols)
    for tile in ("1", "2", "4"):                                  # every Gram tile size the library can pick
        monkeypatch.setenv("MCG_SHAPE_PAIR_TILE", tile)
        Te = pairwise_shape_tanimoto(ref, xe, ne, DEV).cpu()
        assert torch.equal(Te[50:50 + k, 50:50 + k], T), tile
    monkeypatch.delenv("MCG_SHAPE_PAIR_TILE")
    for B in (1, 2, 17):                                          # and cut down
        xs, ns = _pad(mols[:B])
        assert torch.equal(pairwise_shape_tanimoto(ref, xs, ns, DEV).cpu(), T[:B, :B])


def _proper_rotation(g):
    q = torch.randn(4, generator=g, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def test_posed_copies_and_the_reference_row():
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto, shape_overlay
    ref = _reference()
    g = torch.Generator().manual_seed(17)
    copies = []
    for _ in range(6):                                            # rigidly moved copies of one molecule
        R, t = _proper_rotation(g), (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * 20.0
        copies.append((ref.double() @ R + t).to(torch.float32))
    x, n = _pad(copies + _molecules(ref, n_walks=8, seed=23))
    ov = shape_overlay(ref, x, n, DEV)
    posed = ov["coords"]
    xr, nr = _pad([ref] + [posed[b, : int(n[b])].cpu() for b in range(x.shape[0])])   # the reference as row 0
    T = pairwise_shape_tanimoto(ref, xr, nr, DEV).cpu()
    assert float(T[1:7, 1:7].min()) > 0.999                      # the posed copies coincide
    err = float((T[0, 1:].double() - ov["tanimoto"].cpu().double()).abs().max())
    print(f"SHAPE-DIVERSITY reference row vs overlay_tanimoto max |err| {err:.2e}")
    assert err < REF_ROW_ATOL


def test_a_failing_row_gives_nan_and_spares_the_others():
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto
    ref = _reference()
    mols = _molecules(ref, n_walks=12, seed=31)
    x, n = _pad(mols)
    T = pairwise_shape_tanimoto(ref, x, n, DEV).cpu()
    for bad, how in ((3, "nan"), (7, "inf"), (11, "empty")):
        xb, nb = x.clone(), n.clone()
        if how == "nan":
            xb[bad, 2, 1] = float("nan")
        elif how == "inf":
            xb[bad, 0, 0] = float("inf")
        else:
            nb[bad] = 0
        Tb = pairwise_shape_tanimoto(ref, xb, nb, DEV).cpu()
        assert bool(Tb[bad].isnan().all()) and bool(Tb[:, bad].isnan().all()), how
        keep = [i for i in range(len(mols)) if i != bad]
        assert torch.equal(Tb[keep][:, keep], T[keep][:, keep]), how


# ----------------------------------------------------------------------------------------------- generation entries
def test_generation_with_a_diverse_selection_end_to_end(monkeypatch):
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto, select_scored
    from test_shape_frames_gpu import _gen, _molecule_like_shards
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen))
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"])
    kw = dict(reference_conformer=ref, variance=2, optimise_geometry=False, sample_seed=SEED, n_samples=16,
              overlay=True)
    scored = gen.generate_conformers(shape_scores=True, **kw)
    scores, ids = [m.shape_tanimoto for m in scored], [m.sample_id for m in scored]
    x, n = _pad([m.coords for m in scored])
    P = pairwise_shape_tanimoto(ref, x, n, DEV).cpu()
    off = P[~torch.eye(len(scored), dtype=torch.bool)]
    t = float(off.median())                                       # a threshold that excludes about half of the pairs
    min_t = float(torch.tensor(scores).quantile(0.25))
    for top_k in (None, 5):
        got = gen.generate_conformers(max_pairwise_tanimoto=t, min_shape_tanimoto=min_t, top_k=top_k, **kw)
        got_ids = [m.sample_id for m in got]
        xg, ng = _pad([m.coords for m in got])
        Pg = pairwise_shape_tanimoto(ref, xg, ng, DEV).cpu()      # recomputed on the returned molecules alone
        assert bool((Pg[~torch.eye(len(got), dtype=torch.bool)] < t).all())
        if top_k is None:
            passed = select_scored(scores, ids, None, min_t)      # ranking order of the molecules above the threshold
            kept_pos = [ids.index(s) for s in got_ids]
            for rank, i in enumerate(passed):
                if ids[i] in got_ids:
                    continue
                above = [j for j in passed[:rank] if j in kept_pos]
                assert any(float(P[i, j]) >= t for j in above), ids[i]
            assert 0 < len(got) < len(passed)
            full = got_ids
        else:
            assert got_ids == full[:top_k]
    for top_k, min_t2 in ((4, None), (None, min_t), (6, min_t)):  # without it: exactly today's selection
        got = gen.generate_conformers(top_k=top_k, min_shape_tanimoto=min_t2, max_pairwise_tanimoto=None, **kw)
        assert [m.sample_id for m in got] == [ids[i] for i in select_scored(scores, ids, top_k, min_t2)]
    print(f"SHAPE-DIVERSITY e2e t={t:.4f} kept {full}")
    assert not math.isnan(t)
