"""Posing molecules onto the reference conformer on the MI355X (`mcg_shape_frames_tf`, `mcg_shape_overlay`): pose recovery
with and without a handedness flip, rigid proper poses, scores against the CPU oracle, bit-identity with
`mcg_shape_tanimoto`, batch invariance, a failing row, and `overlay=True` through the generation entries."""
import math

import pytest
import torch

from conftest import load_golden
from oracle.shape_oracle import tanimoto_score as oracle_tanimoto

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x5EED_0000_2026_1015


def _pad(coord_list, N=None):
    N = N or max(int(c.shape[0]) for c in coord_list)
    x = torch.zeros(len(coord_list), N, 3)
    for b, c in enumerate(coord_list):
        x[b, : c.shape[0]] = torch.as_tensor(c, dtype=torch.float32)
    return x, torch.tensor([int(c.shape[0]) for c in coord_list], dtype=torch.int32)


def _proper_rotation(g):
    q = torch.randn(4, generator=g, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def _separated_goldens():
    """The golden molecules whose principal moments differ by >= 1 % relative (a unique frame)."""
    g = load_golden("shape_quadrupole.npz")
    out = []
    for k in ("ceyyag", "yibfeu", "paba", "crown_6", "walk12", "walk27"):
        m = g[f"moments_{k}"].double()
        if min(float((m[0] - m[1]).abs() / m[0].abs()), float((m[1] - m[2]).abs() / m[1].abs())) >= 0.01:
            out.append((k, g[f"xyz_{k}"].to(torch.float32)))
    return out


def _copies(x, n_copies, seed):
    """Seeded proper rotations plus translations of up to +-20 A of x, and the transforms."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_copies):
        R = _proper_rotation(g)
        t = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * 20.0
        out.append(((x.double() @ R + t).to(torch.float32), R, t))
    return out


def _self_score(name, xyz):
    if name == "ceyyag":
        return float(load_golden("shape_tanimoto.npz")["ceyyag__ceyyag"].max())
    from ml_conformer_generator_amd.cheminformatics import shape_frames_hip
    x, n = _pad([xyz])
    _, fr = shape_frames_hip(x, n, DEV, centre_atoms=True)
    y = fr[0].cpu()
    return oracle_tanimoto(y, y)


def _walk(n, g, step=1.5, clearance=1.4):
    pts = [torch.zeros(3, dtype=torch.float64)]
    while len(pts) < n:
        d = torch.randn(3, generator=g, dtype=torch.float64)
        p = pts[-1] + d / d.norm() * step
        if min(float((p - q).norm()) for q in pts) >= clearance - 1e-9:
            pts.append(p)
    return torch.stack(pts).to(torch.float32)


def test_pose_recovers_the_reference_with_and_without_a_flip():
    from ml_conformer_generator_amd.cheminformatics import shape_overlay
    flips = []
    for name, ref in _separated_goldens():
        copies = _copies(ref, 6, 100 + len(name))
        n_ref = int(ref.shape[0])
        for N in (n_ref, 41, 64):                            # mixed padded widths
            x, n = _pad([c for c, _, _ in copies], N)
            res = shape_overlay(ref, x, n, DEV)
            posed = res["coords"].cpu()
            self_score = _self_score(name, ref)
            for b in range(len(copies)):
                rmsd = float(((posed[b, :n_ref].double() - ref.double()) ** 2).sum(1).mean().sqrt())
                assert rmsd < 1e-3, (name, N, b, rmsd, bool(res["flipped"][b]))
                assert abs(float(res["tanimoto"][b]) - self_score) < 2e-4, (name, b)
            flips += res["flipped"].cpu().tolist()
    print(f"SHAPE-OVERLAY pose recovery: {len(flips)} rows, {sum(flips)} flipped")
    assert any(flips) and not all(flips)              # both handedness cases were exercised


def test_poses_are_rigid_and_proper():
    from ml_conformer_generator_amd.cheminformatics import shape_overlay
    g = torch.Generator().manual_seed(31)
    ref = load_golden("shape_quadrupole.npz")["xyz_ceyyag"].to(torch.float32)
    mols = [_walk(int(k), g) * 1.0 + torch.randn(3, generator=g) * 10 for k in torch.randint(8, 40, (24,), generator=g)]
    x, n = _pad(mols, 48)
    res = shape_overlay(ref, x, n, DEV)
    R, t, posed = res["rotation"].cpu().double(), res["translation"].cpu().double(), res["coords"].cpu()
    eye = torch.eye(3, dtype=torch.float64)
    for b, m in enumerate(mols):
        k = int(n[b])
        assert abs(float(torch.det(R[b])) - 1.0) < 1e-5
        assert float((R[b] @ R[b].T - eye).abs().max()) < 1e-5
        want = m.double() @ R[b] + t[b]
        assert float((posed[b, :k].double() - want).abs().max()) < 1e-4
        assert float(posed[b, k:].abs().max() if k < 48 else 0.0) == 0.0
        d0, d1 = torch.cdist(m.double(), m.double()), torch.cdist(posed[b, :k].double(), posed[b, :k].double())
        assert float((d0 - d1).abs().max()) < 1e-4


def _reference_transform(ref):
    from ml_conformer_generator_amd.cheminformatics import shape_frames_hip
    x, n = _pad([ref])
    xf = torch.empty(1, 12, device=DEV)
    _, fr = shape_frames_hip(x.to(DEV), n, DEV, centre_atoms=True, xform_out=xf)
    xf = xf[0].cpu()
    return fr[0].cpu(), xf[:9].reshape(3, 3), xf[9:]


def test_overlay_scores_match_the_cpu_oracle():
    from ml_conformer_generator_amd.cheminformatics import _orientations, shape_overlay
    g = torch.Generator().manual_seed(2026)
    gq = load_golden("shape_quadrupole.npz")
    ref = gq["xyz_ceyyag"].to(torch.float32)
    mols = [_walk(int(k), g) for k in torch.randint(10, 65, (65,), generator=g)]
    mols += [gq[f"xyz_{k}"].to(torch.float32) + 3.0 for k in ("yibfeu", "paba", "walk12", "walk27")]
    x, n = _pad(mols)
    res = shape_overlay(ref, x, n, DEV)
    y_r, M_r, t_r = _reference_transform(ref)
    rots = _orientations().double()
    worst = 0.0
    for b, m in enumerate(mols):
        k = int(n[b])
        w = int(res["orientation"][b])
        y = ((res["coords"][b, :k].cpu().double() - t_r.double()) @ M_r.double()).to(torch.float32)
        got = oracle_tanimoto(y_r, y)
        worst = max(worst, abs(got - float(res["tanimoto"][b])))
        assert abs(got - float(res["tanimoto"][b])) < 2e-4, b
        base = y.double() @ rots[w].T                      # the handedness-fixed frame
        for o in range(4):
            if o != w:
                assert got >= oracle_tanimoto(y_r, (base @ rots[o]).to(torch.float32)) - 2e-4, (b, o)
    print(f"SHAPE-OVERLAY max |overlay_tanimoto - oracle| over {len(mols)} molecules = {worst:.3e}")


def test_overlay_scores_and_frames_are_bit_identical_to_the_existing_kernels():
    from ml_conformer_generator_amd.cheminformatics import shape_frames_hip, shape_overlay, shape_tanimoto_batch
    g = torch.Generator().manual_seed(77)
    gq = load_golden("shape_quadrupole.npz")
    ref = gq["xyz_yibfeu"].to(torch.float32)
    mols = [_walk(int(k), g) for k in torch.randint(10, 40, (20,), generator=g)]
    mols += [c for c, _, _ in _copies(ref, 6, 5)]
    n_ref = int(ref.shape[0])
    x, n = _pad([ref] + mols, 40)
    xf = torch.empty(x.shape[0], 12, device=DEV)
    mom_a, fr_a = shape_frames_hip(x, n, DEV, centre_atoms=True)
    mom_b, fr_b = shape_frames_hip(x, n, DEV, centre_atoms=True, xform_out=xf)
    assert torch.equal(mom_a, mom_b) and torch.equal(fr_a, fr_b)
    # frames = (coords - t) @ M on the real rows
    xfc = xf.cpu().double()
    for b in range(x.shape[0]):
        k = int(n[b])
        back = (x[b, :k].double() - xfc[b, 9:]) @ xfc[b, :9].reshape(3, 3)
        assert float((back - fr_a[b, :k].cpu().double()).abs().max()) < 1e-4
    res = shape_overlay(ref, x[1:], n[1:], DEV, with_scores=True)
    fixed = fr_a[1:].clone()
    fixed[res["flipped"], :, 2] = -fixed[res["flipped"], :, 2]
    scores, _, _ = shape_tanimoto_batch(fr_a[0, :n_ref], fixed, n[1:], DEV)
    assert torch.equal(res["scores"], scores)


def test_pose_is_bit_identical_whatever_the_batch():
    from ml_conformer_generator_amd.cheminformatics import shape_overlay
    gq = load_golden("shape_quadrupole.npz")
    ref = gq["xyz_ceyyag"].to(torch.float32)
    mol = gq["xyz_yibfeu"].to(torch.float32) + torch.tensor([4.0, -2.0, 7.5])
    g = torch.Generator().manual_seed(9)
    others = [_walk(int(k), g) for k in torch.randint(10, 64, (40,), generator=g)]
    seen = []
    for row, N in ((0, 23), (0, 64), (17, 64), (40, 64), (3, 30)):
        batch = list(others[:row]) + [mol] + list(others[row:]) if N == 64 else \
            [mol] if row == 0 else [o[:20] for o in others[:row]] + [mol]
        x, n = _pad(batch, N)
        res = shape_overlay(ref, x, n, DEV)
        r = row if N == 64 else len(batch) - 1
        seen.append((res["coords"][r, :23].cpu(), res["rotation"][r].cpu(), res["translation"][r].cpu(),
                     res["tanimoto"][r].cpu(), res["orientation"][r].cpu()))
    for other in seen[1:]:
        for a, b in zip(seen[0], other):
            assert torch.equal(a, b)


def test_a_failing_row_keeps_its_coordinates_and_spares_the_others():
    from ml_conformer_generator_amd.cheminformatics import shape_overlay
    gq = load_golden("shape_quadrupole.npz")
    ref = gq["xyz_ceyyag"].to(torch.float32)
    good = [gq[f"xyz_{k}"].to(torch.float32) for k in ("yibfeu", "paba", "walk12")]
    bad = good[1].clone()
    bad[2, 0] = float("inf")
    x, n = _pad(good[:1] + [bad] + good[1:], 23)
    res = shape_overlay(ref, x, n, DEV)
    alone = shape_overlay(ref, *_pad(good[:1], 23), DEV)
    for key in ("coords", "rotation", "translation", "tanimoto", "orientation"):
        assert torch.equal(res[key][0], alone[key][0]), key
    assert int(res["orientation"][1]) == -1 and bool(torch.isnan(res["tanimoto"][1]))
    assert bool(torch.isnan(res["rotation"][1]).all()) and bool(torch.isnan(res["translation"][1]).all())
    torch.testing.assert_close(res["coords"][1].cpu(), x[1], rtol=0, atol=0)
    assert bool(torch.isfinite(res["tanimoto"][[0, 2, 3]]).all())


# ----------------------------------------------------------------------------------------------- generation entries
def _gen_and_shards():
    from test_shape_frames_gpu import _gen, _molecule_like_shards
    gen = _gen()
    return gen, _molecule_like_shards(gen)


def test_generation_with_overlay_end_to_end(monkeypatch):
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd.cheminformatics import shape_scores
    gen, shards = _gen_and_shards()
    monkeypatch.setattr(gen, "_generate_shard", shards)
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"]) + torch.tensor([12.0, -5.0, 3.0])
    kw = dict(reference_conformer=ref, variance=2, optimise_geometry=False, sample_seed=SEED, n_samples=12)
    plain = gen.generate_conformers(**kw)
    posed = gen.generate_conformers(overlay=True, **kw)
    assert [m.sample_id for m in posed] == [m.sample_id for m in plain] == list(range(12))
    assert all(m.pose is None and m.overlay_tanimoto is None for m in plain)
    for a, b in zip(plain, posed):
        assert a.atomic_numbers == b.atomic_numbers and torch.equal(a.bond_orders, b.bond_orders)
        R, t = b.pose
        assert float((b.coords.double() - (a.coords.double() @ R.double() + t.double())).abs().max()) < 1e-4
        assert 0.0 < b.overlay_tanimoto <= 1.0 + 1e-6 and b.shape_tanimoto is None
    # the molecules now sit on the reference, not at the origin
    centre = torch.stack([m.coords.mean(0) for m in posed]).mean(0)
    assert float((centre - ref.mean(0)).norm()) < 3.0
    scored = gen.generate_conformers(overlay=True, shape_scores=True, **kw)
    x, n = _pad([m.coords for m in scored])
    best, _ = shape_scores(ref, x, n, DEV)
    assert [m.shape_tanimoto for m in scored] == [float(v) for v in best.cpu().tolist()]
    assert [m.overlay_tanimoto for m in scored] == [m.overlay_tanimoto for m in posed]
    sharded = gen.generate_conformers_sharded(overlay=True, **kw)             # no process group: one rank
    assert [m.sample_id for m in sharded] == [m.sample_id for m in posed]
    for a, b in zip(posed, sharded):
        assert torch.equal(a.coords, b.coords) and a.overlay_tanimoto == b.overlay_tanimoto
        assert torch.equal(a.pose[0], b.pose[0]) and torch.equal(a.pose[1], b.pose[1])
    print(f"SHAPE-OVERLAY e2e overlay_tanimoto {[round(m.overlay_tanimoto, 4) for m in posed]}")


def test_generation_with_overlay_keeps_a_failing_row_where_it_was(monkeypatch):
    from ml_conformer_generator_amd import conformer_generator as CG
    from test_shape_frames_gpu import _gen, _molecule_like_shards
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen, nan_ids=(5,)))
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep the invalid one too
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"])
    kw = dict(reference_conformer=ref, variance=2, optimise_geometry=False, sample_seed=SEED, n_samples=8)
    plain = gen.generate_conformers(**kw)
    posed = gen.generate_conformers(overlay=True, **kw)
    for a, b in zip(plain, posed):
        if b.sample_id == 5:
            torch.testing.assert_close(a.coords, b.coords, rtol=0, atol=0, equal_nan=True)
            assert b.pose is None and math.isnan(b.overlay_tanimoto)
        else:
            assert b.pose is not None and math.isfinite(b.overlay_tanimoto)
