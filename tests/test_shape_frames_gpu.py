"""Principal shape frames by HIP (`mcg_shape_moments` / `mcg_shape_frames`) and shape scores of generated molecules on the
MI355X: exact clique enumeration, frames and scores against the reference fixtures and the tensor path, bit-identical
results whatever the batch, row or padded width, and the scoring options of the generation entries end to end."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x5EED_0000_2026_1015
GOLDEN_NAMES = ["ceyyag", "yibfeu", "paba", "crown_6", "walk12", "walk27"]


def _pad(coord_list, N=None):
    N = N or max(int(c.shape[0]) for c in coord_list)
    x = torch.zeros(len(coord_list), N, 3)
    for b, c in enumerate(coord_list):
        x[b, : c.shape[0]] = torch.as_tensor(c, dtype=torch.float32)
    return x, torch.tensor([int(c.shape[0]) for c in coord_list], dtype=torch.int32)


def _walk(n, g, step=1.5, clearance=1.4):
    """A self-avoiding random walk: no atom closer than `clearance` to an earlier one (a molecule-like cloud; a plain
    random walk piles atoms on top of each other, and its inclusion-exclusion sum is then ill-conditioned in fp32)."""
    pts = [torch.zeros(3, dtype=torch.float64)]
    while len(pts) < n:
        d = torch.randn(3, generator=g, dtype=torch.float64)
        p = pts[-1] + d / d.norm() * step
        if min(float((p - q).norm()) for q in pts) >= clearance - 1e-9:
            pts.append(p)
    return torch.stack(pts).to(torch.float32)


def _ragged_batch():
    """64 self-avoiding random-walk molecules of 10..64 atoms plus: walk27 (218 938 six-cliques), a compact 30-atom cloud and a chain
    with no neighbours at all (no cliques)."""
    g = torch.Generator().manual_seed(2026)
    mols = [_walk(int(n), g) for n in torch.randint(10, 65, (64,), generator=g)]
    mols.append(torch.as_tensor(load_golden("shape_quadrupole.npz")["xyz_walk27"]))
    mols.append((torch.rand(30, 3, generator=g) * 4.0))
    mols.append(torch.arange(12, dtype=torch.float32).view(12, 1) * torch.tensor([6.0, 0.0, 0.0]))
    return mols


def _reference_counts(x, n, n_terms=6, thr=5.4):
    from ml_conformer_generator_amd.cheminformatics import _grow_cliques
    x = x.to(DEV)
    B, N, _ = x.shape
    real = torch.arange(N, device=DEV).unsqueeze(0) < n.to(DEV).view(B, 1)
    d = torch.sqrt(((x.unsqueeze(2) - x.unsqueeze(1)) ** 2).sum(-1))
    adj = (d < thr) & (d > 0) & real.unsqueeze(1) & real.unsqueeze(2)
    cl = _grow_cliques(adj, n_terms)
    out = torch.zeros(B, n_terms - 1, dtype=torch.int64)
    for k in range(2, n_terms + 1):
        out[:, k - 2] = torch.bincount(cl[k][:, 0].cpu(), minlength=B)
    return out


def test_clique_counts_are_exact():
    from ml_conformer_generator_amd.cheminformatics import shape_frames_hip
    g = load_golden("shape_quadrupole.npz")
    golden = [torch.as_tensor(g[f"xyz_{k}"]) for k in GOLDEN_NAMES]
    for mols in (golden, _ragged_batch()):
        x, n = _pad(mols)
        _, _, counts = shape_frames_hip(x, n, DEV, with_counts=True)
        ref = _reference_counts(x, n)
        assert torch.equal(counts.cpu(), ref), (counts.cpu() - ref).abs().max()
    six = ref[:, -1]
    print(f"SHAPE-CLIQUES ragged batch of {len(mols)}: six-cliques min {int(six.min())} max {int(six.max())}, "
          f"all orders total {int(ref.sum())}")
    assert int(six.max()) >= 100_000 and int(ref[-1].sum()) == 0
    # other orders of the search: 2 (edges only) and 8
    x, n = _pad(golden)
    for terms in (2, 8):
        _, _, counts = shape_frames_hip(x, n, DEV, n_terms=terms, with_counts=True)
        assert torch.equal(counts.cpu(), _reference_counts(x, n, terms)), terms


def test_frames_and_scores_match_the_reference():
    from ml_conformer_generator_amd.cheminformatics import shape_frames_hip, shape_scores
    g = load_golden("shape_quadrupole.npz")
    names = ["ceyyag", "yibfeu", "paba", "walk12", "walk27"]          # crown_6: degenerate moments (see the tensor test)
    x, n = _pad([torch.as_tensor(g[f"xyz_{k}"]) for k in names])
    mom, frames = shape_frames_hip(x, n, DEV)
    for i, k in enumerate(names):
        assert float((mom[i].cpu() - g[f"moments_{k}"]).abs().max()) < 2e-5, k
        assert float((frames[i, : int(n[i])].cpu() - g[f"frame_{k}"]).abs().max()) < 2e-5, k
        assert float(frames[i, int(n[i]):].abs().max() if int(n[i]) < x.shape[1] else 0.0) == 0.0
    for key in ("best__ceyyag__yibfeu", "best__ceyyag__walk27", "best__yibfeu__paba", "best__walk12__ceyyag"):
        _, ref_name, cand = key.split("__")
        c = torch.as_tensor(g[f"xyz_{cand}"]) + torch.tensor([0.7, -1.1, 0.4])      # scoring re-centres
        best, which = shape_scores(torch.as_tensor(g[f"xyz_{ref_name}"]), c.unsqueeze(0),
                                   torch.tensor([c.shape[0]]), DEV)
        assert abs(float(best[0]) - float(g[key][0])) < 2e-4, key
        assert int(which[0]) == int(g[key][1]), key


def test_frames_match_the_tensor_path_on_a_ragged_batch():
    from ml_conformer_generator_amd.cheminformatics import shape_frames_hip, shape_quadrupole_batch
    # without the chain (no shape tensor worth comparing) and the compact cloud (30 atoms within 4 A: its 10^7-term
    # inclusion-exclusion cancels to a few digits in any summation order)
    mols = _ragged_batch()[:-3] + _ragged_batch()[-3:-2]
    x, n = _pad(mols)
    mom_h, fr_h = shape_frames_hip(x, n, DEV)
    mom_t, fr_t = shape_quadrupole_batch(x, n, DEV)
    m = mom_t.cpu().double()
    gap = torch.minimum((m[:, 0] - m[:, 1]).abs() / m[:, 0].abs(), (m[:, 1] - m[:, 2]).abs() / m[:, 1].abs())
    keep = gap > 1e-3
    print(f"SHAPE-FRAMES vs tensor path: {int(keep.sum())} of {len(mols)} compared, {int((~keep).sum())} excluded "
          "(two main moments within 1e-3 relative)")
    assert int(keep.sum()) >= len(mols) - 8
    rel = float(((mom_h - mom_t).abs() / mom_t.abs().clamp_min(1.0)).max())
    print(f"SHAPE-FRAMES max |moment_hip - moment_tensor| / max(1, |moment|) = {rel:.3e}")
    assert rel < 5e-5        # each fp32 evaluation lies up to ~1.2e-5 from an fp64 one on this batch: two may differ twice that
    # frames: 2e-5 of the molecule's extent (the eigenvectors inherit the moments' fp32 spread, so the coordinate error
    # grows with the distance from the centre); how many also meet 2e-5 absolute is printed
    worst, absolute_ok = 0.0, 0
    for b in torch.nonzero(keep).flatten().tolist():
        k = int(n[b])
        err = float((fr_h[b, :k] - fr_t[b, :k]).abs().max())
        absolute_ok += err < 2e-5
        worst = max(worst, err / max(1.0, float(fr_t[b, :k].abs().max())))
    print(f"SHAPE-FRAMES max |frame_hip - frame_tensor| / max(1, max|frame|) = {worst:.3e}; "
          f"{absolute_ok} of {int(keep.sum())} within 2e-5 absolute")
    assert worst < 2e-5


def test_moments_frames_and_scores_do_not_depend_on_the_batch():
    from ml_conformer_generator_amd.cheminformatics import shape_frames_hip, shape_scores
    g = load_golden("shape_quadrupole.npz")
    mol = torch.as_tensor(g["xyz_yibfeu"]) + torch.tensor([0.3, 0.2, -0.5])
    ref = torch.as_tensor(g["xyz_ceyyag"])
    others = _ragged_batch()[:63]
    layouts = []
    for row, N in ((0, 23), (0, 64), (37, 64), (63, 64)):
        batch = list(others)
        batch.insert(row, mol)
        x, n = _pad(batch if N == 64 else [mol], N)
        r = row if N == 64 else 0
        mom, fr = shape_frames_hip(x, n, DEV, centre_atoms=True)
        best, which = shape_scores(ref, x, n, DEV)
        layouts.append((mom[r].cpu(), fr[r, :23].cpu(), best[r].cpu(), which[r].cpu()))
    layouts.append(layouts[-1])
    x, n = _pad([mol], 23)                                   # a second run of the single-molecule call
    mom, fr = shape_frames_hip(x, n, DEV, centre_atoms=True)
    best, which = shape_scores(ref, x, n, DEV)
    layouts[-1] = (mom[0].cpu(), fr[0, :23].cpu(), best[0].cpu(), which[0].cpu())
    for other in layouts[1:]:
        for a, b in zip(layouts[0], other):
            assert torch.equal(a, b)


_GEN = []


def _gen():
    if not _GEN:
        from ml_conformer_generator_amd import MLConformerGenerator
        from ml_conformer_generator_amd import weights as W
        _GEN.append(MLConformerGenerator(diffusion_steps=20, device=DEV,
                                         edm_weights=W.synth_edm_state_dict(1234, recipe="v2d"),
                                         adj_mat_seer_weights=W.synth_adj_mat_seer_state_dict(4321),
                                         atom_order_provider=None))
    return _GEN[0]


def _molecule_like_shards(gen, nan_ids=()):
    """The generator's real `_generate_shard` (sampler, hand-off, GCN, write-back on the device), with the returned
    coordinates replaced by a molecule-like cloud per sample id: the synthetic weights' own molecules are hundreds of
    angstroms wide and overlap no reference at all (every score 0).  Sample ids in `nan_ids` get non-finite coordinates
    and are marked invalid."""
    real = gen._generate_shard

    def run(*args):
        res = real(*args)
        ids = args[12] if len(args) > 12 and args[12] is not None else torch.arange(args[4])
        n = res["n_nodes"].cpu()
        x = torch.zeros(res["x"].shape)
        valid = res["valid"].cpu().clone()
        for b, sid in enumerate(torch.as_tensor(ids).tolist()):
            c = _walk(int(n[b]), torch.Generator().manual_seed(1000 + sid))
            x[b, : int(n[b])] = c - c.mean(0)
            if sid in nan_ids:
                x[b, 0, 0], valid[b] = float("nan"), 0
        return dict(res, x=x.to(res["x"].device), valid=valid.to(res["valid"].device))
    return run


def test_generation_scores_selection_and_sharded_call(monkeypatch):
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd.cheminformatics import evaluate_shape
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen))
    ceyyag = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"])
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    kw = dict(variance=2, optimise_geometry=False, sample_seed=SEED)
    kw["reference_conformer"] = ref = ceyyag
    plain = gen.generate_conformers(n_samples=12, **kw)
    scored = gen.generate_conformers(n_samples=12, shape_scores=True, **kw)
    assert [m.shape_tanimoto for m in plain] == [None] * 12
    assert [m.sample_id for m in scored] == list(range(12))
    for a, b in zip(plain, scored):
        assert torch.equal(a.coords, b.coords)
    x, n = _pad([m.coords for m in scored])
    _, res = evaluate_shape(ref, x, n, DEV)
    got = torch.tensor([m.shape_tanimoto for m in scored], dtype=torch.float64)
    want = torch.tensor([r["shape_tanimoto"] for r in res], dtype=torch.float64)
    print(f"SHAPE-E2E scores {got.tolist()}  max |score - evaluate_shape| = {float((got - want).abs().max()):.3e}")
    assert bool(torch.isfinite(got).all()) and float((got - want).abs().max()) < 2e-4
    assert bool(((got >= 0.0) & (got <= 1.0 + 1e-6)).all())
    assert float(got.max()) > 0.1 and len(set(got.tolist())) == 12          # scores worth ranking: no ties, no zeros
    top = gen.generate_conformers(n_samples=12, top_k=5, **kw)
    expect = sorted(scored, key=lambda m: (-m.shape_tanimoto, m.sample_id))[:5]
    assert [m.sample_id for m in top] == [m.sample_id for m in expect]
    assert [m.shape_tanimoto for m in top] == [m.shape_tanimoto for m in expect]
    thr = sorted(m.shape_tanimoto for m in scored)[6]
    above = gen(n_samples=12, min_shape_tanimoto=thr, **kw)
    assert [m.sample_id for m in above] == [m.sample_id for m in sorted(scored, key=lambda m: (-m.shape_tanimoto,
                                                                                             m.sample_id))
                                            if m.shape_tanimoto >= thr]
    sharded = gen.generate_conformers_sharded(n_samples=12, shape_scores=True, **kw)      # no process group: one rank
    assert [m.sample_id for m in sharded] == list(range(12))
    assert [m.shape_tanimoto for m in sharded] == [m.shape_tanimoto for m in scored]
    sharded_top = gen.generate_conformers_sharded(n_samples=12, top_k=5, **kw)
    assert [m.sample_id for m in sharded_top] == [m.sample_id for m in top]


def test_a_non_finite_row_does_not_fail_the_batch(monkeypatch):
    """A molecule with non-finite coordinates or no atoms gets a NaN score (LAPACK would refuse the whole batch's eigh);
    every other molecule keeps the score it has alone, bit for bit, and a scored call drops the invalid one as the
    unscored call does."""
    from ml_conformer_generator_amd.cheminformatics import shape_scores
    g = load_golden("shape_quadrupole.npz")
    ref = torch.as_tensor(g["xyz_ceyyag"])
    good = [torch.as_tensor(g[f"xyz_{k}"]) for k in ("yibfeu", "paba", "walk12")]
    bad = good[1].clone()
    bad[3, 1] = float("inf")
    x, n = _pad(good[:1] + [bad] + good[1:], 23)
    n[3] = 0                                                      # and an empty row
    best, _ = shape_scores(ref, x, n, DEV)
    alone, _ = shape_scores(ref, *_pad(good[:1], 23), DEV)
    assert torch.equal(best[0], alone[0]) and bool(torch.isnan(best[1])) and bool(torch.isfinite(best[2]))
    assert float(best[3]) == 0.0
    with pytest.raises(ValueError):
        shape_scores(ref, x, torch.tensor([23, 10, 10, 24], dtype=torch.int32), DEV)      # a count beyond the width
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen, nan_ids=(5,)))
    kw = dict(reference_conformer=ref, variance=2, optimise_geometry=False, sample_seed=SEED, n_samples=8)
    plain = gen.generate_conformers(**kw)
    scored = gen.generate_conformers(shape_scores=True, **kw)
    assert [m.sample_id for m in scored] == [m.sample_id for m in plain] and 5 not in [m.sample_id for m in scored]
    assert all(m.shape_tanimoto == m.shape_tanimoto for m in scored)


def test_defaults_return_what_they_returned_before():
    gen = _gen()
    ctx = torch.tensor([53.6424, 108.3042, 151.4399])
    kw = dict(reference_context=ctx, n_atoms=22, variance=4, optimise_geometry=False, n_samples=6)
    torch.manual_seed(11)
    a = gen.generate_conformers(**kw)
    x_a = gen.last_batch["x_ordered"].clone()
    torch.manual_seed(11)
    b = gen.generate_conformers(**kw, shape_scores=False, top_k=None, min_shape_tanimoto=None)
    assert torch.equal(gen.last_batch["x_ordered"], x_a)
    assert len(a) == len(b) and all(torch.equal(p.coords, q.coords) for p, q in zip(a, b))
    assert all(m.shape_tanimoto is None for m in a + b)
