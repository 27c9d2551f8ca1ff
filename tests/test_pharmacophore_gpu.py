"""Pharmacophore perception and overlap by HIP (`mcg_pharm_perceive`, `mcg_pharm_score`) on the MI355X: every type bit,
ring mask and ring count against the plain-Python restatement (`pharmacophore_ref`), the score against its fp64 sums
under the measured pass rule written there, the same bits whatever the batch, row, widths and padding, sentinels around
every output, and the options of the generation entries end to end."""
import functools
import random

import numpy as np
import pytest
import torch

import pharmacophore_cases as C
import pharmacophore_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U64 = (1 << 64) - 1
GUARD = 256


def _batch(mols, W=None, junk_seed=None):
    """(z [B,W] int32, bonds [B,W,W] int8, n [B] int32); with `junk_seed` the padding and the diagonal hold junk elements
    and junk codes."""
    W = W or max([m[2] for m in mols] + [1])
    B = len(mols)
    if junk_seed is None:
        z, bonds = np.zeros((B, W), np.int32), np.zeros((B, W, W), np.int8)
    else:
        g = np.random.default_rng(junk_seed)
        z = g.integers(-3, 90, (B, W)).astype(np.int32)
        bonds = g.integers(-128, 128, (B, W, W)).astype(np.int8)
    for b, (zs, adj, n) in enumerate(mols):
        if n:
            z[b, :n] = zs
            diag = bonds[b, np.arange(n), np.arange(n)].copy()
            bonds[b, :n, :n] = np.asarray(adj, dtype=np.int8).reshape(n, n)
            bonds[b, np.arange(n), np.arange(n)] = diag
    return torch.from_numpy(z), torch.from_numpy(bonds), torch.tensor([m[2] for m in mols], dtype=torch.int32)


def _guarded(size, dtype, fill):
    return torch.full((GUARD + size + GUARD,), fill, dtype=dtype, device=DEV)


def _intact(t, size, fill):
    return bool((t[:GUARD] == fill).all()) and bool((t[GUARD + size:] == fill).all())


def _perceive(mols, W=None, junk_seed=None):
    """The kernel's (types per molecule, kept ring masks per molecule, ring counts) through the C entry point, every
    output between sentinels."""
    from ml_conformer_generator_amd import _lib
    z, bonds, n = (t.to(DEV).contiguous() for t in _batch(mols, W, junk_seed))
    B, W = int(bonds.shape[0]), int(bonds.shape[1])
    types = _guarded(B * W, torch.uint8, 0xA5)
    count = _guarded(B, torch.int32, 0x5A5A5A5A)
    rings = _guarded(B * 32, torch.int64, 0x5A5A5A5A5A5A5A5A)
    _lib.check(_lib.lib().mcg_pharm_perceive(_lib.dptr(z), _lib.dptr(bonds), _lib.dptr(n), B, W,
                                             types[GUARD:].data_ptr(), count[GUARD:].data_ptr(), rings[GUARD:].data_ptr(),
                                             _lib.current_stream_ptr(DEV)), "mcg_pharm_perceive")
    assert _intact(types, B * W, 0xA5) and _intact(count, B, 0x5A5A5A5A) and _intact(rings, B * 32, 0x5A5A5A5A5A5A5A5A)
    t = types[GUARD:GUARD + B * W].cpu().reshape(B, W).tolist()
    r = rings[GUARD:GUARD + B * 32].cpu().reshape(B, 32).tolist()
    k = count[GUARD:GUARD + B].cpu().tolist()
    for b, m in enumerate(mols):
        assert not any(t[b][m[2]:]), "type bits on padded atoms"
        assert not any(r[b][min(k[b], 32):]), "ring masks beyond the count"
    return ([t[b][: m[2]] for b, m in enumerate(mols)], [[v & U64 for v in r[b][: min(k[b], 32)]] for b in range(B)], k)


def _expected(mols):
    ref = [R.perceive(*m) for m in mols]
    return [t for t, _, _ in ref], [r[:32] for _, r, _ in ref], [len(r) for _, r, _ in ref]


def _assert_equal(got, want, what):
    for part, name in enumerate(("types", "ring masks", "ring counts")):
        bad = [b for b, (x, y) in enumerate(zip(got[part], want[part])) if x != y]
        assert not bad, (what, name, bad[:5], got[part][bad[0]], want[part][bad[0]])


@functools.lru_cache(maxsize=None)
def _molecule_like():
    mols = C.molecule_like_set()
    return mols, _expected(mols)


# ----------------------------------------------------------------------------------------------- perception
def test_pinned_molecules():
    mols = [m for m, _, _, _ in C.PINNED.values()]
    types, rings, counts = _perceive(mols)
    for b, (name, (_, t, r, _)) in enumerate(C.PINNED.items()):
        assert (types[b], rings[b], counts[b]) == (t, r, len(r)), name


def test_molecule_like_graphs_match_the_restatement_bit_for_bit():
    mols, want = _molecule_like()
    assert len(mols) >= 500 and {m[2] for m in mols} == set(range(1, 43))
    assert sum(1 for k in want[2] if k) > 200 and max(want[2]) >= 3          # ring features do occur
    _assert_equal(_perceive(mols), want, "molecule-like")


def test_last_lane_top_bit_and_junk_graphs():
    rng = random.Random(6400)
    mols = C.big_molecules() + [C.junk_graph(rng, 64) for _ in range(6)] + [C.junk_graph(rng, 42) for _ in range(3)] + \
        [C.sparse_aromatic_junk(rng, n) for n in (64, 64, 64, 63, 42, 17)] + [C.k33(), R.mol([], []), R.mol([8], [])]
    want = _expected(mols)
    assert want[1][3][-1] >> 63 == 1                  # the pyridine ring on atoms 58..63 of the 64-atom molecule
    assert max(want[2][13:19]) >= 4                   # the sparse aromatic junk does close rings
    assert want[2][19] == 1                           # K(3,3): six closed paths, one member set
    _assert_equal(_perceive(mols), want, "big and junk")
    _assert_equal(_perceive(mols, 64, junk_seed=3), want, "big and junk, junk on the diagonal")


def test_more_rings_than_are_kept():
    from ml_conformer_generator_amd.pharmacophore import perceive_features, score_features
    mols = [C.PINNED["benzene"][0], C.petersen_field(), C.PINNED["indole"][0]]
    want = _expected(mols)
    assert want[2] == [1, 132, 2] and len(want[1][1]) == 32
    _assert_equal(_perceive(mols), want, "132 rings")
    z, bonds, n = _batch(mols)
    types, rings, count = perceive_features(z, bonds, n, DEV)
    assert count.tolist() == [1, 132, 2]
    xyz = torch.randn(3, 60, 3, generator=torch.Generator().manual_seed(1))
    out = score_features([("ring", (0.0, 0.0, 0.0)), ("donor", (1.0, 0.0, 0.0))], xyz, n, types, rings, count, DEV,
                         per_type=True)
    t, hits = out["tanimoto"].cpu().numpy(), out["matches"].tolist()
    assert np.isnan(t[1]) and hits[1] == -1 and np.isnan(out["o_rm"].cpu().numpy()[1])
    assert np.isnan(out["per_type"].cpu().numpy()[1]).all()
    assert np.isfinite(t[[0, 2]]).all() and min(hits[0], hits[2]) >= 0


def test_same_bits_whatever_numbering_row_batch_width_and_padding():
    rng = random.Random(11)
    mols, base = _molecule_like()
    mols, base = mols[:252], tuple(part[:252] for part in base)
    order = list(range(len(mols)))
    rng.shuffle(order)
    _assert_equal(_perceive([mols[i] for i in order]), tuple([part[i] for i in order] for part in base), "other rows")
    for b in (0, 41, 170, 251):
        _assert_equal(_perceive([mols[b]]), tuple(part[b:b + 1] for part in base), f"alone at W = n, molecule {b}")
        five = [mols[(b + 7 * k) % 252] for k in range(5)]
        for row in range(5):
            batch = five[1:row + 1] + [mols[b]] + five[row + 1:]
            got = _perceive(batch, junk_seed=100 + row)
            assert tuple(part[row] for part in got) == tuple(part[b] for part in base), (b, row)
    for W, seed in ((42, 1), (64, 2), (43, 3)):
        _assert_equal(_perceive(mols, W, junk_seed=seed), base, f"width {W} with junk padding")
    # renumbering: the types move with their atoms, the masks are renumbered and sorted again
    moved = [C.random_permutation(rng, m) for m in mols]
    got = _perceive([m for _, m in moved])
    for b, (p, _) in enumerate(moved):
        assert got[0][b] == [base[0][b][p[i]] for i in range(len(p))], b
        assert got[1][b] == sorted(R.permute_mask(m, p) for m in base[1][b]) and got[2][b] == base[2][b], b


# ----------------------------------------------------------------------------------------------- score
def _ref_tensors(fr):
    return (torch.tensor(np.array([p for _, p in fr], dtype=np.float32).reshape(-1, 3)),
            torch.tensor([t for t, _ in fr], dtype=torch.uint8))


def _score(fr, mols, coords, N=None, W=None, junk_seed=None):
    """The score kernel's outputs of posed molecules (`coords[b]` [n_b,3] fp32) against the features `fr`, through the C
    entry point with every output between sentinels; perception by the kernel too.  Dict of numpy arrays."""
    from ml_conformer_generator_amd import _lib
    from ml_conformer_generator_amd.pharmacophore import perceive_features, reference_self_overlap
    z, bonds, n = _batch(mols, W, junk_seed)
    types, rings, count = perceive_features(z, bonds, n, DEV)
    B, W = int(types.shape[0]), int(types.shape[1])
    N = N or max([m[2] for m in mols] + [1])
    g = np.random.default_rng(junk_seed or 0)
    x = np.zeros((B, N, 3), np.float32) if junk_seed is None else g.normal(0, 50, (B, N, 3)).astype(np.float32)
    for b, c in enumerate(coords):
        x[b, : len(c)] = c
    x = torch.from_numpy(x).to(DEV)
    xyz, typ = (t.to(DEV).contiguous() for t in _ref_tensors(fr))
    o_rr = reference_self_overlap((xyz, typ), DEV)
    out = dict(o_rm=_guarded(B, torch.float64, -7.0), o_mm=_guarded(B, torch.float64, -7.0),
               tanimoto=_guarded(B, torch.float32, -7.0), matches=_guarded(B, torch.int32, 0x5A5A5A5A),
               per_type=_guarded(B * 6, torch.float64, -7.0))
    nn = n.to(DEV)
    _lib.check(_lib.lib().mcg_pharm_score(_lib.dptr(x), _lib.dptr(nn), _lib.dptr(types), _lib.dptr(rings),
                                          _lib.dptr(count), B, N, W, _lib.dptr(xyz), _lib.dptr(typ), int(typ.numel()),
                                          _lib.dptr(o_rr), *(out[k][GUARD:].data_ptr() for k in
                                                             ("o_rm", "o_mm", "tanimoto", "matches", "per_type")),
                                          _lib.current_stream_ptr(DEV)), "mcg_pharm_score")
    res = {}
    for k, t in out.items():
        size = B * 6 if k == "per_type" else B
        assert _intact(t, size, 0x5A5A5A5A if k == "matches" else -7.0), k
        res[k] = t[GUARD:GUARD + size].cpu().numpy()
    res["per_type"] = res["per_type"].reshape(B, 6)
    res["o_rr"] = float(o_rr.cpu()[0])
    return res


def _bits(res, b):
    return tuple(np.asarray(res[k][b]).tobytes() for k in ("o_rm", "o_mm", "tanimoto", "matches", "per_type"))


@functools.lru_cache(maxsize=None)
def _scored_cases():
    """Per reference: (cases, kernel outputs of all of them as one batch at N = W = 64, restatement results)."""
    refs, cases = C.score_cases()
    out = {}
    for rname, fr in refs.items():
        mine = [c for c in cases if c["ref"] == rname]
        got = _score(fr, [c["mol"] for c in mine], [c["coords"] for c in mine], 64, 64)
        out[rname] = (mine, got, [R.score(fr, c["coords"], *c["mol"]) for c in mine])
    return refs, out


def test_score_matches_the_fp64_restatement():
    refs, scored = _scored_cases()
    assert {len(fr) for fr in refs.values()} >= {1, 10, R.MAX_FEATURES}
    worst = dict(tanimoto=0.0, o_rm=0.0, o_mm=0.0)
    for rname, (cases, got, want) in scored.items():
        assert abs(got["o_rr"] - R.overlap(refs[rname], refs[rname])) <= R.SCORE_C * R.EPS32 * got["o_rr"]
        for b, (c, w) in enumerate(zip(cases, want)):
            what = (rname, c["name"])
            assert int(got["matches"][b]) == w["matches"], what
            err = dict(tanimoto=abs(float(got["tanimoto"][b]) - w["tanimoto"]),
                       o_rm=abs(got["o_rm"][b] - w["o_rm"]) / w["o_rm"] if w["o_rm"] else abs(got["o_rm"][b]),
                       o_mm=abs(got["o_mm"][b] - w["o_mm"]) / w["o_mm"] if w["o_mm"] else abs(got["o_mm"][b]))
            for k, e in err.items():
                worst[k] = max(worst[k], e / R.EPS32)
            print(f"PHARM-SCORE {rname:9s} {c['name']:22s} T {w['tanimoto']:.6f} matches {w['matches']:3d}  err / 2^-24: "
                  + "  ".join(f"{k} {e / R.EPS32:6.3f}" for k, e in err.items()))
            # the six parts add up to the total in type order, and each is its fp64 value within the reasoned bound
            total = 0.0
            for t in range(6):
                total += float(got["per_type"][b, t])
                assert abs(got["per_type"][b, t] - w["per_type"][t]) <= R.PART_REL * w["per_type"][t] + 1e-37, what
            assert total == float(got["o_rm"][b]), what
            for k, e in err.items():
                assert e <= R.SCORE_C * R.EPS32, (what, k, e / R.EPS32)
    print("PHARM-SCORE worst err / 2^-24: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"  (pass value SCORE_C = {R.SCORE_C:.2f})")
    cases, got, want = scored["molecule"]
    assert cases[0]["name"] == "reference on itself" and float(got["tanimoto"][0]) == 1.0 and want[0]["matches"] == 10
    assert cases[-1]["name"] == "no features" and float(got["tanimoto"][-1]) == 0.0 and int(got["matches"][-1]) == 0
    assert got["o_rm"][0] == got["o_mm"][0] == got["o_rr"]


def test_score_has_the_same_bits_whatever_batch_row_and_widths():
    refs, scored = _scored_cases()
    for rname in ("molecule", "max"):
        cases, base, _ = scored[rname]
        for b in (1, 7, 10, 13, len(cases) - 1):
            c = cases[b]
            n = c["mol"][2]
            alone = _score(refs[rname], [c["mol"]], [c["coords"]])                      # N = W = n
            assert _bits(alone, 0) == _bits(base, b), (rname, c["name"], "alone")
            others = [cases[(b + 3 * k) % len(cases)] for k in range(1, 5)]
            for row in range(5):
                batch = others[:row] + [c] + others[row:]
                widest = max(x["mol"][2] for x in batch)
                for N, W in ((None, None), (64, max(widest, 42)), (max(widest, 42), 64)):
                    got = _score(refs[rname], [x["mol"] for x in batch], [x["coords"] for x in batch], N, W,
                                 junk_seed=50 + row)
                    assert _bits(got, row) == _bits(base, b), (rname, c["name"], row, N, W)


def test_a_non_finite_coordinate_spoils_its_own_row_only():
    refs, scored = _scored_cases()
    cases, base, _ = scored["molecule"]
    pick = [cases[k] for k in (7, 10, 13)]
    coords = [c["coords"].copy() for c in pick]
    coords[1][pick[1]["mol"][2] - 1, 2] = np.nan
    got = _score(refs["molecule"], [c["mol"] for c in pick], coords, 64, 64)
    assert np.isnan(got["tanimoto"][1]) and np.isnan(got["o_rm"][1]) and np.isnan(got["o_mm"][1])
    assert int(got["matches"][1]) == -1 and np.isnan(got["per_type"][1]).all()
    assert _bits(got, 0) == _bits(base, 7) and _bits(got, 2) == _bits(base, 13)
    coords[1] = pick[1]["coords"]
    padded = _score(refs["molecule"], [c["mol"] for c in pick], coords, 64, 64, junk_seed=9)      # junk beyond n: not read
    assert [_bits(padded, k) for k in range(3)] == [_bits(base, k) for k in (7, 10, 13)]


def test_python_layer_agrees_with_the_entry_points():
    from ml_conformer_generator_amd import pharmacophore as PH
    refs, scored = _scored_cases()
    cases, base, _ = scored["molecule"]
    z, bonds, n = _batch([c["mol"] for c in cases], 64)
    x = torch.zeros(len(cases), 64, 3)
    for b, c in enumerate(cases):
        x[b, : len(c["coords"])] = torch.from_numpy(c["coords"])
    named = [(R.TYPE_NAMES[t], tuple(float(v) for v in p)) for t, p in refs["molecule"]]
    sim, hits = PH.pharmacophore_tanimoto(named, x, z, bonds, n, DEV)
    assert sim.cpu().numpy().tobytes() == base["tanimoto"].tobytes() and hits.cpu().tolist() == base["matches"].tolist()
    # the reference's own features, perceived and placed by the package, are the restatement's
    types, rings, count = PH.perceive_features(z[:1], bonds[:1], n[:1], DEV)
    points = PH.feature_points(x[:1], types, rings, count)[0]
    assert [k for k, _ in points] == [k for k, _ in named]
    assert np.array_equal(np.array([p for _, p in points], np.float32), np.array([p for _, p in named], np.float32))
    with pytest.raises(ValueError):
        PH.perceive_features(torch.zeros(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8),
                             torch.tensor([3]), DEV)
    with pytest.raises(ValueError):
        PH.score_features([], x, n, types, rings, count, DEV)


# ----------------------------------------------------------------------------------------------- generation entries
def _record_graph(m):
    return list(m.atomic_numbers), [[int(v) for v in row] for row in m.bond_orders.tolist()], len(m.atomic_numbers)


def _fields(m):
    return (m.sample_id, m.atomic_numbers, m.coords.tolist(), m.bond_orders.tolist(), m.valid, m.shape_tanimoto,
            m.overlay_tanimoto)


def test_generation_pharmacophore_scores_filter_and_combo_ranking(monkeypatch):
    from conftest import load_golden
    from test_shape_frames_gpu import SEED, _gen, _molecule_like_shards
    from ml_conformer_generator_amd import conformer_generator as CG
    from ml_conformer_generator_amd import pharmacophore as PH
    from ml_conformer_generator_amd import postprocess
    gen = _gen()
    monkeypatch.setattr(gen, "_generate_shard", _molecule_like_shards(gen))
    monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))    # keep every record
    ref = torch.as_tensor(load_golden("context_shape.npz")["ceyyag_xyz"])
    g = torch.Generator().manual_seed(3)
    feats = [(PH.TYPE_NAMES[int(torch.randint(0, 5, (1,), generator=g))], tuple(ref[k].tolist()))
             for k in range(0, ref.shape[0], 2)]
    kw = dict(reference_conformer=ref, n_samples=8, variance=2, optimise_geometry=False, sample_seed=SEED, overlay=True,
              shape_scores=True)
    plain = gen.generate_conformers(**kw)
    assert all(m.pharmacophore_tanimoto is None and m.pharmacophore_matches is None for m in plain)

    scored = gen.generate_conformers(pharmacophore_scores=True, reference_pharmacophore=feats, **kw)
    assert [m.sample_id for m in scored] == list(range(8))
    assert [_fields(m) for m in scored] == [_fields(m) for m in plain]
    graphs = [_record_graph(m) for m in scored]
    z, bonds, n = _batch(graphs, 42)
    x = torch.zeros(8, 42, 3)
    for b, m in enumerate(scored):
        x[b, : n[b]] = m.coords
    sim, hits = PH.pharmacophore_tanimoto(feats, x, z, bonds, n, DEV)
    assert sum(1 for m in scored if m.pose is not None) >= 6
    assert [m.pharmacophore_tanimoto for m in scored] == [float(v) if m.pose is not None else None
                                                          for m, v in zip(scored, sim.cpu().tolist())]
    assert [m.pharmacophore_matches for m in scored] == [v if m.pose is not None else None
                                                         for m, v in zip(scored, hits.cpu().tolist())]
    fr = [(PH.TYPE_NAMES.index(k), np.array(p, dtype=np.float32)) for k, p in feats]
    for b, m in enumerate(scored):
        if m.pose is None:
            continue
        want = R.score(fr, m.coords.numpy(), *graphs[b])
        assert abs(m.pharmacophore_tanimoto - want["tanimoto"]) <= R.SCORE_C * R.EPS32 and \
            m.pharmacophore_matches == want["matches"], b
    assert gen.generate_conformers_sharded(pharmacophore_scores=True, reference_pharmacophore=feats, **kw) == scored
    assert [m.pharmacophore_tanimoto for m in gen.forward(pharmacophore_scores=True, reference_pharmacophore=feats, **kw)] \
        == [m.pharmacophore_tanimoto for m in scored]

    # the reference's features perceived from a graph: record 2's graph on record 2's own atoms as the reference
    t, rings, _ = R.perceive(*graphs[2])
    own_kw = dict(reference_conformer=scored[2].coords, reference_graph=scored[2], n_samples=8, variance=2,
                  optimise_geometry=False, sample_seed=SEED, overlay=True, pharmacophore_scores=True)
    own_feats = R.features(scored[2].coords.numpy(), t, rings)
    if own_feats:
        own = gen.generate_conformers(**own_kw)
        for m in own:
            if m.pose is not None:
                want = R.score(own_feats, m.coords.numpy(), *_record_graph(m))
                assert abs(m.pharmacophore_tanimoto - want["tanimoto"]) <= R.SCORE_C * R.EPS32 and \
                    m.pharmacophore_matches == want["matches"], m.sample_id
    else:
        with pytest.raises(ValueError, match="no pharmacophore features"):
            gen.generate_conformers(**own_kw)

    # the filter and the combined ranking select what `select` says on the host
    values = sorted(m.pharmacophore_tanimoto for m in scored if m.pharmacophore_tanimoto is not None)
    t = values[len(values) // 2]
    kept = gen.generate_conformers(min_pharmacophore_tanimoto=t, reference_pharmacophore=feats, **kw)
    assert [m.sample_id for m in kept] == [m.sample_id for m in scored
                                           if m.pharmacophore_tanimoto is not None and m.pharmacophore_tanimoto >= t]
    assert 0 < len(kept) < 8 or values[0] == values[-1]
    combo = gen.generate_conformers(pharmacophore_scores=True, reference_pharmacophore=feats, rank_by="combo", top_k=3,
                                    **kw)
    req = postprocess.Request(scores_shape=True, top_k=3, scores_pharmacophore=True, rank_by="combo")
    rows = postprocess.Rows(list(scored), [m.sample_id for m in scored], [m._measured for m in scored], list(range(8)))
    assert [m.sample_id for m in combo] == [m.sample_id for m in postprocess.select(rows, req, None, None)]
    best = sorted([m for m in scored if m.pose is not None],
                  key=lambda m: (-(m.shape_tanimoto + m.pharmacophore_tanimoto), m.sample_id))[:3]
    assert [m.sample_id for m in combo] == [m.sample_id for m in best]

    # a call with none of the new arguments returns what it returned
    again = gen.generate_conformers(**kw)
    assert again == plain and [_fields(m) for m in again] == [_fields(m) for m in plain]
    assert [m.pose[0].tolist() for m in again if m.pose] == [m.pose[0].tolist() for m in plain if m.pose]
