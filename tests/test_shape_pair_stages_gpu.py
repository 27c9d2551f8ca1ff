"""`mcg_shape_pair_tanimoto` on the MI355X, stage by stage through the C entry: the densities it leaves in `density_ws` against
the fp64 restatement of `tests/shape_pair_ref.py` and, bit for bit, against `mcg_shape_tanimoto`'s; the Gram matrix it leaves in
`gram_ws` against the fp64 Gram of those density bits; the Tanimoto map bit for bit against numpy float32 on those Gram bits;
every batch size on either side of a tile edge under every tile size, and the batches at which the library changes the
tile size by itself; and the pair matrix against `mcg_shape_tanimoto_field`.  The inputs are the small FULL grids of
`tests/shape_pair_cases.py` (padded columns, partial density workgroups, weight in every k-block); the conditions they meet
and the density tolerance are established without a GPU in `tests/test_shape_pair_stages_host.py`.  Every call writes into
NaN-filled buffers that sit between guard words, and all three buffers are read back."""
import functools

import numpy as np
import pytest
import torch

import shape_pair_cases as C
import shape_pair_ref as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 256                      # words on either side of every output; a multiple of 4, so rows stay 16-byte aligned
FILL = -7.0
IDENTITY = np.eye(3, dtype=np.float32).reshape(1, 9)


def _guarded(size):
    t = torch.full((GUARD + size + GUARD,), FILL, device=DEV)
    t[GUARD:GUARD + size] = float("nan")
    return t


def _read(t, size, what):
    h = t.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + size:] == FILL).all(), f"{what}: guard words overwritten"
    return h[GUARD:GUARD + size].copy()


def _pair_kernel(x, n_nodes, name, n, grid="box"):
    """`mcg_shape_pair_tanimoto` called directly: (density_ws [B, Gp], gram_ws [B, B], tanimoto [B, B]) fp32 on the host."""
    from ml_conformer_generator_amd import _lib
    B, N, _ = x.shape
    Gp = C.padded(n)
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV)
    nd = torch.from_numpy(np.array(n_nodes, dtype=np.int32)).to(DEV)
    xf = torch.from_numpy(C.xform12(name)).to(DEV)
    ax = torch.from_numpy(C.axes(n, grid)).to(DEV).contiguous()
    dens, gram, tani = _guarded(B * Gp), _guarded(B * B), _guarded(B * B)
    _lib.check(_lib.lib().mcg_shape_pair_tanimoto(_lib.dptr(xd), _lib.dptr(nd), B, N, _lib.dptr(xf), _lib.dptr(ax), n,
                                                  float(P.ALPHA), float(P.AMPLITUDE), dens[GUARD:].data_ptr(),
                                                  gram[GUARD:].data_ptr(), tani[GUARD:].data_ptr(),
                                                  _lib.current_stream_ptr(DEV)), "mcg_shape_pair_tanimoto")
    return (_read(dens, B * Gp, "density_ws").reshape(B, Gp), _read(gram, B * B, "gram_ws").reshape(B, B),
            _read(tani, B * B, "tanimoto").reshape(B, B))


@functools.lru_cache(maxsize=None)
def _stage_run(n, name, grid="box"):
    """The stage batch through the kernel, once per grid size, transform and grid."""
    ref = P.stage_reference(n, name, grid)
    return _pair_kernel(ref["x"], ref["n_nodes"], name, n, grid)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_gram(F, G, n_nodes, entries=None):
    """Step 3: `gram_ws` against the fp64 Gram of the density bits F, within `gram_bound`; NaN rows and columns for the
    empty molecules, everything else finite; exact symmetry.  `entries` = (i [K], j [K]): those entries only (between any
    rows).  Returns the worst |error| / bound."""
    live = np.flatnonzero(np.asarray(n_nodes) > 0)
    dead = np.flatnonzero(np.asarray(n_nodes) == 0)
    assert np.array_equal(_bits(G), _bits(G.T)), "gram_ws is not exactly symmetric"
    assert np.isnan(G[dead]).all() and np.isnan(G[:, dead]).all() and np.isfinite(G[np.ix_(live, live)]).all()
    F64 = F.astype(np.float64)
    L = F.shape[1] // C.KSPLIT
    if entries is None:
        want, bound = P.gram(F64[live]), P.gram_bound(F64[live])
        got = G[np.ix_(live, live)].astype(np.float64)
    else:
        i, j = entries
        keep = (np.asarray(n_nodes)[i] > 0) & (np.asarray(n_nodes)[j] > 0)
        i, j = i[keep], j[keep]
        want = np.einsum("kg,kg->k", F64[i], F64[j])
        bound = 2.0 * (L + 2) * P.EPS32 * np.einsum("kg,kg->k", np.abs(F64[i]), np.abs(F64[j]))
        got = G[i, j].astype(np.float64)
    assert got.size > 0 or live.size == 0
    ratio = float((np.abs(got - want) / bound).max()) if got.size else 0.0
    assert ratio <= 1.0, ("gram_ws against the fp64 Gram of its densities", ratio)
    return ratio


def _check_tanimoto(G, T, n_nodes):
    """Step 4: `tanimoto` is numpy float32 g / ((g_ii + g_jj) - g) on the `gram_ws` bits, bit for bit; exactly 1 on the
    diagonal of every non-empty row."""
    assert G.dtype == np.float32
    want = P.tanimoto(G)
    assert want.dtype == np.float32
    assert P.same_bits(T, want), "tanimoto is not the fp32 quotient of the gram_ws bits"
    live = np.flatnonzero(np.asarray(n_nodes) > 0)
    assert (np.diagonal(T)[live] == 1.0).all()


def test_the_constants_are_the_package_s():
    from ml_conformer_generator_amd.cheminformatics import ALPHA, AMPLITUDE
    assert float(ALPHA) == float(P.ALPHA) and float(AMPLITUDE) == float(P.AMPLITUDE)


# ----------------------------------------------------------------------------------------------- 1: density against fp64
@pytest.mark.parametrize("name", C.TRANSFORMS)
@pytest.mark.parametrize("n", C.GRID_SIZES)
@pytest.mark.parametrize("grid", list(C.GRIDS))
def test_density_stage_against_fp64(grid, n, name):
    """`density_ws`: every real column of every non-empty row within 4 x MEASURED_UNITS x unit(p) of the restatement; every
    padded column exactly +0.0; the empty rows NaN over their real columns.  On the cloud grid every atom of every row, the
    64th included, moves some point by hundreds of tolerances (host test); on the box only a row's first 40 or so do."""
    ref = P.stage_reference(n, name, grid)
    F, _, _ = _stage_run(n, name, grid)
    tol_units = P.density_tol_units(grid)
    total = n ** 3
    assert F.shape == (len(C.STAGE_BATCH), C.padded(n))
    assert (_bits(F[:, total:]) == 0).all(), "a padded column is not +0.0"
    worst = 0.0
    for b, k in enumerate(ref["n_nodes"]):
        if k == 0:
            assert np.isnan(F[b, :total]).all(), b
            continue
        r = np.abs(F[b, :total].astype(np.float64) - ref["F"][b, :total]) / (tol_units * ref["unit"][b])
        worst = max(worst, float(r.max()))
        assert float(r.max()) <= 1.0, (grid, n, name, b, int(k), float(r.max()))
    print(f"SHAPE-PAIR-STAGES density {grid} n={n} {name}: worst error / tolerance {worst:.3f} "
          f"(tolerance {tol_units:.2f} units)")


# ----------------------------------------------------------------------------------------------- 2: density against its twin
@pytest.mark.parametrize("n", C.GRID_SIZES)
@pytest.mark.parametrize("grid", list(C.GRIDS))
def test_density_stage_is_the_grid_tanimoto_s_density_bit_for_bit(grid, n):
    """Under the identity transform row b of `density_ws` is, bit for bit, the `f_scratch` that `mcg_shape_tanimoto` writes
    for ref = molecule b on the same axes (the header of csrc/mcg_shape_pair.hip: "the bits `k_shape_density` gives")."""
    from ml_conformer_generator_amd import _lib
    ref = P.stage_reference(n, "identity", grid)
    F, _, _ = _stage_run(n, "identity", grid)
    total = n ** 3
    ax = torch.from_numpy(C.axes(n, grid)).to(DEV).contiguous()
    rot = torch.from_numpy(IDENTITY).to(DEV)
    for b, k in enumerate(ref["n_nodes"]):
        if k == 0:
            continue
        mol = torch.from_numpy(np.array(ref["x"][b, :k])).to(DEV)
        nn = torch.tensor([int(k)], dtype=torch.int32, device=DEV)
        f, score = _guarded(total), _guarded(1)
        _lib.check(_lib.lib().mcg_shape_tanimoto(_lib.dptr(mol), int(k), _lib.dptr(mol), _lib.dptr(nn), 1, int(k),
                                                 _lib.dptr(rot), 1, _lib.dptr(ax), n, float(P.ALPHA), float(P.AMPLITUDE),
                                                 f[GUARD:].data_ptr(), score[GUARD:].data_ptr(),
                                                 _lib.current_stream_ptr(DEV)), "mcg_shape_tanimoto")
        assert np.array_equal(_bits(_read(f, total, "f_scratch")), _bits(F[b, :total])), (grid, n, b, int(k))
        assert float(_read(score, 1, "score")[0]) == 1.0                      # a molecule against itself


# ----------------------------------------------------------------------------------------------- 3 and 4: Gram, Tanimoto
@pytest.mark.parametrize("name", C.TRANSFORMS)
@pytest.mark.parametrize("n", C.GRID_SIZES)
@pytest.mark.parametrize("grid", list(C.GRIDS))
def test_gram_stage_against_the_fp64_gram_of_its_densities(grid, n, name):
    """`gram_ws` against the fp64 Gram of the density bits read back from the same call, within
    2 (L + 2) 2^-24 sum_k |F_ik F_jk| (`shape_pair_ref.gram_bound`: any fp32 order, nothing measured)."""
    F, G, _ = _stage_run(n, name, grid)
    worst = _check_gram(F, G, P.stage_reference(n, name, grid)["n_nodes"])
    print(f"SHAPE-PAIR-STAGES gram {grid} n={n} {name}: worst error / bound {worst:.4f} (L = {C.padded(n) // C.KSPLIT})")


@pytest.mark.parametrize("name", C.TRANSFORMS)
@pytest.mark.parametrize("n", C.GRID_SIZES)
@pytest.mark.parametrize("grid", list(C.GRIDS))
def test_tanimoto_stage_is_the_fp32_quotient_of_the_gram_bits(grid, n, name):
    _, G, T = _stage_run(n, name, grid)
    _check_tanimoto(G, T, P.stage_reference(n, name, grid)["n_nodes"])


# ----------------------------------------------------------------------------------------------- 5: batches and tiles
def _pair_of(cache, i, j, n):
    """(gram_ws, tanimoto) [2, 2] of molecules i and j alone, at their own tight width."""
    if (i, j) not in cache:
        x, nn = C.rows([i, j], "identity", C.tight([i, j]))
        _, G, T = _pair_kernel(x, nn, "identity", n)
        cache[(i, j)] = (G, T)
    return cache[(i, j)]


def _same_as_pairs(G, T, ids, n, cache, tag):
    B = len(ids)
    for i, j in C.sample_pairs(B):
        G2, T2 = _pair_of(cache, int(ids[i]), int(ids[j]), n)
        at = np.ix_([i, j], [i, j])
        assert P.same_bits(G[at], G2), (tag, "gram_ws", i, j)
        assert P.same_bits(T[at], T2), (tag, "tanimoto", i, j)


@pytest.mark.parametrize("n", [5, 13])
def test_every_batch_on_a_tile_edge_under_every_tile_size(n, monkeypatch):
    """B = 1, 2, 15 .. 17, 31 .. 33, 63 .. 65, 97 rows under MCG_SHAPE_PAIR_TILE = 1, 2, 4, each as two batches: "wide",
    molecules 0 .. B - 1 (every kind) at N = 64, and "narrow", the first B molecules of at most 23 atoms at N = 23.
    `gram_ws` and `tanimoto` of a pair have the same bits whatever B, tile size, row and width: against the same two
    molecules in a B = 2 call at their own width, against the other tile sizes and the 97-row batch of the same kind, and -
    the molecules that the two 97-row batches share - between N = 64 and N = 23.  Steps 3 and 4 hold throughout."""
    pairs, runs = {}, {}
    worst = 0.0
    batches = {"wide": (np.arange, 64), "narrow": (C.narrow_ids, 23)}
    for tile in C.TILES:
        monkeypatch.setenv("MCG_SHAPE_PAIR_TILE", str(tile))
        for B in C.FORCED_B:
            for kind, (make, N) in batches.items():
                ids = make(B)
                x, nn = C.rows(ids, "identity", N)
                assert x.shape == (B, N, 3)
                runs[(kind, tile, B)] = (ids, nn) + _pair_kernel(x, nn, "identity", n)
    monkeypatch.delenv("MCG_SHAPE_PAIR_TILE")
    Bmax = max(C.FORCED_B)
    for (kind, tile, B), (ids, nn, F, G, T) in runs.items():
        tag = f"n={n} {kind} tile={tile} B={B}"
        top = runs[(kind, C.TILES[0], Bmax)]
        assert np.array_equal(ids, top[0][:B])
        worst = max(worst, _check_gram(F, G, nn))
        _check_tanimoto(G, T, nn)
        assert np.array_equal(_bits(F), _bits(top[2][:B])), tag                 # NaN rows included: one NaN, one bit pattern
        assert P.same_bits(G, top[3][:B, :B]) and P.same_bits(T, top[4][:B, :B]), tag
        _same_as_pairs(G, T, ids, n, pairs, tag)
    wide, narrow = runs[("wide", C.TILES[0], Bmax)], runs[("narrow", C.TILES[0], Bmax)]
    shared, at_wide, at_narrow = np.intersect1d(wide[0], narrow[0], return_indices=True)
    assert len(shared) > 60 and set(wide[1][at_wide].tolist()) == {0, 1, 2, 23}
    assert np.array_equal(_bits(wide[2][at_wide]), _bits(narrow[2][at_narrow]))
    for k in (3, 4):
        assert P.same_bits(wide[k][np.ix_(at_wide, at_wide)], narrow[k][np.ix_(at_narrow, at_narrow)]), k
    print(f"SHAPE-PAIR-STAGES batches n={n}: {len(runs)} runs, {len(pairs)} pairs alone, {len(shared)} molecules at both "
          f"widths, worst gram error / bound {worst:.4f}")


@pytest.mark.parametrize("B", C.NATURAL_B)
def test_the_library_s_own_tile_choice(B, monkeypatch):
    """B = 992, 993 and 1985 at n = 5, either side of `pick_tile`'s two thresholds (16-row tiles up to 992, 32-row from 993,
    64-row from 1985, where `k_pair_tanimoto` also starts to stride): the run left to itself has the bits of the three forced
    runs; step 3 on 4096 sampled entries and the last row and column, step 4 in full, sampled pairs against B = 2 calls."""
    n = 5
    monkeypatch.delenv("MCG_SHAPE_PAIR_TILE", raising=False)
    ids = np.arange(B)
    x, nn = C.rows(ids, "identity", 64)
    F, G, T = _pair_kernel(x, nn, "identity", n)
    g = np.random.default_rng(B)
    last = np.full(B, B - 1)
    i = np.concatenate([g.integers(0, B, 4096), last, ids])
    j = np.concatenate([g.integers(0, B, 4096), ids, last])
    worst = _check_gram(F, G, nn, entries=(i, j))
    _check_tanimoto(G, T, nn)
    _same_as_pairs(G, T, ids, n, {}, f"B={B} natural")
    for tile in C.TILES:
        monkeypatch.setenv("MCG_SHAPE_PAIR_TILE", str(tile))
        Ff, Gf, Tf = _pair_kernel(x, nn, "identity", n)
        assert np.array_equal(_bits(Ff), _bits(F)) and P.same_bits(Gf, G) and P.same_bits(Tf, T), (B, tile)
    print(f"SHAPE-PAIR-STAGES natural B={B} (restated choice: {16 * C.natural_tile(B)}-row tiles): worst sampled gram error / "
          f"bound {worst:.4f}")


# ----------------------------------------------------------------------------------------------- cross-kernel
@pytest.mark.parametrize("n", C.GRID_SIZES)
def test_pair_matrix_against_the_field_tanimoto(n):
    """T_ab against `mcg_shape_tanimoto_field(f = density row a, cand = molecule b, identity)` on the same grid.  Both kernels
    sum the same density bits (test 2) in fp32 in their own orders - the field kernel in fused chains of ceil(n^3 / 256), six
    butterfly levels and two adds, no deeper than L + 2 on these grids - so each lies within `gram_bound` of the exact sums
    <f,g>, <f,f>, <g,g> of those bits, and within `tanimoto_bound` of their exact quotient.  Both are held to that."""
    from ml_conformer_generator_amd import _lib
    assert -(-n ** 3 // 256) + 8 <= C.padded(n) // C.KSPLIT + 2
    ref = P.stage_reference(n, "identity")
    F, _, T = _stage_run(n, "identity")
    nn_h = ref["n_nodes"]
    live = np.flatnonzero(nn_h > 0)
    F64 = F[live].astype(np.float64)
    S, dS = P.gram(F64), P.gram_bound(F64)
    B, total = len(nn_h), n ** 3
    xd = torch.from_numpy(ref["x"].copy()).to(DEV)
    nd = torch.from_numpy(nn_h.copy()).to(DEV)
    ax = torch.from_numpy(C.axes(n)).to(DEV).contiguous()
    rot = torch.from_numpy(IDENTITY).to(DEV)
    worst = {"field": 0.0, "pair": 0.0}
    for ia, a in enumerate(live):
        f = torch.from_numpy(F[a, :total].copy()).to(DEV)
        score = _guarded(B)
        _lib.check(_lib.lib().mcg_shape_tanimoto_field(_lib.dptr(f), _lib.dptr(xd), _lib.dptr(nd), B, 64, _lib.dptr(rot), 1,
                                                       _lib.dptr(ax), n, float(P.ALPHA), float(P.AMPLITUDE),
                                                       score[GUARD:].data_ptr(), _lib.current_stream_ptr(DEV)),
                   "mcg_shape_tanimoto_field")
        got = _read(score, B, "score")
        for ib, b in enumerate(live):
            exact = S[ia, ib] / (S[ia, ia] + S[ib, ib] - S[ia, ib])
            allowed = P.tanimoto_bound(S[ia, ib], S[ia, ia], S[ib, ib], dS[ia, ib], dS[ia, ia], dS[ib, ib])
            for k, v in (("field", float(got[b])), ("pair", float(T[a, b]))):
                r = abs(v - exact) / allowed
                worst[k] = max(worst[k], r)
                assert r <= 1.0, (n, int(a), int(b), k, v, exact, allowed)
    print(f"SHAPE-PAIR-STAGES field n={n}: worst |T - exact quotient| / allowed: field kernel {worst['field']:.4f}, "
          f"pair kernel {worst['pair']:.4f}")
