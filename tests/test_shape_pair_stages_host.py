"""The pairwise shape kernels pinned stage by stage, host side (no GPU): the conditions the inputs of
`tests/shape_pair_cases.py` must meet for the GPU checks of `tests/test_shape_pair_stages_gpu.py` to have teeth, shown on the
fp64 restatement of `tests/shape_pair_ref.py` - every planted mistake moves a checked quantity by at least 10 tolerances on
every grid, every k-block and quarter of the k range carries weight in every Gram entry - and the measurement of the
density's error unit that sets the GPU tolerance."""
import numpy as np
import pytest

import shape_pair_cases as C
import shape_pair_ref as P
import shape_ref as R

SEEN = 10.0                      # a mistake counts as seen from 10 tolerances on


def _live(ref):
    return np.flatnonzero(ref["n_nodes"] > 0)


# ----------------------------------------------------------------------------------------------- the inputs
def test_the_cases_are_what_the_gpu_tests_rely_on():
    table = {2: (8, 128, 1, 1), 5: (125, 128, 1, 1), 8: (512, 512, 4, 1), 11: (1331, 1408, 11, 1), 13: (2197, 2304, 18, 2),
             16: (4096, 4096, 32, 2)}
    d = C.describe()
    for n, (points, Gp, blocks, groups) in table.items():
        assert (d[n]["points"], d[n]["Gp"], d[n]["blocks_per_wave"], d[n]["density_workgroups"]) == (points, Gp, blocks,
                                                                                                    groups), n
    assert [n for n in C.GRID_SIZES if d[n]["padding"] == 0] == list(C.PADDING_FREE)
    assert d[13]["points"] > C.DENS_POINTS and d[13]["Gp"] < 2 * C.DENS_POINTS      # the second workgroup holds the padding
    assert len({tuple(r) for r in C.AXIS_RANGES}) == 3 and len({tuple(r) for r in C.CLOUD_RANGES}) == 3
    cloud = C.lattice64()
    for (lo, hi), c in zip(C.CLOUD_RANGES, cloud.T):
        assert float(c.min()) - 0.2 <= lo < hi <= float(c.max()) + 0.2 and hi - lo > 3.5     # spans the cloud, inside it
    for B in C.FORCED_B:
        ids = C.narrow_ids(B)
        assert len(ids) == B and C.tight(ids) == 23 and np.array_equal(ids, C.narrow_ids(97)[:B])
    atom0 = C.lattice64()[0]
    for (lo, hi), c in zip(C.AXIS_RANGES, atom0):
        assert lo < c < hi and -2.55 <= lo and hi <= 2.55                           # inside the cloud, atom 0 inside the box
    ids = np.arange(max(C.NATURAL_B))
    sh = C.shift(ids).astype(np.float32)
    assert C.SHIFT <= 0.4 and float(np.abs(sh).max()) <= C.SHIFT
    assert len({tuple(r) for r in sh.tolist()}) == len(ids)                          # unique to the row, in fp32 too
    assert sorted(C.KINDS) == [0, 1, 2, 23, 63, 64]
    for name in C.TRANSFORMS:
        x, n_nodes = C.rows(C.STAGE_BATCH, name)
        assert x.shape == (12, 64, 3) and x.dtype == np.float32 and sorted(set(n_nodes.tolist())) == sorted(C.KINDS)
        xt, _ = C.rows(C.STAGE_BATCH[:4], name, C.tight(C.STAGE_BATCH[:4]))
        assert xt.shape[1] == 23
        for b, m in enumerate(C.STAGE_BATCH):
            k = int(n_nodes[b])
            assert np.array_equal(x[b, :k], C.molecule(m, name)), (name, m)          # a molecule's bits: the same in any batch
            assert np.isnan(x[b, k:]).any() == (k < 64) and np.isfinite(x[b, :k]).all()
            if b < 4:
                assert np.array_equal(xt[b, :k], x[b, :k])
    M, t = C.transform("moved")
    assert float(np.abs(M.astype(np.float64).T @ M.astype(np.float64) - np.eye(3)).max()) < 1e-6 and np.linalg.norm(t) > 3
    # `pick_tile`: the natural batches sit on both sides of its two thresholds; `k_pair_tanimoto` strides above 8192 x 256
    assert [C.natural_tile(B) for B in C.NATURAL_B] == [1, 2, 4] and C.natural_tile(1984) == 2
    assert 1448 ** 2 <= 8192 * 256 < 1449 ** 2 <= max(C.NATURAL_B) ** 2
    for B in C.FORCED_B:
        assert all(0 <= i <= j < B for i, j in C.sample_pairs(B)) and (B - 1, B - 1) in C.sample_pairs(B)
    for e in (16, 32, 64):
        assert {e - 1, e, e + 1} <= set(C.FORCED_B)


def test_the_restatement_agrees_with_the_grid_restatement_of_shape_ref():
    """Two restatements written apart: the density of `shape_ref.grid_density` on the frame coordinates, the Gram matrix as
    one product, Tanimoto's closed properties."""
    for name in C.TRANSFORMS:
        ref = P.stage_reference(5, name)
        M, t = C.transform(name)
        for b in _live(ref):
            y = P.frame_coords(ref["x"][b, : ref["n_nodes"][b]], M, t)
            want = R.grid_density(y, C.axes(5), P.ALPHA, P.AMPLITUDE)
            assert float(np.abs(ref["F"][b, :125] - want).max()) < 1e-13
            assert (ref["F"][b, 125:] == 0.0).all()
    F = P.stage_reference(8, "identity")["F"]
    G = P.gram(F)
    live = _live(P.stage_reference(8, "identity"))
    assert float(np.abs(G - F @ F.T)[np.ix_(live, live)].max()) < 1e-12 * float(G[np.ix_(live, live)].max())
    assert np.isnan(G[1]).all() and np.isnan(G[:, 7]).all()
    T = P.tanimoto(G)
    assert np.array_equal(T, T.T, equal_nan=True) and (np.diagonal(T)[live] == 1.0).all()
    sub = T[np.ix_(live, live)]
    assert float(sub.min()) > 0.0 and float(sub.max()) == 1.0 and float(np.sort(sub.ravel())[-len(live) - 1]) < 1.0


# ----------------------------------------------------------------------------------------------- the tolerance, measured
def test_density_error_unit_is_measured_on_the_host(capsys):
    """The measurement behind `shape_pair_ref.MEASURED_UNITS`: numpy float32 in the kernel's operation order against the fp64
    restatement, in units of `density_unit`, over both grids, every grid size, transform and molecule of the stage batch."""
    worst = {}
    for grid in C.GRIDS:
        for name in C.TRANSFORMS:
            M, t = C.transform(name)
            worst[(grid, name)] = (0.0, "")
            for n in C.GRID_SIZES:
                ref = P.stage_reference(n, name, grid)
                for b in _live(ref):
                    got = P.density_fp32(ref["x"][b, : ref["n_nodes"][b]], M, t, C.axes(n, grid), P.ALPHA, P.AMPLITUDE)
                    r = float((np.abs(got.astype(np.float64) - ref["F"][b, : n ** 3]) / ref["unit"][b]).max())
                    if r > worst[(grid, name)][0]:
                        worst[(grid, name)] = (r, f"n={n} molecule {C.STAGE_BATCH[b]} ({ref['n_nodes'][b]} atoms)")
    with capsys.disabled():
        print()
        for (grid, name), (r, tag) in worst.items():
            print(f"SHAPE-PAIR-REF density emulation {grid:5s} {name:8s}: worst {r:.3f} units at {tag}   "
                  f"(GPU tolerance {P.density_tol_units(grid):.2f})")
    box = max(r for (grid, _), (r, _) in worst.items() if grid == "box")
    top = max(r for r, _ in worst.values())
    assert box <= P.MEASURED_UNITS["pair_density_box"] <= 1.05 * box                 # the records are the measurements
    assert top <= P.MEASURED_UNITS["pair_density"] <= 1.05 * top
    assert all(P.TOL_UNITS[k] == 4.0 * v for k, v in P.MEASURED_UNITS.items())


# ----------------------------------------------------------------------------------------------- every block carries weight
def test_every_kblock_and_quarter_carries_weight():
    """Every 32-point k-block and every quarter of the k range holds at least 1 / 8 of an equal share of EVERY Gram entry
    between non-empty rows: 1 / (8 n^3) per grid point it holds - on the padding-free grids 1 / (8 x blocks) per block and
    1 / 32 per quarter.  Blocks and quarters of pure padding hold nothing and are exempt."""
    for name in C.TRANSFORMS:
        for n in C.GRID_SIZES:
            ref = P.stage_reference(n, name)
            live = _live(ref)
            F = ref["F"][live]
            G = P.gram(F)
            total, Gp = n ** 3, F.shape[1]
            L = Gp // C.KSPLIT
            least = np.inf
            for width in (C.KBLOCK, L):
                for lo in range(0, Gp, width):
                    held = max(0, min(lo + width, total) - lo)
                    if held == 0:
                        continue
                    share = (F[:, lo:lo + width] @ F[:, lo:lo + width].T) / G
                    floor = held / (8.0 * total)
                    if n in C.PADDING_FREE:
                        assert floor == (1.0 / (8 * (Gp // C.KBLOCK)) if width == C.KBLOCK else 1.0 / 32)
                    least = min(least, float(share.min()) / floor)
                    assert float(share.min()) >= floor, (name, n, width, lo, float(share.min()), floor)
            print(f"SHAPE-PAIR-REF shares {name} n={n}: least share / floor = {least:.2f}")


# ----------------------------------------------------------------------------------------------- the checks have teeth
def _density_mutation_ratios(n, mutation, grid):
    """{atoms of the row: least over the rows of that kind of max |mutated - true| / tolerance over the real columns} of the
    stage batch under "moved" on `grid`."""
    ref = P.stage_reference(n, "moved", grid)
    M, t = C.transform("moved")
    bad = P.density_rows(ref["x"], ref["n_nodes"], M, t, C.axes(n, grid), P.ALPHA, P.AMPLITUDE, mutation)
    out = {}
    for b in _live(ref):
        tol = P.density_tol_units(grid) * ref["unit"][b]
        r = float((np.abs(bad[b, : n ** 3] - ref["F"][b, : n ** 3]) / tol).max())
        k = int(ref["n_nodes"][b])
        out[k] = min(out.get(k, np.inf), r)
    return out


def _gram_mutation_ratio(F, mutation, which):
    G = P.gram(F)
    return float((np.abs(P.gram(F, mutation, which) - G) / P.gram_bound(F)).max())


@pytest.mark.parametrize("mutation", P.MUTATIONS)
def test_each_planted_mistake_is_seen_on_every_grid(mutation):
    """On every grid size each mutated restatement is at least 10 tolerances from the true one in the quantity its stage
    checks - the density in 4 x MEASURED_UNITS x unit, a Gram entry in `gram_bound` - or breaks a check that has no
    tolerance (padded columns exactly +0, exact symmetry).  The density mistakes are seen on both grids; the lost last atom on
    the cloud grid in EVERY kind of row, 1, 2, 23, 63 and 64 atoms (on the box the later atoms of a row weigh nothing).  For the k-block, wave and combine mistakes that holds for every
    block, wave and pair of slots that hold grid points at all (two ranges of pure padding are both exactly 0: reading one
    for the other is no mistake that arithmetic can show)."""
    least = np.inf
    for n in C.GRID_SIZES:
        ref = P.stage_reference(n, "identity")
        live = _live(ref)
        F = ref["F"][live]
        total, Gp = n ** 3, F.shape[1]
        L = Gp // C.KSPLIT
        held = [max(0, min((w + 1) * L, total) - w * L) for w in range(C.KSPLIT)]
        if mutation == "drop_last_atom":                  # on the cloud grid, for every kind of row: its last atom counts
            seen = list(_density_mutation_ratios(n, mutation, "cloud").values())
            assert len(seen) == 5
        elif mutation in ("swap_iy_iz", "keep_t", "transpose_m"):                   # on either grid, in some row
            seen = [max(_density_mutation_ratios(n, mutation, grid).values()) for grid in C.GRIDS]
        elif mutation == "pad_nonzero":
            if Gp == total:
                continue
            M, t = C.transform("identity")
            bad = P.density_rows(ref["x"], ref["n_nodes"], M, t, C.axes(n), P.ALPHA, P.AMPLITUDE, mutation)
            assert (bad[live, total:] != 0.0).all() and (ref["F"][:, total:] == 0.0).all()    # "exactly +0" is violated
            continue
        elif mutation == "drop_kblock":
            seen = [_gram_mutation_ratio(F, mutation, (w, blk)) for w in range(C.KSPLIT) for blk in range(L // C.KBLOCK)
                    if w * L + blk * C.KBLOCK < total]
            assert len(seen) == -(-total // C.KBLOCK)
        elif mutation == "drop_wave":
            seen = [_gram_mutation_ratio(F, mutation, w) for w in range(C.KSPLIT) if held[w]]
        elif mutation == "combine_twice":
            seen = [_gram_mutation_ratio(F, mutation, (dst, src)) for dst in range(C.KSPLIT) for src in range(C.KSPLIT)
                    if dst != src and (held[dst] or held[src])]
            assert len(seen) == (6 if n == 2 else 12)
        else:
            assert mutation == "unmirrored"
            Fall = ref["F"]
            for rows, i, j in ((16, 2, 0), (16, 11, 10), (32, 9, 3), (64, 5, 4)):
                G = P.gram(Fall, mutation, (rows, i, j))
                assert not np.array_equal(G, G.T, equal_nan=True)                           # "exactly symmetric" is violated
                assert np.array_equal(P.gram(Fall), P.gram(Fall).T, equal_nan=True)
            continue
        least = min(least, min(seen))
        assert min(seen) >= SEEN, (mutation, n, min(seen))
    if np.isfinite(least):
        print(f"SHAPE-PAIR-REF mutation {mutation}: at least {least:.3g} tolerances on every grid")
