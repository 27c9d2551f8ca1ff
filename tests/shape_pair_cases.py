"""Inputs of the stage tests of `mcg_shape_pair_tanimoto` (`tests/test_shape_pair_stages_host.py`, `_gpu.py`): molecules,
full grids, transforms and batches.  Host only (numpy).

Molecules.  Molecule m (any m >= 0) is a prefix of the compact 64-atom cloud `lattice64` - KINDS[m % 6] atoms of it: 23, 0
(the empty row), 1, 2, 63, 64 - moved by `shift(m)`, at most SHIFT per component and different for every m, so that no two
rows of a batch are copies and a tile written to the wrong place shows.  A batch is a list of molecule numbers; `rows` pads
it to a width N and writes junk (NaN, 1e30, -inf) behind each row's atoms, and into the whole of the empty row.

Two grids, one per stage (GRIDS).
  "cloud", the DENSITY stage (steps 1 and 2 and the density mutations): x in [-2.4, 2.0], y in [-2.0, 2.4], z in [-1.6, 2.2],
    three different ranges that span the cloud, so that every atom of every prefix, atom 63 at (2.40, 2.41, 2.39) included,
    moves some grid point's density by many tolerances: an atom lost at the N = 64 edge, in the LDS staging loop or by a
    wrong row stride shows (`test_each_planted_mistake_is_seen_on_every_grid` asserts the last atom per row kind).
  "box", the GRAM stage and everything behind it: a box of 0.5 x 0.55 x 0.6 A inside the cloud round atom 0, at
    (-2.31, -2.31, -2.40), which every prefix holds, so that EVERY non-empty row, the single atom included, has a density of
    order 1 at every grid point and every 32-point k-block carries weight in every Gram entry
    (`test_every_kblock_and_quarter_carries_weight`).  The cloud grid cannot do that: at n = 8 the single atom puts 1.0e-11 of
    its Gram diagonal into the last quarter of the k range (4.6e-22 into its emptiest 32-point block), the pair 6.7e-12 and
    the 23-atom prefix 2.2e-4; only the 63- and 64-atom rows fill it.  The per-row shift is kept to 0.05 A for the same
    reason.  The price: on the box the atoms from about index 42 on have a factor of exactly 1.0f, so the box says nothing
    about a row's later atoms; that is the cloud grid's job.  The Gram and Tanimoto stages are checked on the cloud grid too
    (their bounds hold for any densities); the weight rule is only met on the box.

Grid sizes.  GRID_SIZES, with Gp = n^3 rounded up to `KALIGN` = 4 L (L = one wave's k range):
    n   n^3    Gp
    2      8   128   120 padded columns; one k-block per wave, three of them pure padding
    5    125   128   3 padded columns
    8    512   512   no padding; four k-blocks per wave
   11   1331  1408   77 padded columns
   13   2197  2304   a second density workgroup (2048 points each), partial, holding the padding
   16   4096  4096   exactly two density workgroups

Transforms.  "identity", and "moved": an arbitrary proper rotation M with t a few angstroms long.  The molecules are moved
with it (x = y @ M^T + t in fp64, rounded to fp32), so y = (x - t) @ M lands on the same grid and the same axes serve both.

Batches.  FORCED_B under every forced tile size (MCG_SHAPE_PAIR_TILE = 1, 2, 4) sit on both sides of every tile edge;
NATURAL_B at n = 5 sit on both sides of `pick_tile`'s two thresholds, restated in `natural_tile`."""
from __future__ import annotations

import functools
from typing import Dict, Sequence, Tuple

import numpy as np

KALIGN = 128                                  # MCG_SHAPE_PAIR_KALIGN
KSPLIT = 4                                    # waves of a Gram workgroup = k ranges
KBLOCK = 32                                   # grid points per wave per step
DENS_POINTS = 2048                            # grid points per density workgroup

KINDS: Tuple[int, ...] = (23, 0, 1, 2, 63, 64)
SHIFT = 0.05
GRID_SIZES: Tuple[int, ...] = (2, 5, 8, 11, 13, 16)
PADDING_FREE: Tuple[int, ...] = (8, 16)
AXIS_RANGES = ((-2.45, -1.95), (-2.40, -1.85), (-2.50, -1.90))              # "box": the Gram, Tanimoto and batch stages
CLOUD_RANGES = ((-2.4, 2.0), (-2.0, 2.4), (-1.6, 2.2))                       # "cloud": the density stage
GRIDS = {"box": AXIS_RANGES, "cloud": CLOUD_RANGES}
TRANSFORMS: Tuple[str, ...] = ("identity", "moved")
TILES: Tuple[int, ...] = (1, 2, 4)
FORCED_B: Tuple[int, ...] = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97)
NATURAL_B: Tuple[int, ...] = (992, 993, 1985)
STAGE_BATCH: Tuple[int, ...] = tuple(range(12))           # two molecules of every kind: the density and Gram stage tests
JUNK = (float("nan"), 1e30, float("-inf"))


def lattice64() -> np.ndarray:
    """A compact 64-atom cloud about the origin: a 4 x 4 x 4 lattice of 1.6 A, each atom moved by up to 0.15 A.  Compact, so
    that a candidate keeps overlapping the reference under any rotation about the origin, and every atom lies on the grid."""
    g = np.random.default_rng(5)
    k = (np.arange(4) - 1.5) * 1.6
    p = np.array([[x, y, z] for x in k for y in k for z in k]) + g.uniform(-0.15, 0.15, (64, 3))
    return p.astype(np.float32)


def padded(n: int) -> int:
    """Gp: n^3 rounded up to a multiple of KALIGN."""
    return (n ** 3 + KALIGN - 1) // KALIGN * KALIGN


def axes(n: int, grid: str = "box") -> np.ndarray:
    """axes [3, n] fp32: n evenly spaced points over each of the three ranges of GRIDS[grid]."""
    return np.stack([np.linspace(lo, hi, n) for lo, hi in GRIDS[grid]]).astype(np.float32)


_STEPS = np.array([0.8191725133961645, 0.6710436067037893, 0.5497004779019703])


def shift(m) -> np.ndarray:
    """The shift of molecule m (or of every molecule of an int array), fp64 [..., 3]: an additive recurrence on three
    irrational steps, so no two m share one."""
    return SHIFT * (2.0 * np.modf((np.asarray(m, dtype=np.float64)[..., None] + 1.0) * _STEPS)[0] - 1.0)


def atoms_of(m: int) -> int:
    return KINDS[m % len(KINDS)]


@functools.lru_cache(maxsize=None)
def transform(name: str) -> Tuple[np.ndarray, np.ndarray]:
    """(M [3,3] fp32, t [3] fp32) of the frame y = (x - t) @ M."""
    if name == "identity":
        return np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    assert name == "moved"
    w, x, y, z = np.array([0.61, -0.43, 0.52, 0.41]) / np.linalg.norm([0.61, -0.43, 0.52, 0.41])
    M = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert np.linalg.det(M) > 0.999 and float(np.abs(M - M.T).max()) > 0.3          # proper, and not symmetric
    return M.astype(np.float32), np.array([3.1, -2.7, 1.9], dtype=np.float32)


def xform12(name: str) -> np.ndarray:
    """ref_xform [12] fp32 as the C entry takes it: M row-major, then t."""
    M, t = transform(name)
    return np.concatenate([M.reshape(9), t]).astype(np.float32)


def _place(y: np.ndarray, name: str) -> np.ndarray:
    """x = y @ M^T + t in fp64, written out element by element so that a molecule has the same bits in any batch."""
    M, t = (a.astype(np.float64) for a in transform(name))
    x = np.stack([(y[..., 0] * M[k, 0] + y[..., 1] * M[k, 1]) + y[..., 2] * M[k, 2] + t[k] for k in range(3)], axis=-1)
    return x.astype(np.float32)


def molecule(m: int, name: str = "identity") -> np.ndarray:
    """Coordinates [atoms_of(m), 3] fp32 of molecule m as the kernel is given them under transform `name`."""
    return _place(lattice64()[: atoms_of(m)].astype(np.float64) + shift(m), name)


def rows(ids: Sequence[int], name: str = "identity", N: int = 64) -> Tuple[np.ndarray, np.ndarray]:
    """(x [B, N, 3] fp32, n_nodes [B] int32) of the molecules `ids`, junk behind every row's atoms."""
    ids = np.asarray(ids, dtype=np.int64)
    n_nodes = np.array(KINDS, dtype=np.int32)[ids % len(KINDS)]
    assert int(n_nodes.max()) <= N <= 64
    x = _place(lattice64()[:N].astype(np.float64)[None, :, :] + shift(ids)[:, None, :], name)
    junk = np.resize(np.array(JUNK, dtype=np.float32), (N, 3))
    beyond = np.arange(N)[None, :] >= n_nodes[:, None]
    x[beyond] = np.broadcast_to(junk, x.shape)[beyond]
    return np.ascontiguousarray(x), n_nodes


def tight(ids: Sequence[int]) -> int:
    """The narrowest N that holds every row of `ids` (at least 1: the C entry takes no N = 0)."""
    return max(1, max(atoms_of(int(m)) for m in ids))


def narrow_ids(B: int) -> np.ndarray:
    """The first B molecules of at most 23 atoms (kinds 23, 0, 1, 2): a batch of any size that runs at N = 23."""
    m = np.arange(2 * B + 6)
    return m[m % len(KINDS) < 4][:B]


def natural_tile(B: int) -> int:
    """`pick_tile` of csrc/mcg_shape_pair.hip restated: the largest tile side 16 RT whose upper triangle of tiles still
    holds 512 workgroups.  A restatement read side by side with the library's function, NOT a check of it: nothing a test
    can observe says which tile size ran, so that the natural batches cross the thresholds rests on that reading."""
    def tiles(rt: int) -> int:
        nt = (B + 16 * rt - 1) // (16 * rt)
        return nt * (nt + 1) // 2
    return 4 if tiles(4) >= 512 else 2 if tiles(2) >= 512 else 1


def sample_pairs(B: int) -> Tuple[Tuple[int, int], ...]:
    """Pairs (i, j) of a batch of B rows that are compared with a B = 2 call of the same two molecules: the corners of the
    matrix and both sides of every 16-, 32- and 64-row tile edge the batch has."""
    edge = sorted({r for e in (16, 32, 64) for r in (e - 1, e) if r < B} | {0, B - 1})
    out = {(0, B - 1), (B - 1, B - 1), (max(B - 2, 0), B - 1)}
    for a, b in zip(edge, edge[1:]):
        out.add((a, b))
        out.add((b, B - 1))
    return tuple(sorted((i, j) for i, j in out if i != j or i == B - 1))


def describe() -> Dict[int, Dict[str, int]]:
    """Per grid size: n^3, Gp, padded columns, k-blocks per wave, density workgroups."""
    return {n: {"points": n ** 3, "Gp": padded(n), "padding": padded(n) - n ** 3,
                "blocks_per_wave": padded(n) // KSPLIT // KBLOCK,
                "density_workgroups": (padded(n) + DENS_POINTS - 1) // DENS_POINTS} for n in GRID_SIZES}
