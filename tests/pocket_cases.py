"""Receptors for the pocket tests (DESIGN.md section 6 "Pockets from the receptor"): a seeded block of jittered carbon /
nitrogen / oxygen / sulphur atoms on a 3 A lattice with an ellipsoidal cavity and a channel to the outside carved out of it
- no protein: it pins the arithmetic and the host pipeline, not chemistry - and the settings the carved-block figures of
tests/test_pocket_host.py were taken at.  Everything is computed once per process and never written to."""
import functools

import numpy as np

VDW = {6: 1.70, 7: 1.55, 8: 1.52, 16: 1.80}          # `receptor.VDW_RADII` of the block's elements
BLOCK = dict(spacing=1.0, radius=12.0, probe=1.4, reach=8.0, min_buriedness=16)      # the carved-block settings


def carved_block(seed=7, edge=36.0, spacing=3.0, jitter=0.3, semi=(9.0, 6.0, 5.0), channel=2.6):
    """(coords [R,3] fp64, atomic numbers [R] int64): the lattice points of a cube of `edge` centred on the origin, each
    moved by up to `jitter` per axis, without those inside the ellipsoid of semi-axes `semi` round the origin and those
    within `channel` of the +x axis."""
    rng = np.random.default_rng(seed)
    g = np.arange(-edge / 2, edge / 2 + 1e-9, spacing)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    p = p + rng.uniform(-jitter, jitter, p.shape)
    inside = ((p / np.array(semi)) ** 2).sum(1) < 1.0
    chan = (p[:, 0] > 0) & (np.hypot(p[:, 1], p[:, 2]) < channel)
    keep = ~(inside | chan)
    z = rng.choice([6, 6, 6, 7, 8, 16], size=p.shape[0])
    return p[keep], z[keep].astype(np.int64)


@functools.lru_cache(maxsize=None)
def block():
    xyz, z = carved_block()
    return xyz, z


def radii(z):
    return np.array([VDW[int(v)] for v in z], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def large_block():
    """A wider block (48 A, 4 869 atoms after carving) for the one shape beyond R = 1 025."""
    return carved_block(seed=11, edge=48.0)


def synthetic_receptor(R=100_000, seed=3, density=0.05):
    """(coords [R,3] fp64, atomic numbers [R]): R atoms spread uniformly at a protein's heavy-atom density (about 0.05 per
    cubic angstrom) in a cube round the origin, those within 6 A of the origin left out by moving them to the faces."""
    rng = np.random.default_rng(seed)
    edge = (R / density) ** (1.0 / 3.0)
    p = rng.uniform(-edge / 2, edge / 2, (R, 3))
    near = np.linalg.norm(p, axis=1) < 6.0
    p[near] = p[near] / np.linalg.norm(p[near], axis=1, keepdims=True) * (edge / 2)
    return p, rng.choice([6, 6, 6, 7, 8, 16], size=R).astype(np.int64)
