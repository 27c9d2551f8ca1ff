"""The meshes and test points of the solid-reference tests (tests/test_mesh_host.py, tests/test_mesh_gpu.py): a tetrahedron,
a cube, boxes, the demo pocket (tests/golden/pocket_6q8k_mesh.npz) and its open prefixes at every tile and split boundary of
`csrc/mcg_mesh.hip`; random points in the padded bounding box and probe points 0.05 A off chosen triangles' centroids."""
import functools
import os

import numpy as np
import torch

from ml_conformer_generator_amd import mesh as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 256                                   # csrc/mcg_mesh.hip MW_TILE
# the kernel cuts F triangles into ceil(ceil(F / 256) / 4) parts: one part up to 1024, two up to 2048, three up to 3072
PREFIXES = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
# triangles either side of every tile edge the pocket's three parts touch (tiles [0,3), [3,6), [6,10)), first and last
EDGE_TRIANGLES = (0, 255, 256, 257, 511, 512, 767, 768, 1023, 1024, 1535, 1536, 2047, 2048, 2303, 2304, 2487)
BATCHES = (1, 63, 64, 65, 257)
PROBE_OFFSET = 0.05

_BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6],
                       [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def box(a, b, c, origin=(0.0, 0.0, 0.0)):
    """The axis-aligned box [0,a] x [0,b] x [0,c] moved to `origin`, as (vertices, faces)."""
    v = np.array([[x, y, z] for x in (0.0, a) for y in (0.0, b) for z in (0.0, c)]) + np.asarray(origin)
    return v, _BOX_FACES.copy()


def tetrahedron():
    v = np.array([[0.25, -0.25, 0.125], [2.125, 0.375, -0.25], [0.5, 1.875, 0.25], [0.75, 0.625, 1.75]])    # exact in fp32
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


@functools.lru_cache(maxsize=None)
def pocket():
    z = np.load(os.path.join(GOLDEN, "pocket_6q8k_mesh.npz"))
    return M.load_mesh((z["v"], z["f"].astype(np.int64)))


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    return {"tetrahedron": lambda: M.load_mesh(tetrahedron()), "cube": lambda: M.load_mesh(box(2.0, 2.0, 2.0, (-1, 3, 0.5))),
            "pocket": pocket}[name]()


def triangles(mesh, F=None):
    """[F,3,3] fp32 corner coordinates of the mesh's first F faces (all by default)."""
    return torch.from_numpy(mesh.vertices[mesh.faces[:F]].copy())


def random_points(mesh, P, seed, pad=3.0):
    g = np.random.default_rng(seed)
    lo, hi = mesh.vertices.min(0) - pad, mesh.vertices.max(0) + pad
    return torch.from_numpy((lo + g.random((P, 3)) * (hi - lo)).astype(np.float32))


def probe_points(mesh, owners, offset=PROBE_OFFSET):
    """Two points per triangle of `owners`, `offset` off its centroid along + and - its normal: ([2k,3] fp32, owner of each).
    The owner contributes about +-0.5 there, so a skipped triangle shows."""
    t = mesh.triangles[list(owners)]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cen = t.mean(axis=1)
    pts = np.concatenate([cen + offset * nrm, cen - offset * nrm]).astype(np.float32)
    return torch.from_numpy(pts), list(owners) * 2


def probe_owners(mesh, extra=30, seed=5):
    F = mesh.faces.shape[0]
    own = [k for k in EDGE_TRIANGLES if k < F]
    own += [int(k) for k in np.random.default_rng(seed).choice(F, min(extra, F), replace=False)]
    return sorted(set(own))


def test_points(name, P, seed):
    """(mesh, points [P + probes, 3] fp32, probe owners, index of the first probe point) for the closed mesh `name`."""
    mesh = mesh_of(name)
    probes, owners = probe_points(mesh, probe_owners(mesh))
    rnd = random_points(mesh, P, seed)
    return mesh, torch.cat([rnd, probes]), owners, P


def lattice(shape=(2, 3, 5), spacing=1.5):
    """A rectangular lattice of points centred on the origin, [n,3] fp32."""
    ax = [(torch.arange(k, dtype=torch.float64) - (k - 1) / 2) * spacing for k in shape]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3).to(torch.float32)


def rigid_motion(seed):
    """A random proper rotation [3,3] and translation [3], fp64."""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r)).unsqueeze(0)
    if float(torch.det(q)) < 0:
        q[:, 2] = -q[:, 2]
    return q, torch.randn(3, generator=g, dtype=torch.float64) * 4.0
