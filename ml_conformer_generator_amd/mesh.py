"""Watertight triangle meshes as reference shapes ("Solid references"): what the reference's notebook
does with `trimesh` (sections 3, 4.1, 4.2: load a watertight STL, `density = 0.02`, `principal_inertia_components` as the
`reference_context`), host side, in fp64 numpy, without `trimesh` and without a GPU.

  load_mesh        STL (binary or ASCII) / (vertices, faces) / an object with both -> a welded, watertight, outward `Mesh`;
  mass_properties  volume, centre of mass, covariance, inertia tensor and its principal components, as exact polyhedral
                   integrals over the signed tetrahedra (origin, a, b, c) of the faces;
  mesh_context     the fp32 [3] tensor the notebook passes as `reference_context`;
  solid_frame      the solid's counterpart of `mcg_shape_frames_tf`'s xform: a proper rotation onto the principal axes of
                   the covariance (descending) and the centroid.
The device side (winding number, occupancy, atoms outside) is `cheminformatics.solid_reference` over `csrc/mcg_mesh.hip`.
"""
from __future__ import annotations

import dataclasses
import io
import os
import re
import struct
from typing import Dict, Tuple

import numpy as np

MAX_FACES = 1 << 20           # include/mlconfgen_hip.h MCG_MESH_MAX_FACES
DEFAULT_DENSITY = 0.02        # the notebook's `density`

_NOT_WATERTIGHT = "The mesh needs to be watertight."


@dataclasses.dataclass(frozen=True, eq=False)
class Mesh:
    """A closed triangle surface: `vertices` [V,3] fp32 (welded: no two rows bit-equal), `faces` [F,3] int64 with outward
    normals (counter-clockwise seen from outside).  Built by `load_mesh`, which checks what the rest relies on."""
    vertices: np.ndarray
    faces: np.ndarray

    @property
    def triangles(self) -> np.ndarray:
        """[F,3,3] fp64: the corner coordinates of every face."""
        return self.vertices.astype(np.float64)[self.faces]


def _read_stl(data: bytes) -> np.ndarray:
    """The corner records [F,3,3] fp32 of an STL file's facets (normals are not read: the orientation is recomputed)."""
    if len(data) >= 84:
        (count,) = struct.unpack_from("<I", data, 80)
        if len(data) == 84 + 50 * count:          # binary: 80-byte header, count, 50 bytes per facet
            rec = np.frombuffer(data, dtype=np.uint8, count=50 * count, offset=84).reshape(count, 50)
            return rec[:, 12:48].copy().view("<f4").reshape(count, 3, 3).astype(np.float32)
    text = data.decode("ascii", errors="replace")
    if "facet" not in text:
        raise ValueError("not an STL file: neither the binary layout nor ASCII facets")
    num = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?|[-+]?(?:nan|inf)"
    rows = re.findall(rf"vertex\s+({num})\s+({num})\s+({num})", text, flags=re.I)
    if len(rows) % 3:
        raise ValueError("ASCII STL: the number of vertex lines is not a multiple of 3")
    return np.array(rows, dtype=np.float64).astype(np.float32).reshape(-1, 3, 3)


def _corner_records(src) -> Tuple[np.ndarray, np.ndarray]:
    """(vertices [V,3] fp32, faces [F,3] int64) of any accepted source, not yet welded or checked."""
    if isinstance(src, Mesh):
        return src.vertices, src.faces
    if isinstance(src, (str, os.PathLike)):
        with open(src, "rb") as fh:
            src = fh.read()
    elif hasattr(src, "read"):
        src = src.read()
        if isinstance(src, str):
            src = src.encode("ascii")
    if isinstance(src, (bytes, bytearray, memoryview)):
        tri = _read_stl(bytes(src))
        return tri.reshape(-1, 3), np.arange(tri.shape[0] * 3, dtype=np.int64).reshape(-1, 3)
    if hasattr(src, "vertices") and hasattr(src, "faces"):
        src = (src.vertices, src.faces)
    if isinstance(src, (tuple, list)) and len(src) == 2:
        v = np.asarray(src[0].cpu() if hasattr(src[0], "cpu") else src[0], dtype=np.float64).astype(np.float32)
        f = np.asarray(src[1].cpu() if hasattr(src[1], "cpu") else src[1])
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
            raise ValueError("a mesh is (vertices [V,3], integer faces [F,3])")
        f = f.astype(np.int64)
        if f.size and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
            raise ValueError("a face names a vertex that does not exist")
        return v, f
    raise ValueError("reference_shape must be an STL path, bytes or file object, a (vertices, faces) pair or an object "
                     "with .vertices and .faces")


def load_mesh(src) -> Mesh:
    """A `Mesh` from a path, bytes or file object holding a binary or ASCII STL, a (vertices [V,3], faces [F,3]) pair or any
    object with `.vertices` and `.faces`.  Vertices whose three fp32 coordinates are bit-equal are welded (first occurrence
    keeps its place).  Refused with ValueError: an empty mesh, more than `MAX_FACES` faces, a non-finite vertex, and -
    "The mesh needs to be watertight." - a face that repeats a vertex, or a directed edge that does not occur exactly once
    with its reverse exactly once (a hole, a duplicated face, a fin).  All faces are reversed if the signed volume is
    negative, so the normals point outward."""
    if isinstance(src, Mesh):
        return src
    v, f = _corner_records(src)
    if f.shape[0] == 0:
        raise ValueError("the mesh has no faces")
    if f.shape[0] > MAX_FACES:
        raise ValueError(f"the mesh has {f.shape[0]} faces, more than the {MAX_FACES} this package takes")
    v = np.ascontiguousarray(v, dtype=np.float32)
    if not np.isfinite(v).all():
        raise ValueError("the mesh has a non-finite vertex")
    _, first, inverse = np.unique(v.view(np.int32).reshape(-1, 3), axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                  # unique row k, in first-occurrence order
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    faces = rank[inverse.reshape(-1)][f]
    vertices = v[first[order]]
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    if bool(((a == b) | (b == c) | (c == a)).any()):
        raise ValueError(_NOT_WATERTIGHT)
    V = vertices.shape[0]
    edges = np.concatenate([a * V + b, b * V + c, c * V + a])
    rev = np.concatenate([b * V + a, c * V + b, a * V + c])
    uniq = np.unique(edges)
    if uniq.size != edges.size or not np.array_equal(uniq, np.unique(rev)):
        raise ValueError(_NOT_WATERTIGHT)
    mesh = Mesh(vertices, faces)
    t = mesh.triangles
    if float(np.einsum("fi,fi->", t[:, 0], np.cross(t[:, 1], t[:, 2]))) < 0.0:
        mesh = Mesh(vertices, np.ascontiguousarray(faces[:, ::-1]))
    return mesh


def mass_properties(mesh, density: float = DEFAULT_DENSITY) -> Dict[str, np.ndarray]:
    """Exact integrals over the solid the mesh bounds, each a sum over the signed tetrahedra (origin, a, b, c) of its
    faces (the origin is moved to the vertex mean first: the sums then cancel less), all fp64:
      volume                         V = sum det[a b c] / 6
      center_mass                    c = (1 / V) sum V_t (a + b + c) / 4
      covariance                     C = integral (x - c)(x - c)^T dV, from  integral x x^T dV = sum V_t / 20 (a a^T + b b^T
                                     + c c^T + s s^T), s = a + b + c
      inertia                        density (tr C  I - C)
      principal_inertia_components   its eigenvalues, ascending (`numpy.linalg.eigvalsh`: what the notebook passes on)."""
    mesh = load_mesh(mesh)
    shift = mesh.vertices.astype(np.float64).mean(axis=0)
    t = mesh.triangles - shift
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    vt = np.einsum("fi,fi->f", a, np.cross(b, c)) / 6.0
    volume = float(vt.sum())
    s = a + b + c
    centre = (vt[:, None] * s).sum(axis=0) / (4.0 * volume)
    second = sum(np.einsum("f,fi,fj->ij", vt, p, p) for p in (a, b, c, s)) / 20.0
    cov = second - volume * np.outer(centre, centre)
    cov = 0.5 * (cov + cov.T)
    inertia = float(density) * (np.trace(cov) * np.eye(3) - cov)
    return dict(volume=volume, center_mass=centre + shift, covariance=cov, inertia=inertia,
                principal_inertia_components=np.linalg.eigvalsh(inertia))


def mesh_context(mesh, density: float = DEFAULT_DENSITY):
    """The `reference_context` of a solid: its principal inertia components at `density`, ascending, as an fp32 tensor [3]
    (the notebook's `torch.tensor(mesh.principal_inertia_components, dtype=torch.float32)`)."""
    import torch
    return torch.tensor(mass_properties(mesh, density)["principal_inertia_components"], dtype=torch.float32)


def solid_frame(mesh) -> Tuple[np.ndarray, np.ndarray]:
    """(M_r [3,3], t_r [3]) fp64 with frame = (x - t_r) @ M_r: t_r the centre of mass, the columns of M_r the eigenvectors
    of the covariance ordered by DESCENDING eigenvalue (the longest extent first, like the molecules' frames; the inertia
    tensor's order is the reverse), the last column negated where `eigh` returned a reflection, so det M_r = +1 - a
    reflection would flip the sign of every winding number."""
    props = mass_properties(mesh)
    _, vecs = np.linalg.eigh(props["covariance"])
    M = np.ascontiguousarray(vecs[:, ::-1])
    if np.linalg.det(M) < 0.0:
        M[:, 2] = -M[:, 2]
    return M, props["center_mass"]


def write_stl(mesh, binary: bool = True) -> bytes:
    """The mesh as STL bytes (binary, or ASCII with 9 significant digits: fp32 round-trips), facet normals included."""
    mesh = load_mesh(mesh)
    t = mesh.vertices[mesh.faces]                              # fp32 [F,3,3]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).astype(np.float64)
    nrm = (nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)).astype(np.float32)
    if binary:
        rec = np.zeros((t.shape[0], 50), dtype=np.uint8)
        rec[:, :12] = nrm.astype("<f4").view(np.uint8).reshape(-1, 12)
        rec[:, 12:48] = t.astype("<f4").reshape(-1, 9).view(np.uint8).reshape(-1, 36)
        return b"mlconfgen mesh".ljust(80, b" ") + struct.pack("<I", t.shape[0]) + rec.tobytes()
    out = io.StringIO()
    out.write("solid mesh\n")
    for n, tri in zip(nrm.tolist(), t.tolist()):
        out.write("facet normal %.9g %.9g %.9g\n outer loop\n" % tuple(n))
        for p in tri:
            out.write("  vertex %.9g %.9g %.9g\n" % tuple(p))
        out.write(" endloop\nendfacet\n")
    out.write("endsolid mesh\n")
    return out.getvalue().encode("ascii")
