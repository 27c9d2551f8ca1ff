"""fp64 restatement of the solid-reference kernels (`csrc/mcg_mesh.hip`, DESIGN.md section 6 "Solid references"), on the
CPU: the generalized winding number, the occupancy, the field Tanimoto as the grid sum written out, `atoms_outside` and
the pass rules.  `dtype=torch.float32` restates the same formula in fp32 (plain torch operations, no fused multiply-add),
which is where the first of WINDING_TOL's two figures comes from."""
import math

import torch

# |w_kernel - w_fp64| allowed at the test points (tests/mesh_cases.py: the closed meshes' random and probe points, the open
# prefixes' and the grid-mode run's): 4 x the larger of
#   the fp32 restatement's deviation from fp64 on those points     9.96e-7  (`test_mesh_host.py` recomputes and prints it)
#   the kernel's first measured deviation on those points          1.73e-6  (MI355X; `test_mesh_gpu.py` prints each case's)
# = 6.9e-6, rounded up.  The smallest per-triangle contribution at a probe point is 0.026 (`probe_contributions`; most are
# near 0.5), so the tolerance is far below a tenth of it and cannot hide a dropped triangle; the tests assert that too.
WINDING_TOL = 7e-6

ATOM_RADIUS, AMPLITUDE = 1.60, 2.70
ALPHA = (math.pi / (4 * math.pi / 3 / AMPLITUDE) ** (2 / 3)) / ATOM_RADIUS ** 2


def _terms(tri, pts, dtype):
    """[P,F] the atan2 terms of every (point, triangle), component by component."""
    t = torch.as_tensor(tri).to(dtype).reshape(-1, 9)
    p = torch.as_tensor(pts).to(dtype).reshape(-1, 3)
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = ([t[None, :, 3 * k + d] - p[:, d:d + 1] for d in range(3)] for k in range(3))
    la, lb, lc = ((x * x + y * y + z * z).sqrt() for x, y, z in ((ax, ay, az), (bx, by, bz), (cx, cy, cz)))
    det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
    ab, bc, ca = ax * bx + ay * by + az * bz, bx * cx + by * cy + bz * cz, cx * ax + cy * ay + cz * az
    return torch.atan2(det, la * lb * lc + ab * lc + bc * la + ca * lb)


def winding(tri, pts, dtype=torch.float64, chunk=256, drop=None):
    """w [P] = (1 / 4 pi) sum_f 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|), a, b, c = v - p.
    NaN for a non-finite point.  `drop`: a triangle index left out (the mutation check)."""
    t = torch.as_tensor(tri).to(dtype).reshape(-1, 3, 3)
    if drop is not None:
        t = torch.cat([t[:drop], t[drop + 1:]])
    p = torch.as_tensor(pts).to(dtype).reshape(-1, 3)
    out = torch.empty(p.shape[0], dtype=dtype)
    for lo in range(0, p.shape[0], chunk):
        out[lo:lo + chunk] = _terms(t, p[lo:lo + chunk], dtype).sum(1) / (2 * math.pi)
    out[~torch.isfinite(p).all(dim=1)] = float("nan")
    return out


def probe_contributions(tri, pts, owners):
    """The winding-number contribution of triangle owners[k] at point k (fp64)."""
    t = torch.as_tensor(tri).to(torch.float64).reshape(-1, 3, 3)
    p = torch.as_tensor(pts).to(torch.float64).reshape(-1, 3)
    return torch.stack([_terms(t[o:o + 1], p[k:k + 1], torch.float64)[0, 0] for k, o in enumerate(owners)]) / (2 * math.pi)


def inside(w):
    """The classification rule: a point is inside where |w| > 0.5 (NaN is not inside)."""
    return torch.as_tensor(w).abs() > 0.5


def grid_points(axes):
    """[n^3,3] the points of axes [3,n] in meshgrid(indexing="ij") flatten order."""
    ax = torch.as_tensor(axes).to(torch.float64)
    return torch.stack(torch.meshgrid(ax[0], ax[1], ax[2], indexing="ij"), dim=-1).reshape(-1, 3)


def occupancy(tri, axes, drop=None):
    """f [n^3] fp64: 1 where the grid point is inside, else 0."""
    return inside(winding(tri, grid_points(axes), drop=drop)).to(torch.float64)


def field_tanimoto(f, axes, coords, alpha=ALPHA, amplitude=AMPLITUDE):
    """<f,g> / (<f,f> + <g,g> - <f,g>) over the grid, g = 1 - prod_atoms (1 - A exp(-alpha |p - c|^2)), all fp64."""
    p = grid_points(axes)
    c = torch.as_tensor(coords).to(torch.float64).reshape(-1, 3)
    d2 = ((p[:, None, :] - c[None, :, :]) ** 2).sum(2)
    g = 1.0 - torch.prod(1.0 - amplitude * torch.exp(-alpha * d2), dim=1)
    f = torch.as_tensor(f).to(torch.float64)
    fg = float((f * g).sum())
    return fg / (float((f * f).sum()) + float((g * g).sum()) - fg)


def atoms_outside(tri, coords, n_nodes):
    """Per row of coords [B,N,3]: the real atoms that are not inside; -1 for a row with a non-finite real coordinate."""
    x = torch.as_tensor(coords).to(torch.float64)
    out = []
    for b in range(x.shape[0]):
        k = int(n_nodes[b])
        if not bool(torch.isfinite(x[b, :k]).all()):
            out.append(-1)
            continue
        out.append(int((~inside(winding(tri, x[b, :k]))).sum()) if k else 0)
    return out


def passes(count, k):
    """`max_atoms_outside=k`: a row passes with at most k atoms outside; one without a count (None: its pose failed) or
    with the kernel's -1 does not."""
    return count is not None and 0 <= count <= k
