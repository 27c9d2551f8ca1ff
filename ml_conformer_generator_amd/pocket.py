"""A receptor's binding pocket, found on the GPU and turned into the watertight mesh a `reference_shape` call generates into
("Pockets from the receptor").  The package's OWN labelled definition, in the family of LIGSITE's and
PocketPicker's buriedness; it is neither program, and its defaults are stated choices that are NOT tuned on any real protein.

Device (`ray_masks`, kernel `mcg_pocket_masks`, include/mlconfgen_hip_pocket.h): a cubic grid of n^3 points round `center`,
n = 2 floor(radius / spacing) + 1, point (i, j, l) at center + ((i, j, l) - (n - 1) / 2) spacing, flat in
meshgrid(indexing="ij") order.  Per point a uint32 mask over the receptor's heavy atoms (radii `receptor.VDW_RADII`):
  bit 31 (occupied)   a probe sphere on the point would overlap an atom: |d|^2 < (r + probe)^2, d = atom - point;
  bit k, k = 0..25    the ray of length `reach` from the point along direction k meets an atom's van der Waals sphere:
                      t = d . u, t_c = min(max(t, 0), reach), e = d - t_c u, |e|^2 <= r^2.  The directions are the 26 vectors
                      of {-1, 0, 1}^3 without (0, 0, 0), normalised, in lexicographic order (`DIRECTIONS`).
A point's buriedness is the number of its blocked rays.

Host (everything else here: numpy, fp64 and integers, no GPU; callable on masks from any source):
  pocket point   not occupied, buriedness >= `min_buriedness`, and within `radius` of the centre;
  seed           the centre point if it is a pocket point, else the nearest pocket point within `SNAP` (ties: the lower flat
                 index), else ValueError("no pocket at the centre ...");
  centres        the 6-connected component of pocket points that holds the seed;
  solid          the union of probe spheres on the centres, as cells of the grid padded by floor(probe / spacing): the cells
                 (di, dj, dl) from a centre with (di^2 + dj^2 + dl^2) spacing^2 <= probe^2.  A centre is at least r + probe
                 from every atom, so the solid stays clear of every van der Waals sphere;
  edge repair    two cells that touch along an edge only would give an edge with four faces, which `mesh.load_mesh`
                 refuses: wherever exactly the two diagonal cells of a 2 x 2 block of an axis-aligned plane are set the other
                 two are set too, until nothing changes.  `cells_filled` counts them; THEY may graze a van der Waals sphere.
                 Cells that touch at a vertex only are left: every directed edge still occurs once;
  mesh           one quad (two outward triangles) per cell face without a solid neighbour, corners at
                 (index +- 1/2) spacing + center in fp64, then cast to fp32, so shared corners are bit-equal and weld.
`find_pocket` runs both and returns a `Pocket`, which `reference_shape=` takes: the call poses into the pocket's mesh and
reads the pocket's own receptor for every receptor option."""
from __future__ import annotations

import collections
import dataclasses
import math
from typing import Optional, Tuple

import numpy as np

from . import _args
from . import mesh as mcg_mesh

MAX_N = 127                    # include/mlconfgen_hip_pocket.h MCG_POCKET_MAX_N
MAX_SPLITS = 256               # MCG_POCKET_MAX_SPLITS
OCCUPIED = np.uint32(1 << 31)  # MCG_POCKET_OCCUPIED
N_DIRECTIONS = 26
RAY_BITS = np.uint32((1 << N_DIRECTIONS) - 1)
SNAP = 3.0                     # angstrom: how far the seed may lie from a centre that is itself no pocket point
# The defaults: stated choices, the package's own, not tuned on any protein structure.
DEFAULT_RADIUS = 10.0          # angstrom: half the edge of the searched box, and the cap on a pocket point's distance
DEFAULT_SPACING = 1.0
DEFAULT_PROBE = 1.4            # angstrom: a water molecule's radius
DEFAULT_REACH = 8.0            # angstrom: between PocketPicker's 10 A rays and the width of a pocket
DEFAULT_MIN_BURIEDNESS = 14    # of 26: the proportion of PocketPicker's 16 of 30
_BRICK = (4, 8, 8)             # csrc/mcg_pocket.hip: the points of one workgroup
_TARGET_WORKGROUPS = 1024      # `receptor._TARGET_WORKGROUPS`
_PREFILTER_SLACK = 0.01        # angstrom, on top of the exact bound of `ray_masks`' prefilter

_UNIT = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)],
                 dtype=np.float64)
DIRECTIONS = _UNIT / np.linalg.norm(_UNIT, axis=1, keepdims=True)             # [26,3] fp64; row k is bit k


# ----------------------------------------------------------------------------------------------- the grid
def grid_size(radius: float, spacing: float) -> int:
    """n = 2 floor(radius / spacing) + 1 points per axis: odd, so the centre is a grid point.  ValueError outside 1..MAX_N."""
    n = 2 * int(math.floor(radius / spacing)) + 1
    if not 1 <= n <= MAX_N:
        raise ValueError(f"radius / spacing = {radius:g} / {spacing:g} gives {n} grid points per axis; at most {MAX_N} "
                         "are taken")
    return n


def grid_points(n: int, spacing: float) -> np.ndarray:
    """[n^3,3] fp64: the grid points relative to the centre, in the masks' flat order."""
    axis = (np.arange(n, dtype=np.float64) - (n - 1) / 2) * spacing
    return np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)


def buriedness(masks) -> np.ndarray:
    """The number of blocked rays (set bits among 0..25) of each mask."""
    m = np.asarray(masks).astype(np.uint32) & RAY_BITS
    count = np.zeros(m.shape, dtype=np.int64)
    for k in range(N_DIRECTIONS):
        count += (m >> np.uint32(k)) & np.uint32(1)
    return count


# ----------------------------------------------------------------------------------------------- masks -> cells
def pocket_centres(masks, n: int, spacing: float, radius: float, min_buriedness: int, snap: float = SNAP
                   ) -> Tuple[np.ndarray, int]:
    """([n,n,n] bool: the centres, the seed's flat index) of masks [n^3] by this module's rule.  ValueError
    "no pocket at the centre ..." where neither the centre point nor a point within `snap` of it is a pocket point."""
    m = np.asarray(masks).astype(np.uint32).reshape(-1)
    if m.size != n ** 3:
        raise ValueError(f"masks holds {m.size} values for a grid of {n}^3 points")
    bur = buriedness(m)
    pts = grid_points(n, spacing)
    dist2 = (pts * pts).sum(axis=1)
    is_pocket = ((m & OCCUPIED) == 0) & (bur >= min_buriedness) & (dist2 <= radius * radius)
    mid = ((n // 2) * n + n // 2) * n + n // 2
    seed = mid
    if not is_pocket[mid]:
        near = np.flatnonzero(is_pocket & (dist2 <= snap * snap))
        if near.size == 0:
            raise ValueError(f"no pocket at the centre: its buriedness is {int(bur[mid])} of {N_DIRECTIONS} "
                             f"(min_buriedness {min_buriedness}), it is "
                             f"{'occupied' if m[mid] & OCCUPIED else 'not occupied'} by a receptor atom, and no pocket point "
                             f"lies within {snap:g} A of it")
        seed = int(near[np.argmin(dist2[near])])                # argmin: the first, i.e. lowest flat index, of equal distances
    grid = is_pocket.reshape(n, n, n)
    centres = np.zeros_like(grid)
    start = (seed // (n * n), (seed // n) % n, seed % n)
    centres[start] = True
    queue = collections.deque([start])
    while queue:
        i, j, l = queue.popleft()
        for a, b, c in ((i - 1, j, l), (i + 1, j, l), (i, j - 1, l), (i, j + 1, l), (i, j, l - 1), (i, j, l + 1)):
            if 0 <= a < n and 0 <= b < n and 0 <= c < n and grid[a, b, c] and not centres[a, b, c]:
                centres[a, b, c] = True
                queue.append((a, b, c))
    return centres, seed


def dilate(centres: np.ndarray, spacing: float, probe: float) -> Tuple[np.ndarray, int]:
    """([n + 2 pad]^3 bool, pad): the union of probe spheres on the centres as cells, on the grid padded by
    pad = floor(probe / spacing) cells on every side, so that nothing is clipped."""
    n = centres.shape[0]
    pad = int(math.floor(probe / spacing))
    solid = np.zeros((n + 2 * pad,) * 3, dtype=bool)
    for di in range(-pad, pad + 1):
        for dj in range(-pad, pad + 1):
            for dl in range(-pad, pad + 1):
                if (di * di + dj * dj + dl * dl) * spacing * spacing <= probe * probe:
                    solid[pad + di: pad + di + n, pad + dj: pad + dj + n, pad + dl: pad + dl + n] |= centres
    return solid, pad


def repair_edges(solid: np.ndarray) -> Tuple[np.ndarray, int]:
    """(`solid` with every edge-only contact filled, the number of cells added): in every 2 x 2 block of every axis-aligned
    plane where exactly the two diagonal cells are set, the other two are set; repeated until nothing changes (monotone,
    and a filled cell lies inside the bounding box of what was there: bounded)."""
    s = solid.copy()
    before = int(s.sum())
    while True:
        changed = False
        for axis in range(3):
            v = np.moveaxis(s, axis, 0)                          # a view: the plane's two axes are the last two
            a, b, c, d = v[:, :-1, :-1], v[:, 1:, :-1], v[:, :-1, 1:], v[:, 1:, 1:]
            main = a & d & ~b & ~c
            anti = b & c & ~a & ~d
            if main.any() or anti.any():
                changed = True
                b |= main
                c |= main
                a |= anti
                d |= anti
        if not changed:
            return s, int(s.sum()) - before


# the four corners (offsets 0 / 1 per axis) of the face of a cell on its low (-) and high (+) side of each axis, counter-
# clockwise seen from outside the cell
_FACES = (
    (0, -1, ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0))), (0, +1, ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1))),
    (1, -1, ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1))), (1, +1, ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0))),
    (2, -1, ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0))), (2, +1, ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))),
)


def cells_mesh(solid: np.ndarray, pad: int, n: int, spacing: float, center) -> Tuple[np.ndarray, np.ndarray]:
    """(vertices [V,3] fp32, faces [F,3] int64) of the surface of the cells of `solid` (the n^3 grid padded by `pad`): per
    cell face without a solid neighbour one quad as two outward triangles; a corner at lattice index q (cell index or cell
    index + 1) lies at (q - pad - (n - 1) / 2 - 1/2) spacing + center, in fp64, cast to fp32; corners are welded by their
    lattice index."""
    center = np.asarray(center, dtype=np.float64).reshape(3)
    m = solid.shape[0]
    wide = np.zeros((m + 2,) * 3, dtype=bool)
    wide[1:-1, 1:-1, 1:-1] = solid
    quads = []
    for axis, side, corners in _FACES:
        neighbour = np.roll(wide, -side, axis=axis)[1:-1, 1:-1, 1:-1]
        cells = np.argwhere(solid & ~neighbour)                                    # [K,3], in flat order
        quads.append(cells[:, None, :] + np.asarray(corners, dtype=np.int64)[None, :, :])
    quads = np.concatenate(quads)                                                  # [Q,4,3] lattice indices
    stride = m + 1
    key = (quads[..., 0] * stride + quads[..., 1]) * stride + quads[..., 2]
    uniq, inverse = np.unique(key.reshape(-1), return_inverse=True)
    q = inverse.reshape(-1, 4)
    faces = np.concatenate([q[:, (0, 1, 2)], q[:, (0, 2, 3)]], axis=1).reshape(-1, 3).astype(np.int64)
    lattice = np.stack([uniq // (stride * stride), (uniq // stride) % stride, uniq % stride], axis=1).astype(np.float64)
    vertices = ((lattice - pad - (n - 1) / 2 - 0.5) * spacing + center).astype(np.float32)
    return vertices, faces


# ----------------------------------------------------------------------------------------------- the pocket
@dataclasses.dataclass(frozen=True, eq=False)
class Pocket:
    """A pocket of a receptor (`find_pocket`, `pocket_from_masks`): plain host data.
      mesh                 the watertight `mesh.Mesh` of the solid, in the receptor's coordinates (`vertices`, `faces`: its
                           arrays, so a `Pocket` is itself "an object with both" for `mesh.load_mesh`);
      receptor             the receptor as it was given (anything `receptor.load_receptor` or
                           `interactions.prepare_receptor` takes): what a `reference_shape=pocket` call reads for its
                           receptor options;
      center, radius, spacing, probe, reach, min_buriedness   the parameters;
      cells, n_centres, cells_filled   solid cells (filled ones included), pocket points in the component, cells the edge
                           repair added;
      volume               cells * spacing^3, cubic angstrom;
      mean_buriedness      the mean number of blocked rays over the centres;
      masks                [n^3] uint32, as they came from the device."""
    mesh: mcg_mesh.Mesh
    receptor: object
    center: Tuple[float, float, float]
    radius: float
    spacing: float
    probe: float
    reach: float
    min_buriedness: int
    cells: int
    n_centres: int
    cells_filled: int
    volume: float
    mean_buriedness: float
    masks: np.ndarray

    @property
    def vertices(self) -> np.ndarray:
        return self.mesh.vertices

    @property
    def faces(self) -> np.ndarray:
        return self.mesh.faces


def pocket_from_masks(masks, receptor, center, radius: float = DEFAULT_RADIUS, spacing: float = DEFAULT_SPACING,
                      probe: float = DEFAULT_PROBE, reach: float = DEFAULT_REACH,
                      min_buriedness: int = DEFAULT_MIN_BURIEDNESS) -> Pocket:
    """The host half of `find_pocket`: the `Pocket` of masks [n^3] (from `ray_masks`, or from any restatement of them) of the
    grid of `radius` / `spacing` round `center`.  `receptor` is only kept; `reach` only recorded.  ValueError: what
    `pocket_centres` refuses, masks of another size."""
    center = tuple(float(v) for v in np.asarray(center, dtype=np.float64).reshape(3))
    n = grid_size(radius, spacing)
    masks = np.ascontiguousarray(np.asarray(masks).astype(np.uint32).reshape(-1))
    centres, _ = pocket_centres(masks, n, spacing, radius, min_buriedness)
    solid, pad = dilate(centres, spacing, probe)
    solid, filled = repair_edges(solid)
    mesh = mcg_mesh.load_mesh(cells_mesh(solid, pad, n, spacing, center))
    cells = int(solid.sum())
    return Pocket(mesh=mesh, receptor=receptor, center=center, radius=float(radius), spacing=float(spacing),
                  probe=float(probe), reach=float(reach), min_buriedness=int(min_buriedness), cells=cells,
                  n_centres=int(centres.sum()), cells_filled=filled, volume=cells * float(spacing) ** 3,
                  mean_buriedness=float(buriedness(masks)[centres.reshape(-1)].mean()), masks=masks)


def _check_parameters(center, radius, spacing, probe, reach):
    try:
        c = np.asarray(center.cpu() if hasattr(center, "cpu") else center, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        c = np.zeros(0)
    if c.size != 3 or not np.isfinite(c).all():
        raise ValueError(f"center must be three finite coordinates, got {center!r}")
    radius = _args.check_real("radius", radius, 0.0, open_low=True)
    spacing = _args.check_real("spacing", spacing, 0.0, open_low=True)
    probe = _args.check_real("probe", probe, 0.0, open_low=True)
    reach = _args.check_real("reach", reach, 0.0, open_low=True)
    return c, radius, spacing, probe, reach, grid_size(radius, spacing)


def _heavy_atoms(receptor):
    """(coords [R,3] fp64, atomic numbers [R]) of the heavy atoms of anything `load_receptor` takes or of a typed triple,
    checked by `load_receptor`.  Coordinates given as numbers (a pair, a triple) are read in fp64, so that the centre is
    subtracted before anything is rounded to fp32; a PDB string's and a Mol's are what `load_receptor` returns."""
    import torch
    from . import receptor as mcg_receptor
    given = isinstance(receptor, (tuple, list)) and len(receptor) in (2, 3)
    coords, z = mcg_receptor.load_receptor((receptor[0], receptor[1]) if given else receptor)
    if given:
        raw_z = torch.as_tensor(receptor[1]).cpu().reshape(-1)
        coords = torch.as_tensor(receptor[0]).to(torch.float64).cpu().reshape(-1, 3)[raw_z != 1]
    return coords.to(torch.float64), z


def default_splits(n: int, R: int) -> int:
    """Parts a workgroup's receptor tiles are cut into, like `receptor.default_splits`: enough workgroups to fill the GPU
    (a 21^3 grid has 54 bricks), at least one tile each."""
    bricks = math.prod(-(-n // b) for b in _BRICK)
    return max(1, min(-(-R // 256), -(-_TARGET_WORKGROUPS // bricks), MAX_SPLITS))


def kept_tiles(spheres, n: int, spacing: float, probe: float, reach: float) -> np.ndarray:
    """[bricks] int64: how many receptor tiles each workgroup of `mcg_pocket_masks` keeps - the kernel's tile test
    (csrc/mcg_receptor_tiles.h `build_tile_list`, slack 0.05 A + 1e-3 of the reach) restated in fp32 numpy over the tile
    spheres [T,4] of `receptor.tile_spheres` and the brick centres of csrc/mcg_pocket.hip.  For measurements and tests; the
    kernel does not read it."""
    q = np.asarray(spheres.cpu() if hasattr(spheres, "cpu") else spheres, dtype=np.float32).reshape(-1, 4)
    f = np.float32
    c = f(0.5) * f(n - 1)
    axes = [(np.arange(-(-n // b), dtype=np.float32) * f(b) + f(0.5) * f(b - 1) - c) * f(spacing) for b in _BRICK]
    centre = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    d = q[None, :, :3] - centre
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    far = (f(5.172041) * f(spacing) + f(max(reach, probe))) + q[None, :, 3]
    lim = far + (f(0.05) + f(1e-3) * far)
    return (~(d2 > lim * lim)).sum(axis=1).astype(np.int64)


def ray_masks(receptor, center, radius: float = DEFAULT_RADIUS, spacing: float = DEFAULT_SPACING,
              probe: float = DEFAULT_PROBE, reach: float = DEFAULT_REACH, device=None, splits: Optional[int] = None,
              skip_tiles: bool = True, prefilter: bool = True):
    """The masks [n^3] of the grid round `center` against `receptor` (what `receptor.load_receptor` takes, or a typed
    triple), on the device, as an int32 tensor holding the uint32 bit patterns (`.cpu().numpy().view(numpy.uint32)`): one
    `mcg_pocket_masks` call on the current stream.  The centre is subtracted from the receptor's coordinates in fp64 before
    the cast to fp32, so the kernel sees small magnitudes; the atoms are sorted into compact tiles (`receptor.sort_receptor`)
    with their bounding spheres (`receptor.tile_spheres`).  `prefilter`: atoms farther from the centre than
    radius sqrt(3) + max(reach, probe) + r + 0.01 A - they cannot reach a corner of the box - are dropped on the host first;
    a receptor of which none is left gives zeros without a launch.  `splits` (default `default_splits`), `skip_tiles` and
    `prefilter` never change a bit.  Refused before any device work: what `load_receptor` refuses, a `center` that is not
    three finite numbers, a radius, spacing, probe or reach that is not a positive real number, a grid of more than MAX_N
    points per axis, `splits` outside 1..MAX_SPLITS."""
    import torch
    from . import _lib
    from . import receptor as mcg_receptor
    c, radius, spacing, probe, reach, n = _check_parameters(center, radius, spacing, probe, reach)
    if splits is not None:
        splits = _args.check_steps("splits", splits, 1, MAX_SPLITS)
    rec_xyz, rec_z = _heavy_atoms(receptor)
    dev = _args.resolve_device(device)
    rel = rec_xyz.to(torch.float64) - torch.from_numpy(c)
    r = mcg_receptor.vdw_radii(rec_z)
    if prefilter:
        keep = rel.norm(dim=1) <= radius * math.sqrt(3.0) + max(reach, probe) + r.to(torch.float64) + _PREFILTER_SLACK
        rel, r = rel[keep], r[keep]
    out = torch.zeros(n ** 3, dtype=torch.int32, device=dev)
    R = int(r.numel())
    if R == 0:
        return out
    xyzr = mcg_receptor.sort_receptor(rel.to(torch.float32), r)
    spheres = mcg_receptor.tile_spheres(xyzr).to(dev) if skip_tiles else None
    rec = xyzr.to(dev)
    S = default_splits(n, R) if splits is None else splits
    _lib.check(_lib.lib().mcg_pocket_masks(_lib.dptr(rec), R, _lib.dptr(spheres), n, spacing, probe, reach, S,
                                           _lib.dptr(out), _lib.current_stream_ptr(dev)), "mcg_pocket_masks")
    return out


def find_pocket(receptor, center, radius: float = DEFAULT_RADIUS, spacing: float = DEFAULT_SPACING,
                probe: float = DEFAULT_PROBE, reach: float = DEFAULT_REACH, min_buriedness: int = DEFAULT_MIN_BURIEDNESS,
                device=None) -> Pocket:
    """The pocket of `receptor` at `center` (receptor coordinates, angstrom): `ray_masks` on the device, then
    `pocket_from_masks` on the host.  `receptor`: anything `receptor.load_receptor` takes - an RDKit Mol, a PDB-format
    string, a (coords, atomic_numbers) pair - or the (coords, atomic_numbers, types) triple `interactions.prepare_receptor`
    takes; it is kept as given on the `Pocket`, so the interaction stages of a `reference_shape=pocket` call can type it.
    The defaults (probe: a water's radius; min_buriedness 14 of 26: the proportion of PocketPicker's 16 of 30; reach between
    PocketPicker's 10 A and a pocket's width) are stated choices, not tuned on any real protein.  Refused with ValueError
    before any device work: what `ray_masks` refuses, `min_buriedness` not an integer in 0..26; behind it: "no pocket at
    the centre ..." with the centre's buriedness and whether it is occupied."""
    min_buriedness = _args.check_steps("min_buriedness", min_buriedness, 0, N_DIRECTIONS)
    masks = ray_masks(receptor, center, radius, spacing, probe, reach, device=device)
    return pocket_from_masks(masks.cpu().numpy().view(np.uint32), receptor, center, radius, spacing, probe, reach,
                             min_buriedness)
