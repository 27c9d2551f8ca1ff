"""Seeded receptors above 65 536 atoms, where `mcg_tiles::build_tile_list` (csrc/mcg_receptor_tiles.h) compacts its tile
list in a second round of 256 tiles, with ligand places and grid centres CHOSEN BY PROPERTY: which rounds keep tiles there.
Importing this module needs no GPU; the host test (tests/test_large_receptor_host.py) asserts every property stated here and
the GPU test (tests/test_large_receptor_gpu.py) launches the six receptor entries on the same cases.

Receptors   a jittered cubic lattice (spacing 3.8 A, jitter +-0.6 A uniform per axis, fp32 from the outset), elements drawn
            from C, C, C, N, O, S, typed by the project's own element typing (`receptor.load_typed_receptor`); a 4 A cavity is
            carved round every site (an atom a site sits exactly on is spared) and the R remaining points nearest the origin
            are kept.  R = 65 536 (T = 256 tiles: one full round, no second), 65 537 (T = 257: round two holds one tile of one
            atom), 68 900 (T = 270: a partial last tile in round two; the 41^3 lattice has 68 921 points, the cavities take
            some) and 131 072 (T = 512: the limit).
Tile test   `kept`: `build_tile_list`'s expression in fp32 numpy, the same operations in the same order, with each tile's
            signed distance from its limit in angstrom.
Sites       one per receptor and property, found on the lattice before it is carved, by a wide margin:
            BOTH      tiles are kept with index below 256 and with index 256 or above;
            HI_ONLY   every kept tile has index >= 256: round one contributes nothing, `base` is 0 when round two starts;
            LO_ONLY   T > 256 and every kept tile has index < 256: round two keeps nothing;
            SEAM      (R = 65 537) the centre of tile 256's sphere - the one atom of round two - and tiles below it;
            LAST      (R = 65 536) tile 255, the last of the one full round, is kept.
Places      carving moves tiles, and a tile sphere of these receptors has a radius of 25-40 A: a shell of +-0.5 A round a
            ligand's limit holds two tile centres on average.  So every ligand row of every entry gets its own place inside
            its site's cavity, the site plus the first of 1 200 seeded offsets of at most 2 A (`place`) at which, on the FINAL
            receptor, the row's own tile list - its own centroid, its own reach - has the property with NO tile closer than
            MARGIN = 0.5 A to its limit: a last-bit difference on the device cannot change the list (the relief reads
            nothing beyond a contact: its rows also touch atoms of every round they keep tiles of).  The 9^3 pocket grid builds
            twelve lists, one per brick, and no centre clears all twelve shells; its centre (`grid_place`) is the first offset
            at which every tile that DECIDES the property is 0.5 A clear in every brick (HI_ONLY: every round-one tile out;
            BOTH, SEAM: in some brick a tile of either round in) - the tiles that may flip are counted by the host test.
Ligands     the stages' own small builders: `interactions_ref.walk` (27 and 14 atoms) for the scoring and the rigid walk,
            `relief_ref.ligand` (20 and 9 carbons) for the relief, `flex_cases`' isopentylbenzene and hexane for the flexible
            walk; every launch has a row with n_nodes = 0 between the good rows and a padded width of 32.
Subsets     the fp64 restatements read the receptor atoms within `Entry.radius` of a row's place - ligand extent + max_shift +
            cut-off + largest radius + 1 A -, in the kernel's order; the host test shows no atom outside can contribute."""
import functools
import math

import numpy as np
import torch

import flex_cases as FC
import interactions_ref as IR
import pose_optimise_ref as PO
import relief_ref as RR
from ml_conformer_generator_amd import interactions as IX
from ml_conformer_generator_amd import pocket as PK
from ml_conformer_generator_amd import receptor as RC

F32 = np.float32
SPACING, JITTER, CAVITY = 3.8, 0.6, 4.0
ELEMENTS = (6, 6, 6, 7, 8, 16)
SIZES = (65536, 65537, 68900, 131072)
LATTICE = {65536: 41, 65537: 41, 68900: 41, 131072: 51}
TILE = 256
ROUND = 256                                       # tiles per round of the compaction
MARGIN = 0.5                                      # angstrom: no tile lies closer to its limit
SLACK_ABS, SLACK_REL = F32(0.05), F32(1e-3)       # csrc/mcg_receptor_tiles.h TILE_SLACK_ABS, TILE_SLACK_REL
MAX_SHIFT = 2.0
STEPS = 4
WIDTH = 32
CUTOFF = 8.0
FLEX_MARGIN = 2.0
OFFSET = np.array([0.6, -0.3, 0.2])               # the flexible cases' push out of the middle (tests/test_pose_flex_gpu.py)
GRID_N, GRID_SPACING, GRID_PROBE, GRID_REACH = 9, 1.0, 1.4, 8.0
KINDS = {65536: ("LAST",), 65537: ("SEAM", "LO_ONLY"), 68900: ("BOTH", "LO_ONLY"), 131072: ("BOTH", "HI_ONLY", "LO_ONLY")}
WALKED = ("BOTH", "HI_ONLY", "SEAM")              # the sites the three walks run at
GRIDS = ((131072, "BOTH"), (131072, "HI_ONLY"), (65537, "SEAM"))      # where the pocket grid is centred


# ----------------------------------------------------------------------------------------------- the tile test
def kept(spheres, centre, reach0):
    """(keep [..., T] bool, margin [..., T] fp64) of tile spheres [T,4] fp32 seen from `centre` [..., 3] with the caller's
    reach `reach0`: `build_tile_list`'s test in fp32, in its order - d = q - c, reach = reach0 + radius, lim = reach +
    (0.05 + 1e-3 reach), keep unless (dx dx + dy dy) + dz dz > lim lim - and how far, in angstrom, each tile's centre lies
    beyond its limit (negative: inside)."""
    q = np.asarray(spheres.cpu() if hasattr(spheres, "cpu") else spheres, dtype=F32).reshape(-1, 4)
    c = np.asarray(centre, dtype=F32).reshape(-1, 1, 3)
    dx, dy, dz = q[None, :, 0] - c[..., 0], q[None, :, 1] - c[..., 1], q[None, :, 2] - c[..., 2]
    reach = F32(reach0) + q[None, :, 3]
    lim = reach + (SLACK_ABS + SLACK_REL * reach)
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F32 and lim.dtype == F32
    keep = ~(d2 > lim * lim)
    margin = np.sqrt(d2.astype(np.float64)) - lim.astype(np.float64)
    shape = np.shape(centre)[:-1] + (q.shape[0],)
    return keep.reshape(shape), margin.reshape(shape)


def rounds(keep):
    """(tiles kept in round one, in round two) of a keep vector [..., T]."""
    keep = np.asarray(keep)
    return keep[..., :ROUND].sum(axis=-1), keep[..., ROUND:].sum(axis=-1)


def brick_centres(n=GRID_N, spacing=GRID_SPACING):
    """[bricks,3] fp32: the brick centres of `mcg_pocket_masks` relative to the grid's centre, as `pocket.kept_tiles`
    forms them."""
    c = F32(0.5) * F32(n - 1)
    axes = [(np.arange(-(-n // b), dtype=F32) * F32(b) + F32(0.5) * F32(b - 1) - c) * F32(spacing) for b in PK._BRICK]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def grid_reach0(spacing=GRID_SPACING, reach=GRID_REACH, probe=GRID_PROBE):
    """What `mcg_pocket_masks` hands `build_tile_list`: half a brick's diagonal + max(reach, probe), fp32."""
    return F32(5.172041) * F32(spacing) + F32(max(reach, probe))


# ----------------------------------------------------------------------------------------------- ligands
class Row:
    """One ligand row about the origin: x [n,3] fp64, z [n], t [n] uint8 type bits, and for the flexible walk its graph."""
    def __init__(self, x, z, t, graph=None):
        self.x, self.z, self.t, self.graph = np.asarray(x, dtype=np.float64).reshape(-1, 3), z, t, graph
        self.n = len(self.x)

    def at(self, point):
        """The row's fp32 coordinates with the origin moved to `point`."""
        return (self.x + np.asarray(point, dtype=np.float64)).astype(F32)


def _walks(seed, sizes):
    g = np.random.default_rng(seed)
    rows = []
    for n in sizes:
        x = IR.walk(n, g) if n else np.zeros((0, 3))
        rows.append(Row(x, g.choice([6, 6, 6, 7, 8, 16, 17], size=n).astype(np.int64), g.integers(0, 8, size=n).astype(np.uint8)))
    return rows


class Entry:
    """One entry's launch: its rows (one empty among them), whose radii tile the receptor ("ix": the interaction radii of
    `interactions.prepare_receptor`; "vdw": `receptor.vdw_radii`), the reach it hands `build_tile_list` for a row, how far an
    atom of the row can come from its place during the launch, and the radius of the receptor subset its restatement reads."""
    def __init__(self, name, rows, radii, moves, cutoff):
        self.name, self.rows, self.radii, self.moves, self.cutoff = name, rows, radii, moves, cutoff

    def centre(self, row, point):
        return PO.centroid(row.at(point))

    def rho(self, row, point):
        x = row.at(point)
        r = (x - self.centre(row, point)[None, :]).astype(F32)
        return F32(np.sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).max()))

    def reach0(self, row, point):
        """fp32, in the kernel's order."""
        rho = self.rho(row, point)
        if self.name == "interactions":
            return rho + F32(CUTOFF)
        if self.name == "optimise":
            return (rho + F32(CUTOFF)) + F32(MAX_SHIFT)
        if self.name == "flex":
            return ((rho + F32(FLEX_MARGIN)) + F32(CUTOFF)) + F32(MAX_SHIFT)
        return (rho + F32(MAX_SHIFT)) + F32(RR.CARBON)                  # relief: (rho + max_shift) + max r_i

    def extent(self, row, point):
        """How far an atom of the row can come from `point` during the launch (angstrom, fp64, 1e-3 to spare)."""
        c = self.centre(row, point).astype(np.float64)
        return float(np.linalg.norm(c - point)) + float(self.rho(row, point)) + self.moves + 1e-3

    def radius(self, row, point, largest_radius, margin=1.0):
        """The subset's radius: extent + cut-off + largest radius + `margin`; a pair further apart than the cut-off - for
        the relief, than a contact's r_i + r_j - contributes exactly nothing."""
        cut = self.cutoff if self.cutoff is not None else RR.CARBON + largest_radius
        return self.extent(row, point) + cut + largest_radius + margin


@functools.lru_cache(maxsize=None)
def entries():
    """The four ligand-taking entries that build a tile list: interactions and the rigid walk on the same typed walks (the
    rigid walk's pushed by OFFSET, so that there is a force to follow), the flexible walk on two graphs, the relief on two
    carbon walks.  Each launch: [row, empty row, row] at padded width WIDTH."""
    by = FC.by_name()
    walks = _walks(7001, (27, 0, 14))
    pushed = [Row(r.x + (OFFSET if r.n else 0.0), r.z, r.t) for r in walks]
    flex = []
    for name in ("isopentylbenzene", "empty", "hexane"):
        g = by[name]
        x = g.x.astype(np.float64) - (g.x.astype(np.float64).mean(axis=0) if g.n else 0.0) + (OFFSET if g.n else 0.0)
        flex.append(Row(x, g.z.astype(np.int64), np.where(g.z == 6, 4, 3).astype(np.uint8), g))
    g = np.random.default_rng(7003)
    relief = [Row(RR.ligand(n, g) if n else np.zeros((0, 3)), np.full(n, 6, dtype=np.int64), np.zeros(n, dtype=np.uint8))
              for n in (20, 0, 9)]
    return {"interactions": Entry("interactions", walks, "ix", 0.0, CUTOFF),
            "optimise": Entry("optimise", pushed, "ix", MAX_SHIFT, CUTOFF),
            "flex": Entry("flex", flex, "ix", FLEX_MARGIN + MAX_SHIFT, CUTOFF),
            "relief": Entry("relief", relief, "vdw", MAX_SHIFT, None)}


# ----------------------------------------------------------------------------------------------- receptors
@functools.lru_cache(maxsize=None)
def _pool(L):
    """(points [L^3,3] fp32, elements [L^3]) of the jittered lattice, nearest the origin first."""
    g = np.random.default_rng(9000 + L)
    ax = (np.arange(L) - (L - 1) / 2) * SPACING
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + g.uniform(-JITTER, JITTER, size=(L ** 3, 3))
    z = g.choice(ELEMENTS, size=L ** 3).astype(np.int64)
    pts = pts.astype(F32)
    order = np.argsort((pts.astype(np.float64) ** 2).sum(axis=1), kind="stable")
    return pts[order], z[order]


class Receptor:
    """A receptor as given (`xyz` [R,3] fp32, `z` [R], `types` [R] uint8; nearest the origin first) and as the kernels read
    it: `ix` / `ix_types` / `ix_spheres` (`interactions.prepare_receptor`: interaction radii) and `vdw` / `vdw_spheres`
    (`receptor.sort_receptor` over `receptor.vdw_radii`); host tensors, never written to.  `sites`: {kind: point [3] fp64}."""
    def __init__(self, R, sites, typed=True):
        pts, z = _pool(LATTICE[R])
        keep = np.ones(len(pts), dtype=bool)
        for s in sites.values():
            d = np.linalg.norm(pts.astype(np.float64) - s[None, :], axis=1)
            keep &= (d > CAVITY) | (d == 0.0)
        assert int(keep.sum()) >= R, (R, int(keep.sum()))
        self.R, self.T, self.sites = R, -(-R // TILE), dict(sites)
        self.xyz, self.z = torch.from_numpy(pts[keep][:R].copy()), torch.from_numpy(z[keep][:R].copy())
        self.vdw = RC.sort_receptor(self.xyz, RC.vdw_radii(self.z))
        self.vdw_spheres = RC.tile_spheres(self.vdw)
        if typed:                                         # (the sites are found without: the types change no tile)
            self.types = RC.load_typed_receptor((self.xyz, self.z))[2]
            prepared = IX.prepare_receptor((self.xyz, self.z, self.types))
            self.prepared, self.ix, self.ix_types, self.ix_spheres = prepared, prepared.xyzr, prepared.types, prepared.spheres

    def spheres(self, radii):
        return self.ix_spheres if radii == "ix" else self.vdw_spheres

    def sorted(self, radii):
        return self.ix if radii == "ix" else self.vdw

    def largest_radius(self, radii):
        return float(self.sorted(radii)[:, 3].max())

    def subset(self, radii, point, radius):
        """The indices, in the kernel's order, of the atoms within `radius` of `point` (fp64)."""
        d = np.linalg.norm(self.sorted(radii)[:, :3].double().numpy() - np.asarray(point)[None, :], axis=1)
        return np.flatnonzero(d <= radius)

    @functools.lru_cache(maxsize=None)
    def _recentred(self, point):
        rel = (self.xyz.double() - torch.tensor(point, dtype=torch.float64)).to(torch.float32)
        xyzr = RC.sort_receptor(rel, RC.vdw_radii(self.z))
        return xyzr, RC.tile_spheres(xyzr)

    def recentred(self, point):
        """The receptor as `pocket.ray_masks` hands it to the kernel for a grid round `point`: the centre subtracted in fp64
        before the cast to fp32, sorted into tiles; ([R,4] fp32, spheres [T,4])."""
        return self._recentred(tuple(float(v) for v in point))


def _coarse_sites(R):
    """{kind: point} on the lattice before it is carved, each by a wide margin at the reaches the cases use (9 to 21 A from
    a point: a ligand's radius of 1 to 7 A + the 8 A cut-off, + max_shift + the flexible walk's 2 A).
      BOTH     where a 4 A cell of round-one atoms touches a cell of round-two atoms - so that atoms of both rounds are in
               contact with a ligand there -, the face with the most tiles of the scarcer round kept at 9 A;
      HI_ONLY, LO_ONLY   the point half a lattice step along every axis from an atom (every 16th is tried) whose nearest
               tile of the other round lies furthest beyond its limit at 21 A;
      SEAM     the one atom of tile 256 - once it stays that atom on the receptor carved round it;
      LAST     the centre of tile 255's sphere."""
    sites = {}
    if "SEAM" in KINDS[R]:
        for _ in range(8):
            rec = Receptor(R, sites, typed=False)
            atom = rec.vdw[-1, :3].double().numpy()
            if "SEAM" in sites and np.array_equal(sites["SEAM"], atom):
                break
            sites["SEAM"] = atom
        else:
            raise AssertionError("the last atom of the 65 537 did not settle")
    rec = Receptor(R, sites, typed=False)
    xyz = rec.vdw[:, :3].double().numpy()
    first = np.arange(rec.T) < ROUND
    for kind in KINDS[R]:
        if kind == "LAST":
            sites[kind] = rec.vdw_spheres[ROUND - 1, :3].double().numpy()
        elif kind in ("HI_ONLY", "LO_ONLY"):
            own = (xyz[ROUND * TILE:: 16] if kind == "HI_ONLY" else xyz[: ROUND * TILE: 16]) + 0.5 * SPACING
            other = first if kind == "HI_ONLY" else ~first
            _, m = kept(rec.vdw_spheres[torch.from_numpy(other)], own, 21.0)
            sites[kind] = own[int(np.argmax(m.min(axis=1)))]
        elif kind == "BOTH":
            faces = _boundary_faces(xyz)
            k, _ = kept(rec.vdw_spheres, faces, 9.0)
            lo, hi = rounds(k)
            sites[kind] = faces[int(np.argmax(np.minimum(lo, hi)))]
    return sites


def _boundary_faces(xyz):
    """[F,3]: the centres of the faces between a 4 A cell that holds round-one atoms (index < 65 536) and a neighbouring
    cell that holds round-two atoms."""
    lo = xyz.min(axis=0)
    cell = np.floor((xyz - lo) / 4.0).astype(np.int64)
    dims = cell.max(axis=0) + 2
    flat = (cell[:, 0] * dims[1] + cell[:, 1]) * dims[2] + cell[:, 2]
    first, second = np.zeros(int(dims.prod()), dtype=np.int64), np.zeros(int(dims.prod()), dtype=np.int64)
    np.add.at(first, flat[: ROUND * TILE], 1)
    np.add.at(second, flat[ROUND * TILE:], 1)
    first, second = first.reshape(dims), second.reshape(dims)
    out = []
    for axis in range(3):
        a, b = np.moveaxis(first, axis, 0), np.moveaxis(second, axis, 0)
        others = [k for k in range(3) if k != axis]
        for near, far in ((a[:-1], b[1:]), (b[:-1], a[1:])):
            idx = np.argwhere((near >= 1) & (far >= 1))                   # the face between cell idx and idx + 1 along axis
            face = np.zeros((len(idx), 3))
            face[:, axis] = idx[:, 0] + 1.0
            face[:, others[0]], face[:, others[1]] = idx[:, 1] + 0.5, idx[:, 2] + 0.5
            out.append(face * 4.0 + lo)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def receptor(R):
    """The receptor of R atoms, carved round its sites; cached per process."""
    return Receptor(R, _coarse_sites(R))


@functools.lru_cache(maxsize=None)
def _offsets():
    """[1200,3]: 0 first, then seeded points of the ball of 2 A, half the cavity's radius."""
    g = np.random.default_rng(7100)
    v = g.normal(size=(1199, 3))
    v *= 2.0 * (g.uniform(0.0, 1.0, size=(1199, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([np.zeros((1, 3)), v])


def has_property(kind, T, keep):
    """Whether one tile list `keep` [T] has the site's property."""
    lo, hi = (int(v) for v in rounds(keep))
    return {"BOTH": lo > 0 and hi > 0, "HI_ONLY": lo == 0 and hi > 0, "LO_ONLY": T > ROUND and lo > 0 and hi == 0,
            "LAST": T == ROUND and bool(keep[ROUND - 1]), "SEAM": T == ROUND + 1 and lo > 0 and hi == 1}[kind]


def row_list(R, kind, name, r, point=None):
    """(keep [T], margin [T]) of the tile list the entry `name` builds for its row `r` placed at `point` (default: its
    place)."""
    rec, e = receptor(R), entries()[name]
    point = place(R, kind, name, r) if point is None else point
    return tuple(v[0] for v in kept(rec.spheres(e.radii), e.centre(e.rows[r], point)[None, :], e.reach0(e.rows[r], point)))


@functools.lru_cache(maxsize=None)
def place(R, kind, name, r):
    """Where row `r` of entry `name` sits at the site `kind` of receptor R: the site + the first offset at which the row's
    tile list has the property with no tile closer than MARGIN to its limit."""
    site = receptor(R).sites[kind]
    for off in _offsets():
        keep, margin = row_list(R, kind, name, r, site + off)
        if has_property(kind, receptor(R).T, keep) and float(np.abs(margin).min()) >= MARGIN:
            if name != "relief" or kind in ("LO_ONLY", "LAST") or _touches(R, kind, r, site + off):
                return site + off
    raise AssertionError(f"no place for {name} row {r} at {kind} of {R}")


def _touches(R, kind, r, point):
    """Whether the relief's row `r` at `point` is in contact (penalty > 0.01 A^2) with atoms of round two and - BOTH, SEAM -
    apart from them with atoms of round one: the relief reads nothing beyond a contact, so a lost round shows only then."""
    rec, e = receptor(R), entries()["relief"]
    row = e.rows[r]
    idx = rec.subset("vdw", point, e.radius(row, point, rec.largest_radius("vdw")))
    for part in (idx[idx >= ROUND * TILE], idx[idx < ROUND * TILE])[: 1 if kind == "HI_ONLY" else 2]:
        xyzr = rec.vdw[torch.from_numpy(part)].numpy()
        if not RR.seven(row.at(point), ligand_radii("relief", row), xyzr[:, :3], xyzr[:, 3])[0] > 0.01:
            return False
    return True


def grid_lists(R, kind, point=None):
    """(keep [bricks,T], margin [bricks,T]) of the twelve tile lists `mcg_pocket_masks` builds for the 9^3 grid centred on
    `point` (default: `grid_place`), on the re-centred receptor it reads."""
    point = grid_place(R, kind) if point is None else point
    return kept(receptor(R).recentred(point)[1], brick_centres(), grid_reach0())


def grid_decided(kind, keep, margin):
    """Whether the grid's twelve lists have the property on the tiles that lie at least MARGIN from their limit alone."""
    sure_in, sure_out = keep & (np.abs(margin) >= MARGIN), ~keep & (np.abs(margin) >= MARGIN)
    lo_in, hi_in = rounds(sure_in)
    if kind == "HI_ONLY":
        return bool(sure_out[:, :ROUND].all() and (hi_in > 0).all())
    if kind == "SEAM":
        return bool(((lo_in > 0) & sure_in[:, ROUND]).any() and keep.shape[1] == ROUND + 1)
    return bool(((lo_in > 0) & (hi_in > 0)).any())


@functools.lru_cache(maxsize=None)
def grid_place(R, kind):
    """The centre of the pocket grid at a site: the site + the first offset at which `grid_decided` holds."""
    site = receptor(R).sites[kind]
    for off in _offsets()[:40]:
        if grid_decided(kind, *grid_lists(R, kind, site + off)):
            return site + off
    raise AssertionError(f"no grid centre at {kind} of {R}")


def cases(kinds=None):
    """[(R, kind)] of every site, optionally of the given kinds only."""
    return [(R, k) for R in SIZES for k in KINDS[R] if kinds is None or k in kinds]


# ----------------------------------------------------------------------------------------------- launches and restatements
N_ROT = (3, 0, 5)                                 # the rows' rotatable bonds, as the scoring entry is handed them


def ligand_radii(name, row):
    return np.full(row.n, RR.CARBON, dtype=F32) if name == "relief" else IR.radii(row.z)


def launch(R, kind, name):
    """The entry's launch at a site, as numpy: dict x [3,WIDTH,3] fp32, r [3,WIDTH] fp32, t [3,WIDTH] uint8 (junk beyond
    every row's atoms), n [3] int32, rows [(row, its fp32 coordinates, its place)]."""
    e = entries()[name]
    x = np.full((len(e.rows), WIDTH, 3), 7.5, dtype=F32)
    r = np.full((len(e.rows), WIDTH), 1.9, dtype=F32)
    t = np.full((len(e.rows), WIDTH), 7, dtype=np.uint8)
    rows = []
    for b, row in enumerate(e.rows):
        point = place(R, kind, name, b) if row.n else receptor(R).sites[kind]
        xb = row.at(point)
        x[b, : row.n], r[b, : row.n], t[b, : row.n] = xb, ligand_radii(name, row), row.t
        rows.append((row, xb, point))
    return dict(x=x, r=r, t=t, n=np.array([row.n for row in e.rows], dtype=np.int32), rows=rows)


def subset(R, kind, name, r, margin=1.0, rounds_kept=None):
    """The receptor atoms (indices in the kernel's order) the restatement of row `r` reads: those within `Entry.radius` of
    the row's place; `rounds_kept` "first" / "second": of these, the atoms of the tiles below 256 / of 256 and above alone -
    what a kernel that lost the other round would see."""
    rec, e = receptor(R), entries()[name]
    point = place(R, kind, name, r)
    idx = rec.subset(e.radii, point, e.radius(e.rows[r], point, rec.largest_radius(e.radii), margin))
    if rounds_kept is not None:
        idx = idx[idx < ROUND * TILE] if rounds_kept == "first" else idx[idx >= ROUND * TILE]
    return idx


def receptor_args(R, name, idx):
    """(xyz [m,3] fp32, radii [m] fp32, types [m] uint8) of the receptor atoms `idx` as the entry's kernel reads them."""
    rec, e = receptor(R), entries()[name]
    xyzr = rec.sorted(e.radii)[torch.from_numpy(idx)].numpy()
    types = rec.ix_types[torch.from_numpy(idx)].numpy() if e.radii == "ix" else np.zeros(len(idx), dtype=np.uint8)
    return xyzr[:, :3].copy(), xyzr[:, 3].copy(), types


def score_args(R, kind, r, idx=None, name="interactions"):
    """What `interactions_ref.score`, `bounds` and `check` take for row `r` of the scoring launch."""
    row, x, _ = launch(R, kind, name)["rows"][r]
    y, rj, tj = receptor_args(R, name, subset(R, kind, name, r) if idx is None else idx)
    return x, ligand_radii(name, row), row.t, y, rj, tj, N_ROT[r]


def grid_subset(R, kind, margin=1.0, rounds_kept=None):
    """(xyz [m,3] fp64 relative to the grid's centre, radii [m] fp64) of the atoms the pocket restatement reads: those within
    the grid's half diagonal + max(reach, probe) + the largest radius + `margin` of the centre, in the kernel's order."""
    xyzr = receptor(R).recentred(grid_place(R, kind))[0].double().numpy()
    radius = GRID_SPACING * (GRID_N // 2) * math.sqrt(3.0) + max(GRID_REACH, GRID_PROBE) + float(xyzr[:, 3].max()) + margin
    idx = np.flatnonzero(np.linalg.norm(xyzr[:, :3], axis=1) <= radius)
    if rounds_kept is not None:
        idx = idx[idx < ROUND * TILE] if rounds_kept == "first" else idx[idx >= ROUND * TILE]
    return xyzr[idx, :3], xyzr[idx, 3]
