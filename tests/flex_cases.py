"""Named heavy-atom graphs with 3D coordinates for the flexible-pose tests (`interactions.torsion_tree`,
`interactions.optimise_pose_flexible`; DESIGN.md section 6, "Flexible pose"), each with the torsion tree written out BY
HAND: the smallest shapes at which the tree or the walk can still go wrong.  Importing this module needs no GPU.

Coordinates come from internal coordinates (bond 1.53 A, angle 112 degrees, the dihedrals given), rings from regular
polygons; they are plausible, not minimised - the walk's tests need a conformer, not a good one."""
import math

import numpy as np

F32 = np.float32


class Graph:
    """z [n] int, bonds [n,n] int8 symmetric codes, x [n,3] fp32, and the hand-written tree: `torsions` [(a, b)] in
    order (b inside the moving side), `sides` [sorted atoms of the moving side], `found` (torsions before the limit)."""

    def __init__(self, name, z, edges, x, torsions, sides, found=None):
        n = len(z)
        self.name, self.n = name, n
        self.z = np.asarray(z, dtype=np.int32)
        self.bonds = np.zeros((n, n), dtype=np.int8)
        for i, j, code in edges:
            self.bonds[i, j] = self.bonds[j, i] = code
        self.x = np.asarray(x, dtype=F32).reshape(n, 3)
        self.torsions, self.sides = list(torsions), [sorted(s) for s in sides]
        self.found = len(self.torsions) if found is None else found


def _place(x, i, j, k, bond, angle_deg, dihedral_deg):
    """The point at `bond` from x[k], at `angle_deg` to x[j], at `dihedral_deg` about j-k from x[i] (NeRF)."""
    a, t = math.radians(angle_deg), math.radians(dihedral_deg)
    bc = x[k] - x[j]
    bc /= np.linalg.norm(bc)
    nrm = np.cross(x[j] - x[i], bc)
    nrm /= np.linalg.norm(nrm)
    m = np.stack([bc, np.cross(nrm, bc), nrm], axis=1)
    d = np.array([-bond * math.cos(a), bond * math.sin(a) * math.cos(t), bond * math.sin(a) * math.sin(t)])
    return x[k] + m @ d


def chain_coords(n, dihedrals=None, bond=1.53, angle=112.0):
    """n atoms in a chain; dihedral k (degrees) places atom k + 3; default alternates 180, 65, -170, 72, ..."""
    default = (180.0, 65.0, -170.0, 72.0, 175.0, -68.0)
    x = np.zeros((max(n, 3), 3))
    x[1] = (bond, 0.0, 0.0)
    a = math.radians(angle)
    x[2] = x[1] + bond * np.array([-math.cos(a), math.sin(a), 0.0])
    for k in range(3, n):
        t = dihedrals[k - 3] if dihedrals is not None else default[(k - 3) % len(default)]
        x = np.vstack([x, np.zeros((1, 3))]) if len(x) <= k else x
        x[k] = _place(x, k - 3, k - 2, k - 1, bond, angle, t)
    return x[:n]


def ring_coords(m, bond, pucker=0.0):
    r = bond / (2.0 * math.sin(math.pi / m))
    return np.array([[r * math.cos(2 * math.pi * k / m), r * math.sin(2 * math.pi * k / m), pucker * (-1) ** k]
                     for k in range(m)])


def _alkane(name, n, limit=16, dihedrals=None):
    edges = [(i, i + 1, 1) for i in range(n - 1)]
    torsions, sides = [], []
    for a in range(1, n - 2):                            # bond (a, a + 1), both ends of degree 2
        low, high = list(range(0, a + 1)), list(range(a + 1, n))
        if len(high) <= len(low):                        # a tie: the part of the higher-indexed end
            torsions.append((a, a + 1)); sides.append(high)
        else:
            torsions.append((a + 1, a)); sides.append(low)
    found = len(torsions)
    return Graph(name, [6] * n, edges, chain_coords(n, dihedrals), torsions[:limit], sides[:limit], found)


def _benzene_edges(first):
    return [(first + k, first + (k + 1) % 6, 4) for k in range(6)]


def cases():
    out = [_alkane("butane", 4)]

    ring = ring_coords(6, 1.39)
    second = ring.copy()
    second[:, 0] = -second[:, 0]                         # mirrored, so that atom 6 faces atom 0
    tilt = math.radians(40.0)                            # twisted about the x axis, moved along it
    rot = np.array([[1, 0, 0], [0, math.cos(tilt), -math.sin(tilt)], [0, math.sin(tilt), math.cos(tilt)]])
    second = second @ rot.T + np.array([2 * 1.39 + 1.48, 0.0, 0.0])
    out.append(Graph("biphenyl", [6] * 12, _benzene_edges(0) + _benzene_edges(6) + [(0, 6, 1)],
                     np.vstack([ring, second]), [(0, 6)], [range(6, 12)]))

    nma = chain_coords(4, [180.0], bond=1.40, angle=120.0)           # C0 - C1 - N3 - C4 with O2 on C1
    o = nma[1] + 1.23 * np.array([0.5, -math.sqrt(3) / 2, 0.0])
    out.append(Graph("n_methylacetamide", [6, 6, 8, 7, 6], [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1)],
                     np.vstack([nma[0], nma[1], o, nma[2], nma[3]]), [], []))

    methyl = ring[0] + 1.51 * ring[0] / np.linalg.norm(ring[0])
    out.append(Graph("toluene", [6] * 7, _benzene_edges(0) + [(0, 6, 1)], np.vstack([ring, methyl]), [], []))
    out.append(Graph("benzene", [6] * 6, _benzene_edges(0), ring, [], []))
    out.append(_alkane("hexane", 6))

    # isopentylbenzene: ring 0..5, C6 on C0, C7, C8 with the two methyls C9 and C10
    x = np.vstack([ring, np.zeros((5, 3))])
    x[6] = methyl
    x[7] = _place(x, 1, 0, 6, 1.53, 112.0, 80.0)
    x[8] = _place(x, 0, 6, 7, 1.53, 112.0, 175.0)
    x[9] = _place(x, 6, 7, 8, 1.53, 112.0, 60.0)
    x[10] = _place(x, 6, 7, 8, 1.53, 112.0, -62.0)
    out.append(Graph("isopentylbenzene", [6] * 11,
                     _benzene_edges(0) + [(0, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (8, 10, 1)], x,
                     [(0, 6), (6, 7), (7, 8)], [range(6, 11), range(7, 11), range(8, 11)]))

    out.append(Graph("ring12", [6] * 12, [(k, (k + 1) % 12, 1) for k in range(12)], ring_coords(12, 1.37, 0.35), [], []))

    # two fragments: propane 0..2 (no torsion) and butane 3..6, 6 A away
    frag = np.vstack([chain_coords(3), chain_coords(4) + np.array([0.0, 0.0, 6.0])])
    out.append(Graph("two_fragments", [6] * 7, [(0, 1, 1), (1, 2, 1), (3, 4, 1), (4, 5, 1), (5, 6, 1)], frag,
                     [(4, 5)], [[5, 6]]))

    out.append(_alkane("c19", 19))
    out.append(_alkane("c20", 20))
    out.append(_alkane("c64", 64))
    out.append(_alkane("folded_heptane", 7, dihedrals=[28.0, 22.0, 26.0, 18.0]))     # its ends overlap: CLASH > 0
    # two benzene fragments 2.1 A apart, face to face: no torsion, yet CLASH > 0 - its bits must survive a rigid walk
    out.append(Graph("stacked_benzenes", [6] * 12, _benzene_edges(0) + _benzene_edges(6),
                     np.vstack([ring, ring + np.array([0.3, 0.2, 2.1])]), [], []))
    out.append(Graph("one_atom", [8], [], np.array([[0.3, -0.2, 0.1]]), [], []))
    out.append(Graph("empty", [], [], np.zeros((0, 3)), [], []))
    return out


def stereo_cases():
    """A chiral case (butan-2-ol: C0 - C1(O4) - C2 - C3) and a C=C case (hex-2-ene: C0 - C1 = C2 - C3 - C4 - C5), each
    with a torsion next to its stereo element."""
    x = chain_coords(4, [65.0])
    o = _place(x, 3, 2, 1, 1.43, 109.5, -120.0)
    butanol = Graph("butan_2_ol", [6, 6, 6, 6, 8], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (1, 4, 1)], np.vstack([x, o]),
                    [(1, 2)], [[2, 3]])
    hexene = Graph("hex_2_ene", [6] * 6, [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 1), (4, 5, 1)],
                   chain_coords(6, [180.0, 115.0, 68.0]), [(2, 3), (3, 4)], [[3, 4, 5], [4, 5]])
    return [butanol, hexene]


def by_name():
    return {g.name: g for g in cases() + stereo_cases()}


def padded(graphs, width=None, junk_seed=None):
    """(z [B,W] int32, bonds [B,W,W] int8, n [B] int32, x [B,W,3] fp32) of the graphs padded to `width` (default: the
    widest); `junk_seed`: everything at and beyond a row's atoms - and every diagonal - holds seeded junk, not zeros."""
    W = max([g.n for g in graphs] + [1]) if width is None else width
    B = len(graphs)
    if junk_seed is None:
        z, bonds = np.zeros((B, W), dtype=np.int32), np.zeros((B, W, W), dtype=np.int8)
    else:
        g = np.random.default_rng(junk_seed)
        z = g.integers(1, 36, size=(B, W)).astype(np.int32)
        bonds = g.integers(-3, 9, size=(B, W, W)).astype(np.int8)
    x = np.zeros((B, W, 3), dtype=F32)
    for b, gr in enumerate(graphs):
        assert gr.n <= W
        z[b, :gr.n] = gr.z
        diag = np.diagonal(bonds[b]).copy()
        bonds[b, :gr.n, :gr.n] = gr.bonds
        if junk_seed is not None:
            idx = np.arange(gr.n)
            bonds[b, idx, idx] = diag[:gr.n]
        x[b, :gr.n] = gr.x
    return z, bonds, np.array([g.n for g in graphs], dtype=np.int32), x
