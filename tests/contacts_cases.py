"""Inputs of the receptor-contact tests (tests/test_contacts_host.py, tests/test_contacts_gpu.py): seeded ligands in typed,
grouped pockets, hand-placed pairs at the thresholds, lattices that fill the kernel's two capacities exactly, and the recipe
of the PDB fixture tests/golden/contacts_pocket.pdb.  Importing this module needs no GPU."""
import functools
import os

import numpy as np

import contacts_ref as CR
import interactions_ref as IR

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PDB_FIXTURE = os.path.join(GOLDEN, "contacts_pocket.pdb")


class Case:
    """One ligand against one typed, grouped receptor as given: x [n,3] fp32, z [n], t [n] type bits; rec [R,3] fp32, rec_z
    [R], rec_t [R], groups [R] (any order: the fingerprint does not depend on it)."""
    def __init__(self, name, x, z, t, rec, rec_z, rec_t, groups):
        self.name = name
        self.x, self.z, self.t = np.asarray(x, dtype=F32).reshape(-1, 3), np.asarray(z, dtype=np.int64), np.asarray(t, dtype=np.uint8)
        self.rec, self.rec_z = np.asarray(rec, dtype=F32).reshape(-1, 3), np.asarray(rec_z, dtype=np.int64)
        self.rec_t, self.groups = np.asarray(rec_t, dtype=np.uint8), np.asarray(groups, dtype=np.int64)
        self.n = len(self.x)

    @property
    def receptor(self):
        """The (coords, atomic numbers, types) triple `contacts.prepare_receptor` takes beside `groups=`."""
        import torch
        return torch.from_numpy(self.rec), torch.from_numpy(self.rec_z), torch.from_numpy(self.rec_t)

    def expected(self, mistake=None, order=None):
        return CR.fingerprint(self.x, IR.radii(self.z), self.t, self.rec, IR.radii(self.rec_z), self.rec_t, self.groups,
                              mistake, order)

    def __repr__(self):
        return f"Case({self.name}: n={self.n}, R={len(self.rec)})"


def pocket(name, seed, n, R, n_groups=None):
    """A random walk of n atoms in a jittered 2.6 A lattice carved 2.6 A round its atoms - close enough for full hydrogen
    bonds (d <= -0.7 A needs a centre distance of about 2.8 A) - the R atoms nearest the ligand's middle.  Atom j belongs to
    group j % n_groups (default: about R / 6 groups), so a group's atoms lie apart and, beyond 256 atoms, in different
    tiles."""
    g = np.random.default_rng(seed)
    lig = IR.walk(n, g)
    axis = np.arange(-6, 7) * 2.6
    pts = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3) + lig.mean(0)
    pts = pts + g.normal(size=pts.shape) * 0.3
    pts = pts[np.linalg.norm(pts[:, None, :] - lig[None, :, :], axis=2).min(axis=1) > 2.6]
    pts = pts[np.argsort(np.linalg.norm(pts - lig.mean(0), axis=1), kind="stable")[:R]]
    assert len(pts) == R, (name, len(pts))
    n_groups = max(1, R // 6) if n_groups is None else n_groups
    return Case(name, lig, g.choice([6, 6, 6, 7, 8, 16, 17], size=n), g.integers(0, 8, size=n), pts,
                g.choice([6, 6, 6, 7, 8, 16, 30], size=R), g.integers(0, 8, size=R), np.arange(R) % n_groups + 3)


@functools.lru_cache(maxsize=None)
def cases():
    """Receptor sizes 1, 255, 256, 257 and 513 (the tile tail and several tiles) and ligand sizes 1, 27, 63 and 64."""
    return (pocket("R1", 31, 27, 1), pocket("R255", 32, 27, 255), pocket("R256", 33, 27, 256), pocket("R257", 34, 27, 257),
            pocket("R513", 35, 27, 513, n_groups=40), pocket("n1", 36, 1, 300), pocket("n63", 37, 63, 600),
            pocket("n64", 38, 64, 600))


def two_kinds_one_group():
    """Two atoms of one group, in one tile, touched by different ligand atoms with different kinds: a donor N 2.7 A from an
    acceptor O (d = -0.8: a full hydrogen bond) and, 12 A away, a hydrophobic C 4.0 A from a hydrophobic C (d = 0.2); a third
    receptor atom of another group lies between them out of contact.  The entry is (5, CONTACT | HYDROPHOBIC |
    HBOND_DONOR)."""
    x = [[0.0, 0.0, 0.0], [12.0, 0.0, 0.0]]
    rec = [[0.0, 2.7, 0.0], [12.0, 0.0, 4.0], [6.0, 6.0, 0.0]]
    return Case("two_kinds", x, [7, 6], [CR.T_DONOR, CR.T_HYDROPHOBIC], rec, [8, 6, 6],
                [CR.T_ACCEPTOR, CR.T_HYDROPHOBIC, CR.T_HYDROPHOBIC], [5, 5, 9])


def threshold_rows(which):
    """Seven one-atom ligands against one receptor atom at the origin, the ligand's x the fp32 neighbours -3 .. +3 of the
    distance at which d meets the threshold: "contact" - a hydrophobic carbon and a chlorine (1.9 + 1.8) round r = 4.2, where
    the middle row has d = 0.5f EXACTLY (the fp32 radius sum is a multiple of 2^-21, so sum + 0.5f and the difference back
    are exact): the row that tells `<=` from `<`; "hbond" - a donor N (1.8) and an acceptor O (1.7) round r = 2.8, d = -0.7f.
    The restatement decides each side."""
    z_l, t_l, z_r, t_r, r0 = ((6, CR.T_HYDROPHOBIC, 17, CR.T_HYDROPHOBIC, F32(F32(F32(1.9) + F32(1.8)) + F32(0.5)))
                              if which == "contact" else (7, CR.T_DONOR, 8, CR.T_ACCEPTOR, F32(2.8)))
    rows = []
    for k in range(-3, 4):
        r = r0
        for _ in range(abs(k)):
            r = np.nextafter(r, F32(np.inf if k > 0 else -np.inf))
        rows.append(Case(f"{which}{k:+d}", [[r, 0.0, 0.0]], [z_l], [t_l], [[0.0, 0.0, 0.0]], [z_r], [t_r], [4]))
    return rows


def capacity(kind, extra):
    """One carbon at the origin in a cubic lattice of carbons, every receptor atom hydrophobic: the `count` lattice points
    nearest the origin all lie within 4.2 A (d <= 0.4: in contact, clear of the threshold), every other kept point beyond
    4.6 A (d >= 0.8: not in contact).  "groups": spacing 1.0 A, every atom its own group, count = 256 + extra - exactly the
    entry capacity, or one over.  "candidates": spacing 0.4 A, 200 groups, count = 2048 + extra - exactly the candidate
    capacity, or one over."""
    spacing, count = (1.0, 256 + extra) if kind == "groups" else (0.4, 2048 + extra)
    k = int(6.0 / spacing)
    axis = (np.arange(-k, k + 1) + 0.37) * spacing             # off the origin: no receptor atom on the ligand's
    pts = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    dist = np.linalg.norm(pts, axis=1)
    order = np.argsort(dist, kind="stable")
    inner = order[:count]
    assert dist[inner].max() < 4.2, (kind, extra, dist[inner].max())
    outer = order[count:][dist[order[count:]] > 4.6][:60]
    pts = np.concatenate([pts[inner], pts[outer]])
    g = np.random.default_rng(5)
    pts = pts[g.permutation(len(pts))]
    groups = np.arange(len(pts)) if kind == "groups" else np.arange(len(pts)) % 200
    return Case(f"{kind}{count}", [[0.0, 0.0, 0.0]], [6], [CR.T_HYDROPHOBIC], pts, np.full(len(pts), 6),
                np.full(len(pts), CR.T_HYDROPHOBIC), groups)


# ----------------------------------------------------------------------------------------------- the PDB fixture
_RESIDUES = (("SER", (("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C"), ("OG", "O"))),
             ("LEU", (("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C"), ("CG", "C"), ("CD1", "C"), ("CD2", "C"))),
             ("ASP", (("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C"), ("CG", "C"), ("OD1", "O"), ("OD2", "O"))),
             ("LYS", (("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C"), ("CG", "C"), ("NZ", "N"))),
             ("PHE", (("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C"), ("CG", "C"), ("CZ", "C"))))


def reference_conformer():
    """The reference conformer of the generation tests (`test_receptor_relief_gpu._posed_setup`), fp64 [n,3]."""
    ref = np.load(os.path.join(GOLDEN, "context_shape.npz"))["ceyyag_xyz"]
    return np.asarray(ref, dtype=np.float64) + np.array([12.0, -5.0, 3.0])


def pdb_from_points(pts):
    """PDB text with one heavy atom per point: the points are taken in runs of neighbours (sorted by 5 A cell, then x) as the
    atoms of residues that cycle through `_RESIDUES` on the chains A and B, so that a residue's atoms lie together."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cell = np.floor(pts / 5.0).astype(np.int64)
    pts = pts[np.lexsort((pts[:, 0], cell[:, 2], cell[:, 1], cell[:, 0]))]
    lines, serial, j, res = [], 1, 0, 0
    while j < len(pts):
        name, atoms = _RESIDUES[res % len(_RESIDUES)]
        chain = "A" if res % 2 == 0 else "B"
        for atom, element in atoms:
            if j == len(pts):
                break
            x, y, z = pts[j]
            lines.append(f"ATOM  {serial:5d} {atom:<4s} {name} {chain}{res // 2 + 1:4d}    {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00"
                         f"          {element:>2s}")
            serial, j = serial + 1, j + 1
        res += 1
    return "\n".join(lines + ["END", ""])


def pocket_pdb_text():
    """The text of tests/golden/contacts_pocket.pdb: a seeded, jittered 2.4 A lattice within 7 A of the reference conformer's
    atoms, carved 3.0 A round them, as `pdb_from_points` writes it: residues that cycle through SER, LEU, ASP, LYS and PHE on two
    chains - atom names and elements of the residue templates, so the typing reads donors, acceptors and hydrophobic
    carbons."""
    ref = reference_conformer()
    g = np.random.default_rng(2024)
    lo, hi = ref.min(0) - 7.0, ref.max(0) + 7.0
    axes = [np.arange(lo[d], hi[d], 2.4) for d in range(3)]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    pts = pts + g.normal(size=pts.shape) * 0.25
    near = np.linalg.norm(pts[:, None, :] - ref[None, :, :], axis=2).min(axis=1)
    pts = pts[(near > 3.0) & (near < 7.0)]
    return pdb_from_points(pts)


def pocket_pdb():
    with open(PDB_FIXTURE) as f:
        return f.read()
