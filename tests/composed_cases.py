"""A batch of known molecules with real geometry, and the shared pieces of one generation call with every post-generation
option on ("Which coordinates and which graph each returned value reads"): what
`tests/test_composed_path_host.py` proves fit to judge by - through the restatements alone - and what
`tests/test_composed_path_gpu.py` runs through `generate_conformers*`.

An item is a dict like the other case modules': name, mol (z, codes, n) and xyz fp32 [n,3].  The molecules are those of
`hydrogens_cases.fixtures()`, `geometry_ref.fused56()` and `pharmacophore_cases.REFERENCE_MOLECULE`; a two-fragment row
is two of them, the second moved `FRAGMENT_GAP` A from the first; every coordinate carries seeded Gaussian noise of
`SIGMA` A, so that the relaxation has something to do.  No row has a degenerate geometry (`hydrogens_cases._degenerate`,
acetonitrile and propyne stay out: the hydrogens' tolerance does not hold on them).

The module also holds the reference (conformer and graph), the carved receptor pocket (`carved_pocket`, which
`test_receptor_relief_gpu.py` imports back), the fp64 pose of a molecule onto the reference (`pose_fp64`) and the
injection harness of the generation tests (`substituted`, which `test_standardize_gpu.py` imports back).  Importing it
needs no GPU."""
import functools
import math
import types

import numpy as np
import torch

import geometry_ref as GR
import hydrogens_cases as HC
import hydrogens_ref as HR
import overlay_refine_ref as ORR
import pharmacophore_cases as PC
import standardize_cases as SC
import standardize_ref as SR

SIGMA = 0.15                                        # A: the seeded noise on every coordinate
NOISE_SEED = 30                                     # chosen on the CPU: `test_composed_path_host.py` holds with it
FRAGMENT_GAP = 8.0                                  # A between the centroids of the two fragments of a row
WIDTH = 16                                          # the sampler's N of the injected batch (> the largest row)
RELAX_STEPS, REFINE_STEPS = 8, 16                   # `relax_geometry`, `refine_overlay` of the composed call


def _radial(ring, k, dist):
    u = np.asarray(ring[k]) / np.linalg.norm(ring[k])
    return u * dist, u


def _turned(u, deg):
    """u turned by `deg` about z."""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([c * u[0] - s * u[1], s * u[0] + c * u[1], u[2]])


def _reference_fixture():
    """`pharmacophore_cases.REFERENCE_MOLECULE` at an idealised geometry: the benzene ring of `hydrogens_cases` in the
    xy-plane, every substituent's first atom on its ring atom's radius, the carboxyl group in the plane, the amine's N
    and the ethyl's end carbon at the tetrahedral angle above and below it."""
    ring = HC._ring_xyz(6, HC.R6)
    x = [np.array(p) for p in ring] + [None] * 8
    tet, up = math.radians(180.0 - 109.4712), np.array([0.0, 0.0, 1.0])
    x[6], u0 = _radial(ring, 0, HC.R6 + 1.50)                                  # carboxyl C on 0
    x[7] = x[6] + 1.23 * _turned(u0, 60.0)                                      # =O
    x[8] = x[6] + 1.35 * _turned(u0, -60.0)                                     # -OH
    x[10], u3 = _radial(ring, 3, HC.R6 + 1.51)                                  # CH2 on 3
    x[9] = x[10] + HC.CN * (math.cos(tet) * u3 + math.sin(tet) * up)            # its NH2
    x[11], _ = _radial(ring, 2, HC.R6 + 1.74)                                   # Cl on 2
    x[12], u4 = _radial(ring, 4, HC.R6 + 1.51)                                  # ethyl on 4
    x[13] = x[12] + HC.CC * (math.cos(tet) * u4 - math.sin(tet) * up)
    z, adj, n = PC.REFERENCE_MOLECULE
    return dict(mol=(list(z), [list(r) for r in adj], n),
                xyz=(np.array(x) @ HC.GENERIC.T + HC.SHIFT).astype(np.float32), hydrogens=None, degenerate=False)


def _indole_fixture():
    """Indole's graph (N6 next to the fusion atom 1; every bond aromatic) on the planar 5-6 system of `geometry_ref`."""
    base = GR.fused56()
    z = [6] * 9
    z[6] = 7
    codes = [[4 if v else 0 for v in row] for row in base["bonds"].tolist()]
    return dict(mol=(z, codes, 9), xyz=(base["x"] @ HC.GENERIC.T + HC.SHIFT).astype(np.float32), hydrogens=None,
                degenerate=False)


def _joined(a, b):
    """Two fixtures as one row: b's atoms behind a's, b moved so that the centroids lie `FRAGMENT_GAP` A apart."""
    (za, ca, na), (zb, cb, nb) = a["mol"], b["mol"]
    codes = [[0] * (na + nb) for _ in range(na + nb)]
    for i in range(na):
        codes[i][:na] = ca[i]
    for i in range(nb):
        codes[na + i][na:] = cb[i]
    d = np.array([0.48, -0.6, 0.64])                                            # a unit vector off every axis
    move = a["xyz"].astype(np.float64).mean(0) + FRAGMENT_GAP * d - b["xyz"].astype(np.float64).mean(0)
    return dict(mol=(list(za) + list(zb), codes, na + nb),
                xyz=np.vstack([a["xyz"], (b["xyz"].astype(np.float64) + move).astype(np.float32)]))


# name -> what the standardisation must make of it: (status, atom_map, n_fragments)
def _rows():
    f = HC.fixtures()
    dead = dict(f["pyrrole"], mol=([6] * 5, f["pyrrole"]["mol"][1], 5))         # cyclopentadienyl: no Kekule form
    rows = [("phenol", f["phenol"], (0, list(range(7)), 1)),
            ("benzene and water", _joined(f["benzene"], f["water"]), (0, list(range(6)), 2)),
            ("imidazole", f["imidazole"], (0, list(range(5)), 1)),
            ("acetamide", f["acetamide"], (0, list(range(4)), 1)),
            ("one atom", f["water"], (0, [0], 1)),
            ("cyclopentadienyl", dead, (SR.NOT_KEKULIZABLE, list(range(5)), 1)),           # the dropped row, mid-batch
            ("propane and ethanol", _joined(f["propane"], f["ethanol"]), (0, [3, 4, 5], 2)),
            ("indole", _indole_fixture(), (0, list(range(9)), 1)),
            ("reference molecule", _reference_fixture(), (0, list(range(14)), 1)),
            ("two atoms", f["formaldehyde"], (0, [0, 1], 1)),
            ("pyridine", f["pyridine"], (0, list(range(6)), 1)),
            ("benzene", f["benzene"], (0, list(range(6)), 1))]                             # the graph of row 1's parent, again
    return rows


@functools.lru_cache(maxsize=None)
def batch():
    """The items of the composed batch, in batch order: dict(name, mol, xyz fp32 with the seeded noise, expect)."""
    rng = np.random.RandomState(NOISE_SEED)
    out = []
    for name, fx, expect in _rows():
        z, codes, n = fx["mol"]
        xyz = (fx["xyz"].astype(np.float64) + rng.normal(0.0, SIGMA, size=(n, 3))).astype(np.float32)
        out.append(dict(name=name, mol=(list(z), [list(r) for r in codes], n), xyz=xyz, expect=expect))
    return out


DROPPED = "cyclopentadienyl"


@functools.lru_cache(maxsize=None)
def standardized():
    """name -> `standardize_ref.standardize` of the item with its coordinates: computed once, never written to."""
    return {it["name"]: SR.standardize(*it["mol"], coords=it["xyz"]) for it in batch()}


def parent(item):
    """(mol (z, codes, n), xyz fp32 [n,3]) of an item's parent fragment, by the restatement."""
    s = standardized()[item["name"]]
    return (s["atomic_numbers"], s["bond_orders"], s["n_out"]), item["xyz"][s["atom_map"]]


def hydrogen_conditions(mol, xyz, name):
    """What `test_hydrogens_gpu.test_fixtures_meet_the_conditions_of_the_tolerance` asserts of a fixture without a
    written-in degeneracy, of one molecule (z, codes, n) at the coordinates `xyz`: where these hold, fp32 and fp64 take
    every decision alike and the derivation of the 1e-4 A applies.  Returns the restatement's result."""
    r = HR.place(*mol, xyz)
    t = r["trace"]
    assert np.abs(np.asarray(xyz)).max(initial=0.0) <= 16.0, name
    assert all(v >= 0.2 for v in t["sums"]), (name, t["sums"])
    assert all(v >= 1e-2 for v in t["tested"]), (name, t["tested"])
    assert all(g == 0.0 or g >= 1e-3 for g in t["perp_gaps"]), (name, t["perp_gaps"])
    for best, second in t["gaps"]:
        assert second - best >= 1e-3 or (best == 0.0 and second == 0.0), (name, best, second)
    return r


# ---- the reference ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference():
    """(coords [14,3] fp32 torch, graph (atomic numbers, bond codes [14,14] int8 torch)): `REFERENCE_MOLECULE` at its
    idealised geometry, without noise."""
    fx = _reference_fixture()
    z, adj, _ = fx["mol"]
    return torch.from_numpy(fx["xyz"].copy()), (list(z), torch.tensor(adj, dtype=torch.int8))


def reference_features():
    """The reference's pharmacophore features by the restatement: [(type index, fp32 xyz)]."""
    import pharmacophore_ref as PR
    xyz, (z, adj) = reference()
    t, rings, _ = PR.perceive(z, adj.tolist(), len(z))
    return PR.features(xyz.numpy(), t, rings)


def pose_fp64(ref_xyz, xyz, steps=REFINE_STEPS):
    """`xyz` [n,3] posed onto the reference in fp64, in the reference's own coordinates (fp32 [n,3]): the best of the four
    starts of `overlay_refine_ref.starts`, replaced by the first best refined candidate where that scores strictly
    better on the oracle's grid (what `refined_pose_scores` scores), taken back out of the reference's principal frame."""
    ref, x = torch.as_tensor(ref_xyz, dtype=torch.float32), torch.as_tensor(xyz, dtype=torch.float32)
    y, zs = ORR.starts(ref, x)
    start, which = ORR.first_max([ORR.oracle_tanimoto(y, z) for z in zs])
    pose = zs[which].double()
    cand = []
    for z in zs:
        G, t, _, _ = ORR.refine(y, z, steps)
        cand.append(z.double() @ G + t)
    best, pick = ORR.first_max([ORR.oracle_tanimoto(y, c.to(torch.float32)) for c in cand])
    if best > start:
        pose = cand[pick]
    centre = ref.double().mean(0)
    A = torch.cat([ref.double() - centre, torch.ones(ref.shape[0], 1, dtype=torch.float64)], 1)
    sol = torch.linalg.lstsq(A, y.double()).solution                           # y = (ref - centre) @ M + b
    return ((pose - sol[3]) @ torch.linalg.inv(sol[:3]) + centre).to(torch.float32)


@functools.lru_cache(maxsize=None)
def posed_parents():
    """name -> the fp64 pose (fp32 [n,3] torch) of every kept row's parent fragment of three or more atoms (a smaller
    one has no principal frame to pose by) at its input coordinates."""
    ref = reference()[0]
    out = {}
    for it in batch():
        (z, codes, n), xyz = parent(it)
        if standardized()[it["name"]]["status"] == 0 and n >= 3:
            out[it["name"]] = pose_fp64(ref, xyz)
    return out


# ---- the receptor -----------------------------------------------------------------------------------------------------
def carved_pocket(ref, base, spacing=2.6, shift=1.5):
    """The recipe's lattice around the posed molecules and the reference, carved 3.8 A around all of their atoms, then
    shifted by `shift` A along x so that the poses clash with one wall (and a move of `shift` A clears them again).
    `base`: records with `coords` and `pose` (None: not posed, left out).  `spacing`: the lattice constant in A."""
    g = np.random.default_rng(77)
    atoms = torch.cat([ref.float()] + [m.coords for m in base if m.pose is not None]).double().numpy()
    lo, hi = atoms.min(0) - 8.0, atoms.max(0) + 8.0
    axes = [np.arange(lo[d], hi[d], spacing) for d in range(3)]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    pts = pts + g.normal(size=pts.shape) * 0.3
    near = np.linalg.norm(pts[:, None, :] - atoms[None, :, :], axis=2).min(axis=1)
    pts = pts[near > 3.8] + np.array([shift, 0.0, 0.0])
    return torch.from_numpy(pts.astype(np.float32)), torch.full((len(pts),), 6)


@functools.lru_cache(maxsize=None)
def receptor():
    """The receptor of the composed call: the carved pocket round the reference and the fp64 poses of `posed_parents`,
    once with its wall moved in from -x and once from +x.  The molecules are smaller than the reference and lie inside
    its envelope, so the lattice is finer and the walls come closer than the recipe's defaults, and with a wall on
    either side the widest rows cannot be moved clear of both: chosen on the CPU so that `test_composed_path_host.py`
    finds clashing and clean rows, and rows the relief's restatement clears and rows it cannot."""
    base = [types.SimpleNamespace(coords=x, pose=True) for x in posed_parents().values()]
    walls = [carved_pocket(reference()[0], base, spacing=1.6, shift=s) for s in (2.5, -2.5)]
    return torch.cat([w[0] for w in walls]), torch.cat([w[1] for w in walls])


# ---- the injection harness --------------------------------------------------------------------------------------------
def substituted(monkeypatch, items, width=WIDTH, finish_all=False):
    """The shared generator (`test_shape_frames_gpu._gen`: 20 diffusion steps, synthetic weights, cached) with the items'
    chemistry substituted at its seams: the sampler stage (`edm_tensors`) returns the items' own coordinates and one-hot
    elements, and the bond write-back is given the items' codes in place of the GCN's argmax - the real hand-off, GCN,
    write-back, standardisation and everything behind it run on them.  `finish_all`: `_finish` keeps every record.
    Returns (generator, the items' full tensors on the host, the proxy's own flags for them)."""
    from test_shape_frames_gpu import DEV, _gen
    from ml_conformer_generator_amd import conformer_generator as CG
    gen = _gen()
    xyz, z, bonds, n = (torch.from_numpy(t) for t in SC.pad_batch(items, 42, width))
    h = torch.zeros(len(items), width, 8)
    for b in range(len(items)):
        for a in range(int(n[b])):
            h[b, a, list(gen.class_z).index(int(z[b, a]))] = 1.0
    mask = (torch.arange(width).view(1, -1) < n.view(-1, 1)).float().unsqueeze(-1)

    def edm_tensors(**kw):
        ids = kw.get("sample_ids")
        rows = torch.arange(kw["n_samples"]) if ids is None else torch.as_tensor(ids).long().cpu()
        return xyz[rows].to(DEV), h[rows].to(DEV), mask[rows].to(DEV)
    real_writeback = CG.bond_writeback_hip
    monkeypatch.setattr(gen, "edm_tensors", edm_tensors)
    monkeypatch.setattr(CG, "bond_writeback_hip", lambda bond, el, ng: real_writeback(bonds.to(bond.device), el, ng))
    if finish_all:
        monkeypatch.setattr(CG, "_finish", lambda mols, og, use_rdkit=None: (list(mols), 1.0))
    _, proxy = real_writeback(bonds.to(DEV), z.long().to(DEV), n.to(DEV))
    return gen, dict(xyz=xyz, z=z, bonds=bonds, n=n), proxy.cpu().tolist()
