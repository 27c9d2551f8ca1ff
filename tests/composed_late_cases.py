"""A second batch of known molecules for the composed post-generation path ("Which coordinates and
which graph each returned value reads"): the rows the option families added behind `composed_cases` need before a record
can tell a right value from a wrong one - a parent fragment BEHIND a smaller one (so that `atom_map` does not start at 0),
tetrahedral centres and a pair of stereoisomers, double-bond descriptors, an undefined centre, rows with and without a
torsion, rows that share a scaffold or a framework but not a graph, a dropped row and rows of one and of two atoms.
`tests/test_composed_late_host.py` proves the batch fit to judge by - through the restatements alone - and
`tests/test_composed_late_gpu.py` runs it through `generate_conformers*`.

Every molecule but one is a fixture of `hydrogens_cases`, `stereo_cases`, `flex_cases` or `composed_cases`; the one new
graph is the undefined centre (`_planar_centre`, which says why no existing fixture serves).  The fixtures with a crowded
methyl group - the 2,3-dichlorobutanes, the dimethylcyclohexanes, `flex_cases`' butan-2-ol - stay out: under the noise
their methyl rotors tie, and the hydrogens' tolerance does not hold on them (`composed_cases.hydrogen_conditions`).  The
noise, the joining of two fragments, the reference, the fp64 pose, the carved pocket and the injection harness are
`composed_cases`' own.  Importing this module needs no GPU."""
import functools
import inspect
import types

import numpy as np
import torch

import composed_cases as CC
import flex_cases as FC
import hydrogens_cases as HC
import standardize_ref as SR
import stereo_cases as STC

SIGMA = CC.SIGMA                                    # A: the seeded noise on every coordinate
NOISE_SEED = 18                                     # chosen on the CPU: `test_composed_late_host.py` holds with it
WIDTH = 16                                          # the sampler's N of the injected batch (> the largest row, 14)
RELAX_STEPS, REFINE_STEPS = CC.RELAX_STEPS, CC.REFINE_STEPS
RELIEF_STEPS = 16                                   # `relieve_clashes`: trials of the relief
OPTIMISE_STEPS = 2                                  # `optimise_pose`: trials of either walk.  Chosen by the host file's condition
#                                                     (from the fp64 pose the restatement keeps no trial on one row at 2, one of
#                                                     the first three on every row); on the GPU, from the product's own relieved
#                                                     poses, every row keeps a trial
POCKET_SEMI_AXES = (6.0, 4.0, 3.5)                  # A: call B's cavity, tight enough for rows of up to 14 atoms to reach its wall
MAX_SHIFT = 2.0                                     # `interactions.OPTIMISE_MAX_SHIFT`, what the entries walk with
RECEPTOR_SEED = 5                                   # elements and interaction types of the receptor's atoms
DROPPED = "cyclopentadienyl"
SHIFTED = ("ethanol and isopentylbenzene", "water and butan-2-ol")       # the parent behind a smaller fragment
STEREOISOMERS = ("CHFClBr", "mirror CHFClBr")                            # one graph, two stereo identities
SAME_STEREOISOMER = "CHFClBr again"                                      # the first of them once more, other noise
UNDEFINED = "planar CFClBr(CN)"
ONE_ATOM = "one atom"                                                   # no principal frame to pose by

# what `test_stereo_gpu`'s fuzz keeps every |chi| and |cos| outside of, so that fp32 and fp64 take every decision alike
STEREO_BAND = tuple(inspect.signature(STC.fuzz_set).parameters[k].default for k in ("low", "high"))

# the substructure options of call A: each of the first two is present on some kept rows and absent on others
REQUIRE = ["[CH3]"]                                 # constrains the hydrogen count: the `nh` column of the table
EXCLUDE = ["[#17]"]
COUNTS = ["c:1:c:c:c:c:c:1", "[#6]~!@[#6]", "[#6;H0]"]


def _of_stereo(mol):
    z, adj, n, xyz = mol
    return dict(mol=(list(z), [list(r) for r in adj], n), xyz=np.asarray(xyz, dtype=np.float64).astype(np.float32))


def _of_flex(g):
    return dict(mol=(g.z.tolist(), g.bonds.tolist(), g.n), xyz=g.x.copy())


def _planar_centre():
    """A carbon with four different single-bonded neighbours - F, Cl, Br and a cyano carbon - in one plane with it: a
    tetrahedral candidate whose signed volume is 0, so the centre is undefined.  (The planar centre of `stereo_cases` has
    three neighbours: its hydrogen would sit on the degenerate sum of three coplanar directions, where the hydrogens'
    tolerance does not hold.)"""
    return _of_stereo(STC._mol([6, 9, 17, 35, 6, 7], [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (4, 5, 3)],
                               [(0, 0, 0), (1.35, 0, 0), (0, 1.76, 0), (-1.94, 0, 0), (0, -1.46, 0), (0, -2.62, 0)]))


def _rows():
    """name -> fixture, in batch order, with what the standardisation must make of it: (status, atom_map, n_fragments)."""
    f, flex = HC.fixtures(), FC.by_name()
    dead = dict(f["pyrrole"], mol=([6] * 5, f["pyrrole"]["mol"][1], 5))         # cyclopentadienyl: no Kekule form
    whole = lambda n: (0, list(range(n)), 1)                                     # noqa: E731
    return [(SHIFTED[0], CC._joined(f["ethanol"], _of_flex(flex["isopentylbenzene"])), (0, list(range(3, 14)), 2)),
            (STEREOISOMERS[0], _of_stereo(STC.CHFCLBR), whole(4)),
            ("toluene", _of_flex(flex["toluene"]), whole(7)),
            (STEREOISOMERS[1], _of_stereo(STC.mirror(STC.CHFCLBR)), whole(4)),
            (DROPPED, dead, (SR.NOT_KEKULIZABLE, list(range(5)), 1)),              # the dropped row, mid-batch
            (SHIFTED[1], CC._joined(f["water"], _of_stereo(STC.BUTAN_2_OL)), (0, list(range(1, 6)), 2)),
            ("hexa-2,4-diene", _of_stereo(STC.HEXADIENE), whole(6)),
            ("biphenyl", _of_flex(flex["biphenyl"]), whole(12)),
            ("pyridine", f["pyridine"], whole(6)),
            ("two atoms", f["formaldehyde"], whole(2)),
            (UNDEFINED, _planar_centre(), whole(6)),
            ("benzene", f["benzene"], whole(6)),
            ("reference molecule", CC._reference_fixture(), whole(14)),
            ("hexa-2,4-diene, cis-trans", _of_stereo(STC.HEXADIENE_CIS_TRANS), whole(6)),
            (SAME_STEREOISOMER, _of_stereo(STC.CHFCLBR), whole(4)),                # `unique="stereo"` merges it with row 1
            (ONE_ATOM, f["water"], whole(1))]


@functools.lru_cache(maxsize=None)
def batch():
    """The items of the batch, in batch order: dict(name, mol, xyz fp32 with the seeded noise, expect)."""
    rng = np.random.RandomState(NOISE_SEED)
    out = []
    for name, fx, expect in _rows():
        z, codes, n = fx["mol"]
        xyz = (fx["xyz"].astype(np.float64) + rng.normal(0.0, SIGMA, size=(n, 3))).astype(np.float32)
        out.append(dict(name=name, mol=(list(z), [list(r) for r in codes], n), xyz=xyz, expect=expect))
    return out


@functools.lru_cache(maxsize=None)
def standardized():
    """name -> `standardize_ref.standardize` of the item with its coordinates: computed once, never written to."""
    return {it["name"]: SR.standardize(*it["mol"], coords=it["xyz"]) for it in batch()}


def parent(item):
    """(mol (z, codes, n), xyz fp32 [n,3]) of an item's parent fragment, by the restatement."""
    s = standardized()[item["name"]]
    return (s["atomic_numbers"], s["bond_orders"], s["n_out"]), item["xyz"][s["atom_map"]]


def kept():
    return [it for it in batch() if standardized()[it["name"]]["status"] == 0]


reference = CC.reference                            # the reference of `composed_cases`: conformer and graph


@functools.lru_cache(maxsize=None)
def posed_parents():
    """name -> the fp64 pose (`composed_cases.pose_fp64`, fp32 [n,3] torch) of every kept row's parent fragment of three
    or more atoms at its input coordinates."""
    ref = reference()[0]
    return {it["name"]: CC.pose_fp64(ref, parent(it)[1]) for it in kept() if parent(it)[0][2] >= 3}


@functools.lru_cache(maxsize=None)
def receptor():
    """The typed receptor of call A, (coords [R,3] fp32, atomic numbers [R], interaction types [R]): the carved pocket of
    `composed_cases.receptor` - a wall moved in from either side - round the reference and the fp64 poses of this batch,
    its atoms given seeded elements and interaction types as `test_pose_optimise_gpu.test_generation_with_optimise_pose`
    gives them.  Chosen on the CPU so that `test_composed_late_host.py` finds rows the relief moves and rows either walk
    moves, turns or leaves alone."""
    base = [types.SimpleNamespace(coords=x, pose=True) for x in posed_parents().values()]
    walls = [CC.carved_pocket(reference()[0], base, spacing=1.8, shift=s) for s in (3.0, -3.0)]
    pts = torch.cat([w[0] for w in walls])
    g = torch.Generator().manual_seed(RECEPTOR_SEED)
    z = torch.tensor([6, 6, 7, 8])[torch.randint(0, 4, (len(pts),), generator=g)]
    return pts, z, torch.randint(0, 8, (len(pts),), generator=g)


def pocket(device):
    """The `Pocket` of call B: `pocket.find_pocket` with the settings of `test_pocket_gpu`'s end-to-end case on the carved
    block of `pocket_cases` - the same cube, lattice and seed, so a receptor of the same size - with a tighter cavity
    (`POCKET_SEMI_AXES` against 9 x 6 x 5 A, where every row of this batch lies inside the mesh before and after the
    receptor stages): here the relief and the walk carry atoms across the mesh."""
    import pocket_cases as PKC
    from ml_conformer_generator_amd import pocket as PK
    xyz, z = PKC.carved_block(semi=POCKET_SEMI_AXES)
    return PK.find_pocket((torch.from_numpy(xyz), torch.from_numpy(z)), (0.0, 0.0, 0.0), device=device, **PKC.BLOCK)
