"""Receptor interactions of posed molecules, on the GPU ("Receptor interactions"): does a posed
molecule interact with the pocket - hydrogen bonds to its donors and acceptors, contact with its hydrophobic wall - or does
it merely not bump into it (`receptor.py`)?

THE PACKAGE'S OWN, LABELLED DEFINITION.  It has the functional form of the AutoDock Vina scoring function (O. Trott, A. J.
Olson, J. Comput. Chem. 31, 455 (2010)), on the package's own atom typing, on heavy atoms only, with the intermolecular
terms only.  It is NOT AutoDock Vina's output and NOT a binding free energy: there is no search, no intramolecular term and
no hydrogen on either side; no agreement with any docking program is claimed.

Pair geometry   ligand atom i at x_i with interaction radius R_i, receptor atom j at y_j with R_j:
                r2 = dx*dx + dy*dy + dz*dz in fp32, unfused, in exactly this order (as `k_receptor_overlap` does); the pair
                COUNTS iff r2 < 64.0f - an 8 A cut-off decided in fp32; a pair that does not count contributes exactly +0
                to everything.  For a counted pair d = sqrtf(r2) - (R_i + R_j): the square root correctly rounded, the
                radius sum rounded first.
Radii           the form's own (`INTERACTION_RADII`, angstrom, keyed by Z), not `receptor.VDW_RADII`: C 1.9, N 1.8, O 1.7,
                F 1.5, P 2.1, S 2.0, Cl 1.8, Br 2.0, I 2.2, Si 2.2; the metals Mg, Ca, Mn, Fe, Co, Ni, Cu, Zn 1.2; any other
                element its `receptor.VDW_RADII` value (else `receptor.DEFAULT_RADIUS`).
Terms           of a counted pair, the piecewise ones evaluated from the fp32 d:
                g1 = exp(-(d / 0.5)^2);  g2 = exp(-((d - 3) / 2)^2);  rep = d*d if d < 0, else 0;
                hyd, only if both atoms are hydrophobic: 1 for d <= 0.5, 0 for d >= 1.5, linear between;
                hb, only if one atom is a donor and the other an acceptor, in either direction: 1 for d <= -0.7, 0 for
                d >= 0, linear between.
Score           per molecule E = (-0.0356 G1 - 0.00516 G2 + 0.840 REP - 0.0351 HYD - 0.587 HB) / (1 + 0.0585 n_rot), G1 ...
                HB the sums over the counted pairs, the weights constants of this definition; negative is better.
                `receptor_hbonds`: the counted donor / acceptor pairs with d <= -0.7f, an exact integer.  Per atom the
                same five sums over j alone and the atom's weighted, unnormalised contribution.
Ligand types    per-atom bits perceived from the returned graph alone (with `standardize`: the parent fragment's): donor
                (1) and acceptor (2) are `pharmacophore.perceive_features`' bits, unchanged; hydrophobic (4) is a C,
                aromatic or not, with no N or O neighbour, and F, Cl, Br, I.  This is WIDER than the pharmacophore's
                hydrophobe (a non-aromatic C all of whose neighbours are C; Cl, Br, I) on purpose: the term is a contact
                term over every apolar carbon, aromatic ones included, as in the form it follows.
Rotatable bonds n_rot = the code-1 chain bonds whose two ends both have heavy-atom degree >= 2 - one
                `substructure.match_substructures` call with `ROTATABLE_BOND`, count // 2.  THE PACKAGE'S RULE: amide and
                other conjugated single bonds are counted.
Receptor types  `receptor.load_typed_receptor` (a residue-template table for a PDB string, the element rules otherwise).
A molecule without atoms scores zeros, E = 0; one with a non-finite coordinate on a real atom NaN, hbonds = -1, the other
rows unaffected.  A molecule's outputs depend on its own atoms and the receptor's atoms only: the same bits in any batch, at
any row, at any padded width, with and without tile skipping, and whatever the order the receptor's atoms were listed in.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import torch

from . import _args, _lib
from . import config as _config
from . import pharmacophore as mcg_pharm
from . import receptor as mcg_receptor
from . import substructure as mcg_sub

CUTOFF = 8.0                    # angstrom; decided as r2 < 64.0f
WEIGHTS = dict(g1=-0.0356, g2=-0.00516, rep=0.840, hyd=-0.0351, hb=-0.587)
ROTOR_WEIGHT = 0.0585
TERM_NAMES = ("g1", "g2", "rep", "hyd", "hb")
HBOND_DISTANCE = -0.7           # angstrom of surface distance: a hydrogen bond counts in full at or below it
MAX_ATOMS = 64
MAX_BATCH = mcg_receptor.MAX_BATCH
TYPE_DONOR, TYPE_ACCEPTOR, TYPE_HYDROPHOBIC = (mcg_receptor.TYPE_DONOR, mcg_receptor.TYPE_ACCEPTOR,
                                               mcg_receptor.TYPE_HYDROPHOBIC)
INTERACTION_RADII = {6: 1.9, 7: 1.8, 8: 1.7, 9: 1.5, 15: 2.1, 16: 2.0, 17: 1.8, 35: 2.0, 53: 2.2, 14: 2.2,
                     **{z: 1.2 for z in mcg_receptor.METALS}}
REFUSAL_WITH_FINISHER = ("interaction_scores, max_interaction_score and rank_by='interaction' cannot be combined with a "
                         "finisher (RDKit's or a custom one): the values go onto the GeneratedMolecule records")
ROTATABLE_BOND = mcg_sub.Pattern((mcg_sub.atom(degree=(2, 8)), mcg_sub.atom(degree=(2, 8))),
                                 (mcg_sub.bond(0, 1, codes=(1,), ring=False),), name="rotatable bond")

_RADIUS_TABLE = torch.tensor([INTERACTION_RADII.get(z, mcg_receptor.VDW_RADII.get(z, mcg_receptor.DEFAULT_RADIUS))
                              for z in range(len(mcg_receptor._SYMBOLS) + 1)], dtype=torch.float32)


def interaction_radius(z: int) -> float:
    """The interaction radius (angstrom) of atomic number `z`: `INTERACTION_RADII`, else `receptor.vdw_radius`."""
    return INTERACTION_RADII.get(int(z), mcg_receptor.vdw_radius(z))


def interaction_radii(atomic_numbers: torch.Tensor) -> torch.Tensor:
    """fp32 interaction radii of a tensor of atomic numbers (same shape, on its device); Z outside 1..118 gets
    `receptor.DEFAULT_RADIUS`."""
    z = torch.as_tensor(atomic_numbers).to(torch.long)
    z = torch.where((z >= 1) & (z < _RADIUS_TABLE.numel()), z, torch.zeros_like(z))
    return _RADIUS_TABLE.to(z.device)[z]


class PreparedReceptor(NamedTuple):
    """A typed receptor as the kernel reads it, on the host (`prepare_receptor`)."""
    xyzr: torch.Tensor            # [R,4] fp32: x, y, z, interaction radius, in `receptor.sort_typed_receptor`'s order
    types: torch.Tensor           # [R] uint8
    spheres: torch.Tensor         # [ceil(R / 256), 4] fp32: `receptor.tile_spheres`


def prepare_receptor(receptor) -> PreparedReceptor:
    """`receptor` - what `receptor.load_typed_receptor` takes, or a `PreparedReceptor`, returned as it is - loaded, typed,
    given its interaction radii and sorted (`receptor.sort_typed_receptor`), with the bounding spheres of its tiles: host
    work, once per receptor."""
    if isinstance(receptor, PreparedReceptor):
        return receptor
    xyz, z, types = mcg_receptor.load_typed_receptor(receptor)
    xyzr, types = mcg_receptor.sort_typed_receptor(xyz, interaction_radii(z), types)
    return PreparedReceptor(xyzr, types, mcg_receptor.tile_spheres(xyzr))


# ----------------------------------------------------------------------------------------------- device
def _posed_graphs(coords, n_nodes, atomic_numbers, bond_orders, what: str):
    """(B, N, z, bonds) of posed, padded molecules with their graphs: `_args.ligand_arguments`, and `bond_orders`
    [B, >= N, >= N]."""
    B, N, z = _args.ligand_arguments(coords, n_nodes, atomic_numbers, MAX_ATOMS, MAX_BATCH, what)
    bonds = torch.as_tensor(bond_orders)
    if bonds.dim() != 3 or bonds.shape[0] != B or bonds.shape[1] != bonds.shape[2] or bonds.shape[1] < N:
        raise ValueError(f"bond_orders must be [B, >= N, >= N] = [{B}, >= {N}, >= {N}], got {list(bonds.shape)}")
    return B, N, z, bonds


@torch.no_grad()
def ligand_types(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                 perceived=None) -> torch.Tensor:
    """Interaction types [B,W] uint8 on the device of B molecular graphs (bits TYPE_DONOR, TYPE_ACCEPTOR,
    TYPE_HYDROPHOBIC; 0 at and beyond a molecule's atoms): `atomic_numbers` [B, >= W], `bond_orders` [B,W,W], `n_nodes`
    [B].  One `pharmacophore.perceive_features` launch (`perceived`: its result for the same graphs, when the caller has
    it) for the donor and acceptor bits, and a few tensor operations behind it for the hydrophobic bit - a C without an N
    or O neighbour, F, Cl, Br, I.  Exact.  ValueError: what `perceive_features` refuses."""
    types = (perceived if perceived is not None else
             mcg_pharm.perceive_features(atomic_numbers, bond_orders, n_nodes, device))[0]
    dev = types.device
    B, W = int(types.shape[0]), int(types.shape[1])
    bonds = torch.as_tensor(bond_orders)
    if bonds.shape[1] == 0:                     # `perceive_features` ran at its smallest width: no atoms anywhere
        return torch.zeros(B, W, dtype=torch.uint8, device=dev)
    z = torch.as_tensor(atomic_numbers)[:, :W].to(dev, torch.long)
    bonds = bonds.to(dev)
    real = torch.arange(W, device=dev).view(1, -1) < torch.as_tensor(n_nodes).to(dev).reshape(-1, 1)
    bonded = (bonds >= 1) & (bonds <= 4) & real[:, :, None] & real[:, None, :] & ~torch.eye(W, dtype=torch.bool, device=dev)
    polar = (z == 7) | (z == 8)
    hydrophobic = (z == 6) & ~(bonded & polar[:, None, :]).any(dim=2)
    for h in mcg_receptor.HALOGENS:
        hydrophobic |= z == h
    out = (types & (TYPE_DONOR | TYPE_ACCEPTOR)) | (hydrophobic.to(torch.uint8) * TYPE_HYDROPHOBIC)
    return torch.where(real, out, torch.zeros_like(out))


@torch.no_grad()
def rotatable_bonds(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                    check: bool = True) -> torch.Tensor:
    """n_rot [B] int32 on the device: the code-1 chain bonds of each graph whose two ends both have heavy-atom degree >= 2
    (THE PACKAGE'S RULE: amide and other conjugated single bonds are counted), by one `substructure.match_substructures`
    call with `ROTATABLE_BOND`; each bond is embedded twice, so the number is count // 2.  ValueError: what that call
    refuses."""
    out = mcg_sub.match_substructures(atomic_numbers, bond_orders, n_nodes, [ROTATABLE_BOND], hydrogens=False,
                                      device=device, check=check)
    return (out["count"][:, 0] // 2).to(torch.int32)


@torch.no_grad()
def score_typed(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, radii: torch.Tensor, types: torch.Tensor,
                n_rot: torch.Tensor, skip_tiles: bool = True, device=None) -> Dict[str, torch.Tensor]:
    """The `mcg_receptor_interactions` launch itself, on ligand atoms that are already typed: `coords` [B,N,3], `n_nodes`
    [B], `radii` [B,N] fp32 interaction radii, `types` [B,N] uint8 type bits, `n_rot` [B] rotatable bonds; `receptor` as
    in `interaction_scores`.  Device tensors: atom_terms [B,N,6], mol_terms [B,8], hbonds [B] as the kernel writes them
    (include/mlconfgen_hip.h).  B or N of 0 launches nothing and returns zeros."""
    prepared = prepare_receptor(receptor)
    dev = _args.resolve_device(device, coords)
    B, N, _ = _args.ligand_arguments(coords, n_nodes, None, MAX_ATOMS, MAX_BATCH, "interaction scores take")
    for name, t, shape in (("radii", radii, (B, N)), ("types", types, (B, N)), ("n_rot", n_rot, (B,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    return _score_typed(prepared, coords, n_nodes, B, N, radii, types, n_rot, skip_tiles, dev)


def _score_typed(prepared, coords, n_nodes, B, N, radii, types, n_rot, skip_tiles, dev) -> Dict[str, torch.Tensor]:
    """`score_typed` behind its checks."""
    atoms = torch.zeros(B, N, 6, device=dev)
    mol = torch.zeros(B, 8, device=dev)
    hbonds = torch.zeros(B, dtype=torch.int32, device=dev)
    if B > 0 and N > 0:
        x = coords.to(dev, torch.float32).contiguous()
        lig_r = radii.to(dev, torch.float32).contiguous()
        lig_t = types.to(dev, torch.uint8).contiguous()
        nn = torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous()
        rot = n_rot.to(dev, torch.int32).contiguous()
        rec, rec_t = prepared.xyzr.to(dev), prepared.types.to(dev)
        spheres = prepared.spheres.to(dev) if skip_tiles else None
        _lib.check(_lib.lib().mcg_receptor_interactions(
            _lib.dptr(x), _lib.dptr(lig_r), _lib.dptr(lig_t), _lib.dptr(nn), _lib.dptr(rot), B, N, _lib.dptr(rec),
            _lib.dptr(rec_t), int(rec.shape[0]), _lib.dptr(spheres), _lib.dptr(atoms), _lib.dptr(mol), _lib.dptr(hbonds),
            _lib.current_stream_ptr(dev)), "mcg_receptor_interactions")
    return dict(atom_terms=atoms, mol_terms=mol, hbonds=hbonds)


@torch.no_grad()
def interaction_scores(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                       bond_orders: torch.Tensor, skip_tiles: bool = True, device=None, check: bool = True
                       ) -> Dict[str, torch.Tensor]:
    """The interaction score of every molecule of the padded, posed coordinates `coords` [B,N,3] (`n_nodes` [B] real
    atoms, `atomic_numbers` [B, >= N], `bond_orders` [B,N,N]) with `receptor` - what `receptor.load_typed_receptor` takes,
    or a `prepare_receptor` result - by this module's definition: one perceive launch (`ligand_types`), one substructure
    launch (`rotatable_bonds`) and one `mcg_receptor_interactions` launch (`score_typed`).  Device tensors:
      score [B]           fp32: E
      terms [B,6]         fp32: G1, G2, REP, HYD, HB and the weighted sum before the n_rot division
      hbonds [B]          int32: `receptor_hbonds`
      atom_scores [B,N]   fp32: each atom's weighted, unnormalised contribution (0 on padded atoms)
      atom_terms [B,N,5]  fp32: each atom's five sums
      n_rot [B]           int32
      types [B,N]         uint8: the ligand types
    A molecule with no atoms: zeros; one with a non-finite coordinate on a real atom: NaN, hbonds = -1; the other rows
    unaffected.  `skip_tiles`: whether a molecule's workgroup walks only the receptor tiles within the cut-off of it; never
    a bit of the result.  Refused before any device work: what `load_typed_receptor` refuses, atom counts outside [0, N],
    N > 64, B > MAX_BATCH, shapes that do not fit."""
    prepared = prepare_receptor(receptor)
    dev = _args.resolve_device(device, coords)
    B, N, z, bonds = _posed_graphs(coords, n_nodes, atomic_numbers, bond_orders, "interaction scores take")
    n_rot = torch.zeros(B, dtype=torch.int32, device=dev)
    types = torch.zeros(B, N, dtype=torch.uint8, device=dev)
    if B > 0 and N > 0:
        bonds = bonds[:, :N, :N]
        types = ligand_types(z[:, :N], bonds, n_nodes, dev)
        n_rot = rotatable_bonds(z[:, :N], bonds, n_nodes, dev, check=check)
    out = _score_typed(prepared, coords, n_nodes, B, N, interaction_radii(z[:, :N].to(dev)), types, n_rot, skip_tiles, dev)
    atoms, mol, hbonds = out["atom_terms"], out["mol_terms"], out["hbonds"]
    return dict(score=mol[:, 6], terms=mol[:, :6], hbonds=hbonds, atom_scores=atoms[:, :, 5], atom_terms=atoms[:, :, :5],
                n_rot=n_rot, types=types)


# ----------------------------------------------------------------------------------------------- optimised pose
OPTIMISE_STEPS = 64             # what `optimise_pose=True` stands for
OPTIMISE_MAX_SHIFT = 2.0        # angstrom the centroid may move from where the walk started
MAX_OPTIMISE_STEPS = mcg_receptor.MAX_RELIEF_STEPS     # csrc/mcg_rigid_step.h WALK_MAX_STEPS
TRACE_WIDTH = 24                # F[3], torque[3], s_r, s_t, G'[9], p'[3], W', evaluated, kept, W of the current pose
OPTIMISE_REFUSAL_WITH_FINISHER = ("optimise_pose cannot be combined with a finisher (RDKit's or a custom one): the "
                                  "values go onto the GeneratedMolecule records")


def check_max_shift(value, name: str = "max_shift") -> float:
    """`max_shift` as a float: a finite real number >= 0 (not a bool), else ValueError."""
    return _args.check_real(name, value, 0.0)


@torch.no_grad()
def optimise_typed(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, radii: torch.Tensor, types: torch.Tensor,
                   steps: int = OPTIMISE_STEPS, max_shift: float = OPTIMISE_MAX_SHIFT, skip_tiles: bool = True,
                   device=None, trace: bool = False) -> Dict[str, torch.Tensor]:
    """The `mcg_receptor_optimise` launch itself, on ligand atoms that are already typed: `coords` [B,N,3], `n_nodes`
    [B], `radii` [B,N] fp32 interaction radii, `types` [B,N] uint8 type bits; `receptor` as in `interaction_scores`.
    Device tensors as the kernel writes them (include/mlconfgen_hip.h): coords [B,N,3], xform [B,12], stats [B,8],
    gradient [B,6] and - `trace` - trace [B,steps,24].  B or N of 0 launches nothing and returns the rows as they came."""
    prepared = prepare_receptor(receptor)
    steps = mcg_receptor.check_relief_steps(steps)
    max_shift = check_max_shift(max_shift)
    dev = _args.resolve_device(device, coords)
    B, N, _ = _args.ligand_arguments(coords, n_nodes, None, MAX_ATOMS, MAX_BATCH, "pose optimisation takes")
    for name, t, shape in (("radii", radii, (B, N)), ("types", types, (B, N))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    return _walk_typed(prepared, coords, n_nodes, B, N, radii, types, steps, max_shift, skip_tiles, dev, trace)


def _walk_typed(prepared, coords, n_nodes, B, N, radii, types, steps, max_shift, skip_tiles, dev, trace, clash=None,
                tree=None) -> Dict[str, torch.Tensor]:
    """The walk's launch behind its checks: `mcg_receptor_optimise`, or - with `clash` [B,N] and `tree`, a `torsion_tree`
    result for the same rows - `mcg_receptor_optimise_flex`.  Device tensors as the kernel writes them
    (include/mlconfgen_hip.h, include/mlconfgen_hip_flex.h): coords, xform, stats, gradient, with a tree angles [B,16], with
    `trace` trace.  B or N of 0 launches nothing and returns the rows as they came."""
    flex = tree is not None
    name = "mcg_receptor_optimise_flex" if flex else "mcg_receptor_optimise"
    x = coords.to(dev, torch.float32).contiguous()
    res = dict(coords=torch.empty_like(x) if B > 0 and N > 0 else x.clone(), xform=torch.zeros(B, 12, device=dev),
               stats=torch.zeros(B, 12 if flex else 8, device=dev))
    if flex:
        res["angles"] = torch.zeros(B, FLEX_MAX_TORSIONS, device=dev)
    res["gradient"] = torch.zeros(B, 6 + FLEX_MAX_TORSIONS if flex else 6, device=dev)
    if trace:
        res["trace"] = torch.zeros(B, steps, FLEX_TRACE_WIDTH if flex else TRACE_WIDTH, device=dev)
    if B > 0 and N > 0:
        lig_r = radii.to(dev, torch.float32).contiguous()
        lig_t = types.to(dev, torch.uint8).contiguous()
        nn = torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous()
        rec, rec_t = prepared.xyzr.to(dev), prepared.types.to(dev)
        spheres = prepared.spheres.to(dev) if skip_tiles else None
        torsions = ()
        if flex:
            torsions = (clash.to(dev, torch.float32).contiguous(), tree["torsion_atoms"], tree["side_mask"],
                        tree["near_mask"], tree["counts"][:, 1].contiguous())
        outs = [res[k] for k in ("coords", "xform", "stats", "angles", "gradient") if k in res] + [res.get("trace")]
        _lib.check(getattr(_lib.lib(), name)(
            _lib.dptr(x), _lib.dptr(lig_r), _lib.dptr(lig_t), _lib.dptr(nn), B, N, _lib.dptr(rec), _lib.dptr(rec_t),
            int(rec.shape[0]), _lib.dptr(spheres), steps, max_shift, *map(_lib.dptr, torsions), *map(_lib.dptr, outs),
            _lib.current_stream_ptr(dev)), name)
    else:
        res["xform"][:, 0] = res["xform"][:, 4] = res["xform"][:, 8] = 1.0
    return res


def _pose_result(coords, xform, stats, gradient, tree=None, angles=None, best=None) -> Dict[str, torch.Tensor]:
    """What `optimise_pose` returns, from a walk's `xform` [B,12] and `stats`; with `tree` and `angles` the torsion and
    clash fields of the flexible walk too; `best` [B]: the winning start of a search, which also counts as a move."""
    ok = torch.isfinite(stats[:, 0])
    count = lambda col: torch.where(ok, stats[:, col], torch.full_like(stats[:, col], -1.0)).to(torch.int32)   # noqa: E731
    moved = stats[:, 3] > 0 if best is None else (stats[:, 3] > 0) | (best > 0)
    res = dict(coords=coords, rotation=xform[:, :9].reshape(len(xform), 3, 3), translation=xform[:, 9:], moved=ok & moved,
               weighted_before=stats[:, 0], weighted_after=stats[:, 1], trials=count(2), kept=count(3), rmsd=stats[:, 4],
               gradient=gradient)
    if tree is not None:
        res.update(torsions=count(8), torsions_found=tree["counts"][:, 0], torsion_angles=angles,
                   torsion_atoms=tree["torsion_atoms"], clash_before=stats[:, 6], clash_after=stats[:, 7],
                   conformer_rmsd=stats[:, 9], step_trans=stats[:, 5])
    return res


@torch.no_grad()
def optimise_pose(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                  bond_orders: torch.Tensor, steps: int = OPTIMISE_STEPS, max_shift: float = OPTIMISE_MAX_SHIFT,
                  device=None, trace: bool = False) -> Dict[str, torch.Tensor]:
    """Every molecule of the padded, posed coordinates `coords` [B,N,3] (`n_nodes` [B] real atoms, `atomic_numbers`
    [B, >= N], `bond_orders` [B,N,N]) moved as a rigid body to where this module's interaction score with `receptor` is
    lower: one perceive launch (`ligand_types`) and one `mcg_receptor_optimise` launch (`optimise_typed`).

    THE PACKAGE'S OWN PROCEDURE ("Optimised pose"): NOT a docking run and NOT AutoDock Vina's local
    optimisation.  Rigid body only: no torsions, no intramolecular term, no hydrogens, no global search
    (`optimise_pose_flexible` is this walk with the rotatable bonds turned and an intramolecular guard).

    Objective       W = -0.0356 G1 - 0.00516 G2 + 0.840 REP - 0.0351 HYD - 0.587 HB, the weighted sum of this module's
                    five terms (`terms[:, 5]` of `interaction_scores`).  E = W / (1 + 0.0585 n_rot) divides by a positive
                    constant of the molecule, so less W is less E and the walk needs no n_rot.
    Force           on atom i: F_i = - sum_j (dW/dd) (x_i - y_j) / r over its counted pairs, direction 0 at r = 0; the
                    branches decided on the same fp32 d as the terms: g1' = -8 d g1; g2' = -((d - 3) / 2) g2; rep' = 2 d
                    where d < 0; hyd' = -1 on 0.5 < d < 1.5 (both hydrophobic); hb' = -1 / 0.7 on -0.7 < d < 0 (donor
                    facing acceptor); 0 elsewhere.
    Pose            x' = (x - c) @ G + p, c the atom centroid summed in atom order; G = I, p = c at the start, and the
                    first evaluation reads the input rows as they came.  Torque about p: sum_i u_i x F_i, u_i = (x_i - c)
                    @ G.
    Walk            from s_r = 0.05 rad, s_t = 0.25 A.  A trial rotates by s_r about the torque (G' = G @ D, then
                    Gram-Schmidt on its rows) and moves p by s_t along the net force; a zero or non-finite vector skips
                    its part, both skipped ends the walk.  |p' - c| > `max_shift`: rejected unevaluated.  Else kept iff
                    W' < W strictly (NaN never is).  Kept: both lengths x 1.2; rejected: x 0.5.  Ends after `steps`
                    trials or once s_t < 2^-8 A.
    Returns device tensors:
      coords [B,N,3]      the kept pose - exactly the coordinates whose W was evaluated and kept (padded rows zero)
      rotation [B,3,3], translation [B,3]   with coords = x @ rotation + translation (`postprocess.compose_pose` applies)
      moved [B] bool      whether a trial was kept; an unmoved molecule returns its input bits, the identity and zero
      weighted_before, weighted_after [B]   W at the input and at `coords`: the bits `interaction_scores` gives there
      trials, kept [B]    int32: trials used and kept
      rmsd [B]            heavy-atom RMSD between input and output
      gradient [B,6]      net force and torque at the input pose
      trace [B,steps,24]  with `trace`: one row per trial (include/mlconfgen_hip.h), for tests
    A molecule without atoms or with a non-finite coordinate on a real atom keeps its rows and gets NaN (trials, kept: -1);
    the others are unaffected.  A molecule's outputs depend on its own atoms and the receptor only.  Refused before any
    device work: what `load_typed_receptor` refuses, `steps` outside 0..1024, `max_shift` negative or not finite, atom
    counts outside [0, N], N > 64, B > MAX_BATCH, shapes that do not fit."""
    prepared = prepare_receptor(receptor)
    steps = mcg_receptor.check_relief_steps(steps)
    max_shift = check_max_shift(max_shift)
    dev = _args.resolve_device(device, coords)
    B, N, z, bonds = _posed_graphs(coords, n_nodes, atomic_numbers, bond_orders, "pose optimisation takes")
    types = torch.zeros(B, N, dtype=torch.uint8, device=dev)
    if B > 0 and N > 0:
        types = ligand_types(z[:, :N], bonds[:, :N, :N], n_nodes, dev)
    out = _walk_typed(prepared, coords, n_nodes, B, N, interaction_radii(z[:, :N].to(dev)), types, steps, max_shift, True,
                      dev, trace)
    res = _pose_result(out["coords"], out["xform"], out["stats"], out["gradient"])
    if trace:
        res["trace"] = out["trace"]
    return res


# ----------------------------------------------------------------------------------------------- flexible pose
FLEX_MAX_TORSIONS = 16          # include/mlconfgen_hip_flex.h MCG_FLEX_MAX_TORSIONS
FLEX_TRACE_WIDTH = 43           # the rigid trace's 24 columns, s_tau, tau[16], C, C'
FLEX_STEP_TAU = 0.1             # rad: what the torsion with the largest |tau| turns by in the first trial
FLEX_MARGIN = 2.0               # angstrom an atom may leave the input's radius about p by
CLASH_PAD = 0.45                # angstrom: half the 0.9 A of `geometry.py`'s non-bonded d0
FLEXIBLE = "flexible"           # the value of `optimise_pose` that asks for this walk

_CLASH_TABLE = torch.tensor([_config.ELEMENTS.get(z, _config.ELEMENTS[6])[1] + CLASH_PAD
                             for z in range(len(mcg_receptor._SYMBOLS) + 1)], dtype=torch.float32)


def clash_radii(atomic_numbers: torch.Tensor) -> torch.Tensor:
    """fp32 c_i of the intramolecular guard for a tensor of atomic numbers (same shape, on its device): the covalent
    radius `rcov` of `config.ELEMENTS` + 0.45 A; an element without a row there gets carbon's."""
    z = torch.as_tensor(atomic_numbers).to(torch.long)
    z = torch.where((z >= 1) & (z < _CLASH_TABLE.numel()), z, torch.full_like(z, 6))
    return _CLASH_TABLE.to(z.device)[z]


@torch.no_grad()
def torsion_tree(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                 check: bool = True) -> Dict[str, torch.Tensor]:
    """The torsion tree of B heavy-atom graphs (`atomic_numbers` [B, >= W], `bond_orders` [B,W,W] symmetric codes
    0 / 1 / 2 / 3 / 4, `n_nodes` [B]; W <= 64) by the rules of `optimise_pose_flexible`, one `mcg_torsion_tree` launch per
    16 384 rows.  Device tensors, exact - the same bits in any batch, at any row and at any padded width:
      torsion_atoms [B,16,2]  int32: per torsion (a, b), b the end inside the moving side; -1 in unused slots
      side_mask [B,16]        int64 holding the unsigned bit pattern: bit i set iff atom i is in the moving side
      near_mask [B,W]         int64 bit patterns: i itself, its bonded neighbours, every atom sharing a neighbour with i
      counts [B,2]            int32: torsions found, torsions used (at most 16)
    A width of 0 is taken as 1.  ValueError before the kernel as `scaffold.ring_perception` raises them."""
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS,
                                           f"the torsion tree takes molecules of at most {MAX_ATOMS} atoms")
    dev = _args.resolve_device(device, bonds)
    if W == 0:
        z, bonds, W = torch.zeros(B, 1, dtype=torch.int32), torch.zeros(B, 1, 1, dtype=torch.int8), 1
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
    if check and B:
        _args.check_graphs(zd, bd, nn, W)
    out = dict(torsion_atoms=torch.full((B, FLEX_MAX_TORSIONS, 2), -1, dtype=torch.int32, device=dev),
               side_mask=torch.zeros(B, FLEX_MAX_TORSIONS, dtype=torch.int64, device=dev),
               near_mask=torch.zeros(B, W, dtype=torch.int64, device=dev),
               counts=torch.zeros(B, 2, dtype=torch.int32, device=dev))
    for lo in range(0, B, MAX_BATCH):
        hi = min(B, lo + MAX_BATCH)
        _lib.check(_lib.lib().mcg_torsion_tree(
            _lib.dptr(zd[lo:hi]), _lib.dptr(bd[lo:hi]), _lib.dptr(nn[lo:hi]), hi - lo, W,
            _lib.dptr(out["torsion_atoms"][lo:hi]), _lib.dptr(out["side_mask"][lo:hi]), _lib.dptr(out["near_mask"][lo:hi]),
            _lib.dptr(out["counts"][lo:hi]), _lib.current_stream_ptr(dev)), "mcg_torsion_tree")
    return out


@torch.no_grad()
def optimise_pose_flexible(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                           bond_orders: torch.Tensor, steps: int = OPTIMISE_STEPS, max_shift: float = OPTIMISE_MAX_SHIFT,
                           device=None, trace: bool = False, skip_tiles: bool = True) -> Dict[str, torch.Tensor]:
    """`optimise_pose` with the molecule's rotatable bonds turned beside the rigid move: one perceive launch
    (`ligand_types`), one `mcg_torsion_tree` launch (`torsion_tree`) and one `mcg_receptor_optimise_flex` launch.

    THE PACKAGE'S OWN PROCEDURE ("Flexible pose"): NOT a docking run, NOT AutoDock Vina's optimiser;
    no hydrogens, no global search (`search_pose` runs this walk from several keyed starts and keeps the best).  It works
    on the returned heavy-atom graph (symmetric codes 0 / 1 / 2 / 3 / 4, at most 64 atoms).

    Torsions        a torsion is a bond `ROTATABLE_BOND` matches - code 1, not a ring bond, both ends of heavy degree >= 2 -
                    unless it joins a nitrogen to a carbon that has a code-2 bond to N, O or S (amide, urea, carbamate;
                    `n_rot` and the score's divisor do not change).  Leaving the bond out splits its connected component
                    in two; the MOVING side is the part with fewer atoms, on a tie the part that holds the bond's
                    higher-indexed end; b is the bond's end inside the moving side, a the other end; atoms of other
                    components never move.  Torsions are taken in ascending (min(a, b), max(a, b)) order; at most 16 are
                    used, the number found is reported and the rest stay frozen.
    Near mask       near[i] = i itself, its bonded neighbours and every atom that shares a bonded neighbour with i.
    Guard           CLASH = sum over real pairs i < j with j not in near[i] of max(0, (c_i + c_j) - r_ij)^2, c = `rcov`
                    (`config.ELEMENTS`) + 0.45 A (`clash_radii`), weighted by the score's own REP weight 0.840, evaluated
                    from the molecule-frame coordinates q: while no torsion turns, its bits do not change.
    State           (q, G, p) from q_i = x_i - c, G = I, p = c; world coordinates x_i = q_i @ G + p, formed as
                    `optimise_pose` forms them.
    Evaluation      the five term sums, the net force F and the torque about p exactly as `optimise_pose` forms them,
                    CLASH, and per torsion k the generalised force tau_k = n_k . sum_{i in side_k} (x_i - x_b) x f_i, n_k
                    the unit vector from a to b, f_i the receptor force on atom i plus its clash force -0.840 dCLASH/dx_i.
                    Positive tau_k: W + 0.840 CLASH falls as the side turns right-handed about n_k.
    Trial           turns the torsions, in ascending k, on a copy of q: torsion k by delta_k = s_tau tau_k / max_j |tau_j|
                    about the line through the copy's q_b along its current axis (a delta of 0 leaves the bits); then
                    rotates by s_r about the torque and moves p by s_t along F, as `optimise_pose` does.  A zero or
                    non-finite vector skips its part; the walk ends when all three parts are skipped.
    Step lengths    from s_r = 0.05 rad, s_t = 0.25 A, s_tau = 0.1 rad; all three x 1.2 after a kept trial, x 0.5 after a
                    rejected one.  Ends after `steps` trials or once s_t < 2^-8 A.
    Unevaluated     a trial with |p' - c| > `max_shift` or any |q'_i| > rho0 + 2 A (rho0 the input's largest |x_i - c|) is
                    rejected unevaluated; the tile list is built once with the reach (rho0 + 2 + 8) + `max_shift`.
    Acceptance      kept iff (W' - W) + 0.840f (C' - C) < 0 in fp32, in that order; NaN is never kept.
    Consequence     a molecule without a torsion walks exactly as `optimise_pose` walks it: the same bits in coords,
                    transform, W before / after, trials, kept, rmsd and gradient.

    Returns what `optimise_pose` returns (`rotation`, `translation`: the rigid part (G, p) alone - it maps the input to
    `coords` only up to `conformer_rmsd`; `gradient` [B,22]: F, torque, tau at the input; `trace` [B,steps,43]) and
      torsions [B]          int32: torsions used (`torsions_found` [B]: found); -1 on a row that got NaN
      torsion_angles [B,16] fp32: the summed kept delta_k, rad
      torsion_atoms [B,16,2] int32: the (a, b) of each slot, -1 where unused
      clash_before, clash_after [B]   CLASH at the input and at `coords`
      conformer_rmsd [B]    RMSD of q at the end against q at the start: the change of the conformer alone
    Rows without atoms or with a non-finite coordinate behave as in `optimise_pose`.  Refused before any device work: what
    `optimise_pose` refuses."""
    prepared = prepare_receptor(receptor)
    steps = mcg_receptor.check_relief_steps(steps)
    max_shift = check_max_shift(max_shift)
    dev = _args.resolve_device(device, coords)
    B, N, z, bonds = _posed_graphs(coords, n_nodes, atomic_numbers, bond_orders, "pose optimisation takes")
    types = torch.zeros(B, N, dtype=torch.uint8, device=dev)
    tree = dict(torsion_atoms=torch.full((B, FLEX_MAX_TORSIONS, 2), -1, dtype=torch.int32, device=dev),
                counts=torch.zeros(B, 2, dtype=torch.int32, device=dev))
    if B > 0 and N > 0:
        types = ligand_types(z[:, :N], bonds[:, :N, :N], n_nodes, dev)
        tree = torsion_tree(z[:, :N], bonds[:, :N, :N], n_nodes, dev, check=False)
    out = _walk_typed(prepared, coords, n_nodes, B, N, interaction_radii(z[:, :N].to(dev)), types, steps, max_shift,
                      skip_tiles, dev, trace, clash_radii(z[:, :N].to(dev)), tree)
    res = _pose_result(out["coords"], out["xform"], out["stats"], out["gradient"], tree, out["angles"])
    if trace:
        res["trace"] = out["trace"]
    return res


# ----------------------------------------------------------------------------------------------- pose search
SEARCH = "search"               # the value of `optimise_pose` that asks for this stage
SEARCH_STARTS = 8               # what `optimise_pose="search"` stands for
SEARCH_MAX_STARTS = 64          # include/mlconfgen_hip_search.h MCG_SEARCH_MAX_STARTS
SEARCH_PARAMS = 24              # include/mlconfgen_hip_search.h MCG_SEARCH_PARAMS
SEARCH_SPREAD = 2.0             # angstrom: the largest shift of a start's centroid
SEARCH_MAX_TURN = math.pi       # rad: the largest rigid turn of a start
SEARCH_COUNTER_WORD = 0xFFFFFFFE    # c3 of a start's Philox counter: no noise counter ((run << 8) | block, block 0..2)
#                                     and not the size draw (0xFFFFFFFF) reaches it


def check_starts(value, name: str = "starts") -> int:
    """`starts` as an int in 1..64 (not a bool), else ValueError."""
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= SEARCH_MAX_STARTS:
        raise ValueError(f"{name} must be an integer in 1..{SEARCH_MAX_STARTS}, got {value!r}")
    return int(value)


def _check_search_options(starts, spread, max_turn, seed):
    """(`starts`, `spread`, `max_turn`, `seed`) as `search_pose` takes them, else ValueError."""
    from . import seeding
    starts = check_starts(starts)
    spread = _args.check_real("spread", spread, 0.0)
    max_turn = _args.check_real("max_turn", max_turn, 0.0)
    if max_turn > math.pi:
        raise ValueError(f"max_turn must lie in [0, pi], got {max_turn!r}")
    return starts, spread, max_turn, seeding.check_seed(seed)


def _repeat_tree(tree: Dict[str, torch.Tensor], idx: torch.Tensor) -> Dict[str, torch.Tensor]:
    return {k: tree[k].index_select(0, idx).contiguous() for k in ("torsion_atoms", "side_mask", "near_mask", "counts")}


@torch.no_grad()
def pose_starts(coords: torch.Tensor, n_nodes: torch.Tensor, tree: Dict[str, torch.Tensor], sample_ids: torch.Tensor,
                seed: int = 0, starts: int = SEARCH_STARTS, spread: float = SEARCH_SPREAD,
                max_turn: float = SEARCH_MAX_TURN, device=None, params: bool = False) -> Dict[str, torch.Tensor]:
    """The `mcg_pose_starts` launch itself (include/mlconfgen_hip_search.h): `starts` keyed starts of every row of `coords`
    [B,N,3] (`n_nodes` [B], `tree` a `torsion_tree` result for the same rows, `sample_ids` [B] int64 in [0, 2^32)).  Device
    tensors as the kernel writes them: coords [B,S,N,3], xform [B,S,12], angles [B,S,16] and - `params` - params [B,S,24].
    Start 0 is the input's bits.  The checks are `search_pose`'s; B >= 1, N >= 1."""
    from . import seeding
    starts, spread, max_turn, seed = _check_search_options(starts, spread, max_turn, seed)
    dev = _args.resolve_device(device, coords)
    B, N, _ = _args.ligand_arguments(coords, n_nodes, None, MAX_ATOMS, MAX_BATCH, "the pose search takes")
    ids = seeding.check_sample_ids(sample_ids, B).to(dev, torch.int64).contiguous()
    x = coords.to(dev, torch.float32).contiguous()
    nn = torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous()
    out = dict(coords=torch.zeros(B, starts, N, 3, device=dev), xform=torch.zeros(B, starts, 12, device=dev),
               angles=torch.zeros(B, starts, FLEX_MAX_TORSIONS, device=dev))
    if params:
        out["params"] = torch.zeros(B, starts, SEARCH_PARAMS, device=dev)
    used = tree["counts"][:, 1].contiguous()
    _lib.check(_lib.lib().mcg_pose_starts(
        _lib.dptr(x), _lib.dptr(nn), B, N, _lib.dptr(tree["torsion_atoms"]), _lib.dptr(tree["side_mask"]), _lib.dptr(used),
        _lib.dptr(ids), seed, starts, spread, max_turn, _lib.dptr(out["coords"]), _lib.dptr(out["xform"]),
        _lib.dptr(out["angles"]), _lib.dptr(out.get("params")), _lib.current_stream_ptr(dev)), "mcg_pose_starts")
    return out


@torch.no_grad()
def select_starts(walk_coords: torch.Tensor, walk_xform: torch.Tensor, walk_stats: torch.Tensor, walk_angles: torch.Tensor,
                  start_xform: torch.Tensor, start_angles: torch.Tensor, coords: torch.Tensor, n_nodes: torch.Tensor,
                  device=None) -> Dict[str, torch.Tensor]:
    """The `mcg_pose_search_select` launch itself (include/mlconfgen_hip_search.h) on the walk's rows [B,S,...] of the starts
    of `coords` [B,N,3].  Device tensors as the kernel writes them: coords [B,N,3], xform [B,12], stats [B,12], angles
    [B,16], best_start [B] int32, start_scores [B,S]."""
    dev = _args.resolve_device(device, coords)
    B, S, N = int(walk_coords.shape[0]), int(walk_coords.shape[1]), int(walk_coords.shape[2])
    for name, t, shape in (("walk_coords", walk_coords, (B, S, N, 3)), ("walk_xform", walk_xform, (B, S, 12)),
                           ("walk_stats", walk_stats, (B, S, 12)), ("walk_angles", walk_angles, (B, S, FLEX_MAX_TORSIONS)),
                           ("start_xform", start_xform, (B, S, 12)), ("start_angles", start_angles, (B, S, FLEX_MAX_TORSIONS)),
                           ("coords", coords, (B, N, 3))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    f32 = lambda t: t.to(dev, torch.float32).contiguous()                                  # noqa: E731
    nn = torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous()
    out = dict(coords=torch.zeros(B, N, 3, device=dev), xform=torch.zeros(B, 12, device=dev),
               stats=torch.zeros(B, 12, device=dev), angles=torch.zeros(B, FLEX_MAX_TORSIONS, device=dev),
               best_start=torch.zeros(B, dtype=torch.int32, device=dev), start_scores=torch.zeros(B, S, device=dev))
    _lib.check(_lib.lib().mcg_pose_search_select(
        _lib.dptr(f32(walk_coords)), _lib.dptr(f32(walk_xform)), _lib.dptr(f32(walk_stats)), _lib.dptr(f32(walk_angles)),
        _lib.dptr(f32(start_xform)), _lib.dptr(f32(start_angles)), _lib.dptr(f32(coords)), _lib.dptr(nn), B, N, S,
        _lib.dptr(out["coords"]), _lib.dptr(out["xform"]), _lib.dptr(out["stats"]), _lib.dptr(out["angles"]),
        _lib.dptr(out["best_start"]), _lib.dptr(out["start_scores"]), _lib.current_stream_ptr(dev)),
        "mcg_pose_search_select")
    return out


@torch.no_grad()
def search_pose(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                bond_orders: torch.Tensor, starts: int = SEARCH_STARTS, steps: int = OPTIMISE_STEPS,
                max_shift: float = OPTIMISE_MAX_SHIFT, spread: float = SEARCH_SPREAD, max_turn: float = SEARCH_MAX_TURN,
                seed: int = 0, sample_ids: Optional[torch.Tensor] = None, device=None, skip_tiles: bool = True
                ) -> Dict[str, torch.Tensor]:
    """`optimise_pose_flexible` from `starts` keyed starts per molecule, the best result kept: one perceive launch
    (`ligand_types`), one `mcg_torsion_tree` launch, one `mcg_pose_starts` launch, the flexible walk
    (`mcg_receptor_optimise_flex`, untouched) over the B x `starts` start rows in chunks of at most 16 384, and one
    `mcg_pose_search_select` launch.

    THE PACKAGE'S OWN, LABELLED PROCEDURE ("Pose search"): a bounded multi-start of the package's own
    downhill walk.  NOT a docking run and NOT AutoDock Vina's Monte Carlo search: no Metropolis chain, no random restarts
    beyond the `starts` asked for, no hydrogens.  The defaults (8 starts, 2 A, any turn, any torsion angle) are stated
    choices, not tuned on any complex; no agreement with any docking program is claimed.

    Starts          start 0 is the input as it came.  Start s >= 1 of the molecule with sample id i: Philox4x32-10 with the
                    key of the keyed sampler noise (`seed` & 0xffffffff, `seed` >> 32) and the counter (i, s, j,
                    0xfffffffe), j = 0..5; a word w gives the uniform u = (w >> 8) 2^-24.  c the atom centroid, q = x - c.
                    j = 0: a rotation axis uniform on the sphere (z = 2 u0 - 1, phi = 2 pi u1) and the angle
                    `max_turn` u2.  j = 1: a shift d, its direction drawn like the axis, its length `spread` cbrt(u2):
                    uniform in the ball.  j = 2..5: one angle theta_k = 2 pi u - pi per torsion slot k = 0..15.  The
                    torsions the walk would use are turned in ascending k on q, each by theta_k about its current axis
                    through q_b (the walk's own turn); then x_s = q' @ R_s + (c + d), R_s the walk's trial rotation.
    Walk            every start is walked by `optimise_pose_flexible`'s kernel with `steps` trials and `max_shift` about the
                    START's own centroid: the returned centroid lies within `spread` + `max_shift` of the input's.
    Choice          J_s = W_after + 0.840f CLASH_after in fp32, the product and the sum each rounded once - the walk's own
                    acceptance quantity.  The smallest finite J wins; NaN never wins; a tie goes to the lowest s.  So the
                    result's J is never above that of `optimise_pose_flexible` alone (start 0), and with `starts` = 1 every
                    tensor is that function's, bit for bit.
    Reproducible    a molecule's starts depend on (`seed`, its sample id, s) and its own data only: the same bits in any
                    batch, at any row, at any padded width and on any number of GPUs.  `sample_ids` defaults to 0..B-1.

    Returns what `optimise_pose_flexible` returns (no trace) - `rotation`, `translation`: the start's rigid part followed by
    the walk's (R_s @ G_w, t_s @ G_w + t_w); `torsion_angles`: theta + the walk's summed turns; `weighted_before`,
    `clash_before`, `gradient`: the input's (start 0's); `weighted_after`, `clash_after`, `trials`, `kept`, `torsions`,
    `step_trans`: the winner's; `rmsd`, `conformer_rmsd`: the input against `coords`; `moved`: a trial was kept or a start
    >= 1 won - and
      best_start [B]        int32: the winning start; -1 where no start has a finite J (the row is start 0's)
      start_scores [B,S]    fp32: every J_s
      starts                dict of the per-start device tensors: coords [B,S,N,3], xform [B,S,12], angles [B,S,16] as
                            `mcg_pose_starts` wrote them and walk_coords, walk_xform, walk_stats, walk_angles as the walk
                            returned them for those rows
    Rows without atoms or with a non-finite coordinate behave as in `optimise_pose`.  Refused before any device work: what
    `optimise_pose_flexible` refuses, `starts` outside 1..64, `spread` negative or not finite, `max_turn` outside [0, pi],
    a `seed` outside [0, 2^64), sample ids outside [0, 2^32) or not [B]."""
    from . import seeding
    prepared = prepare_receptor(receptor)
    steps = mcg_receptor.check_relief_steps(steps)
    max_shift = check_max_shift(max_shift)
    starts, spread, max_turn, seed = _check_search_options(starts, spread, max_turn, seed)
    dev = _args.resolve_device(device, coords)
    B, N, z, bonds = _posed_graphs(coords, n_nodes, atomic_numbers, bond_orders, "pose optimisation takes")
    ids = seeding.check_sample_ids(torch.arange(B) if sample_ids is None else sample_ids, B)
    if B == 0 or N == 0:
        res = optimise_pose_flexible(prepared, coords, n_nodes, atomic_numbers, bond_orders, steps, max_shift, dev,
                                     skip_tiles=skip_tiles)
        return dict(res, best_start=torch.zeros(B, dtype=torch.int32, device=dev),
                    start_scores=torch.zeros(B, starts, device=dev), starts={})
    S = starts
    types = ligand_types(z[:, :N], bonds[:, :N, :N], n_nodes, dev)
    tree = torsion_tree(z[:, :N], bonds[:, :N, :N], n_nodes, dev, check=False)
    radii, clash = interaction_radii(z[:, :N].to(dev)), clash_radii(z[:, :N].to(dev))
    nn = torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B)
    st = pose_starts(coords, nn, tree, ids, seed, S, spread, max_turn, dev)
    # the walk, on the B * S start rows: the rows' own data replicated by an index, at most 16 384 rows a launch
    idx = torch.arange(B, device=dev).repeat_interleave(S)
    rows = st["coords"].reshape(B * S, N, 3)
    parts = []
    for lo in range(0, B * S, MAX_BATCH):
        hi = min(B * S, lo + MAX_BATCH)
        pick = idx[lo:hi]
        parts.append(_walk_typed(prepared, rows[lo:hi], nn.index_select(0, pick), hi - lo, N, radii.index_select(0, pick),
                                 types.index_select(0, pick), steps, max_shift, skip_tiles, dev, False,
                                 clash.index_select(0, pick), _repeat_tree(tree, pick)))
    walk = {k: torch.cat([p[k] for p in parts], dim=0) for k in ("coords", "xform", "stats", "angles", "gradient")}
    shaped = lambda k: walk[k].reshape(B, S, *walk[k].shape[1:])                           # noqa: E731
    out = select_starts(shaped("coords"), shaped("xform"), shaped("stats"), shaped("angles"), st["xform"], st["angles"],
                        coords, nn, dev)
    res = _pose_result(out["coords"], out["xform"], out["stats"], shaped("gradient")[:, 0].contiguous(), tree, out["angles"],
                       out["best_start"])
    return dict(res, best_start=out["best_start"], start_scores=out["start_scores"],
                starts=dict(coords=st["coords"], xform=st["xform"], angles=st["angles"], walk_coords=shaped("coords"),
                            walk_xform=shaped("xform"), walk_stats=shaped("stats"), walk_angles=shaped("angles")))


# ----------------------------------------------------------------------------------------------- options
check_threshold = _args.check_real             # (name, value): `max_interaction_score`, a finite real number
check_rank_by = _args.check_rank_by


def select_score(interaction: Optional[float]) -> float:
    """The ranking value of `rank_by="interaction"`: -E, so that the best - most negative - score ranks first; NaN where
    the score is NaN or missing (such a molecule ranks last)."""
    if interaction is None:
        return math.nan
    return -interaction
