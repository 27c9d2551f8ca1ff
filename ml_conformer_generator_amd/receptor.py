"""Steric contacts of posed molecules with a receptor, on the GPU ("Receptor clashes").

Only heavy atoms count, on both sides.  For ligand atom i (posed coordinates x_i, van der Waals radius r_i) and receptor
atom j (y_j, r_j) the overlap is (r_i + r_j) - |x_i - y_j|, in fp32 in that order; an atom's overlap is its largest over
all receptor atoms, and it clashes when that is >= CLASH_OVERLAP (UCSF ChimeraX's default clash criterion; no H-bond
allowance: no donors or acceptors are typed).  Per molecule: `receptor_clashes` = the number of clashing atoms,
`receptor_max_overlap` = the largest atom overlap in angstrom (negative when nothing touches).

The radii are one table keyed by atomic number (`VDW_RADII`): Bondi (1964) where Bondi gives a value, Mantina et al.
(2009) for boron, DEFAULT_RADIUS for every other element.  The kernel (`mcg_receptor_overlap`) sees radii only.

Clash relief (`relieve_clashes`, kernel `mcg_receptor_relieve`; DESIGN.md section 6, "Clash relief").  The package's own,
labelled procedure: NOT a docking score and NOT a force field - no attraction term, no trade of shape against fit.  It
walks a posed molecule, as a rigid body, to the nearest clash-free pose it finds and stops there; a molecule for which it
finds none ends with a lower penalty and is reported as it is.  Heavy atoms only, radii `VDW_RADII`.
  Contact depth   h_ij = max(0, (r_i + r_j - RELIEF_MARGIN) - |x_i - y_j|), RELIEF_MARGIN = 0.4 A: 0.2 A under
                  CLASH_OVERLAP, so a pose with P = 0 has no clashing atom by the criterion above, with 0.2 A to spare.
  Penalty         P = sum_ij h_ij^2.
  Force, torque   F_i = sum_j 2 h_ij (x_i - y_j) / |x_i - y_j| (the direction is 0 where the distance is 0), F = sum_i F_i,
                  tau = sum_i (x_i - p) x F_i about the ligand's current atom centroid p.
  Motion          x' = (x - c) @ G + p: c the input pose's atom centroid, G a proper rotation applied to row vectors;
                  the start is G = I, p = c.
  Step rule       the refined pose's rule (`shape_overlay(refine_steps=...)`) turned downhill.  A trial rotates by s_r
                  about tau / |tau| and translates by s_t along F / |F|; it is kept only if P strictly decreases, then s_r
                  and s_t are multiplied by 1.2, otherwise by 0.5.  A trial whose centroid would lie more than `max_shift`
                  (default 2.0 A) from c is rejected the same way.  The walk starts from s_r = 0.05 rad, s_t = 0.25 A,
                  takes `steps` trials and stops early only when P == 0 (force and torque are then exactly zero).
  Finish          G is re-orthonormalised (Gram-Schmidt, rows, third = first x second) as each trial is formed, so the
                  pose whose P was evaluated is, bit for bit, the pose returned and there is nothing left to do at the
                  end.  A molecule no trial of which was kept - one whose start has P == 0 included - is returned bit for
                  bit: its coordinates, rotation = I, translation = 0.  A molecule with no atoms or a non-finite
                  coordinate is left exactly as it came, with NaN transform and stats; the other rows are unaffected.
A molecule's result depends on its own atoms and the receptor's atoms only: the same bits in any batch, at any row, at any
padded width, with and without tile skipping, and whatever the order the receptor's atoms were listed in.

Interaction types (`load_typed_receptor`, `sort_typed_receptor`; DESIGN.md section 6, "Receptor interactions").  The clash
criterion and the relief above type no donors or acceptors and read `load_receptor` as before; the interaction score of
`interactions.py` reads one more byte per receptor atom - donor, acceptor, hydrophobic - from a residue-template table over
a PDB string's names, from the elements alone, or as given.
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Tuple

import torch

from . import _args, _lib

CLASH_OVERLAP = 0.6            # angstrom: UCSF ChimeraX `clashes` default overlap cutoff
SELF_CONTACT = 0.5             # angstrom: a receptor atom this close to a reference atom means the ligand is in it
MAX_RECEPTOR_ATOMS = 1 << 17   # include/mlconfgen_hip.h MCG_RECEPTOR_MAX_ATOMS (heavy atoms)
MAX_BATCH = 16384              # MCG_RECEPTOR_MAX_B
MAX_LIGAND_ATOMS = 64          # the kernel's N limit (the shape kernels' MAX_ATOMS)
_MAX_SPLITS = 256              # MCG_RECEPTOR_MAX_SPLITS
_TILE = 256                    # receptor atoms per LDS tile of the kernel
_TARGET_WORKGROUPS = 1024      # four 256-lane workgroups per CU of the MI355X
DEFAULT_RADIUS = 2.00
RELIEF_MARGIN = 0.4            # angstrom: a contact starts 0.2 A under CLASH_OVERLAP
RELIEF_STEPS = 32              # what `relieve_clashes=True` stands for
MAX_RELIEF_STEPS = 1024        # csrc/mcg_receptor_relief.hip RL_MAX_STEPS
RELIEF_MAX_SHIFT = 2.0         # angstrom: how far the walk may carry a molecule's centroid
_SORT_CELL = 4.0               # angstrom: edge of the cells the receptor is sorted by, so that a tile is compact

# Z -> van der Waals radius (angstrom).  A. Bondi, J. Phys. Chem. 68, 441 (1964), Table I, for every element it lists;
# boron (the one element of config.ELEMENTS Bondi lacks): M. Mantina et al., J. Phys. Chem. A 113, 5806 (2009).
VDW_RADII = {
    1: 1.20, 2: 1.40, 3: 1.82, 5: 1.92, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 10: 1.54, 11: 2.27, 12: 1.73, 14: 2.10,
    15: 1.80, 16: 1.80, 17: 1.75, 18: 1.88, 19: 2.75, 28: 1.63, 29: 1.40, 30: 1.39, 31: 1.87, 33: 1.85, 34: 1.90,
    35: 1.85, 36: 2.02, 46: 1.63, 47: 1.72, 48: 1.58, 49: 1.93, 50: 2.17, 52: 2.06, 53: 1.98, 54: 2.16, 78: 1.72,
    79: 1.66, 80: 1.55, 81: 1.96, 82: 2.02, 92: 1.86,
}

_SYMBOLS = ("H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y "
            "Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re "
            "Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg "
            "Cn Nh Fl Mc Lv Ts Og").split()
_Z_OF = {s.upper(): z for z, s in enumerate(_SYMBOLS, 1)}
_Z_OF["D"] = 1                 # deuterium: a hydrogen
_RADIUS_TABLE = torch.tensor([VDW_RADII.get(z, DEFAULT_RADIUS) for z in range(len(_SYMBOLS) + 1)], dtype=torch.float32)


def vdw_radius(z: int) -> float:
    """The van der Waals radius (angstrom) of atomic number `z`: `VDW_RADII`, else DEFAULT_RADIUS."""
    return VDW_RADII.get(int(z), DEFAULT_RADIUS)


def vdw_radii(atomic_numbers: torch.Tensor) -> torch.Tensor:
    """fp32 radii of a tensor of atomic numbers (same shape, on its device); Z outside 1..118 gets DEFAULT_RADIUS."""
    z = torch.as_tensor(atomic_numbers).to(torch.long)
    z = torch.where((z >= 1) & (z <= len(_SYMBOLS)), z, torch.zeros_like(z))
    return _RADIUS_TABLE.to(z.device)[z]


# ----------------------------------------------------------------------------------------------- loading
def _pdb_element(line: str) -> str:
    """The element symbol (upper case) of an ATOM / HETATM line: columns 77-78, else from the atom name (columns 13-16)
    by the PDB convention - a one-letter element sits in column 14, a two-letter one starts in column 13, and a
    four-character name starting with H or D is a hydrogen."""
    el = line[76:78].strip()
    if el:
        return el.upper()
    name = line[12:16].ljust(4)
    if name[0] in "HD" and name.strip() == name and name.isalnum():
        return name[0]
    if name[0] == " " or name[0].isdigit():
        rest = [c for c in name[1:] if c.isalpha()]
        return rest[0].upper() if rest else ""
    two = name[:2].upper()
    return two if two.isalpha() and two in _Z_OF else name[0].upper()


def parse_pdb(text: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(coords [R,3] fp32, atomic numbers [R] int64) of the heavy atoms of a PDB-format string: the ATOM / HETATM
    records of the first model (reading stops at the first ENDMDL), alternate location blank or A, hydrogens and
    deuteriums skipped.  A record whose coordinates or element cannot be read is a ValueError."""
    xyz, zs = [], []
    for k, line in enumerate(text.splitlines(), 1):
        rec = line[:6].rstrip()
        if rec == "ENDMDL":
            break
        if rec not in ("ATOM", "HETATM") or line[16:17] not in ("", " ", "A"):
            continue
        sym = _pdb_element(line)
        z = _Z_OF.get(sym)
        if z is None:
            raise ValueError(f"receptor PDB line {k}: unreadable element {sym!r}: {line!r}")
        if z == 1:
            continue
        try:
            xyz.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
        except ValueError:
            raise ValueError(f"receptor PDB line {k}: unreadable coordinates: {line!r}") from None
        zs.append(z)
    return torch.tensor(xyz, dtype=torch.float32).reshape(-1, 3), torch.tensor(zs, dtype=torch.long)


def load_receptor(receptor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(coords [R,3] fp32, atomic numbers [R] int64) on the host: the heavy atoms of `receptor`, which is an RDKit Mol
    (or anything with `GetConformer().GetPositions()` and `GetAtoms()`), a PDB-format string (`parse_pdb`), or a
    `(coords [R,3], atomic_numbers [R])` pair (hydrogens, Z = 1, are dropped).  Refused with ValueError: no heavy atoms,
    more than MAX_RECEPTOR_ATOMS, a non-finite coordinate, an unreadable record."""
    if isinstance(receptor, str):
        coords, z = parse_pdb(receptor)
    elif hasattr(receptor, "GetConformer") and hasattr(receptor, "GetAtoms"):
        import numpy as np
        pos = torch.as_tensor(np.asarray(receptor.GetConformer().GetPositions(), dtype=np.float64)).reshape(-1, 3)
        z = torch.tensor([a.GetAtomicNum() for a in receptor.GetAtoms()], dtype=torch.long)
        if z.numel() != pos.shape[0]:
            raise ValueError(f"receptor Mol: {z.numel()} atoms but {pos.shape[0]} conformer positions")
        coords, z = pos[z != 1].to(torch.float32), z[z != 1]
    elif isinstance(receptor, (tuple, list)) and len(receptor) == 2:
        try:
            coords = torch.as_tensor(receptor[0], dtype=torch.float32).cpu().reshape(-1, 3)
            z = torch.as_tensor(receptor[1]).cpu().reshape(-1)
        except (TypeError, RuntimeError, ValueError) as e:
            raise ValueError(f"receptor (coords, atomic_numbers): unreadable: {e}") from None
        if z.dtype.is_floating_point or z.dtype == torch.bool or z.numel() != coords.shape[0]:
            raise ValueError("receptor (coords [R,3], atomic_numbers [R]): R integer atomic numbers are needed, got "
                             f"{z.numel()} of type {z.dtype} for {coords.shape[0]} coordinates")
        z = z.to(torch.long)
        if z.numel() and int(z.min()) < 1:
            raise ValueError(f"receptor atomic numbers must be >= 1, got {int(z.min())}")
        coords, z = coords[z != 1], z[z != 1]
    else:
        raise ValueError("receptor must be an RDKit Mol, a PDB-format string or a (coords, atomic_numbers) pair, got "
                         f"{type(receptor).__name__}")
    R = int(z.numel())
    if R == 0:
        raise ValueError("the receptor has no heavy atoms")
    if R > MAX_RECEPTOR_ATOMS:
        raise ValueError(f"the receptor has {R} heavy atoms; at most {MAX_RECEPTOR_ATOMS} are supported")
    if not bool(torch.isfinite(coords).all()):
        raise ValueError("the receptor has a non-finite coordinate")
    return coords.contiguous(), z.contiguous()


# ----------------------------------------------------------------------------------------------- typed loading
# Interaction types of a receptor heavy atom ("Receptor interactions"; `interactions.py` reads them):
# one byte of bits, the package's own typing - no hydrogens, no protonation states.
TYPE_DONOR, TYPE_ACCEPTOR, TYPE_HYDROPHOBIC = 1, 2, 4
TYPE_MAX = TYPE_DONOR | TYPE_ACCEPTOR | TYPE_HYDROPHOBIC
METALS = (12, 20, 25, 26, 27, 28, 29, 30)      # Mg Ca Mn Fe Co Ni Cu Zn: typed as donors
HALOGENS = (9, 17, 35, 53)
POLAR_CARBON_DISTANCE = 1.75   # angstrom: a carbon with a receptor N or O this close is bonded to it - not hydrophobic
_AMINO_ACIDS = frozenset("ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split())
_WATERS = frozenset(("HOH", "WAT", "H2O", "DOD"))
# (residue, atom) -> type of the side-chain N and O atoms of the standard residues
_SIDE_CHAIN = {("ARG", "NE"): 1, ("ARG", "NH1"): 1, ("ARG", "NH2"): 1, ("ASN", "ND2"): 1, ("GLN", "NE2"): 1,
               ("LYS", "NZ"): 1, ("TRP", "NE1"): 1, ("HIS", "ND1"): 3, ("HIS", "NE2"): 3, ("SER", "OG"): 3,
               ("THR", "OG1"): 3, ("TYR", "OH"): 3, ("ASP", "OD1"): 2, ("ASP", "OD2"): 2, ("GLU", "OE1"): 2,
               ("GLU", "OE2"): 2, ("ASN", "OD1"): 2, ("GLN", "OE1"): 2}


def template_type(residue: str, atom: str, z: int) -> Optional[int]:
    """The donor / acceptor bits of an N or O atom named `atom` in a residue named `residue` by the residue-template
    table: the backbone N (a donor, except in PRO), O and OXT (acceptors) and the side-chain atoms of `_SIDE_CHAIN` of the
    twenty standard residues, and a water's O (both).  None: the table does not know the atom."""
    if residue in _WATERS:
        return (TYPE_DONOR | TYPE_ACCEPTOR) if z == 8 else None
    if residue not in _AMINO_ACIDS:
        return None
    if atom == "N" and z == 7:
        return 0 if residue == "PRO" else TYPE_DONOR
    if atom in ("O", "OXT") and z == 8:
        return TYPE_ACCEPTOR
    return _SIDE_CHAIN.get((residue, atom))


def parse_pdb_names(text: str):
    """[(residue name, atom name)] of exactly the records `parse_pdb` keeps, in its order."""
    names = []
    for line in text.splitlines():
        rec = line[:6].rstrip()
        if rec == "ENDMDL":
            break
        if rec not in ("ATOM", "HETATM") or line[16:17] not in ("", " ", "A"):
            continue
        if _Z_OF.get(_pdb_element(line)) == 1:
            continue
        names.append((line[17:20].strip().upper(), line[12:16].strip().upper()))
    return names


def parse_pdb_groups(text: str):
    """(ids [R] int32, labels list[str]) of exactly the records `parse_pdb` keeps, in its order: the residue each heavy
    atom belongs to - (chain id column 22, resSeq columns 23-26, iCode column 27, resName columns 18-20) - as a dense id
    numbered by first appearance, and per id the label "{chain}:{resName}{resSeq}{iCode}" (a blank chain is written `_`, a
    blank iCode is omitted).  What `contacts.py` groups a PDB receptor's atoms by."""
    ids, labels, seen = [], [], {}
    for line in text.splitlines():
        rec = line[:6].rstrip()
        if rec == "ENDMDL":
            break
        if rec not in ("ATOM", "HETATM") or line[16:17] not in ("", " ", "A"):
            continue
        if _Z_OF.get(_pdb_element(line)) == 1:
            continue
        key = (line[21:22].strip(), line[22:26].strip(), line[26:27].strip(), line[17:20].strip().upper())
        if key not in seen:
            seen[key] = len(labels)
            labels.append(f"{key[0] or '_'}:{key[3]}{key[1]}{key[2]}")
        ids.append(seen[key])
    return torch.tensor(ids, dtype=torch.int32), labels


def polar_carbons(coords: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """[R] bool: the carbons of (coords [R,3], z [R]) with an N or O of the same set within POLAR_CARBON_DISTANCE,
    decided in fp64 on the host.  A cell sort: the N and O atoms are keyed by their cell (edge POLAR_CARBON_DISTANCE) and
    sorted once, every carbon looks at the 27 cells round its own - never an R x R matrix.  A set too spread out for 2^20
    cells per axis is compared in chunks of at most 2^22 pairs instead."""
    xyz = coords.to(torch.float64).reshape(-1, 3)
    carbon = (z == 6).nonzero().reshape(-1)
    polar = ((z == 7) | (z == 8)).nonzero().reshape(-1)
    out = torch.zeros(xyz.shape[0], dtype=torch.bool)
    if carbon.numel() == 0 or polar.numel() == 0:
        return out
    c, p = xyz[carbon], xyz[polar]
    lim2 = POLAR_CARBON_DISTANCE * POLAR_CARBON_DISTANCE
    lo = xyz.min(dim=0).values
    dims = ((xyz.max(dim=0).values - lo) / POLAR_CARBON_DISTANCE).floor().to(torch.long) + 3
    hit = torch.zeros(c.shape[0], dtype=torch.bool)
    if int(dims.max()) > (1 << 20):
        step = max(1, (1 << 22) // int(p.shape[0]))
        for k in range(0, int(c.shape[0]), step):
            d2 = ((c[k: k + step, None, :] - p[None, :, :]) ** 2).sum(dim=2)
            hit[k: k + step] = (d2 <= lim2).any(dim=1)
    else:
        def key(cell):
            return (cell[:, 0] * dims[1] + cell[:, 1]) * dims[2] + cell[:, 2]
        pc = ((p - lo) / POLAR_CARBON_DISTANCE).floor().to(torch.long) + 1
        order = torch.sort(key(pc), stable=True)
        pkey, p = order.values, p[order.indices]
        cc = ((c - lo) / POLAR_CARBON_DISTANCE).floor().to(torch.long) + 1
        for off in [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]:
            want = key(cc + torch.tensor(off, dtype=torch.long))
            first, last = torch.searchsorted(pkey, want), torch.searchsorted(pkey, want, right=True)
            for k in range(int((last - first).max())):           # the k-th N or O of that cell, where it has one
                rows = (first + k < last).nonzero().reshape(-1)
                d2 = ((c[rows] - p[first[rows] + k]) ** 2).sum(dim=1)
                hit[rows] |= d2 <= lim2
    out[carbon] = hit
    return out


def _element_types(coords: torch.Tensor, z: torch.Tensor, polar: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[R] uint8: the types of atoms without names - N and O donor and acceptor both (`polar` [R]: their bits from a
    template instead), the METALS donors, a carbon hydrophobic unless `polar_carbons`, the HALOGENS hydrophobic, S and
    every other element nothing."""
    types = torch.zeros(z.shape[0], dtype=torch.uint8)
    no = (z == 7) | (z == 8)
    both = torch.full_like(types, TYPE_DONOR | TYPE_ACCEPTOR)
    types = torch.where(no, both if polar is None else polar.to(torch.uint8), types)
    for m in METALS:
        types = torch.where(z == m, torch.full_like(types, TYPE_DONOR), types)
    hydrophobic = ((z == 6) & ~polar_carbons(coords, z))
    for h in HALOGENS:
        hydrophobic |= z == h
    return torch.where(hydrophobic, torch.full_like(types, TYPE_HYDROPHOBIC), types)


def typed_receptor(receptor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """(coords [R,3] fp32, atomic numbers [R] int64, types [R] uint8, untemplated) on the host: `load_receptor`'s heavy
    atoms with their interaction types (bits TYPE_DONOR / TYPE_ACCEPTOR / TYPE_HYDROPHOBIC).
      a PDB-format string: the N and O atoms by `template_type` over (residue name, atom name); an N or O the table does
        not know (a non-standard residue, a HETATM ligand or cofactor) is donor and acceptor both; the METALS are donors;
        a carbon is hydrophobic unless a receptor N or O lies within POLAR_CARBON_DISTANCE (`polar_carbons`); the HALOGENS
        are hydrophobic; S is not an acceptor.  `untemplated`: the N, O and metal atoms typed without a template.
      a (coords, atomic_numbers) pair or an RDKit Mol: there are no names - N and O are both, the rest as above;
        `untemplated` is 0.
      a (coords, atomic_numbers, types) triple: `types` [R] integers in 0..TYPE_MAX are used verbatim (those of the
        hydrogens are dropped with them); ValueError for another shape, a non-integer or a value out of range."""
    if isinstance(receptor, (tuple, list)) and len(receptor) == 3:
        try:
            given = torch.as_tensor(receptor[2]).cpu().reshape(-1)
            raw_z = torch.as_tensor(receptor[1]).cpu().reshape(-1)
        except (TypeError, RuntimeError, ValueError) as e:
            raise ValueError(f"receptor (coords, atomic_numbers, types): unreadable: {e}") from None
        if given.dtype.is_floating_point or given.dtype == torch.bool or given.numel() != raw_z.numel():
            raise ValueError("receptor (coords [R,3], atomic_numbers [R], types [R]): R integer types are needed, got "
                             f"{given.numel()} of type {given.dtype} for {raw_z.numel()} atoms")
        if given.numel() and (int(given.min()) < 0 or int(given.max()) > TYPE_MAX):
            raise ValueError(f"receptor types must be in 0..{TYPE_MAX} (bits 1 donor, 2 acceptor, 4 hydrophobic), got "
                             f"{int(given.min())}..{int(given.max())}")
        coords, z = load_receptor((receptor[0], receptor[1]))
        return coords, z, given[raw_z != 1].to(torch.uint8).contiguous(), 0
    coords, z = load_receptor(receptor)
    if not isinstance(receptor, str):
        return coords, z, _element_types(coords, z), 0
    names = parse_pdb_names(receptor)
    polar = torch.full((z.shape[0],), TYPE_DONOR | TYPE_ACCEPTOR, dtype=torch.uint8)
    untemplated = 0
    metals = set(METALS)
    for k, ((residue, atom), zk) in enumerate(zip(names, z.tolist())):
        if zk in (7, 8):
            t = template_type(residue, atom, zk)
            if t is None:
                untemplated += 1
            else:
                polar[k] = t
        elif zk in metals:
            untemplated += 1
    return coords, z, _element_types(coords, z, polar), untemplated


def load_typed_receptor(receptor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(coords [R,3] fp32, atomic numbers [R] int64, types [R] uint8) on the host: `typed_receptor` of an RDKit Mol, a
    PDB-format string, a (coords, atomic_numbers) pair or a (coords, atomic_numbers, types) triple; one warning where N, O
    or metal atoms of a PDB string were typed without a template.  Refused with ValueError: what `load_receptor` refuses,
    and types of the wrong shape, kind or range."""
    coords, z, types, untemplated = typed_receptor(receptor)
    if untemplated:
        import warnings
        warnings.warn(f"receptor typing: {untemplated} N, O or metal atom(s) are in no residue template (non-standard "
                      "residues, HETATM groups, ions); such an N or O counts as donor and acceptor both, a metal as a donor")
    return coords, z, types


def sort_typed_receptor(rec_xyz: torch.Tensor, rec_radius: torch.Tensor, rec_type: torch.Tensor
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`sort_receptor` with a type byte carried along: ([R,4] fp32 (x, y, z, radius), [R] uint8) on the host, by the same
    Morton-cell sort over the canonical lexicographic order (x, y, z, radius, then the type as the last tie-break).  The
    result does not depend on the order the atoms came in."""
    xyzr = torch.cat([rec_xyz.to(torch.float32).reshape(-1, 3), rec_radius.to(torch.float32).reshape(-1, 1)], dim=1).cpu()
    types = torch.as_tensor(rec_type).to(torch.uint8).reshape(-1).cpu()
    order = torch.sort(types.to(torch.int64), stable=True).indices
    for col in (3, 2, 1, 0):
        order = order[torch.sort(xyzr[order, col], stable=True).indices]
    xyzr, types = xyzr[order], types[order]
    cell = ((xyzr[:, :3] - xyzr[:, :3].min(dim=0).values) / _SORT_CELL).floor().to(torch.long).clamp_(0, 1023)
    key = _spread_bits(cell[:, 0]) | (_spread_bits(cell[:, 1]) << 1) | (_spread_bits(cell[:, 2]) << 2)
    order = torch.sort(key, stable=True).indices
    return xyzr[order].contiguous(), types[order].contiguous()


def sort_grouped_receptor(rec_xyz: torch.Tensor, rec_radius: torch.Tensor, rec_type: torch.Tensor, rec_group: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`sort_typed_receptor` with a group id carried along as well: ([R,4] fp32, [R] uint8, [R] int32) on the host.  The
    group id is the last tie-break of the canonical order, behind the type: atoms that tie on (x, y, z, radius, type) are
    equal in the first two outputs, so these are `sort_typed_receptor`'s, bit for bit, and the result does not depend on the
    order the atoms came in."""
    xyzr = torch.cat([rec_xyz.to(torch.float32).reshape(-1, 3), rec_radius.to(torch.float32).reshape(-1, 1)], dim=1).cpu()
    types = torch.as_tensor(rec_type).to(torch.uint8).reshape(-1).cpu()
    groups = torch.as_tensor(rec_group).to(torch.int32).reshape(-1).cpu()
    order = torch.sort(groups.to(torch.int64), stable=True).indices
    order = order[torch.sort(types[order].to(torch.int64), stable=True).indices]
    for col in (3, 2, 1, 0):
        order = order[torch.sort(xyzr[order, col], stable=True).indices]
    xyzr, types, groups = xyzr[order], types[order], groups[order]
    cell = ((xyzr[:, :3] - xyzr[:, :3].min(dim=0).values) / _SORT_CELL).floor().to(torch.long).clamp_(0, 1023)
    key = _spread_bits(cell[:, 0]) | (_spread_bits(cell[:, 1]) << 1) | (_spread_bits(cell[:, 2]) << 2)
    order = torch.sort(key, stable=True).indices
    return xyzr[order].contiguous(), types[order].contiguous(), groups[order].contiguous()


def check_clear_of_reference(rec_coords: torch.Tensor, ref_coord: torch.Tensor) -> None:
    """ValueError if any reference heavy atom lies within SELF_CONTACT of a receptor heavy atom: the receptor holds
    the reference ligand itself (a whole complex), and every molecule posed onto it would clash."""
    ref = torch.as_tensor(ref_coord, dtype=torch.float64).reshape(-1, 3)
    d = torch.cdist(ref, rec_coords.to(torch.float64), compute_mode="donot_use_mm_for_euclid_dist")
    close = d <= SELF_CONTACT
    if bool(close.any()):
        i, j = (int(v) for v in close.nonzero()[0])
        raise ValueError(f"the receptor contains the reference ligand: reference atom {i} lies {float(d[i, j]):.3f} A "
                         f"from receptor atom {j} (<= {SELF_CONTACT} A); remove the ligand from the receptor")


check_max_receptor_clashes = functools.partial(_args.check_at_least, "max_receptor_clashes", lowest=0)     # -> int


def check_relief_steps(value, name: str = "steps", lowest: int = 0, if_true: Optional[int] = None) -> int:
    """A trial budget of the clash relief as an int in `lowest`..MAX_RELIEF_STEPS (an integer type, not a bool), else a
    ValueError that names `name`.  `if_true`: the budget True stands for, where the option accepts True
    (`relieve_clashes`: RELIEF_STEPS, with `lowest` 1)."""
    return _args.check_steps(name, value, lowest, MAX_RELIEF_STEPS, if_true)


def _spread_bits(v: torch.Tensor) -> torch.Tensor:
    """The low 10 bits of each int64 spread to every third bit (the Morton code's one axis)."""
    v = v & 0x3FF
    v = (v | (v << 16)) & 0x30000FF
    v = (v | (v << 8)) & 0x300F00F
    v = (v | (v << 4)) & 0x30C30C3
    return (v | (v << 2)) & 0x9249249


def sort_receptor(rec_xyz: torch.Tensor, rec_radius: torch.Tensor) -> torch.Tensor:
    """The receptor as the relief kernel reads it: [R,4] fp32 (x, y, z, radius) on the host, sorted so that 256 consecutive
    atoms - one tile - are close in space: by the Morton code of the atom's cell (edge _SORT_CELL, counted from the
    smallest coordinate; cells beyond 1 024 per axis share the last), ties by x, y, z, radius.  One stable sort on the
    cell key over that canonical order, once per receptor; the result does not depend on the order the atoms came in."""
    xyzr = torch.cat([rec_xyz.to(torch.float32).reshape(-1, 3), rec_radius.to(torch.float32).reshape(-1, 1)], dim=1).cpu()
    for col in (3, 2, 1, 0):                                        # the canonical order: lexicographic (x, y, z, radius)
        xyzr = xyzr[torch.sort(xyzr[:, col], stable=True).indices]
    cell = ((xyzr[:, :3] - xyzr[:, :3].min(dim=0).values) / _SORT_CELL).floor().to(torch.long).clamp_(0, 1023)
    key = _spread_bits(cell[:, 0]) | (_spread_bits(cell[:, 1]) << 1) | (_spread_bits(cell[:, 2]) << 2)
    return xyzr[torch.sort(key, stable=True).indices].contiguous()


def tile_spheres(xyzr: torch.Tensor) -> torch.Tensor:
    """[ceil(R / _TILE), 4] fp32: centre (the bounding box's) and radius of each tile of _TILE consecutive atoms of `xyzr`
    [R,4]; the radius reaches the far side of every atom of the tile: max_j |y_j - centre| + r_j, rounded up."""
    R = int(xyzr.shape[0])
    T = -(-R // _TILE)
    pad = torch.cat([xyzr, xyzr[-1:].expand(T * _TILE - R, 4)]).reshape(T, _TILE, 4)      # the last atom again: no effect
    centre = (pad[:, :, :3].amin(dim=1) + pad[:, :, :3].amax(dim=1)) * 0.5
    far = ((pad[:, :, :3] - centre[:, None, :]).double().norm(dim=2) + pad[:, :, 3].double()).amax(dim=1)
    radius = torch.nextafter(far.to(torch.float32), torch.full_like(far, math.inf, dtype=torch.float32))
    return torch.cat([centre, radius[:, None]], dim=1).contiguous()


# ----------------------------------------------------------------------------------------------- device
def default_splits(B: int, N: int, R: int) -> int:
    """Receptor ranges per ligand block: enough workgroups to fill the GPU, at least one tile each."""
    blocks = -(-B * N // _TILE)
    return max(1, min(-(-R // _TILE), -(-_TARGET_WORKGROUPS // blocks), _MAX_SPLITS))


@torch.no_grad()
def receptor_overlap(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor, device=None,
                     splits: Optional[int] = None) -> torch.Tensor:
    """Per-atom overlap [B,N] fp32 on the device: max over the receptor's heavy atoms of (r_i + r_j) - |x_i - y_j| for
    each atom of the padded ligand coordinates `coords` [B,N,3] with `n_nodes` [B] real atoms and `atomic_numbers`
    [B, >= N]; -inf on padded atoms, NaN for an atom with a non-finite coordinate.  `receptor`: what `load_receptor`
    takes.  One `mcg_receptor_overlap` call; `splits` (default `default_splits`) only decides how the receptor is cut
    across workgroups, never a bit of the result.  Refused before any device work: what `load_receptor` refuses, atom
    counts outside [0, N], N > 64, B > MAX_BATCH, atomic numbers narrower than N."""
    rec_xyz, rec_z = load_receptor(receptor)
    dev = _args.resolve_device(device, coords)
    B, N, z = _args.ligand_arguments(coords, n_nodes, atomic_numbers, MAX_LIGAND_ATOMS, MAX_BATCH, "receptor contacts take")
    if B == 0 or N == 0:
        return torch.full((B, N), -math.inf, device=dev)
    R = int(rec_z.numel())
    S = default_splits(B, N, R) if splits is None else int(splits)
    x = coords.to(dev, torch.float32).contiguous()
    lig_r = vdw_radii(z[:, :N].to(dev)).contiguous()
    nn = torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous()
    rec = rec_xyz.to(dev)
    rec_r = vdw_radii(rec_z).to(dev)
    ws = torch.empty(S * B * N if S > 1 else 0, device=dev)
    out = torch.empty(B, N, device=dev)
    _lib.check(_lib.lib().mcg_receptor_overlap(_lib.dptr(x), _lib.dptr(lig_r), _lib.dptr(nn), B, N, _lib.dptr(rec),
                                               _lib.dptr(rec_r), R, S, _lib.dptr(ws) if S > 1 else None,
                                               _lib.dptr(out), _lib.current_stream_ptr(dev)),
               "mcg_receptor_overlap")
    return out


@torch.no_grad()
def relieve_clashes(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                    steps: int = RELIEF_STEPS, max_shift: float = RELIEF_MAX_SHIFT, device=None,
                    return_gradient: bool = False, skip_tiles: bool = True) -> dict:
    """Every molecule of the padded, posed coordinates `coords` [B,N,3] (`n_nodes` [B] real atoms, `atomic_numbers`
    [B, >= N]) moved as a rigid body out of its contacts with `receptor` (what `load_receptor` takes), by the procedure of
    this module's docstring, in one `mcg_receptor_relieve` call.  Returns device tensors:
      coords [B,N,3]        the moved rows (padded rows zero);
      rotation [B,3,3], translation [B,3]   with coords = input @ rotation + translation on the real rows;
      penalty_before [B], penalty_after [B]  P at the input and at the returned pose;
      accepted_steps [B] int32, rmsd [B]     trials kept, and the heavy-atom RMSD between input and output;
      moved [B] bool        P before > 0 and at least one trial kept;
      (return_gradient) gradient [B,6]       net force and torque at the input pose.
    A molecule with no atoms or a non-finite coordinate: NaN rotation, translation, penalties, rmsd and gradient, 0
    accepted steps, its rows as they came.  `skip_tiles`: whether a molecule's workgroup walks only the receptor tiles
    within its reach; never a bit of the result.  Refused before any device work: what `receptor_overlap` refuses, `steps`
    outside 0..MAX_RELIEF_STEPS, a bool or a non-integer, a `max_shift` that is negative or not finite."""
    steps = check_relief_steps(steps)
    max_shift = _args.check_real("max_shift", max_shift, 0.0)
    rec_xyz, rec_z = load_receptor(receptor)
    dev = _args.resolve_device(device, coords)
    B, N, z = _args.ligand_arguments(coords, n_nodes, atomic_numbers, MAX_LIGAND_ATOMS, MAX_BATCH, "clash relief takes")
    x = coords.to(dev, torch.float32).contiguous()
    out = torch.zeros(B, N, 3, device=dev)
    xform = torch.full((B, 12), math.nan, device=dev)
    stats = torch.full((B, 4), math.nan, device=dev)
    grad = torch.full((B, 6), math.nan, device=dev) if return_gradient else None
    if B > 0 and N > 0:
        xyzr = sort_receptor(rec_xyz, vdw_radii(rec_z))
        spheres = tile_spheres(xyzr).to(dev) if skip_tiles else None
        rec = xyzr.to(dev)
        lig_r = vdw_radii(z[:, :N].to(dev)).contiguous()
        nn = torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous()
        _lib.check(_lib.lib().mcg_receptor_relieve(_lib.dptr(x), _lib.dptr(lig_r), _lib.dptr(nn), B, N, _lib.dptr(rec),
                                                   int(xyzr.shape[0]), _lib.dptr(spheres), steps, RELIEF_MARGIN,
                                                   max_shift, _lib.dptr(out), _lib.dptr(xform), _lib.dptr(stats),
                                                   _lib.dptr(grad), _lib.current_stream_ptr(dev)),
                   "mcg_receptor_relieve")
    accepted = torch.nan_to_num(stats[:, 2], nan=0.0).to(torch.int32)
    res = dict(coords=out, rotation=xform[:, :9].reshape(B, 3, 3), translation=xform[:, 9:], penalty_before=stats[:, 0],
               penalty_after=stats[:, 1], accepted_steps=accepted, rmsd=stats[:, 3],
               moved=(stats[:, 0] > 0) & (accepted > 0))
    if return_gradient:
        res["gradient"] = grad
    return res


def clash_summary(overlap: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(receptor_clashes [B] int32, receptor_max_overlap [B] fp32) of a per-atom overlap [B,N] (on its device): the
    atoms with an overlap >= CLASH_OVERLAP, and the largest overlap (-inf for a molecule without atoms, NaN for one
    with a non-finite atom)."""
    B = int(overlap.shape[0])
    if overlap.shape[1] == 0:
        return (torch.zeros(B, dtype=torch.int32, device=overlap.device),
                torch.full((B,), -math.inf, device=overlap.device))
    return (overlap >= CLASH_OVERLAP).sum(dim=1, dtype=torch.int32), overlap.amax(dim=1)
