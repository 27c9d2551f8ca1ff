"""Receptor contacts of posed molecules, on the GPU ("Receptor contacts"): WHICH residues does a posed
molecule touch, with which kind of contact, and does it keep the contacts a reference ligand makes?  `interactions.py` says
how good one empirical number is; a pose walk that lowers it can quietly trade three hydrogen bonds to a hinge for greasy
contact with a lid.  This module keeps the identity of the receptor atoms a molecule touches.

THE PACKAGE'S OWN, LABELLED DEFINITION, in the family of the structural interaction fingerprints (SIFt, PLIF, ProLIF-style
"interaction recovery").  It is NOT the output of ProLIF, PLIP or SIFt: heavy atoms only, no hydrogens and so no angles, the
package's own atom typing.  There are NO ionic, aromatic (pi-stacking, cation-pi) or metal kinds: the type byte
(`receptor.TYPE_*`) has no such bits.

Groups          every receptor heavy atom belongs to a group.  For a PDB string the group is the residue - (chain id column
                22, resSeq columns 23-26, iCode column 27, resName columns 18-20) - read from exactly the records
                `receptor.parse_pdb` keeps, in its order (same altloc rule, hydrogens dropped, stop at ENDMDL); ids are dense
                int32, numbered by first appearance; labels are "{chain}:{resName}{resSeq}{iCode}", a blank chain written
                `_`, a blank iCode omitted (`receptor.parse_pdb_groups`).  For any other receptor form the caller passes
                `groups=`: [R] integers >= 0 aligned with the atoms as given (those of hydrogens are dropped with their
                atoms); the labels are then the integers.
Pair geometry   that of `interactions.py`, bit for bit (one device text, csrc/mcg_interaction_pair.h): r2 = dx*dx + dy*dy +
                dz*dz in fp32, unfused; the pair is looked at iff r2 < 64.0f; d = sqrtf(r2) - (R_i + R_j) on the interaction
                radii (`interactions.INTERACTION_RADII`).
Kinds           a pair sets
                  CONTACT (1)         d <= 0.5f;
                  HYDROPHOBIC (2)     both atoms hydrophobic and d <= 0.5f - where the score's `hyd` term is 1;
                  HBOND_DONOR (4)     the ligand atom a donor, the receptor atom an acceptor, d <= -0.7f - the score's full
                                      hydrogen bond, the ligand donating;
                  HBOND_ACCEPTOR (8)  the ligand atom an acceptor, the receptor atom a donor, d <= -0.7f.
                The ligand's types are `interactions.ligand_types`, the receptor's `receptor.load_typed_receptor`.
Fingerprint     of a molecule: the set of (group, kinds), kinds the OR over all pairs of the molecule's real atoms with the
                group's atoms; given as entries in ascending group id, only groups with kinds != 0, at most MAX_GROUPS = 256
                of them.  Per ligand atom also the OR of the kinds it takes part in ([B,N] uint8, 0 on padded atoms).
Comparison      with a reference fingerprint, over the bits of a `kinds` mask - by default HYDROPHOBIC | HBOND_DONOR |
                HBOND_ACCEPTOR: CONTACT is reported but not counted.  Exact integers: n_bits (the molecule's (group, kind)
                bits under the mask), n_ref_bits (the reference's), n_common (in both).  contact_recovery = n_common /
                n_ref_bits; contact_tanimoto = n_common / (n_bits + n_ref_bits - n_common); both formed on the host in fp64
                from the integers, NaN where the denominator is 0.
Status          per row: OK (0); EMPTY (1) - no atoms: no entries, n_bits = n_common = 0, compared like any other empty
                fingerprint; NONFINITE (2) - a non-finite coordinate on a real atom: no entries, the counts -1; OVERFLOW (3) -
                more than 256 groups in contact, or more than MAX_CANDIDATES = 2048 receptor atoms in contact (the unique
                receptor atoms within about 5 A of a molecule of at most 64 atoms stay well below it in a protein): no
                entries, the counts -1.  Other rows are never affected.
A row's outputs depend on its own atoms, the receptor's atoms and their group ids only: the same bits in any batch, at any
row, at any padded width, with and without tile skipping; with explicit `groups=` also whatever the order the receptor's
atoms were listed in.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _args, _lib
from . import interactions as mcg_interactions
from . import receptor as mcg_receptor

CONTACT, HYDROPHOBIC, HBOND_DONOR, HBOND_ACCEPTOR = 1, 2, 4, 8
ALL_KINDS = CONTACT | HYDROPHOBIC | HBOND_DONOR | HBOND_ACCEPTOR
DEFAULT_KINDS = HYDROPHOBIC | HBOND_DONOR | HBOND_ACCEPTOR
KIND_NAMES = ((CONTACT, "contact"), (HYDROPHOBIC, "hydrophobic"), (HBOND_DONOR, "hbond_donor"),
              (HBOND_ACCEPTOR, "hbond_acceptor"))
MAX_GROUPS = 256                # include/mlconfgen_hip_contacts.h MCG_CONTACT_MAX_GROUPS
MAX_CANDIDATES = 2048           # MCG_CONTACT_MAX_CANDIDATES
CONTACT_DISTANCE = 0.5          # angstrom of surface distance, decided as d <= 0.5f
OK, EMPTY, NONFINITE, OVERFLOW = 0, 1, 2, 3
STATUS_NAMES = ("ok", "empty", "nonfinite", "overflow")
MAX_ATOMS = mcg_interactions.MAX_ATOMS
MAX_BATCH = mcg_interactions.MAX_BATCH
OPTION = "contacts"             # the value of `interaction_scores` that asks for the fingerprint
REFUSAL_WITHOUT_RESIDUES = ("interaction_scores='contacts' needs the receptor's residue identities: pass the receptor as a "
                            "PDB-format string (or a reference_shape pocket found on one); for any other receptor form "
                            "call contacts.contact_fingerprint(groups=...) on the returned coordinates")
REFUSAL_WITHOUT_GRAPH = ("interaction_scores=('contacts', t) filters by the recovery of the reference's contacts, which needs "
                         "the reference conformer typed by its molecular graph: pass reference_graph= or a reference "
                         "conformer with bonds (a reference_context, a reference_shape or a pocket has none)")


class PreparedReceptor(NamedTuple):
    """A typed, grouped receptor as `mcg_receptor_contacts` reads it, on the host (`prepare_receptor`)."""
    xyzr: torch.Tensor            # [R,4] fp32: x, y, z, interaction radius - `interactions.PreparedReceptor`'s, bit for bit
    types: torch.Tensor           # [R] uint8
    spheres: torch.Tensor         # [ceil(R / 256), 4] fp32: `receptor.tile_spheres`
    groups: torch.Tensor          # [R] int32: the group id of each atom, in the sorted order
    group_labels: Optional[Tuple[str, ...]] = None      # per dense id of a PDB receptor; None: the ids are their own labels

    @property
    def typed(self) -> "mcg_interactions.PreparedReceptor":
        """The same receptor as the interaction kernels take it."""
        return mcg_interactions.PreparedReceptor(self.xyzr, self.types, self.spheres)


def check_kinds(value, name: str = "kinds") -> int:
    """A kinds mask as an int in 0..15 (an integer, not a bool), else ValueError."""
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= ALL_KINDS:
        raise ValueError(f"{name} must be an integer mask in 0..{ALL_KINDS} (bits 1 contact, 2 hydrophobic, 4 hbond_donor, "
                         f"8 hbond_acceptor), got {value!r}")
    return int(value)


def _raw_atomic_numbers(receptor) -> torch.Tensor:
    """The atomic numbers of `receptor`'s atoms AS GIVEN, hydrogens included: what `groups=` is aligned with."""
    if hasattr(receptor, "GetAtoms"):
        return torch.tensor([a.GetAtomicNum() for a in receptor.GetAtoms()], dtype=torch.long)
    return torch.as_tensor(receptor[1]).cpu().reshape(-1).to(torch.long)


def prepare_receptor(receptor, groups=None) -> PreparedReceptor:
    """`receptor` - what `receptor.load_typed_receptor` takes, or a `PreparedReceptor` of this module, returned as it is -
    loaded, typed, given its interaction radii and group ids and sorted (`receptor.sort_grouped_receptor`), with the bounding
    spheres of its tiles: host work, once per receptor.  A PDB-format string brings its residues (`groups` must then be
    None); every other form needs `groups`, [R] integers >= 0 aligned with the atoms as given.  ValueError: what
    `load_typed_receptor` refuses, missing, misplaced, non-integer or negative groups, a count that does not fit."""
    if isinstance(receptor, PreparedReceptor):
        if groups is not None:
            raise ValueError("groups= cannot be given beside a prepared receptor: it carries its own")
        return receptor
    if isinstance(receptor, mcg_interactions.PreparedReceptor):
        raise ValueError("an interactions.PreparedReceptor carries no group ids: pass the receptor itself to "
                         "contacts.prepare_receptor")
    labels = None
    if isinstance(receptor, str):
        if groups is not None:
            raise ValueError("groups= cannot be given beside a PDB-format string: its residues are the groups")
        xyz, z, types = mcg_receptor.load_typed_receptor(receptor)
        ids, names = mcg_receptor.parse_pdb_groups(receptor)
        labels = tuple(names)
    else:
        if groups is None:
            raise ValueError("this receptor form carries no residue identities: pass groups= ([R] integers >= 0, one per "
                             "atom as given) or the receptor as a PDB-format string")
        xyz, z, types = mcg_receptor.load_typed_receptor(receptor)
        try:
            given = torch.as_tensor(groups).cpu().reshape(-1)
        except (TypeError, RuntimeError, ValueError) as e:
            raise ValueError(f"groups: unreadable: {e}") from None
        raw_z = _raw_atomic_numbers(receptor)
        if given.dtype.is_floating_point or given.dtype == torch.bool or given.numel() != raw_z.numel():
            raise ValueError(f"groups must be [R] integers, one per receptor atom as given: got {given.numel()} of type "
                             f"{given.dtype} for {raw_z.numel()} atoms")
        if given.numel() and (int(given.min()) < 0 or int(given.max()) > 0x7FFFFFFF):
            raise ValueError(f"groups must lie in 0..2^31-1, got {int(given.min())}..{int(given.max())}")
        ids = given[raw_z != 1].to(torch.int32)
    if int(ids.numel()) != int(z.numel()):
        raise ValueError(f"{int(ids.numel())} group ids for {int(z.numel())} receptor heavy atoms")
    xyzr, types, ids = mcg_receptor.sort_grouped_receptor(xyz, mcg_interactions.interaction_radii(z), types, ids)
    return PreparedReceptor(xyzr, types, mcg_receptor.tile_spheres(xyzr), ids, labels)


def load_reference(reference) -> Tuple[torch.Tensor, torch.Tensor]:
    """A reference fingerprint as (groups [K] int32 ascending, kinds [K] uint8) on the host: `reference` is a pair
    (groups, kinds) of equally long sequences or tensors - a row of `contact_fingerprint`'s result cut at its `n_groups`, say
    - or a dict with those two keys.  ValueError: more than MAX_GROUPS entries, a group twice or out of order, kinds outside
    0..15, lengths that differ."""
    if isinstance(reference, dict):
        reference = (reference["groups"], reference["kinds"])
    if not isinstance(reference, (tuple, list)) or len(reference) != 2:
        raise ValueError("reference must be a (groups, kinds) pair or a dict with those keys")
    try:
        g = torch.as_tensor(reference[0]).cpu().reshape(-1)
        k = torch.as_tensor(reference[1]).cpu().reshape(-1)
    except (TypeError, RuntimeError, ValueError) as e:
        raise ValueError(f"reference: unreadable: {e}") from None
    if g.numel() == 0 and k.numel() == 0:           # (an empty list has no integer type of its own)
        return torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.uint8)
    if g.dtype.is_floating_point or k.dtype.is_floating_point or g.numel() != k.numel():
        raise ValueError(f"reference (groups, kinds): two integer lists of one length, got {g.numel()} and {k.numel()}")
    if g.numel() > MAX_GROUPS:
        raise ValueError(f"a reference fingerprint holds at most {MAX_GROUPS} entries, got {g.numel()}")
    g, k = g.to(torch.int64), k.to(torch.int64)
    if g.numel() and (int(g.min()) < 0 or int(g.max()) > 0x7FFFFFFF or bool((g[1:] <= g[:-1]).any())):
        raise ValueError("reference groups must be >= 0 and strictly ascending")
    if k.numel() and (int(k.min()) < 0 or int(k.max()) > ALL_KINDS):
        raise ValueError(f"reference kinds must lie in 0..{ALL_KINDS}")
    return g.to(torch.int32).contiguous(), k.to(torch.uint8).contiguous()


def compare_counts(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(recovery, tanimoto) [B] fp64 on the host from the kernel's integer counts [B,3] (n_bits, n_ref_bits, n_common): the
    quotients of this module's definition, NaN where the denominator is 0 or the counts are -1."""
    c = counts.cpu().to(torch.float64)
    nan = torch.full((c.shape[0],), float("nan"), dtype=torch.float64)
    ok = c[:, 0] >= 0
    union = c[:, 0] + c[:, 1] - c[:, 2]
    recovery = torch.where(ok & (c[:, 1] > 0), c[:, 2] / torch.where(c[:, 1] > 0, c[:, 1], torch.ones_like(c[:, 1])), nan)
    tanimoto = torch.where(ok & (union > 0), c[:, 2] / torch.where(union > 0, union, torch.ones_like(union)), nan)
    return recovery, tanimoto


@torch.no_grad()
def fingerprint_typed(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, radii: torch.Tensor, types: torch.Tensor,
                      groups=None, reference=None, kinds: int = DEFAULT_KINDS, skip_tiles: bool = True, device=None
                      ) -> Dict[str, torch.Tensor]:
    """The `mcg_receptor_contacts` launch itself, on ligand atoms that are already typed: `coords` [B,N,3], `n_nodes` [B],
    `radii` [B,N] fp32 interaction radii, `types` [B,N] uint8 type bits; `receptor`, `groups`, `reference`, `kinds` as in
    `contact_fingerprint`.  Device tensors as the kernel writes them (include/mlconfgen_hip_contacts.h): groups [B,256],
    kinds [B,256], n_groups [B], atom_kinds [B,N], status [B] and - with `reference` - n_bits, n_ref_bits, n_common [B] and
    the fp64 recovery and tanimoto [B].  B or N of 0 launches nothing and returns EMPTY rows."""
    prepared = prepare_receptor(receptor, groups)
    mask = check_kinds(kinds)
    ref = None if reference is None else load_reference(reference)
    dev = _args.resolve_device(device, coords)
    B, N, _ = _args.ligand_arguments(coords, n_nodes, None, MAX_ATOMS, MAX_BATCH, "the contact fingerprint takes")
    for name, t, shape in (("radii", radii, (B, N)), ("types", types, (B, N))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    return _fingerprint_typed(prepared, coords, n_nodes, B, N, radii, types, ref, mask, skip_tiles, dev)


def _fingerprint_typed(prepared, coords, n_nodes, B, N, radii, types, ref, mask, skip_tiles, dev) -> Dict[str, torch.Tensor]:
    """`fingerprint_typed` behind its checks."""
    out = dict(groups=torch.zeros(B, MAX_GROUPS, dtype=torch.int32, device=dev),
               kinds=torch.zeros(B, MAX_GROUPS, dtype=torch.uint8, device=dev),
               n_groups=torch.zeros(B, dtype=torch.int32, device=dev),
               atom_kinds=torch.zeros(B, N, dtype=torch.uint8, device=dev),
               status=torch.full((B,), EMPTY, dtype=torch.int32, device=dev))
    counts = None
    if ref is not None:
        counts = torch.zeros(B, 3, dtype=torch.int32, device=dev)
        counts[:, 1] = sum(bin(int(k) & mask).count("1") for k in ref[1].tolist())      # (what an unlaunched call reports)
    if B > 0 and N > 0:
        x = coords.to(dev, torch.float32).contiguous()
        lig_r = radii.to(dev, torch.float32).contiguous()
        lig_t = types.to(dev, torch.uint8).contiguous()
        nn = torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous()
        rec, rec_t, rec_g = prepared.xyzr.to(dev), prepared.types.to(dev), prepared.groups.to(dev)
        spheres = prepared.spheres.to(dev) if skip_tiles else None
        ref_g = ref_k = None
        if ref is not None and ref[0].numel():
            ref_g, ref_k = ref[0].to(dev), ref[1].to(dev)
        _lib.check(_lib.lib().mcg_receptor_contacts(
            _lib.dptr(x), _lib.dptr(lig_r), _lib.dptr(lig_t), _lib.dptr(nn), B, N, _lib.dptr(rec), _lib.dptr(rec_t),
            _lib.dptr(rec_g), int(rec.shape[0]), _lib.dptr(spheres), _lib.dptr(ref_g), _lib.dptr(ref_k),
            0 if ref is None else int(ref[0].numel()), mask, _lib.dptr(out["groups"]), _lib.dptr(out["kinds"]),
            _lib.dptr(out["n_groups"]), _lib.dptr(out["atom_kinds"]), _lib.dptr(out["status"]), _lib.dptr(counts),
            _lib.current_stream_ptr(dev)), "mcg_receptor_contacts")
    if counts is not None:
        recovery, tanimoto = compare_counts(counts)
        out.update(n_bits=counts[:, 0], n_ref_bits=counts[:, 1], n_common=counts[:, 2], recovery=recovery.to(dev),
                   tanimoto=tanimoto.to(dev))
    return out


@torch.no_grad()
def contact_fingerprint(receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                        bond_orders: torch.Tensor, groups=None, reference=None, kinds: int = DEFAULT_KINDS,
                        skip_tiles: bool = True, device=None) -> Dict[str, torch.Tensor]:
    """The contact fingerprint of every molecule of the padded, posed coordinates `coords` [B,N,3] (`n_nodes` [B] real
    atoms, `atomic_numbers` [B, >= N], `bond_orders` [B,N,N]) with `receptor` - a PDB-format string, any other form
    `receptor.load_typed_receptor` takes together with `groups` ([R] integers >= 0, one per atom as given), or a
    `prepare_receptor` result - by this module's definition: one perceive launch (`interactions.ligand_types`) and one
    `mcg_receptor_contacts` launch.  Device tensors:
      groups [B,256]      int32: the groups in contact, ascending, 0 behind the count
      kinds [B,256]       uint8: their kind bits
      n_groups [B]        int32
      atom_kinds [B,N]    uint8: per ligand atom the OR of the kinds it takes part in (0 on padded atoms)
      status [B]          int32: OK, EMPTY, NONFINITE, OVERFLOW
    and with `reference` - a (groups, kinds) pair, `load_reference` - over the bits of the `kinds` mask:
      n_bits, n_ref_bits, n_common [B]   int32, exact (-1 on a NONFINITE or OVERFLOW row)
      recovery, tanimoto [B]             fp64: n_common / n_ref_bits and n_common / (n_bits + n_ref_bits - n_common), NaN
                                         where the denominator is 0
    `skip_tiles`: whether a molecule's workgroup walks only the receptor tiles within the cut-off of it; never a bit of the
    result.  Refused before any device work: what `prepare_receptor` and `load_reference` refuse, a `kinds` outside 0..15,
    atom counts outside [0, N], N > 64, B > MAX_BATCH, shapes that do not fit."""
    prepared = prepare_receptor(receptor, groups)
    mask = check_kinds(kinds)
    ref = None if reference is None else load_reference(reference)
    dev = _args.resolve_device(device, coords)
    B, N, z, bonds = mcg_interactions._posed_graphs(coords, n_nodes, atomic_numbers, bond_orders,
                                                    "the contact fingerprint takes")
    types = torch.zeros(B, N, dtype=torch.uint8, device=dev)
    if B > 0 and N > 0:
        types = mcg_interactions.ligand_types(z[:, :N], bonds[:, :N, :N], n_nodes, dev)
    return _fingerprint_typed(prepared, coords, n_nodes, B, N, mcg_interactions.interaction_radii(z[:, :N].to(dev)), types,
                              ref, mask, skip_tiles, dev)


def kind_names(kinds: int) -> Tuple[str, ...]:
    """The names of the bits of `kinds`, in bit order: ("contact", "hydrophobic", "hbond_donor", "hbond_acceptor")."""
    return tuple(name for bit, name in KIND_NAMES if int(kinds) & bit)


def group_label(prepared: Optional[PreparedReceptor], group: int):
    """The label of a group id: the residue label of a PDB receptor, else the integer itself."""
    names = None if prepared is None else prepared.group_labels
    return int(group) if names is None else names[int(group)]


def labels(prepared: Optional[PreparedReceptor], groups, kinds, n_groups=None) -> List[tuple]:
    """Per row of `groups` / `kinds` ([B,256] as `contact_fingerprint` returns them, or any [B,K]) a tuple of (label, kind
    names) over its entries, on the host: entries with kinds 0 - the zeros behind a row's count - are left out, or, with
    `n_groups`, everything behind it."""
    g, k = torch.as_tensor(groups).cpu().tolist(), torch.as_tensor(kinds).cpu().tolist()
    n = None if n_groups is None else torch.as_tensor(n_groups).cpu().tolist()
    rows = []
    for b, (gr, kr) in enumerate(zip(g, k)):
        if n is not None:
            gr, kr = gr[: n[b]], kr[: n[b]]
        rows.append(tuple((group_label(prepared, gi), kind_names(ki)) for gi, ki in zip(gr, kr) if ki))
    return rows


def compare_entries(groups: Sequence[int], kinds: Sequence[int], ref_groups: Sequence[int], ref_kinds: Sequence[int],
                    mask: int = DEFAULT_KINDS) -> Tuple[List[tuple], List[tuple]]:
    """(recovered, missed) of a fingerprint against a reference, on the host: per reference group the bits under `mask` the
    fingerprint also has, and those it lacks, each as [(group, kinds)] over the groups where that is not 0."""
    have = dict(zip(groups, kinds))
    recovered, missed = [], []
    for g, k in zip(ref_groups, ref_kinds):
        both, lack = k & have.get(g, 0) & mask, k & ~have.get(g, 0) & mask
        if both:
            recovered.append((g, both))
        if lack:
            missed.append((g, lack))
    return recovered, missed


# ----------------------------------------------------------------------------------------------- options
def parse_option(value):
    """(`interaction_scores` as the bool the score's own parser reads, whether the call fingerprints contacts, the recovery
    threshold or None): "contacts" and ("contacts", t), t a real number in [0, 1]; every other value is handed back
    untouched - True, False and what is refused today stay exactly as they are."""
    if isinstance(value, str) and value == OPTION:
        return True, True, None
    if isinstance(value, (tuple, list)) and len(value) == 2 and isinstance(value[0], str) and value[0] == OPTION:
        return True, True, _args.check_real("interaction_scores: t of ('contacts', t)", value[1], 0.0, 1.0)
    return value, False, None
