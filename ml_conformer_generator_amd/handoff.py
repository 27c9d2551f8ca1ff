"""EDM -> GCN hand-off and bond write-back on the device.

The reference goes through RDKit here (`samples_to_rdkit_mol`, `canonicalise`,
`prepare_adj_mat_seer_input`, `redefine_bonds`, `standardize_mol`;
mol_utils.py:18-57,110-223, standardizer.py).  The tensor halves (atom decode, distances + I,
connectivity + I, pad 42, lower-triangle bond write-back) run in two HIP launches
(`mcg_handoff_elements`, `mcg_bond_writeback`), follow the reference and are checked against
`oracle/host_oracle.py` and reference-generated fixtures; one D2H copy at the end.
The two decisions RDKit OWNS in front of the GCN - the canonical-SMILES atom order and the
1-order connectivity (`canonicalise`, mol_utils.py:110-126) - are INPUTS of the hand-off launch
(`order`, `connectivity`): RDKit's own where RDKit imports (`rdkit_order.py`), a caller's, or -
when neither is given - the labelled substitutes (generation order, covalent-radius rule:
parity unpinned against RDKit).  "valid" without RDKit is a valence / connectivity proxy.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .config import DIMENSION, N_ATOM_CLASSES
from .elements import Z_TO_SYMBOL

_COV_FACTOR = 1.3          # RDKit DetermineConnectivity's default covFactor (radii: config.ELEMENTS, csrc/mcg_elements.h)


class _HostBatch:
    """The gathered result tensors of one generation call on the HOST (one D2H copy per tensor); the molecule records
    below are views into it."""
    __slots__ = ("x", "elements", "bonds", "n")

    def __init__(self, x, elements, bonds, n):
        self.x, self.elements, self.bonds, self.n = x, elements, bonds, n


@dataclasses.dataclass
class Measured:
    """What a generation call measured of one molecule; None = not measured (`GeneratedMolecule`'s properties of the same
    names say what each value is)."""
    shape_tanimoto: Optional[float] = None
    overlay_tanimoto: Optional[float] = None
    pose: Optional[torch.Tensor] = None           # [12] fp32: rotation row-major, then translation
    receptor_clashes: Optional[int] = None
    receptor_max_overlap: Optional[float] = None
    atoms_outside: Optional[int] = None
    chemical_tanimoto: Optional[float] = None
    graph_key: Optional[int] = None               # unsigned 64-bit
    strain_before: Optional[float] = None
    strain_after: Optional[float] = None
    pharmacophore_tanimoto: Optional[float] = None
    pharmacophore_matches: Optional[int] = None
    relief_rmsd: Optional[float] = None
    receptor_clashes_before: Optional[int] = None
    hydrogen_coords: Optional[object] = None      # [nH,3] fp32, host - or (batch [B,H,3], row, count), sliced on first read
    hydrogen_parents: Optional[List[int]] = None
    hydrogens_unplaced: Optional[int] = None
    receptor_hydrogen_clashes: Optional[int] = None
    atoms_removed: Optional[int] = None
    n_fragments: Optional[int] = None
    atom_map: Optional[List[int]] = None
    kekule_bond_orders: Optional[object] = None   # [n,n] int8, host - or (batch [B,W,W], row, n), sliced on first read
    electrostatic_tanimoto: Optional[float] = None
    partial_charges: Optional[object] = None      # [n] fp32, host - or (batch [B,W], row, n), sliced on first read
    hydrogen_charges: Optional[object] = None     # [n] fp32, host - likewise
    canonical_order: Optional[object] = None      # List[int] - or (batch [B,W] int32, row, n), sliced on first read
    canonical_status: Optional[int] = None        # `canonical.describe_status`; 0 = the order is canonical
    substructure_counts: Optional[object] = None  # List[int], one per pattern - or (batch [B,P] int32, row), sliced on first read
    substructure_status: Optional[object] = None  # List[int] (`substructure.describe_status`) - likewise
    substructure_first: Optional[object] = None   # per pattern the first embedding or None - or (batch [B,P,M], row), likewise
    substructure_patterns: Optional[tuple] = None     # the call's `substructure.Pattern`s: require, exclude, counts, in order
    interaction_score: Optional[float] = None     # E of `interactions.py`; negative is better
    interaction_terms: Optional[dict] = None      # g1, g2, rep, hyd, hb (the five sums) and n_rot
    receptor_hbonds: Optional[int] = None
    interaction_atom_scores: Optional[object] = None  # [n] fp32, host - or (batch [B,W], row, n), sliced on first read
    interaction_score_before: Optional[float] = None  # E of the pose `optimise_pose` started from
    pose_optimisation_rmsd: Optional[float] = None
    pose_trials_kept: Optional[int] = None
    pose_torsions: Optional[int] = None           # `optimise_pose="flexible"`: torsions the walk used (at most 16)
    pose_torsion_angles: Optional[List[float]] = None   # rad, one per used torsion: the summed kept turns
    pose_conformer_rmsd: Optional[float] = None   # A: the change of the conformer alone, the rigid part taken out
    intramolecular_clash_before: Optional[float] = None     # CLASH of `interactions.optimise_pose_flexible` at the start
    intramolecular_clash: Optional[float] = None  # ... and at the returned coordinates
    pose_starts: Optional[int] = None             # `optimise_pose="search"`: starts the pose search walked
    pose_best_start: Optional[int] = None         # ... and the one that won (0: the pose as it came; -1: none was finite)
    contact_groups: Optional[List[int]] = None    # `contacts.py`: the group ids of the receptor groups in contact, ascending
    contact_kinds: Optional[List[int]] = None     # ... and the kind bits of each
    contact_atom_kinds: Optional[List[int]] = None    # per atom the OR of the kinds it takes part in
    contact_status: Optional[int] = None          # `contacts.STATUS_NAMES`
    contact_recovery: Optional[float] = None      # n_common / n_ref_bits against the reference conformer's fingerprint
    contact_tanimoto: Optional[float] = None
    contact_labels: Optional[tuple] = None        # the call's group labels, shared by its records (None: the ids themselves)
    contact_reference: Optional[tuple] = None     # (groups, kinds, mask) of the reference conformer's fingerprint, shared
    stereo_order: Optional[List[int]] = None      # the stereo search's atom order, -1 beyond the atoms as it comes
    stereo_status: Optional[int] = None           # `canonical.describe_status`; 0 = the stereo identity is defined
    stereo_descriptors: Optional[list] = None     # [the row of v as it comes, None -> per atom in record order on first read]
    n_stereo_defined: Optional[int] = None
    n_stereo_undefined: Optional[int] = None
    n_rings: Optional[int] = None                 # `scaffold.py`: the cyclomatic number
    n_ring_systems: Optional[int] = None
    min_ring_size: Optional[int] = None
    max_ring_size: Optional[int] = None
    ring_sizes: Optional[object] = None           # List[int] per atom - or (batch [B,W] int32, row), sliced on first read
    ring_systems: Optional[object] = None         # List[int] per atom - likewise
    scaffold_atoms: Optional[List[int]] = None    # sorted indices into the record's atoms
    scaffold_key: Optional[int] = None            # unsigned 64-bit; 0 for the empty scaffold and where the status is not 0
    scaffold_status: Optional[int] = None         # `canonical.describe_status` of the scaffold graph; EMPTY = no scaffold
    scaffold_smiles: Optional[str] = None         # "" for the empty scaffold


_UNMEASURED = Measured()          # shared by every record that carries no values: never written to


def measured_from_tensors(values: Dict[str, Optional[torch.Tensor]], n: int) -> List[Measured]:
    """The records of n samples from per-sample tensors by field name of `Measured` (a name left out or None: not
    measured), one D2H copy each.  The one place that reads the tensors' spellings of "not measured": a negative
    `receptor_clashes` (both contact values None), a negative `atoms_outside`, a `pose` row [12] with a non-finite entry
    (`overlay_tanimoto` keeps its NaN), a negative `pharmacophore_matches` (both pharmacophore values None), a negative
    `receptor_clashes_before` (both relief values None); `graph_key` is int64 holding the unsigned bit pattern.
    The hydrogens of a call with `add_hydrogens` come as `hydrogen_coords` [n,H,3], `hydrogen_parents` [n,H] (-1 beyond a
    row's count) and `hydrogens_unplaced` [n] (negative: the row had a non-finite coordinate, the record gets None for all
    three); a record's `hydrogen_coords` is left as (the one host copy, row, count) and sliced on first read
    (`GeneratedMolecule.hydrogen_coords`).  A negative `receptor_hydrogen_clashes`: not measured.
    The standardisation of a call with `standardize` comes as `atoms_removed` [n], `n_fragments` [n], `atom_map` [n,W] (-1
    beyond a row's atoms) and `kekule_bond_orders` [n,W,W] (all four or none); a record's `kekule_bond_orders` is left as
    (the one host copy, row, atom count) and sliced on first read.
    The charges of a call with `partial_charges` come as `partial_charges` [n,W] and `hydrogen_charges` [n,W] fp32 (both or
    neither), +inf at and beyond a row's atoms (a real atom's charge is finite or NaN); a record's fields are left as (the
    one host copy, row, atom count) and sliced on first read.  `electrostatic_tanimoto` [n] fp32 is taken as it comes.
    The canonical labelling of a call with `smiles` comes as `canonical_order` [n,W] int32 (-1 beyond a row's atoms, and
    throughout a row that has no canonical order) and `canonical_status` [n] (both or neither); a record's
    `canonical_order` is left as (the one host copy, row, atom count) and sliced on first read.
    The matches of a call with a substructure option come as `substructure_counts` [n,P], `substructure_status` [n,P],
    `substructure_first` [n,P,M] int32 (the caller's pattern atom order, -1 beyond a pattern's atoms) and
    `substructure_patterns`, the tuple of the P patterns, which every record shares (all four or none); a record's three
    fields are left as (the one host copy, row) and sliced on first read (`substructure_row`).
    The interactions of a call with `interaction_scores` come as `interaction_score` [n] fp32, `interaction_terms` [n,6]
    fp32 (G1, G2, REP, HYD, HB, n_rot), `receptor_hbonds` [n] (negative: posing failed - the record gets None for all four)
    and `interaction_atom_scores` [n,W] fp32, +inf at and beyond a row's atoms (all four or none); a record's
    `interaction_atom_scores` is left as (the one host copy, row, atom count) and sliced on first read.
    The pose optimisation of a call with `optimise_pose` comes as `interaction_score_before` [n] fp32,
    `pose_optimisation_rmsd` [n] fp32 and `pose_trials_kept` [n] (negative: posing failed - the record gets None for all
    three).  `optimise_pose="flexible"` adds `pose_torsions` [n] int32, `pose_torsion_angles` [n,16] fp32 (a record keeps
    the first `pose_torsions`), `pose_conformer_rmsd`, `intramolecular_clash_before` and `intramolecular_clash` [n] fp32
    (all five or none; None on the same rows).  `optimise_pose="search"` adds `pose_starts` and `pose_best_start` [n] int32
    beside them (both or neither; None on the same rows).
    The contacts of a call with `interaction_scores="contacts"` come as `postprocess.contacts` spells them: `contact_status`
    [n] (negative: posing failed - the record gets None throughout), `contact_groups` [n,256] int32, `contact_kinds` [n,256]
    uint8 (an entry's kinds are never 0: the zeros behind a row's count end it), `contact_atom_kinds` [n,W] uint8 (255 at and
    beyond a row's atoms), with a reference `contact_recovery` / `contact_tanimoto` [n] fp64, and the two values every record
    shares: `contact_labels` (a tuple of group labels or None) and `contact_reference` ((groups, kinds, mask) or None).
    The stereo identity of a call with `smiles="isomeric"` comes as `stereo_order` [n,W] int32, `stereo_status` [n],
    `stereo_descriptors` [n,W] int8 - `stereo.stereo_order`'s `stereo`: v in canonical position order, which a record
    turns into its own order on first read -, `n_stereo_defined` [n] and `n_stereo_undefined` [n] (all five or none).
    The rings and the scaffold of a call with `unique="scaffold"` / `"framework"` come as `scaffold.record_fields` spells
    them: `n_rings`, `n_ring_systems`, `min_ring_size`, `max_ring_size`, `scaffold_status` [n], `scaffold_key` [n] int64
    holding the unsigned bit pattern, `ring_sizes` / `ring_systems` [n,W] int32 - a record's are left as (the one host
    copy, row) and sliced to its atoms on first read -, `scaffold_atoms` [n,W] (-1 behind the kept atoms) and, where the
    call also writes SMILES, `scaffold_smiles`, a host list of n strings (None: no canonical order)."""
    hyd = {k: values.get(k) for k in ("ring_sizes", "ring_systems", "scaffold_atoms", "scaffold_smiles",
                                      "stereo_descriptors", "hydrogen_coords", "hydrogen_parents", "atom_map", "kekule_bond_orders",
                                      "partial_charges", "hydrogen_charges", "canonical_order", "substructure_counts",
                                      "substructure_status", "substructure_first", "substructure_patterns",
                                      "interaction_atom_scores", "contact_groups", "contact_kinds", "contact_atom_kinds",
                                      "contact_labels", "contact_reference")}
    cols = {k: v.cpu().tolist() for k, v in values.items() if v is not None and k != "pose" and k not in hyd}
    if values.get("pose") is not None:
        poses = values["pose"].cpu().to(torch.float32)
        cols["pose"] = [poses[b] if ok else None for b, ok in enumerate(torch.isfinite(poses).all(dim=1).tolist())]
    if "receptor_clashes" in cols:
        missing = [c < 0 for c in cols["receptor_clashes"]]
        for k in ("receptor_clashes", "receptor_max_overlap"):
            cols[k] = [None if gone else v for gone, v in zip(missing, cols[k])]
    if "atoms_outside" in cols:
        cols["atoms_outside"] = [None if c < 0 else c for c in cols["atoms_outside"]]
    if "pharmacophore_matches" in cols:
        missing = [c < 0 for c in cols["pharmacophore_matches"]]
        for k in ("pharmacophore_matches", "pharmacophore_tanimoto"):
            if k in cols:
                cols[k] = [None if gone else v for gone, v in zip(missing, cols[k])]
    if "receptor_clashes_before" in cols:
        missing = [c < 0 for c in cols["receptor_clashes_before"]]
        for k in ("receptor_clashes_before", "relief_rmsd"):
            if k in cols:
                cols[k] = [None if gone else v for gone, v in zip(missing, cols[k])]
    if "graph_key" in cols:
        cols["graph_key"] = [k & 0xFFFFFFFFFFFFFFFF for k in cols["graph_key"]]
    if "receptor_hydrogen_clashes" in cols:
        cols["receptor_hydrogen_clashes"] = [None if c < 0 else c for c in cols["receptor_hydrogen_clashes"]]
    if "hydrogens_unplaced" in cols:
        missing = [c < 0 for c in cols["hydrogens_unplaced"]]
        cols["hydrogens_unplaced"] = [None if gone else c for gone, c in zip(missing, cols["hydrogens_unplaced"])]
        xyz = hyd["hydrogen_coords"].cpu().to(torch.float32)
        parents = [[p for p in row if p >= 0] for row in hyd["hydrogen_parents"].cpu().tolist()]
        cols["hydrogen_parents"] = [None if gone else p for gone, p in zip(missing, parents)]
        cols["hydrogen_coords"] = [None if gone else (xyz, b, len(p)) for b, (gone, p) in enumerate(zip(missing, parents))]
    if hyd["atom_map"] is not None:
        cols["atom_map"] = [[a for a in row if a >= 0] for row in hyd["atom_map"].cpu().tolist()]
        orders = hyd["kekule_bond_orders"].cpu().to(torch.int8)
        cols["kekule_bond_orders"] = [(orders, b, len(kept)) for b, kept in enumerate(cols["atom_map"])]
    if hyd["partial_charges"] is not None:
        q, qh = hyd["partial_charges"].cpu().to(torch.float32), hyd["hydrogen_charges"].cpu().to(torch.float32)
        counts = (~torch.isinf(q)).sum(dim=1).tolist()
        cols["partial_charges"] = [(q, b, k) for b, k in enumerate(counts)]
        cols["hydrogen_charges"] = [(qh, b, k) for b, k in enumerate(counts)]
    if hyd["canonical_order"] is not None:
        orders = hyd["canonical_order"].cpu().to(torch.int32)
        cols["canonical_order"] = [(orders, b, k) for b, k in enumerate((orders >= 0).sum(dim=1).tolist())]
    if hyd["stereo_descriptors"] is not None:
        cols["stereo_descriptors"] = [[row, None] for row in hyd["stereo_descriptors"].cpu().tolist()]
    if hyd["substructure_counts"] is not None:
        for k in ("substructure_counts", "substructure_status", "substructure_first"):
            host = hyd[k].cpu().to(torch.int32)
            cols[k] = [(host, b) for b in range(n)]
        cols["substructure_patterns"] = [tuple(hyd["substructure_patterns"])] * n
    if "receptor_hbonds" in cols:
        missing = [c < 0 for c in cols["receptor_hbonds"]]
        names = ("g1", "g2", "rep", "hyd", "hb")
        cols["interaction_terms"] = [None if gone else dict(zip(names, row[:5]), n_rot=int(row[5]))
                                     for gone, row in zip(missing, cols["interaction_terms"])]
        per_atom = hyd["interaction_atom_scores"].cpu().to(torch.float32)
        counts = (~torch.isinf(per_atom)).sum(dim=1).tolist()
        cols["interaction_atom_scores"] = [(per_atom, b, k) for b, k in enumerate(counts)]
        for k in ("interaction_score", "interaction_terms", "receptor_hbonds", "interaction_atom_scores"):
            cols[k] = [None if gone else v for gone, v in zip(missing, cols[k])]
    if "contact_status" in cols:
        missing = [c < 0 for c in cols["contact_status"]]
        groups, kinds = hyd["contact_groups"].cpu().to(torch.int32), hyd["contact_kinds"].cpu().to(torch.uint8)
        atoms = hyd["contact_atom_kinds"].cpu().to(torch.uint8)
        counts, widths = (kinds != 0).sum(dim=1).tolist(), (atoms != 255).sum(dim=1).tolist()
        cols["contact_groups"] = [groups[b, :k].tolist() for b, k in enumerate(counts)]
        cols["contact_kinds"] = [kinds[b, :k].tolist() for b, k in enumerate(counts)]
        cols["contact_atom_kinds"] = [atoms[b, :k].tolist() for b, k in enumerate(widths)]
        cols["contact_labels"] = [hyd["contact_labels"]] * n
        cols["contact_reference"] = [hyd["contact_reference"]] * n
        for k in ("contact_status", "contact_groups", "contact_kinds", "contact_atom_kinds", "contact_recovery",
                  "contact_tanimoto", "contact_labels", "contact_reference"):
            if k in cols:
                cols[k] = [None if gone else v for gone, v in zip(missing, cols[k])]
    if hyd["scaffold_atoms"] is not None:
        cols["scaffold_atoms"] = [[a for a in row if a >= 0] for row in hyd["scaffold_atoms"].cpu().tolist()]
        for k in ("ring_sizes", "ring_systems"):
            host = hyd[k].cpu().to(torch.int32)
            cols[k] = [(host, b) for b in range(n)]
        cols["scaffold_key"] = [k & 0xFFFFFFFFFFFFFFFF for k in cols["scaffold_key"]]
        if hyd["scaffold_smiles"] is not None:
            cols["scaffold_smiles"] = list(hyd["scaffold_smiles"])
    if "pose_trials_kept" in cols:
        missing = [c < 0 for c in cols["pose_trials_kept"]]
        if "pose_torsions" in cols:             # a flexible walk: the angles of the torsions it used
            cols["pose_torsion_angles"] = [row[: max(k, 0)] for row, k in zip(cols["pose_torsion_angles"], cols["pose_torsions"])]
        for k in ("pose_trials_kept", "pose_optimisation_rmsd", "interaction_score_before", "pose_torsions",
                  "pose_torsion_angles", "pose_conformer_rmsd", "intramolecular_clash_before", "intramolecular_clash",
                  "pose_starts", "pose_best_start"):
            if k in cols:
                cols[k] = [None if gone else v for gone, v in zip(missing, cols[k])]
    return [Measured(**{k: col[b] for k, col in cols.items()}) for b in range(n)]


def substructure_row(measured: Measured) -> None:
    """Slices a record's substructure fields from the batch's host tensors, once: counts and status become one int per
    pattern, first per pattern the molecule's atom each pattern atom lands on (the pattern's own atom order), None where
    the pattern was not found."""
    if isinstance(measured.substructure_counts, tuple):
        for k in ("substructure_counts", "substructure_status"):
            host, b = getattr(measured, k)
            setattr(measured, k, host[b].tolist())
        host, b = measured.substructure_first
        measured.substructure_first = [row[: len(p.atoms)] if c > 0 else None for row, p, c in
                                       zip(host[b].tolist(), measured.substructure_patterns, measured.substructure_counts)]


class GeneratedMolecule:
    """RDKit-free result record: heavy atoms, coordinates and bond orders.

    `atomic_numbers` List[int]; `coords` [n,3] float32 (CPU); `bond_orders` [n,n] int8, symmetric, 0 none / 1 / 2 / 3 /
    4 aromatic; `valid` bool.  Records built by `molecules_from_tensors` are LAZY views into the batch's host tensors: the
    per-molecule slices are taken on first access, so assembling a batch costs one object per molecule (2 048 molecules:
    a few ms instead of 70-170 ms of slicing + cloning on every rank of a sharded call).  `sample_id`: which sample of
    its generation call the record is (invalid molecules are dropped, so a kept record's position says nothing).
    `shape_tanimoto`: its shape score against the reference when the call asked for scores, else None.
    `overlay_tanimoto` / `pose`: the score and rigid pose of a call that posed its molecules onto the reference
    (`overlay=True`), else None.  `receptor_clashes` / `receptor_max_overlap`: its steric contacts with the call's
    receptor, else None.  `chemical_tanimoto` / `graph_key`: its chemical similarity to the reference and its graph
    identity key (`fingerprint.py`: the package's own Morgan-type fingerprint, a substitute for RDKit's), else None.
    `atoms_outside`: how many of its atoms lie outside the mesh of a call posed into a `reference_shape`, else None.
    `strain_before` / `strain_after`: the energy of the package's own force field (`geometry.py`, NOT MMFF94) before and
    after the relaxation of a call with `relax_geometry`, else None.
    `pharmacophore_tanimoto` / `pharmacophore_matches`: the overlap of its pharmacophore features with the reference's and
    the reference features it matches (`pharmacophore.py`: the package's own definition) when the call asked for
    `pharmacophore_scores`, else None.
    `relief_rmsd` / `receptor_clashes_before`: how far the clash relief of a call with `relieve_clashes` moved it and the
    clashes of its pose before that (`receptor.py`: the package's own procedure), else None.
    `hydrogen_coords` / `hydrogen_parents` / `hydrogens_unplaced`: its explicit hydrogens when the call asked for
    `add_hydrogens` (`hydrogens.py`: the package's own definition, NOT RDKit's AddHs), else None; with a receptor also
    `receptor_hydrogen_clashes`.  `to_molblock(hydrogens=True)` / `to_xyz_block(hydrogens=True)` write them.
    `atoms_removed` / `n_fragments` / `atom_map` / `kekule_bond_orders`: what the standardisation of a call with
    `standardize` did to it (`standardize.py`: the package's own definition, NOT RDKit's FragmentParent / Kekulize /
    SanitizeMol) - the record then IS the largest fragment - else None.  `to_molblock(kekulize=True)` writes the Kekule
    form.
    `electrostatic_tanimoto`: the similarity of its charge distribution, as posed, to the reference's when the call asked
    for `electrostatic_scores`; `partial_charges` / `hydrogen_charges`: its partial charges when the call asked for
    `partial_charges` (`electrostatics.py`: the package's own definition, NOT RDKit's Gasteiger charges), else None;
    `to_xyz_block(charges=True)` writes them.
    `canonical_order` / `canonical_status` / `smiles`: its exact canonical atom order and canonical SMILES when the call
    asked for `smiles` (`canonical.py`, `smiles.py`: the package's own definition - valid OpenSMILES, NOT RDKit's canonical
    SMILES), else None; `to_smiles()` writes the string, `to_smiles(canonical=False)` one in the record's own atom order.
    `stereo_order` / `stereo_status` / `stereo_descriptors` / `n_stereo_defined` / `n_stereo_undefined`: which
    stereoisomer its returned coordinates are when the call asked for `smiles="isomeric"` (`stereo.py`: the package's own
    definition, NOT RDKit's stereo perception, no CIP labels), else None; `smiles` and `to_smiles()` are then isomeric.
    `interaction_score` / `interaction_terms` / `receptor_hbonds` / `interaction_atom_scores`: its empirical interaction
    score with the call's typed receptor, the sums behind it, its hydrogen-bond count and per-atom contributions when the
    call asked for `interaction_scores` (`interactions.py`: the package's own definition, NOT AutoDock Vina's output), else
    None.
    `substructure_patterns` / `substructure_counts` / `substructure_status` / `substructure_first`: the patterns the call
    matched (`require_substructures`, `exclude_substructures`, `substructure_counts`, in that order) and, per pattern, how
    many embeddings this molecule has, how the search ended and the first embedding (`substructure.py`: the package's own
    definition, NOT RDKit's substructure matcher), else None.
    `n_rings` / `n_ring_systems` / `min_ring_size` / `max_ring_size` / `ring_sizes` / `ring_systems` / `scaffold_atoms` /
    `scaffold_key` / `scaffold_status` / `scaffold_smiles`: its rings and its scaffold when the call asked for
    `unique="scaffold"` or `"framework"` (`scaffold.py`: the package's own definitions, NOT RDKit's ring perception or
    MurckoScaffold), else None; `scaffold.of_records` writes them onto records after the fact."""
    __slots__ = ("_z", "_coords", "_bonds", "valid", "_batch", "_b", "_sid", "_measured", "_smiles", "_unmarked")

    def __init__(self, atomic_numbers: List[int], coords: torch.Tensor, bond_orders: torch.Tensor, valid: bool = True,
                 sample_id: Optional[int] = None):
        self._z, self._coords, self._bonds, self.valid = list(atomic_numbers), coords, bond_orders, bool(valid)
        self._batch, self._b, self._sid, self._measured = None, -1, sample_id, _UNMEASURED
        self._smiles = self._unmarked = None

    @classmethod
    def _view(cls, batch: _HostBatch, b: int, valid: bool, sample_id: Optional[int] = None,
              measured: Measured = _UNMEASURED) -> "GeneratedMolecule":
        m = cls.__new__(cls)
        m._z = m._coords = m._bonds = None
        m.valid, m._batch, m._b = valid, batch, b
        m._sid = b if sample_id is None else sample_id
        m._measured = measured
        m._smiles = m._unmarked = None
        return m

    @property
    def interaction_score(self) -> Optional[float]:
        """The empirical interaction score E of this molecule's returned coordinates with the call's typed receptor
        (`interactions.py`: the package's own definition - the functional form of the AutoDock Vina scoring function on
        the package's heavy-atom types, intermolecular terms only; NOT AutoDock Vina's output, not a binding free energy);
        negative is better.  When the call asked for `interaction_scores` or `max_interaction_score`; None otherwise and
        where posing failed."""
        return self._measured.interaction_score

    @property
    def interaction_terms(self) -> Optional[dict]:
        """The five sums behind `interaction_score` over the counted atom pairs - "g1", "g2", "rep", "hyd", "hb" - and
        "n_rot", the rotatable bonds of its divisor; None where `interaction_score` is None."""
        return self._measured.interaction_terms

    @property
    def receptor_hbonds(self) -> Optional[int]:
        """The donor / acceptor pairs of this molecule and the receptor at hydrogen-bond distance (surface distance <=
        -0.7 A; heavy atoms only, no angle: `interactions.py`); None where `interaction_score` is None."""
        return self._measured.receptor_hbonds

    @property
    def interaction_atom_scores(self) -> Optional[torch.Tensor]:
        """[n] fp32 (CPU): each atom's weighted contribution to the interaction score before the division by the
        rotatable-bond term (a view into the batch's host tensor, sliced on first access); None where
        `interaction_score` is None."""
        v = self._measured.interaction_atom_scores
        if isinstance(v, tuple):
            v = self._measured.interaction_atom_scores = v[0][v[1], : v[2]]
        return v

    @property
    def substructure_patterns(self) -> Optional[tuple]:
        """The `substructure.Pattern`s this call matched - those of `require_substructures`, then `exclude_substructures`,
        then `substructure_counts` - which the three fields below are indexed by; None in a call without them."""
        return self._measured.substructure_patterns

    @property
    def substructure_counts(self) -> Optional[List[int]]:
        """Per pattern of `substructure_patterns` the embeddings of it in this molecule's graph (`substructure.py`: every
        injective map counts, so benzene's ring is found 12 times; a lower bound where the status is BUDGET).  With
        `standardize` the parent fragment's graph is read.  None in a call without a substructure option."""
        substructure_row(self._measured)
        return self._measured.substructure_counts

    @property
    def substructure_status(self) -> Optional[List[int]]:
        """Per pattern 0, or `substructure.STATUS_BUDGET` (`substructure.describe_status`): a root's search was stopped at
        the node budget, the count is a lower bound and a count of 0 proves nothing."""
        substructure_row(self._measured)
        return self._measured.substructure_status

    @property
    def substructure_first(self) -> Optional[List[Optional[List[int]]]]:
        """Per pattern the embedding found first: entry i is the index, in this record, of the atom that pattern atom i (the
        pattern's own atom order) lands on - for highlighting; None where the pattern was not found."""
        substructure_row(self._measured)
        return self._measured.substructure_first

    @property
    def n_rings(self) -> Optional[int]:
        """Ring bonds - ring atoms + ring systems of the molecular graph, the cyclomatic number (`scaffold.py`: the
        package's own definition, no SSSR): cubane 5, naphthalene 2.  When the call asked for `unique="scaffold"` /
        `"framework"` (or `scaffold.of_records` annotated the record); None otherwise."""
        return self._measured.n_rings

    @property
    def n_ring_systems(self) -> Optional[int]:
        """The connected components of the ring-bond sub-graph: fused, bridged and spiro rings are one system."""
        return self._measured.n_ring_systems

    @property
    def min_ring_size(self) -> Optional[int]:
        """The smallest cycle through any ring bond; 0 for an acyclic molecule."""
        return self._measured.min_ring_size

    @property
    def max_ring_size(self) -> Optional[int]:
        """The largest, over the ring bonds, of the smallest cycle through each - the largest ring one cannot avoid (a
        14-membered macrocycle 14, bicyclo[2.2.2]octane 6); 0 for an acyclic molecule."""
        return self._measured.max_ring_size

    def _per_atom(self, name: str) -> Optional[List[int]]:
        v = getattr(self._measured, name)
        if isinstance(v, tuple):
            v = v[0][v[1], : len(self.atomic_numbers)].tolist()
            setattr(self._measured, name, v)
        return v

    @property
    def ring_sizes(self) -> Optional[List[int]]:
        """Per atom the smallest cycle through one of its ring bonds, 0 for a non-ring atom (sliced from the batch's host
        tensor on first access)."""
        return self._per_atom("ring_sizes")

    @property
    def ring_systems(self) -> Optional[List[int]]:
        """Per atom the label of its ring system - the lowest atom index in it -, -1 for a non-ring atom."""
        return self._per_atom("ring_systems")

    @property
    def scaffold_atoms(self) -> Optional[List[int]]:
        """The atoms of this record, ascending, that form its scaffold - ring, linker and doubly bonded exo atoms
        (`scaffold.py`: the package's OWN definition, NOT RDKit's MurckoScaffold); with `unique="framework"` the ring and
        linker atoms.  Empty for an acyclic molecule."""
        return self._measured.scaffold_atoms

    @property
    def scaffold_key(self) -> Optional[int]:
        """64 bits of the scaffold graph's canonical certificate (`canonical.py`), for grouping: equal scaffolds have equal
        keys; 0 for the empty scaffold and where `scaffold_status` says the graph has no canonical order."""
        return self._measured.scaffold_key

    @property
    def scaffold_status(self) -> Optional[int]:
        """The status word of the scaffold graph's canonical labelling (`canonical.describe_status`): 0, EMPTY for an
        acyclic molecule, or DEGREE / BUDGET - such a scaffold is not proven equal to anything and always stays."""
        return self._measured.scaffold_status

    @property
    def scaffold_smiles(self) -> Optional[str]:
        """The canonical SMILES of the scaffold graph (`smiles.write_smiles` in its canonical order), "" for the empty
        scaffold, where the call also asked for `smiles`; None otherwise and where there is no canonical order."""
        return self._measured.scaffold_smiles

    @property
    def canonical_status(self) -> Optional[int]:
        """The status word of this molecule's canonical labelling (`canonical.describe_status`: 0, or EMPTY / DEGREE /
        BUDGET - the graph has no canonical order by the package's definition) when the call asked for `smiles`; None
        otherwise."""
        return self._measured.canonical_status

    @property
    def canonical_order(self) -> Optional[List[int]]:
        """The exact canonical atom order of the molecular graph (`canonical.canonical_order`: the package's own
        definition, not RDKit's canonical ranking): position k holds the index, in this record, of the atom of canonical
        rank k; isomorphic graphs relabelled this way are equal.  When the call asked for `smiles`; None otherwise, and
        where `canonical_status` is not 0.  Sliced from the batch's host tensor on first access."""
        o = self._measured.canonical_order
        if isinstance(o, tuple):
            o = self._measured.canonical_order = o[0][o[1], : o[2]].tolist()
        return o if self._measured.canonical_status == 0 else None

    @property
    def stereo_status(self) -> Optional[int]:
        """The status word of this molecule's stereo search (`canonical.describe_status`; its leaf count differs from the
        graph search's, so BUDGET may be set here alone) when the call asked for `smiles="isomeric"`; None otherwise."""
        return self._measured.stereo_status

    @property
    def stereo_order(self) -> Optional[List[int]]:
        """The atom order of the stereo identity (`stereo.stereo_order`): position k holds the index, in this record, of
        the atom of rank k.  The graph relabelled this way equals the one relabelled by `canonical_order`; among the
        orders of which that is true, this one has the smallest stereo vector.  With `smiles="isomeric"`; None
        otherwise, and where `stereo_status` is not 0."""
        if self._measured.stereo_status != 0:
            return None
        return [a for a in self._measured.stereo_order if a >= 0]

    @property
    def stereo_descriptors(self) -> Optional[List[int]]:
        """Per atom, in this record's order and RELATIVE TO IT, 4 tet + db (`stereo.own_order_descriptors`): tet 1 / 2 is
        the handedness of the atom's neighbours in ascending index (the implicit H last) in the returned coordinates, db
        1 cis / 2 trans of the lowest-indexed substituents of a double bond's ends, stored at the end of larger index; 0 =
        no candidate or undefined.  The package's OWN definition (`stereo.py`), not CIP labels.  With
        `smiles="isomeric"`; None otherwise, and where `stereo_status` is not 0."""
        order = self.stereo_order
        if order is None:
            return None
        d = self._measured.stereo_descriptors
        if d[1] is None:
            from .stereo import own_order_descriptors
            d[1] = own_order_descriptors(order, d[0][: len(order)], self.bond_orders)
        return d[1]

    @property
    def n_stereo_defined(self) -> Optional[int]:
        """The defined descriptors - tetrahedral centres plus double bonds - of the returned coordinates
        (`smiles="isomeric"`; None otherwise)."""
        return self._measured.n_stereo_defined

    @property
    def n_stereo_undefined(self) -> Optional[int]:
        """The candidates left undefined: a centre flatter than |chi| = 0.1, a double bond twisted to |cos| < 0.1 or with
        inconsistent sides (`smiles="isomeric"`; None otherwise)."""
        return self._measured.n_stereo_undefined

    @property
    def n_stereo_unmarked(self) -> Optional[int]:
        """The defined double bonds the isomeric `smiles` could not give a mark of their own (`smiles.py`, "Isomeric";
        0 in all but contrived ring systems); None where `smiles` is not isomeric."""
        return self._unmarked if self.smiles is not None else None

    @property
    def smiles(self) -> Optional[str]:
        """The canonical SMILES of the heavy-atom graph (`smiles.write_smiles` on the graph in `canonical_order`: valid
        OpenSMILES by the package's OWN definition - NOT RDKit's canonical SMILES; no charges), built
        on first access, when the call asked for `smiles`; None otherwise, and where `canonical_status` is not 0.  Equal
        strings: the same graph.  Its "[nH]" may sit on the other N than the hydrogen `add_hydrogens` placed.
        With `smiles="isomeric"` and a `stereo_status` of 0 the string is isomeric - the graph in `stereo_order` with the
        marks of its stereo vector: equal strings then mean the same stereoisomer by `stereo.py`'s definition."""
        if self._smiles is None and self.canonical_order is not None:
            self._smiles = self.to_smiles(canonical=True)
        return self._smiles

    @property
    def electrostatic_tanimoto(self) -> Optional[float]:
        """Tanimoto of the Coulomb overlap of this molecule's Gaussian-smeared partial charges - heavy atoms and placed
        hydrogens, as posed - with the reference's, in [-1/3, 1] (`electrostatics.py`: the package's own definition - NOT
        RDKit's Gasteiger charges, not a vendor's electrostatic score) when the call asked for `electrostatic_scores` or
        `min_electrostatic_tanimoto`; NaN where posing failed or the molecule holds an element without charge parameters;
        None otherwise."""
        return self._measured.electrostatic_tanimoto

    @property
    def partial_charges(self) -> Optional[torch.Tensor]:
        """[n] fp32 (CPU): the partial charge of each heavy atom by the electronegativity equalisation of
        `electrostatics.py` (the package's own definition, NOT RDKit's Gasteiger charges; its hydrogens' charges are in
        `hydrogen_charges`; a view into the batch's host tensor, sliced on first access) when the call asked for
        `partial_charges`; NaN throughout where the molecule holds an element without parameters; None otherwise."""
        q = self._measured.partial_charges
        if isinstance(q, tuple):
            q = self._measured.partial_charges = q[0][q[1], : q[2]]
        return q

    @property
    def hydrogen_charges(self) -> Optional[torch.Tensor]:
        """[n] fp32 (CPU): the partial charge of EACH hydrogen of that heavy atom, 0 where it has none - with
        `partial_charges` and the hydrogen counts the molecule's charges sum to 0; None where `partial_charges` is None."""
        q = self._measured.hydrogen_charges
        if isinstance(q, tuple):
            q = self._measured.hydrogen_charges = q[0][q[1], : q[2]]
        return q

    @property
    def atoms_removed(self) -> Optional[int]:
        """How many atoms of the generated graph lay outside its largest fragment and were removed, when the call asked
        to `standardize` (`standardize.py`: the package's own definition); None otherwise."""
        return self._measured.atoms_removed

    @property
    def n_fragments(self) -> Optional[int]:
        """How many connected fragments the generated graph had before the largest was kept; None without `standardize`."""
        return self._measured.n_fragments

    @property
    def atom_map(self) -> Optional[List[int]]:
        """For each atom of this record its index in the graph as generated (the GCN's atom order, the rows of
        `last_batch["elements"]`); None without `standardize`."""
        return self._measured.atom_map

    @property
    def kekule_bond_orders(self) -> Optional[torch.Tensor]:
        """[n,n] int8 (CPU): `bond_orders` with every aromatic bond written as 1 or 2 by the Kekule search of
        `standardize.py` (the package's own definition, NOT RDKit's Kekulize; a view into the batch's host tensor, sliced
        on first access); all zero for a record the standardisation found invalid; None without `standardize`."""
        k = self._measured.kekule_bond_orders
        if isinstance(k, tuple):
            k = self._measured.kekule_bond_orders = k[0][k[1], : k[2], : k[2]]
        return k

    @property
    def hydrogen_coords(self) -> Optional[torch.Tensor]:
        """[nH,3] fp32 (CPU): the explicit hydrogens of the returned coordinates, in ascending order of their heavy atom,
        when the call asked for `add_hydrogens` (`hydrogens.py`: the package's own definition - NOT RDKit's AddHs; a view
        into the batch's host tensor, sliced on first access); None otherwise, and where the molecule has a non-finite
        coordinate."""
        h = self._measured.hydrogen_coords
        if isinstance(h, tuple):
            h = self._measured.hydrogen_coords = h[0][h[1], : h[2]]
        return h

    @property
    def hydrogen_parents(self) -> Optional[List[int]]:
        """The heavy atom each hydrogen of `hydrogen_coords` is bonded to, ascending; None where that is None."""
        return self._measured.hydrogen_parents

    @property
    def hydrogens_unplaced(self) -> Optional[int]:
        """Hydrogens the count rule of `hydrogens.py` gives to atoms in a situation its placement has no direction for
        (they are not in `hydrogen_coords`; 0 for an ordinary molecule); None where `hydrogen_coords` is None."""
        return self._measured.hydrogens_unplaced

    @property
    def receptor_hydrogen_clashes(self) -> Optional[int]:
        """Hydrogens of `hydrogen_coords` overlapping a receptor heavy atom by >= 0.6 A at the Bondi radius 1.20 A, when
        the call asked for `add_hydrogens` and passed a `receptor`; None otherwise, and where posing failed.
        `receptor_clashes` keeps counting the heavy atoms alone."""
        return self._measured.receptor_hydrogen_clashes

    @property
    def interaction_score_before(self) -> Optional[float]:
        """`interaction_score` of the pose the pose optimisation of a call with `optimise_pose` started from
        (`interaction_score` itself describes the returned coordinates; the same `n_rot` divides both); None in a call
        without it, and where posing failed."""
        return self._measured.interaction_score_before

    @property
    def pose_optimisation_rmsd(self) -> Optional[float]:
        """How far, as a heavy-atom RMSD in A, the pose optimisation moved this molecule as a rigid body towards a lower
        interaction score (`interactions.optimise_pose`: the package's own procedure - not a docking run, not AutoDock
        Vina's local optimisation); 0.0 where it did not move.  None in a call without `optimise_pose`, and where posing
        failed."""
        return self._measured.pose_optimisation_rmsd

    @property
    def pose_trials_kept(self) -> Optional[int]:
        """The trials of the pose optimisation that were kept; None in a call without `optimise_pose`, and where posing
        failed."""
        return self._measured.pose_trials_kept

    @property
    def pose_torsions(self) -> Optional[int]:
        """The rotatable bonds the flexible pose optimisation used (`interactions.optimise_pose_flexible`: at most 16, in
        ascending order of their ends); None in a call without `optimise_pose="flexible"`, and where posing failed."""
        return self._measured.pose_torsions

    @property
    def pose_torsion_angles(self) -> Optional[List[float]]:
        """Per used torsion the angle in rad the flexible pose optimisation turned its moving side by, right-handed about
        the bond; None in a call without `optimise_pose="flexible"`, and where posing failed."""
        return self._measured.pose_torsion_angles

    @property
    def pose_conformer_rmsd(self) -> Optional[float]:
        """How far, as a heavy-atom RMSD in A, the flexible pose optimisation changed the conformer itself (the rigid part
        of the move taken out): `pose` maps `x_relaxed` to the returned coordinates only up to this.  None in a call
        without `optimise_pose="flexible"`, and where posing failed."""
        return self._measured.pose_conformer_rmsd

    @property
    def intramolecular_clash_before(self) -> Optional[float]:
        """CLASH, the intramolecular guard of `interactions.optimise_pose_flexible` (A^2), of the conformer the walk
        started from; None in a call without `optimise_pose="flexible"`, and where posing failed."""
        return self._measured.intramolecular_clash_before

    @property
    def intramolecular_clash(self) -> Optional[float]:
        """CLASH of the returned coordinates; None in a call without `optimise_pose="flexible"`, and where posing failed."""
        return self._measured.intramolecular_clash

    @property
    def pose_starts(self) -> Optional[int]:
        """The starts per molecule the pose search walked (`interactions.search_pose`: the package's own bounded multi-start
        of its flexible walk, not a docking run); None in a call without `optimise_pose="search"`, and where posing
        failed."""
        return self._measured.pose_starts

    @property
    def pose_best_start(self) -> Optional[int]:
        """The start of the pose search whose walk ended lowest: 0 the pose as it came, 1.. a keyed start, -1 where no
        start had a finite objective; None in a call without `optimise_pose="search"`, and where posing failed."""
        return self._measured.pose_best_start

    @property
    def contact_groups(self) -> Optional[List[int]]:
        """The ids of the receptor groups - residues - this molecule's returned coordinates are in contact with, ascending
        (`contacts.py`: the package's own definition - NOT ProLIF, PLIP or SIFt output; heavy atoms only; no ionic, aromatic
        or metal kinds).  When the call asked for `interaction_scores="contacts"`; None otherwise and where posing failed."""
        return self._measured.contact_groups

    @property
    def contact_kinds(self) -> Optional[List[int]]:
        """Per entry of `contact_groups` the kind bits: 1 contact, 2 hydrophobic, 4 hydrogen bond with the molecule
        donating, 8 with the molecule accepting (`contacts.KIND_NAMES`); None where `contact_groups` is None."""
        return self._measured.contact_kinds

    @property
    def contact_atom_kinds(self) -> Optional[List[int]]:
        """Per atom of this molecule the OR of the kind bits of the contacts it takes part in; None where `contact_groups`
        is None."""
        return self._measured.contact_atom_kinds

    @property
    def contact_status(self) -> Optional[int]:
        """0 ok, 1 empty, 2 a non-finite coordinate, 3 overflow - more groups or receptor atoms in contact than the kernel
        holds; the last two leave no entries (`contacts.STATUS_NAMES`); None where `contact_groups` is None."""
        return self._measured.contact_status

    @property
    def residue_contacts(self) -> Optional[tuple]:
        """`contact_groups` / `contact_kinds` by name (`receptor_contacts`, the older property, is the steric pair of clash
        count and largest overlap): a tuple of (label, kind names), the label "{chain}:{resName}{resSeq}
        {iCode}" of the receptor's PDB records ("A:SER195"), the names of `contacts.KIND_NAMES`; None where `contact_groups`
        is None."""
        from . import contacts
        m = self._measured
        if m.contact_groups is None:
            return None
        return tuple((g if m.contact_labels is None else m.contact_labels[g], contacts.kind_names(k))
                     for g, k in zip(m.contact_groups, m.contact_kinds))

    @property
    def contact_recovery(self) -> Optional[float]:
        """How much of the reference conformer's contact fingerprint this molecule keeps: the (group, kind) bits they share
        over the reference's, on hydrophobic contacts and hydrogen bonds (`contacts.DEFAULT_KINDS`); NaN where the reference
        has none.  None in a call without `interaction_scores="contacts"` or without a reference graph, and where posing
        failed."""
        return self._measured.contact_recovery

    @property
    def contact_tanimoto(self) -> Optional[float]:
        """The shared (group, kind) bits over the union of this molecule's and the reference conformer's; None where
        `contact_recovery` is None."""
        return self._measured.contact_tanimoto

    @property
    def contact_labels(self) -> Optional[tuple]:
        """The labels of the call's receptor groups, indexed by group id - what `residue_contacts` names the entries of
        `contact_groups` by; shared by the call's records.  None where `contact_groups` is None."""
        return self._measured.contact_labels

    @property
    def contact_reference(self) -> Optional[tuple]:
        """(groups, kinds, kinds mask) of the reference conformer's contact fingerprint `contact_recovery` compares with;
        shared by the call's records.  None where `contact_recovery` is None."""
        return self._measured.contact_reference

    def _contacts_against_reference(self, which: int) -> Optional[tuple]:
        from . import contacts
        m = self._measured
        if m.contact_groups is None or m.contact_reference is None:
            return None
        ref_groups, ref_kinds, mask = m.contact_reference
        found = contacts.compare_entries(m.contact_groups, m.contact_kinds, ref_groups, ref_kinds, mask)[which]
        return tuple((g if m.contact_labels is None else m.contact_labels[g], contacts.kind_names(k)) for g, k in found)

    @property
    def contacts_recovered(self) -> Optional[tuple]:
        """The reference conformer's contacts this molecule also makes, as (label, kind names) like `residue_contacts`;
        None where `contact_recovery` is None."""
        return self._contacts_against_reference(0)

    @property
    def contacts_missed(self) -> Optional[tuple]:
        """The reference conformer's contacts this molecule does not make; None where `contact_recovery` is None."""
        return self._contacts_against_reference(1)

    @property
    def relief_rmsd(self) -> Optional[float]:
        """How far, as a heavy-atom RMSD in A, the clash relief moved this molecule as a rigid body out of its contacts
        with the call's receptor (`receptor.relieve_clashes`: the package's own procedure - not a docking score, not a
        force field); 0.0 where it did not move.  None in a call without `relieve_clashes`, and where posing failed."""
        return self._measured.relief_rmsd

    @property
    def receptor_clashes_before(self) -> Optional[int]:
        """`receptor_clashes` of the pose before the clash relief of a call with `relieve_clashes` (`receptor_clashes`
        itself describes the returned coordinates); None in a call without it, and where posing failed."""
        return self._measured.receptor_clashes_before

    @property
    def pharmacophore_tanimoto(self) -> Optional[float]:
        """Tanimoto of the Gaussian overlap of this molecule's pharmacophore features, as posed, with the reference's
        (`pharmacophore.py`: the package's own feature definition - NOT RDKit's feature factory, not a vendor's colour
        score) when the call asked for `pharmacophore_scores` or `min_pharmacophore_tanimoto`; None otherwise, and where
        posing failed."""
        return self._measured.pharmacophore_tanimoto

    @property
    def pharmacophore_matches(self) -> Optional[int]:
        """How many of the reference's pharmacophore features have a feature of this molecule of the same type within
        1.5 A, when the call asked for `pharmacophore_scores`; None otherwise, and where posing failed."""
        return self._measured.pharmacophore_matches

    @property
    def strain_before(self) -> Optional[float]:
        """The energy of the package's own restrained valence force field (`geometry.py`: NOT MMFF94; kcal/mol by its
        constants) at the coordinates the sampler produced, when the call relaxed (`relax_geometry`); None otherwise."""
        return self._measured.strain_before

    @property
    def strain_after(self) -> Optional[float]:
        """That energy at the returned, relaxed coordinates (restraint included; <= `strain_before`) when the call
        relaxed (`relax_geometry`); None otherwise."""
        return self._measured.strain_after

    @property
    def atoms_outside(self) -> Optional[int]:
        """How many heavy atoms of the returned pose lie outside the call's `reference_shape` mesh (generalized winding
        number |w| <= 0.5) when the call posed the molecule into it (`overlay=True`); None otherwise, and where posing
        failed."""
        return self._measured.atoms_outside

    @property
    def chemical_tanimoto(self) -> Optional[float]:
        """Tanimoto of this molecule's chemical fingerprint with the reference graph's (`fingerprint.py`: radius 2, 2 048
        bits, the package's own definition - NOT RDKit's Morgan fingerprint) when the call asked for `chemical_scores` or
        `max_chemical_tanimoto`; None otherwise."""
        return self._measured.chemical_tanimoto

    @property
    def graph_key(self) -> Optional[int]:
        """The unsigned 64-bit identity key of the molecular graph (`fingerprint.graph_fingerprints`) when the call asked
        for `chemical_scores` or `unique`; None otherwise.  Isomorphic graphs have equal keys; unequal graphs with equal
        keys are possible (colour refinement's blind spots, hash collisions)."""
        return self._measured.graph_key

    @property
    def receptor_contacts(self) -> Optional[Tuple[int, float]]:
        """(receptor_clashes, receptor_max_overlap), or None."""
        c = self._measured.receptor_clashes
        return None if c is None else (c, self._measured.receptor_max_overlap)

    @property
    def receptor_clashes(self) -> Optional[int]:
        """Heavy atoms overlapping a receptor heavy atom by >= 0.6 A (`receptor.CLASH_OVERLAP`) when the call passed a
        `receptor`; None otherwise, and where posing failed (the molecule is not in the receptor's frame)."""
        return self._measured.receptor_clashes

    @property
    def receptor_max_overlap(self) -> Optional[float]:
        """The largest overlap (r_i + r_j) - d_ij of a heavy atom with a receptor heavy atom, in A (negative when nothing
        touches), when the call passed a `receptor`; None otherwise, and where posing failed."""
        return self._measured.receptor_max_overlap

    @property
    def overlay_tanimoto(self) -> Optional[float]:
        """Shape Tanimoto of the pose onto the reference (`overlay=True`: the returned coordinates ARE that pose; NaN
        where posing failed and the generated coordinates were kept); None when the call did not pose."""
        return self._measured.overlay_tanimoto

    @property
    def pose(self) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """(rotation [3,3], translation [3]) with returned = generated @ rotation + translation (rotation proper, det +1)
        when the call posed the molecule (`overlay=True`); None otherwise, and where posing failed."""
        p = self._measured.pose
        return None if p is None else (p[:9].reshape(3, 3), p[9:])

    @property
    def shape_tanimoto(self) -> Optional[float]:
        """Gaussian-volume shape Tanimoto of these coordinates against the call's reference - what
        `evaluate_samples(reference, [mol])` reports - when the call scored (`shape_scores`, `top_k`,
        `min_shape_tanimoto`); None otherwise."""
        return self._measured.shape_tanimoto

    @property
    def sample_id(self) -> Optional[int]:
        """Global sample index of this molecule in its generation call (with `sample_seed`: what its noise and size are
        keyed on, so `edm_tensors(..., sample_ids=[sample_id])` regenerates it); None for a record built by hand."""
        return self._sid

    @property
    def batch_row(self) -> int:
        """The row of its call's result tensors that a record built by `molecules_from_tensors` views - what indexes the
        device tensors of the same batch (posed coordinates, fingerprints); -1 for a record built by hand."""
        return self._b

    @property
    def atomic_numbers(self) -> List[int]:
        if self._z is None:
            self._z = self._batch.elements[self._b, : self._batch.n[self._b]].tolist()
        return self._z

    @property
    def coords(self) -> torch.Tensor:
        if self._coords is None:
            self._coords = self._batch.x[self._b, : self._batch.n[self._b]]
        return self._coords

    @property
    def bond_orders(self) -> torch.Tensor:
        if self._bonds is None:
            n = self._batch.n[self._b]
            self._bonds = self._batch.bonds[self._b, :n, :n]
        return self._bonds

    def __repr__(self) -> str:
        return f"GeneratedMolecule(n_atoms={self.GetNumAtoms()}, valid={self.valid})"

    def __eq__(self, other) -> bool:
        """Value equality (atoms, coordinates, bond orders, validity) - whether or not the records are views of a batch."""
        if not isinstance(other, GeneratedMolecule):
            return NotImplemented
        return (self.valid == other.valid and self.atomic_numbers == other.atomic_numbers
                and torch.equal(self.coords, other.coords) and torch.equal(self.bond_orders, other.bond_orders))

    __hash__ = None            # mutable value object, like the dataclass it replaced

    @property
    def symbols(self) -> List[str]:
        """Element symbols of the atoms (`config.ELEMENTS`: the atomic numbers already follow the generator's decoder)."""
        return [Z_TO_SYMBOL[z] for z in self.atomic_numbers]

    def GetNumAtoms(self) -> int:          # RDKit-like convenience
        return len(self._z) if self._z is not None else int(self._batch.n[self._b])

    def _hydrogens(self) -> Tuple[List[List[float]], List[int]]:
        """(coordinates, parents) of the record's hydrogens for the writers; ValueError where it carries none."""
        xyz, parents = self.hydrogen_coords, self.hydrogen_parents
        if xyz is None or parents is None:
            raise ValueError("this record carries no hydrogens: generate with add_hydrogens=True (a molecule with a "
                             "non-finite coordinate gets none)")
        return xyz.tolist(), list(parents)

    def _kekule_orders(self, hydrogen_parents: Optional[List[int]]) -> torch.Tensor:
        """The record's Kekule orders for the writer; ValueError where it carries none, where it has no Kekule form, and -
        with the parents of its placed hydrogens - where an atom's Kekule valence plus its hydrogens exceeds v0
        (`hydrogens.VALENCE`): the Kekule search and the hydrogen count are two definitions and can disagree."""
        orders = self.kekule_bond_orders
        if orders is None:
            raise ValueError("this record carries no Kekule form: generate with standardize=True")
        if bool(((orders == 0) & (self.bond_orders != 0)).any()):
            raise ValueError("this record has no Kekule form: its standardisation found it invalid")
        if hydrogen_parents is not None:
            from .hydrogens import VALENCE
            for a, z in enumerate(self.atomic_numbers):
                total = int(orders[a].sum()) + sum(1 for p in hydrogen_parents if p == a)
                if total > VALENCE.get(z, 0):
                    raise ValueError(f"atom {a} ({Z_TO_SYMBOL.get(z, z)}) has Kekule valence {int(orders[a].sum())} and "
                                     f"{total - int(orders[a].sum())} placed hydrogens, more than v0 = {VALENCE.get(z, 0)}: "
                                     "the Kekule form and the hydrogen count disagree on this atom")
        return orders

    def to_molblock(self, name: str = "generated", hydrogens: bool = False, kekulize: bool = False) -> str:
        """V2000 MOL block (heavy atoms, bond orders 1/2/3, aromatic = 4) - consumable by RDKit
        (`Chem.MolFromMolBlock`) or any other toolkit without going through this package.  `hydrogens=True`: the
        record's explicit hydrogens (`add_hydrogens`) follow the heavy atoms, each with a single bond to its parent;
        ValueError where the record carries none.  `kekulize=True`: the bonds are the record's `kekule_bond_orders`
        (`standardize`), orders 1/2/3 only - a structure, where a block with bond type 4 is a query; ValueError where the
        record carries none or has no Kekule form, and with `hydrogens=True` also where an atom's Kekule valence plus its
        placed hydrogens exceeds v0 (the message names the atom)."""
        n = len(self.atomic_numbers)
        orders = self.bond_orders
        if kekulize:
            orders = self._kekule_orders(self._hydrogens()[1] if hydrogens else None)
        bonds = [(i + 1, j + 1, int(orders[i, j])) for i in range(n) for j in range(i) if int(orders[i, j]) != 0]
        atoms = list(zip(self.symbols, self.coords.tolist()))
        if hydrogens:
            xyz, parents = self._hydrogens()
            atoms += [("H", c) for c in xyz]
            bonds += [(n + 1 + k, p + 1, 1) for k, p in enumerate(parents)]
        lines = [name, "  mlconfgen-mi355x", "", "%3d%3d  0  0  0  0  0  0  0  0999 V2000" % (len(atoms), len(bonds))]
        for s, c in atoms:
            lines.append("%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0" % (c[0], c[1], c[2], s))
        for i, j, o in bonds:
            lines.append("%3d%3d%3d  0" % (i, j, o))
        lines.append("M  END")
        return "\n".join(lines) + "\n"

    def to_smiles(self, canonical: bool = True, isomeric: Optional[bool] = None) -> str:
        """SMILES of the heavy-atom graph by `smiles.write_smiles` (the package's own writer: valid OpenSMILES, not RDKit's
        canonical SMILES).  `canonical=True`: the atoms in the record's `canonical_order` - the package's canonical
        string; ValueError, naming the status, where the record has no canonical order (a call without `smiles`, or a
        graph the labelling refused).  `canonical=False` always works: the atoms are written in the record's OWN order, so
        two records of one molecule may get different strings.
        `isomeric`: None - isomeric where the record has a stereo identity (`smiles="isomeric"`, `stereo_status` 0);
        False - never: the string `smiles=True` gives; True - ValueError where the record has none.  The canonical
        isomeric string is written in `stereo_order`, the other in the record's own order from `stereo_descriptors`."""
        from .smiles import write_smiles, write_smiles_counted
        z, bonds = self.atomic_numbers, torch.as_tensor(self.bond_orders)
        stereo_order = self.stereo_order if isomeric is not False else None
        if isomeric and stereo_order is None:
            from .canonical import describe_status
            status = self._measured.stereo_status
            raise ValueError("this record has no stereo identity: " + (
                'generate with smiles="isomeric"' if status is None else f"its search ended with {describe_status(status)}"))
        if stereo_order is not None:
            if not canonical:
                return write_smiles(z, bonds, self.stereo_descriptors)
            idx = torch.tensor(stereo_order, dtype=torch.long)
            text, self._unmarked = write_smiles_counted([z[a] for a in stereo_order],
                                                        bonds.index_select(0, idx).index_select(1, idx),
                                                        self._measured.stereo_descriptors[0][: len(stereo_order)])
            return text
        if not canonical:
            return write_smiles(z, bonds)
        order = self.canonical_order
        if order is None:
            from .canonical import describe_status
            status = self._measured.canonical_status
            raise ValueError("this record has no canonical order: " + (
                "generate with smiles=True" if status is None else f"its labelling ended with {describe_status(status)}")
                + "; to_smiles(canonical=False) writes the atoms in the record's own order")
        idx = torch.tensor(order, dtype=torch.long)
        return write_smiles([z[a] for a in order], bonds.index_select(0, idx).index_select(1, idx))

    def to_xyz_block(self, hydrogens: bool = False, charges: bool = False) -> str:
        """XYZ block of the heavy atoms; `hydrogens=True`: the record's explicit hydrogens (`add_hydrogens`) follow them;
        ValueError where the record carries none.  `charges=True`: a fifth column holds each atom's partial charge
        (`partial_charges`; a hydrogen's is its parent's `hydrogen_charges`), so with `hydrogens=True` the column sums to
        0 for a molecule all of whose hydrogens were placed; ValueError where the record carries no charges."""
        atoms = list(zip(self.symbols, self.coords.tolist()))
        column = None
        if charges:
            q, qh = self.partial_charges, self.hydrogen_charges
            if q is None or qh is None:
                raise ValueError("this record carries no charges: generate with partial_charges=True")
            column = q.tolist()
        if hydrogens:
            xyz, parents = self._hydrogens()
            atoms += [("H", c) for c in xyz]
            if charges:
                column += [float(qh[p]) for p in parents]
        lines = [f"{len(atoms)}", ""]
        for k, (s, c) in enumerate(atoms):
            line = "%s %.9f %.9f %.9f" % (s, c[0], c[1], c[2])
            lines.append(line if column is None else line + " %.6f" % column[k])
        return "\n".join(lines) + "\n"


def _order_tensor(order, n_host: List[int], dimension: int) -> torch.Tensor:
    """[B,42] int32 (CPU) from per-molecule permutations, CHECKED: row b's first n_b entries must be a permutation of
    0..n_b-1 (the argument of `Chem.RenumberAtoms`, mol_utils.py:124); None rows = generation order."""
    if torch.is_tensor(order):
        rows = order.detach().to("cpu", torch.int64).reshape(len(n_host), -1).tolist()
    else:
        rows = [None if r is None else [int(v) for v in r] for r in order]
    if len(rows) != len(n_host):
        raise ValueError(f"order has {len(rows)} rows for a batch of {len(n_host)} molecules")
    out = torch.arange(dimension, dtype=torch.int32).repeat(len(n_host), 1)
    for b, (r, n) in enumerate(zip(rows, n_host)):
        if r is None:
            continue
        if len(r) < n or sorted(r[:n]) != list(range(n)):
            raise ValueError(f"order[{b}] is not a permutation of the molecule's {n} atoms")
        out[b, :n] = torch.tensor(r[:n], dtype=torch.int32)
    return out


def _conn_tensor(conn, n_host: List[int], dimension: int) -> torch.Tensor:
    """[B,42,42] uint8 (CPU) from per-molecule [n,n] (or padded) {0,1} connectivities in generation order."""
    if torch.is_tensor(conn) and conn.dim() == 3 and tuple(conn.shape[1:]) == (dimension, dimension):
        return (conn.detach().to("cpu") != 0).to(torch.uint8).contiguous()
    if len(conn) != len(n_host):
        raise ValueError(f"connectivity has {len(conn)} entries for a batch of {len(n_host)} molecules")
    out = torch.zeros(len(n_host), dimension, dimension, dtype=torch.uint8)
    for b, (c, n) in enumerate(zip(conn, n_host)):
        c = torch.as_tensor(c)
        if c.dim() != 2 or c.shape[0] < n or c.shape[1] < n:
            raise ValueError(f"connectivity[{b}] must be at least [{n},{n}]")
        c = c[:n, :n] != 0
        if not bool(torch.equal(c, c.t())):
            raise ValueError(f"connectivity[{b}] is not symmetric")
        out[b, :n, :n] = c.to(torch.uint8)
    return out


def prepare_adj_mat_seer_input_hip(x: torch.Tensor, h: torch.Tensor, n_nodes: torch.Tensor,
                                   dimension: int = DIMENSION, order=None, connectivity=None, with_coords: bool = False,
                                   class_z=None):
    """elements[B,42] i64, dist_mat[B,42,42] (+I, zero padded), adj_mat[B,42,42] {0,1} (+I) - the tensors
    `prepare_adj_mat_seer_input` (mol_utils.py:146-194) builds, by ONE HIP launch (`mcg_handoff_elements`).
    `class_z`: atomic number of each of the 8 atom classes (`elements.class_z_from_decoder` of the caller's
    `atom_decoder`, mol_utils.py:41-45); None = the default decoder.  An unsupported element raises before any launch.
    `order` (per-molecule permutations: position p holds generation atom order[b][p] - the reference's canonical SMILES
    order, `canonicalise` :110-126) and `connectivity` (per-molecule {0,1} matrices in GENERATION order - RDKit's
    `DetermineConnectivity`, :117) are the two RDKit-owned decisions; None = generation order / covalent-radius rule.
    `with_coords`: also return x[B,N,3] in the order of the GCN input (the reference's `canonicalised_samples`)."""
    from . import _lib
    if dimension != DIMENSION:
        raise ValueError("the hand-off kernel is specialised for DIMENSION = 42")
    B, N, _ = x.shape
    dev = x.device
    el = torch.empty(B, dimension, dtype=torch.long, device=dev)
    dm = torch.empty(B, dimension, dimension, dtype=torch.float32, device=dev)
    am = torch.empty(B, dimension, dimension, dtype=torch.float32, device=dev)
    xo = torch.empty(B, N, 3, dtype=torch.float32, device=dev) if with_coords else None
    if B == 0:
        return (el, dm, am, xo) if with_coords else (el, dm, am)
    nn = n_nodes.to(dev, torch.int32).contiguous()
    od = cd = None
    if order is not None or connectivity is not None:
        n_host = [int(v) for v in n_nodes.detach().to("cpu").reshape(-1).tolist()]
        if order is not None:
            od = _order_tensor(order, n_host, dimension).to(dev)
        if connectivity is not None:
            cd = _conn_tensor(connectivity, n_host, dimension).to(dev)
    cz = None
    if class_z is not None:
        if len(class_z) != N_ATOM_CLASSES:
            raise ValueError(f"class_z must hold {N_ATOM_CLASSES} atomic numbers, got {len(class_z)}")
        cz = (ctypes.c_int32 * N_ATOM_CLASSES)(*[int(z) for z in class_z])
    _lib.check(_lib.lib().mcg_handoff_elements(_lib.dptr(x.contiguous()), _lib.dptr(h.to(torch.float32).contiguous()),
                                               _lib.dptr(nn), B, N, _COV_FACTOR, _lib.dptr(od), _lib.dptr(cd), _lib.dptr(el),
                                               _lib.dptr(dm), _lib.dptr(am), _lib.dptr(xo), None, cz,
                                               _lib.current_stream_ptr(dev)), "mcg_handoff_elements")
    return (el, dm, am, xo) if with_coords else (el, dm, am)


def bond_writeback_hip(bond: torch.Tensor, elements: torch.Tensor, n_nodes: torch.Tensor
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(bond_sym [B,42,42] int8, valid_proxy [B] bool) by ONE HIP launch (`mcg_bond_writeback`): the strict lower
    triangle of the GCN's bond argmax mirrored (`redefine_bonds`, mol_utils.py:210-211) and the valence /
    single-fragment pre-filter that stands in for `standardize_mol(...) is not None` (a labelled proxy)."""
    from . import _lib
    B = int(bond.shape[0])
    dev = bond.device
    sym = torch.empty(B, DIMENSION, DIMENSION, dtype=torch.int8, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    if B == 0:
        return sym, valid.bool()
    nn = n_nodes.to(dev, torch.int32).contiguous()
    _lib.check(_lib.lib().mcg_bond_writeback(_lib.dptr(bond.to(torch.int8).contiguous()), _lib.dptr(elements.contiguous()),
                                             _lib.dptr(nn), B, _lib.dptr(sym), _lib.dptr(valid),
                                             _lib.current_stream_ptr(dev)), "mcg_bond_writeback")
    return sym, valid.bool()


def molecules_from_tensors(x: torch.Tensor, elements: torch.Tensor, bond_sym: torch.Tensor, n_nodes: torch.Tensor,
                           valid: torch.Tensor, sample_ids: Optional[Sequence[int]] = None,
                           shape_tanimoto: Optional[torch.Tensor] = None, overlay_tanimoto: Optional[torch.Tensor] = None,
                           pose: Optional[torch.Tensor] = None, receptor_clashes: Optional[torch.Tensor] = None,
                           receptor_max_overlap: Optional[torch.Tensor] = None,
                           chemical_tanimoto: Optional[torch.Tensor] = None,
                           graph_key: Optional[torch.Tensor] = None,
                           atoms_outside: Optional[torch.Tensor] = None, strain_before: Optional[torch.Tensor] = None,
                           strain_after: Optional[torch.Tensor] = None,
                           pharmacophore_tanimoto: Optional[torch.Tensor] = None,
                           pharmacophore_matches: Optional[torch.Tensor] = None,
                           relief_rmsd: Optional[torch.Tensor] = None,
                           receptor_clashes_before: Optional[torch.Tensor] = None,
                           hydrogen_coords: Optional[torch.Tensor] = None,
                           hydrogen_parents: Optional[torch.Tensor] = None,
                           hydrogens_unplaced: Optional[torch.Tensor] = None,
                           receptor_hydrogen_clashes: Optional[torch.Tensor] = None,
                           atoms_removed: Optional[torch.Tensor] = None, n_fragments: Optional[torch.Tensor] = None,
                           atom_map: Optional[torch.Tensor] = None,
                           kekule_bond_orders: Optional[torch.Tensor] = None,
                           electrostatic_tanimoto: Optional[torch.Tensor] = None,
                           partial_charges: Optional[torch.Tensor] = None,
                           hydrogen_charges: Optional[torch.Tensor] = None,
                           canonical_order: Optional[torch.Tensor] = None,
                           canonical_status: Optional[torch.Tensor] = None,
                           substructure_counts: Optional[torch.Tensor] = None,
                           substructure_status: Optional[torch.Tensor] = None,
                           substructure_first: Optional[torch.Tensor] = None,
                           substructure_patterns: Optional[tuple] = None,
                           interaction_score: Optional[torch.Tensor] = None,
                           interaction_terms: Optional[torch.Tensor] = None,
                           receptor_hbonds: Optional[torch.Tensor] = None,
                           interaction_atom_scores: Optional[torch.Tensor] = None,
                           interaction_score_before: Optional[torch.Tensor] = None,
                           pose_optimisation_rmsd: Optional[torch.Tensor] = None,
                           pose_trials_kept: Optional[torch.Tensor] = None,
                           pose_torsions: Optional[torch.Tensor] = None,
                           pose_torsion_angles: Optional[torch.Tensor] = None,
                           pose_conformer_rmsd: Optional[torch.Tensor] = None,
                           intramolecular_clash_before: Optional[torch.Tensor] = None,
                           intramolecular_clash: Optional[torch.Tensor] = None,
                           pose_starts: Optional[torch.Tensor] = None, pose_best_start: Optional[torch.Tensor] = None,
                           contact_groups: Optional[torch.Tensor] = None, contact_kinds: Optional[torch.Tensor] = None,
                           contact_atom_kinds: Optional[torch.Tensor] = None,
                           contact_status: Optional[torch.Tensor] = None, contact_recovery: Optional[torch.Tensor] = None,
                           contact_tanimoto: Optional[torch.Tensor] = None, contact_labels: Optional[tuple] = None,
                           contact_reference: Optional[tuple] = None,
                           stereo_order: Optional[torch.Tensor] = None, stereo_status: Optional[torch.Tensor] = None,
                           stereo_descriptors: Optional[torch.Tensor] = None,
                           n_stereo_defined: Optional[torch.Tensor] = None,
                           n_stereo_undefined: Optional[torch.Tensor] = None,
                           n_rings: Optional[torch.Tensor] = None, n_ring_systems: Optional[torch.Tensor] = None,
                           min_ring_size: Optional[torch.Tensor] = None, max_ring_size: Optional[torch.Tensor] = None,
                           ring_sizes: Optional[torch.Tensor] = None, ring_systems: Optional[torch.Tensor] = None,
                           scaffold_atoms: Optional[torch.Tensor] = None, scaffold_key: Optional[torch.Tensor] = None,
                           scaffold_status: Optional[torch.Tensor] = None,
                           scaffold_smiles: Optional[List[Optional[str]]] = None) -> List[GeneratedMolecule]:
    """Host pass over (already gathered) result tensors: ONE D2H copy per tensor, then one lazy record per molecule
    (no per-molecule slicing or cloning here: `GeneratedMolecule._view`).  `sample_ids[b]`: the sample id of row b
    (default: b, the row IS the sample index).  `shape_tanimoto[b]`: row b's shape score (None: unscored records).
    `overlay_tanimoto[b]` / `pose[b]` (rotation row-major, then translation: [B,12], NaN where posing failed): row b's
    pose onto the reference (None: records of a call that did not pose).  `receptor_clashes[b]` / `receptor_max_overlap[b]`:
    row b's receptor contacts (a negative clash count: not measured, the record gets None; None: a call without a
    receptor).  `chemical_tanimoto[b]` (fp32) / `graph_key[b]` (int64 holding the unsigned bit pattern): row b's chemical
    similarity to the reference and graph identity key (either may be None: not asked for).  `atoms_outside[b]`: row b's
    atoms outside the call's mesh (negative: its pose failed, the record gets None; None: a call without a mesh).
    `strain_before[b]` / `strain_after[b]`: row b's force-field energy before and after the relaxation of a call with
    `relax_geometry` (both or neither; None: a call that did not relax).  `pharmacophore_tanimoto[b]` /
    `pharmacophore_matches[b]`: row b's pharmacophore overlap with the reference and matched reference features (negative
    matches: not measured, the record gets None for both; None: a call without `pharmacophore_scores`).
    `relief_rmsd[b]` / `receptor_clashes_before[b]`: how far the clash relief moved row b and its clashes before it (a
    negative count: its pose failed, the record gets None for both; None: a call without `relieve_clashes`).
    `hydrogen_coords[b]` [H,3] / `hydrogen_parents[b]` [H] (-1 beyond the row's count) / `hydrogens_unplaced[b]`: row b's
    explicit hydrogens as `hydrogens.add_hydrogens` returns them (all three or none; a negative unplaced count: the row had
    a non-finite coordinate, the record gets None for all three; None: a call without `add_hydrogens`).
    `receptor_hydrogen_clashes[b]`: row b's hydrogens clashing with the receptor (negative: its pose failed, None).
    `atoms_removed[b]` / `n_fragments[b]` / `atom_map[b]` [W] (-1 beyond the row's atoms) / `kekule_bond_orders[b]` [W,W]:
    row b's standardisation as `standardize.standardize_graphs` returns it (all four or none; None: a call without
    `standardize`).  `electrostatic_tanimoto[b]`: row b's electrostatic similarity to the reference (None: a call without
    `electrostatic_scores`); `partial_charges[b]` [W] / `hydrogen_charges[b]` [W]: row b's partial charges as
    `electrostatics.partial_charges` returns them, +inf at and beyond the row's atoms (both or neither; None: a call
    without `partial_charges`).  `canonical_order[b]` [W] int32 (-1 beyond the row's atoms) / `canonical_status[b]`: row b's
    canonical labelling as `canonical.canonical_order` returns it (both or neither; None: a call without `smiles`).
    `substructure_counts[b]` [P] / `substructure_status[b]` [P] / `substructure_first[b]` [P,M] with the P patterns
    `substructure_patterns`: row b's matches as `substructure.match_substructures` returns them (all four or none).
    `interaction_score[b]` / `interaction_terms[b]` [6] / `receptor_hbonds[b]` / `interaction_atom_scores[b]` [W] (+inf at
    and beyond the row's atoms): row b's receptor interactions as `postprocess.interactions` spells them (all four or
    none; negative hbonds: its pose failed, the record gets None for all four; None: a call without `interaction_scores`).
    `interaction_score_before[b]` / `pose_optimisation_rmsd[b]` / `pose_trials_kept[b]`: row b's pose optimisation as
    `postprocess.optimise_rows` spells it (negative trials kept: its pose failed, the record gets None for all three;
    None: a call without `optimise_pose`).  `pose_torsions[b]` / `pose_torsion_angles[b]` [16] / `pose_conformer_rmsd[b]` /
    `intramolecular_clash_before[b]` / `intramolecular_clash[b]`: what `optimise_pose="flexible"` adds (all five or none).
    `pose_starts[b]` / `pose_best_start[b]`: what `optimise_pose="search"` adds beside them (both or neither).
    `contact_status[b]` / `contact_groups[b]` [256] / `contact_kinds[b]` [256] / `contact_atom_kinds[b]` [W] / `contact_recovery[b]`
    / `contact_tanimoto[b]` with the shared `contact_labels` and `contact_reference`: row b's receptor contacts as
    `postprocess.contacts` spells them (a negative status: its pose failed, the record gets None throughout; None: a call
    without `interaction_scores="contacts"`; the two comparison values only where the call has a reference fingerprint).
    `stereo_order[b]` [W] / `stereo_status[b]` / `stereo_descriptors[b]` [W] int8 / `n_stereo_defined[b]` /
    `n_stereo_undefined[b]`: row b's stereo identity as `stereo.stereo_order` returns it - `stereo_descriptors` is its
    `stereo`, v in canonical position order; the counts are defined tetrahedral + defined double bonds, and the undefined
    candidates (all five or none; None: a call without `smiles="isomeric"`).
    `n_rings[b]` ... `scaffold_status[b]` and the host list `scaffold_smiles`: row b's rings and scaffold as
    `scaffold.record_fields` spells them (all nine, the strings only with `smiles`; None: a call without
    `unique="scaffold"` / `"framework"`).
    The value keywords are the fields of `Measured`
    and go to `measured_from_tensors`; a call with no ids and no values builds the views and nothing else."""
    batch = _HostBatch(x.cpu(), elements.cpu(), bond_sym.cpu(), n_nodes.cpu().tolist())
    view = GeneratedMolecule._view
    values = dict(shape_tanimoto=shape_tanimoto, overlay_tanimoto=overlay_tanimoto, pose=pose,
                  receptor_clashes=receptor_clashes, receptor_max_overlap=receptor_max_overlap,
                  atoms_outside=atoms_outside, chemical_tanimoto=chemical_tanimoto, graph_key=graph_key,
                  strain_before=strain_before, strain_after=strain_after,
                  pharmacophore_tanimoto=pharmacophore_tanimoto, pharmacophore_matches=pharmacophore_matches,
                  relief_rmsd=relief_rmsd, receptor_clashes_before=receptor_clashes_before,
                  hydrogen_coords=hydrogen_coords, hydrogen_parents=hydrogen_parents,
                  hydrogens_unplaced=hydrogens_unplaced, receptor_hydrogen_clashes=receptor_hydrogen_clashes,
                  atoms_removed=atoms_removed, n_fragments=n_fragments, atom_map=atom_map,
                  kekule_bond_orders=kekule_bond_orders, electrostatic_tanimoto=electrostatic_tanimoto,
                  partial_charges=partial_charges, hydrogen_charges=hydrogen_charges,
                  canonical_order=canonical_order, canonical_status=canonical_status,
                  substructure_counts=substructure_counts, substructure_status=substructure_status,
                  substructure_first=substructure_first, substructure_patterns=substructure_patterns,
                  interaction_score=interaction_score, interaction_terms=interaction_terms,
                  receptor_hbonds=receptor_hbonds, interaction_atom_scores=interaction_atom_scores,
                  interaction_score_before=interaction_score_before, pose_optimisation_rmsd=pose_optimisation_rmsd,
                  pose_trials_kept=pose_trials_kept, pose_torsions=pose_torsions,
                  pose_torsion_angles=pose_torsion_angles, pose_conformer_rmsd=pose_conformer_rmsd,
                  intramolecular_clash_before=intramolecular_clash_before, intramolecular_clash=intramolecular_clash,
                  pose_starts=pose_starts, pose_best_start=pose_best_start, contact_groups=contact_groups,
                  contact_kinds=contact_kinds, contact_atom_kinds=contact_atom_kinds, contact_status=contact_status,
                  contact_recovery=contact_recovery, contact_tanimoto=contact_tanimoto, contact_labels=contact_labels,
                  contact_reference=contact_reference, stereo_order=stereo_order, stereo_status=stereo_status,
                  stereo_descriptors=stereo_descriptors, n_stereo_defined=n_stereo_defined,
                  n_stereo_undefined=n_stereo_undefined, n_rings=n_rings, n_ring_systems=n_ring_systems,
                  min_ring_size=min_ring_size, max_ring_size=max_ring_size, ring_sizes=ring_sizes,
                  ring_systems=ring_systems, scaffold_atoms=scaffold_atoms, scaffold_key=scaffold_key,
                  scaffold_status=scaffold_status, scaffold_smiles=scaffold_smiles)
    if sample_ids is None and all(v is None for v in values.values()):
        return [view(batch, b, bool(v)) for b, v in enumerate(valid.cpu().tolist())]
    flags = valid.cpu().tolist()
    ids = list(range(len(flags))) if sample_ids is None else \
        [int(i) for i in (sample_ids.tolist() if torch.is_tensor(sample_ids) else sample_ids)]
    measured = measured_from_tensors(values, len(flags))
    return [view(batch, b, bool(v), ids[b], measured[b]) for b, v in enumerate(flags)]


def assemble_molecules(x: torch.Tensor, elements: torch.Tensor, bond: torch.Tensor, n_nodes: torch.Tensor
                       ) -> List[GeneratedMolecule]:
    """Bond write-back + validity proxy on the device (one launch), ONE D2H copy of (x, elements, bonds, valid),
    then a slicing-only host pass (the reference standardises one molecule at a time,
    conformer_generator.py:362-366)."""
    sym, valid = bond_writeback_hip(bond, elements, n_nodes)
    return molecules_from_tensors(x, elements, sym, n_nodes, valid)
