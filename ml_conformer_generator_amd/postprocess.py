"""What a generation call does between "the shard's result tensors / finished Mols exist" and "the list it returns":
the opt-in measuring, filtering and selecting of `MLConformerGenerator.generate_conformers*` (whose docstring says what
each option means).  The generator generates, parses its keywords into one `Request` (`parse_request`) and hands over.

Stages, in this order:
  BEFORE the gather, on the rank that generated the shard, one batched device call each (`measure_tensors` on the result
  tensors where no finisher runs, `measure_finished` on the finished Mols' heavy atoms where one does):
    1. pose onto the reference (`overlay`, refined with `refine_overlay`) - a conformer, or the solid of a
       `reference_shape` mesh, which also counts the posed atoms outside it; right behind it, with `relieve_clashes`, the
       posed rows are moved out of their receptor contacts (`relieve_rows`) and, with `optimise_pose`, directly behind that to
       where their interaction score is lower (`optimise_rows`), and everything below reads - and the call returns - the
       coordinates so moved;
    2. shape score of the RETURNED coordinates (`shape_scores`, or implied by a shape selection);
    3. receptor contacts of the returned coordinates (`receptor`).
  BEHIND the gather, on the rows a rank returns (`return_records` / `return_finished`):
    4. chemical fingerprints, graph keys and the Tanimoto to the reference's graph: one launch over the rows, one for
       the reference (`fingerprints`); beside it the pharmacophore overlap of the posed rows with the reference's
       features: one perceive and one score launch over the rows, one each for the reference (`pharmacophore`); and
       the explicit hydrogens of the returned coordinates: one perceive and one placement launch over the rows, plus -
       with a receptor - the receptor kernel over the hydrogens (`hydrogens`; records only: refused with a finisher);
       and the electrostatic step (`electrostatics`; records only): one perceive launch, the hydrogens placed once - the
       placement of `add_hydrogens` is reused when that is on too - one charge launch and, with `electrostatic_scores`,
       the overlap launches against the reference's charge points; and the canonical step (`identities`; `smiles`,
       `unique="exact"`, `exclude_graphs`): one `_canonical_order` launch over the rows - the excluded graphs were
       labelled by the same seam directly in front of the generation (`label_excluded`); and the stereo step
       (`stereo_identities`; `smiles="isomeric"`, `unique="stereo"`; records only): one `_stereo_order` launch over the
       rows, on the returned coordinates and graphs; and the scaffold step (`unique="scaffold"` / `"framework"`): one
       `_ring_scaffolds` call over the rows - one launch of each entry of `scaffold.py` and one `_canonical_order` launch
       on the sub-graphs -, on the returned graphs, no coordinates; and the substructure step
       (`substructures`; `require_substructures`, `exclude_substructures`, `substructure_counts`): one
       `_match_substructures` call over the rows, every pattern of the three lists in it; and the interaction step
       (`interactions`; `interaction_scores`, `max_interaction_score`, `rank_by="interaction"`; records only): one
       `_interaction_scores` call over the rows, on the returned coordinates and graphs, against the typed receptor the
       request carries - loaded, typed and sorted once, in `parse_request`, uploaded once, in that call; and, directly
       behind it, the contact step (`contacts`; `interaction_scores="contacts"` / `("contacts", t)`; records only): one
       `_contact_fingerprint` call over the rows, on the same returned coordinates and graphs, against the same receptor
       with its residues as groups, and - where the call has the reference's graph - one more for the reference conformer,
       whose fingerprint the rows are compared with;
    5. the values are attached - each molecule's `handoff.Measured`, behind a record's properties or written onto the
       Mol by `rdkit_finish.tag_measured` (Mols lose their properties in the object gather) - and validity is taken
       (`last_valid_fraction`);
    6. `select`, written once for both paths: `max_receptor_clashes`, `max_atoms_outside`, `max_chemical_tanimoto`,
       `min_pharmacophore_tanimoto`, `min_electrostatic_tanimoto`, `max_interaction_score`, the contact recovery of
       `interaction_scores=("contacts", t)`, `require_substructures`,
       `exclude_substructures`, `exclude_graphs`, `unique`, then the threshold / sphere exclusion / `top_k` walk of
       `cheminformatics.select_diverse`.  The two pair matrices are computed only when their threshold is set, over the
       rows that survived the filters.
A call with no option on takes none of these steps: its records / live Mols are returned as they come.
`standardize` is not a stage here: the generator standardises right behind the bond write-back, so the result tensors
that arrive are already the parent fragments'; its four per-sample tensors (`atoms_removed`, `n_fragments`, `atom_map`,
`kekule_bond_orders`) ride through the gather and into each record's `Measured` like the strain energies do.

The device work goes through the generator's seams (`_pose`, `_score`, `_pair`, `_receptor_coords`, `_relieve`,
`_optimise_pose`, `_score_placed`, `_graph_fingerprints`, `_chem_tanimoto`, `_chem_pair`, `_pharm_perceive`,
`_pharm_score`, `_add_hydrogens`, `_peoe_charges`, `_esp_score`, `_canonical_order`, `_stereo_order`, `_ring_scaffolds`,
`_match_substructures`,
`_interaction_scores`, `_contact_fingerprint`), looked up on the instance at the time of the call.  The shape seams take the request's reference
object; which kind it is - a conformer or a solid - is `cheminformatics`' business."""
from __future__ import annotations

import dataclasses
import inspect
import time
import types
import warnings
from typing import List, NamedTuple, Optional, Union

import torch

from . import _args
from . import canonical as mcg_canonical
from . import contacts as mcg_contacts
from . import stereo as mcg_stereo
from . import cheminformatics
from . import electrostatics as mcg_esp
from . import fingerprint as mcg_fp
from . import geometry as mcg_geometry
from . import host_pool
from . import hydrogens as mcg_hydrogens
from . import interactions as mcg_interactions
from . import pharmacophore as mcg_pharm
from . import receptor as mcg_receptor
from . import scaffold as mcg_scaffold
from . import standardize as mcg_standardize
from . import substructure as mcg_sub
from .handoff import Measured, measured_from_tensors, molecules_from_tensors


@dataclasses.dataclass(frozen=True)
class Request:
    """The options of one generation call (`parse_request`); `Request()` is the call that asked for none."""
    reference: Optional[object] = None            # `cheminformatics.SolidReference` of a `reference_shape` call, else the
    #                                               `ConformerReference` of a call with a shape option, else None
    overlay: bool = False
    scores_shape: bool = False                    # `shape_scores`, or implied by any of the three selection options
    top_k: Optional[int] = None
    min_shape_tanimoto: Optional[float] = None
    max_pairwise_tanimoto: Optional[float] = None
    refine_steps: int = 0                         # `refine_overlay`: ascent steps of the refined pose, 0 = not refined
    receptor: Optional[tuple] = None              # (coords [R,3] fp32, atomic numbers [R]) of its heavy atoms, host
    max_receptor_clashes: Optional[int] = None
    relief_steps: int = 0                         # `relieve_clashes`: trials of the clash relief, 0 = not relieved
    ref_graph: Optional[tuple] = None             # (atomic numbers, bond codes [n,n] int8) of the reference, when it scores
    scores_chemistry: bool = False                # `chemical_scores`, or implied by `max_chemical_tanimoto`
    max_chemical_tanimoto: Optional[float] = None
    unique: Union[bool, str] = False
    max_pairwise_chemical_tanimoto: Optional[float] = None
    max_atoms_outside: Optional[int] = None
    relax_steps: int = 0                          # `relax_geometry`: trial steps of the relaxation, 0 = not relaxed
    scores_pharmacophore: bool = False            # `pharmacophore_scores`, or implied by `min_pharmacophore_tanimoto`
    ref_features: Optional[tuple] = None          # `reference_pharmacophore`: (xyz [F,3] fp32, type index [F] uint8), host
    ref_pharm_graph: Optional[tuple] = None       # else (atomic numbers, bond codes [n,n] int8, coords [n,3]) to perceive
    min_pharmacophore_tanimoto: Optional[float] = None
    rank_by: str = "shape"                        # "combo": rank by shape + pharmacophore Tanimoto; "electrostatic": shape
    #                                               + electrostatic Tanimoto; "interaction": minus the interaction score
    add_hydrogens: bool = False                   # `add_hydrogens`: explicit hydrogens on the returned records
    standardize: bool = False                     # `standardize`: largest fragment + Kekule form, behind the bond write-back
    scores_electrostatics: bool = False           # `electrostatic_scores`, or implied by `min_electrostatic_tanimoto`
    ref_charge_points: Optional[tuple] = None     # `reference_charges`: (xyz [P,3] fp32, charge [P] fp32), host
    ref_charge_graph: Optional[tuple] = None      # else (atomic numbers, bond codes [n,n] int8, coords [n,3]) to charge
    min_electrostatic_tanimoto: Optional[float] = None
    partial_charges: bool = False                 # `partial_charges`: the charges on the returned records
    smiles: Union[bool, str] = False              # `smiles`: canonical order and SMILES on the returned records;
    #                                               "isomeric": the stereo identity too, and the isomeric string
    excluded_graphs: Optional[tuple] = None       # `exclude_graphs` as read on the host: (atomic numbers, bond codes) each
    exclude: Optional[frozenset] = None           # their (key, identity bytes), once `label_excluded` has labelled them
    # `unique` above is False, True (one row per `graph_key`), "exact" (one row per exact identity) or "stereo" (one row
    # per stereo identity, `stereo.stereo_identity_bytes`), "scaffold" or "framework" (one row per scaffold / generic
    # framework identity, `scaffold.murcko_scaffolds`)
    substructures: Optional[object] = None        # `substructure.Compiled`: the patterns of `require_substructures`, then
    #                                               `exclude_substructures`, then `substructure_counts`, compiled together
    n_required: int = 0                           # how many of them must be proven present,
    n_excluded: int = 0                           # and how many, behind those, drop a row where proven present
    scores_interactions: bool = False             # `interaction_scores`, or implied by `max_interaction_score`
    typed_receptor: Optional[tuple] = None        # `interactions.PreparedReceptor`: typed, sorted, with tile spheres, host
    max_interaction_score: Optional[float] = None
    optimise_steps: int = 0                       # `optimise_pose`: trials of the pose optimisation, 0 = not optimised
    optimise_flexible: bool = False               # `optimise_pose="flexible"` / `("flexible", n)`: torsions turn too
    optimise_starts: int = 0                      # `optimise_pose="search"` / `("search", S[, n])`: starts of the pose search, 0 = none
    scores_contacts: bool = False                 # `interaction_scores="contacts"` / `("contacts", t)`
    contact_receptor: Optional[tuple] = None      # `contacts.PreparedReceptor`: `typed_receptor` with its residues as groups
    ref_contact_graph: Optional[tuple] = None     # (atomic numbers, bond codes [n,n] int8, coords [n,3]) of the reference
    min_contact_recovery: Optional[float] = None  # t of `("contacts", t)`

    @property
    def selects_by_shape(self) -> bool:
        return not (self.top_k is None and self.min_shape_tanimoto is None and self.max_pairwise_tanimoto is None)

    @property
    def needs_fingerprints(self) -> bool:
        return self.scores_chemistry or self.unique is True or self.max_pairwise_chemical_tanimoto is not None

    @property
    def tags_graph_keys(self) -> bool:
        return self.scores_chemistry or self.unique is True

    @property
    def needs_identity(self) -> bool:
        """Whether `select` compares exact identities (`unique="exact"`, `exclude_graphs`)."""
        return self.unique == "exact" or self.excluded_graphs is not None

    @property
    def needs_canonical(self) -> bool:
        return bool(self.smiles) or self.needs_identity

    @property
    def needs_stereo(self) -> bool:
        """Whether the call launches the stereo search (`smiles="isomeric"`, `unique="stereo"`)."""
        return self.smiles == "isomeric" or self.unique == "stereo"

    @property
    def needs_scaffold(self) -> bool:
        """Whether the call perceives rings and scaffolds (`unique="scaffold"`, `unique="framework"`)."""
        return isinstance(self.unique, str) and self.unique in mcg_scaffold.UNIQUE_VALUES

    @property
    def measures(self) -> bool:
        """Whether any option is on (a receptor needs the pose, a selection implies its score)."""
        return (self.overlay or self.scores_shape or self.needs_fingerprints or self.needs_canonical
                or self.needs_stereo or self.needs_scaffold or self.substructures is not None)

    @property
    def removes(self) -> bool:
        """Whether the call filters or selects, i.e. may return fewer molecules than are valid."""
        return (self.max_receptor_clashes is not None or self.max_chemical_tanimoto is not None or bool(self.unique)
                or self.excluded_graphs is not None or self.selects_by_shape or self.max_pairwise_chemical_tanimoto is not None
                or self.max_atoms_outside is not None or self.min_pharmacophore_tanimoto is not None
                or self.min_electrostatic_tanimoto is not None or self.n_required > 0 or self.n_excluded > 0
                or self.max_interaction_score is not None or self.min_contact_recovery is not None)

    @property
    def needs_charges(self) -> bool:
        return self.scores_electrostatics or self.partial_charges

    def ranking_score(self, measured: Measured) -> Optional[float]:
        """What `unique`, the diversity walk and `top_k` rank a molecule by: its shape score, or - `rank_by="combo"` - shape
        + pharmacophore Tanimoto (`pharmacophore.select_score`: NaN, which ranks last, where either is missing) or -
        `rank_by="electrostatic"` - shape + electrostatic Tanimoto (`electrostatics.select_score`, likewise) or -
        `rank_by="interaction"` - minus the interaction score (`interactions.select_score`: NaN where it is missing)."""
        if self.rank_by == "interaction":
            return mcg_interactions.select_score(measured.interaction_score)
        if self.rank_by == "combo":
            return mcg_pharm.select_score(measured.shape_tanimoto, measured.pharmacophore_tanimoto)
        if self.rank_by == "electrostatic":
            return mcg_esp.select_score(measured.shape_tanimoto, measured.electrostatic_tanimoto)
        return measured.shape_tanimoto


def parse_request(gen, reference_conformer, *, reference_context=None, shape_scores: bool = False,
                  top_k: Optional[int] = None, min_shape_tanimoto: Optional[float] = None, overlay: bool = False,
                  max_pairwise_tanimoto: Optional[float] = None, refine_overlay: Union[bool, int] = False, receptor=None,
                  max_receptor_clashes: Optional[int] = None, chemical_scores: bool = False, reference_graph=None,
                  max_chemical_tanimoto: Optional[float] = None, unique: Union[bool, str] = False,
                  max_pairwise_chemical_tanimoto: Optional[float] = None, reference_shape=None,
                  shape_density: float = 0.02, max_atoms_outside: Optional[int] = None,
                  relax_geometry: Union[bool, int] = False, pharmacophore_scores: bool = False,
                  reference_pharmacophore=None, min_pharmacophore_tanimoto: Optional[float] = None,
                  rank_by: str = "shape", relieve_clashes: Union[bool, int] = False, add_hydrogens: bool = False,
                  standardize: bool = False, electrostatic_scores: bool = False, reference_charges=None,
                  min_electrostatic_tanimoto: Optional[float] = None, partial_charges: bool = False,
                  smiles: bool = False, exclude_graphs=None, require_substructures=None, exclude_substructures=None,
                  substructure_counts=None, interaction_scores: bool = False,
                  max_interaction_score: Optional[float] = None, optimise_pose: Union[bool, int] = False) -> Request:
    """The public option keywords of a generation entry of `gen` as a `Request`: the shape options first, then the chemical
    ones (`top_k` / `min_shape_tanimoto` / `max_pairwise_tanimoto` imply the shape score, `max_chemical_tanimoto` the
    chemical one).  Keyword only, behind `reference_context` in the entries' own names, order and defaults
    (`REQUEST_KEYWORDS`, `entry_request`).  Each family of options is read by its own helper, in the order below; what a
    helper's options mean is in its docstring.  `relax_geometry`: `geometry.check_steps`; it works with every other option
    and every finisher.
    Every refusal happens here, before any device work."""
    o = types.SimpleNamespace(**locals())          # the options as given: a helper reads `o.<keyword>`, what was derived
    finisher = getattr(gen, "finisher", None)      # from them is handed to it by name
    o.pocket = _pocket_receptor(o)                 # a `pocket.Pocket` brings its own receptor: `o.receptor` from here on
    custom_finisher = isinstance(finisher, host_pool.TaskRef)
    fields = _record_flags(o, finisher)
    esp = _electrostatic_flags(o, finisher)
    interact, optimise_steps, flexible = _interaction_flags(o, finisher)
    starts = _optimise_pose_value(optimise_pose)[2] if optimise_steps else 0
    fields.update(partial_charges=partial_charges, relax_steps=mcg_geometry.check_steps(relax_geometry))
    fields.update(_mesh_reference(o))
    solid = fields["reference"]
    relief = _receptor_flags(o)
    shape = _shape_fields(o, custom_finisher, solid)
    if shape:                                     # the call scores shape or poses: the receptor's options are its fields
        fields.update(shape, **relief)
        # a receptor beside a plain mesh was refused above: this is a conformer call's, or - once the call poses - a pocket's own
        if o.receptor is not None and (o.pocket is None or o.overlay):
            fields.update(_receptor_fields(o, fields["reference"], interact, optimise_steps, flexible, starts))
    scores_shape = fields.get("scores_shape")
    _args.check_flag("pharmacophore_scores", pharmacophore_scores)
    if min_pharmacophore_tanimoto is not None:
        mcg_pharm.check_threshold("min_pharmacophore_tanimoto", min_pharmacophore_tanimoto)
    conformer = None if solid is not None else fields["reference"]
    if fields.get("scores_contacts"):
        fields.update(_contact_fields(o, conformer))
    fields.update(_electrostatic_fields(o, esp, scores_shape, conformer))
    fields.update(_pharmacophore_fields(o, scores_shape, conformer))
    _args.check_flag("chemical_scores", chemical_scores)
    if not (isinstance(unique, str) and unique in ("exact", "stereo") + mcg_scaffold.UNIQUE_VALUES):
        _args.check_flag("unique", unique)
    if isinstance(unique, str) and unique == "stereo" and finisher is not None:
        raise ValueError(mcg_stereo.REFUSAL_UNIQUE_WITH_FINISHER)
    excluded = None if exclude_graphs is None else read_excluded(exclude_graphs)
    fields.update(_substructure_fields(o, custom_finisher))
    graph_read = (fields.get("ref_pharm_graph") is not None or fields.get("ref_charge_graph") is not None
                  or fields.get("ref_contact_graph") is not None)
    fields.update(_chemistry_fields(o, custom_finisher, excluded, graph_read))
    return Request(**fields)


REQUEST_KEYWORDS = tuple(name for name, p in inspect.signature(parse_request).parameters.items()
                         if p.kind is inspect.Parameter.KEYWORD_ONLY)      # `reference_context`, then the options


def entry_request(gen, arguments: dict) -> Request:
    """`parse_request` for a generation entry: `arguments` is the entry's `locals()`, out of which the reference conformer
    and every keyword of `REQUEST_KEYWORDS` is handed on under its own name."""
    return parse_request(gen, arguments["reference_conformer"], **{name: arguments[name] for name in REQUEST_KEYWORDS})


def _record_flags(o, finisher) -> dict:
    """`smiles`: True, False or "isomeric"; refused with a finisher (the order and the string go onto the records).
    `add_hydrogens`: True or False; it works with every other option, but not with a finisher, RDKit's or a custom one
    (the hydrogens go onto the records).  `standardize`: True or False; likewise refused with a finisher (RDKit's
    `standardize_mol` already does it on Mols)."""
    for name, refusal in (("smiles", mcg_canonical.REFUSAL_WITH_FINISHER),
                          ("add_hydrogens", mcg_hydrogens.REFUSAL_WITH_FINISHER),
                          ("standardize", mcg_standardize.REFUSAL_WITH_FINISHER)):
        value = getattr(o, name)
        isomeric = name == "smiles" and isinstance(value, str) and value == "isomeric"
        if (isomeric or _args.check_flag(name, value)) and finisher is not None:
            raise ValueError(refusal)
    return dict(smiles=o.smiles, add_hydrogens=o.add_hydrogens, standardize=bool(o.standardize))


def _electrostatic_flags(o, finisher) -> bool:
    """Whether the call scores electrostatics: `electrostatic_scores` (implied by `min_electrostatic_tanimoto`, a real
    number in [-1, 1]) needs `overlay`.  `partial_charges`: True or False; it needs no reference and no pose.  Both are
    refused with a finisher: they read the placed hydrogens of the records."""
    _args.check_flag("electrostatic_scores", o.electrostatic_scores)
    _args.check_flag("partial_charges", o.partial_charges)
    if o.min_electrostatic_tanimoto is not None:
        mcg_esp.check_threshold("min_electrostatic_tanimoto", o.min_electrostatic_tanimoto)
    esp = o.electrostatic_scores or o.min_electrostatic_tanimoto is not None
    if (esp or o.partial_charges) and finisher is not None:
        raise ValueError(mcg_esp.REFUSAL_WITH_FINISHER)
    if o.reference_charges is not None and not esp:
        raise ValueError("reference_charges is only read with electrostatic_scores or min_electrostatic_tanimoto")
    if esp and not o.overlay:
        raise ValueError("electrostatic_scores needs overlay=True: molecules that are not posed onto the reference are not "
                         "in the coordinates of its charges")
    return esp


def _optimise_pose_value(value):
    """(budget, flexible, starts) of an `optimise_pose` that is not False: the trial budget as given (True or an integer,
    still unchecked), whether the walk is the flexible one, and the starts of the pose search (0: none).  "flexible" and
    ("flexible", n); "search" (`interactions.SEARCH_STARTS` starts), ("search", S) and ("search", S, n) with S in 1..64
    (`interactions.check_starts`); every other string or tuple is a ValueError."""
    budget, flexible, starts = value, False, 0
    if isinstance(budget, str) and budget == mcg_interactions.FLEXIBLE:
        budget, flexible = True, True
    elif (isinstance(budget, (tuple, list)) and len(budget) == 2 and isinstance(budget[0], str)
          and budget[0] == mcg_interactions.FLEXIBLE and budget[1] is not True):
        budget, flexible = budget[1], True
    elif isinstance(budget, str) and budget == mcg_interactions.SEARCH:
        budget, flexible, starts = True, True, mcg_interactions.SEARCH_STARTS
    elif (isinstance(budget, (tuple, list)) and len(budget) in (2, 3) and isinstance(budget[0], str)
          and budget[0] == mcg_interactions.SEARCH and (len(budget) == 2 or budget[2] is not True)):
        starts = mcg_interactions.check_starts(budget[1], "optimise_pose: S of ('search', S)")
        budget, flexible = (budget[2] if len(budget) == 3 else True), True
    elif isinstance(budget, (str, tuple, list)):
        raise ValueError(f"optimise_pose must be False, True, an integer step budget in 1..{mcg_receptor.MAX_RELIEF_STEPS}, "
                         f"'flexible' or ('flexible', n) with n in 1..{mcg_receptor.MAX_RELIEF_STEPS}, 'search', "
                         f"('search', S) or ('search', S, n) with S in 1..{mcg_interactions.SEARCH_MAX_STARTS}, "
                         f"got {budget!r}")
    return budget, flexible, starts


def _interaction_flags(o, finisher):
    """(whether the call scores interactions, the trials of `optimise_pose`, whether its walk is the flexible one).
    `interaction_scores` (implied by `max_interaction_score`, a finite real number) needs a `receptor` - and with it
    `overlay`.  `rank_by="interaction"`
    needs the score.  Refused with a finisher: the values go onto the records.  `optimise_pose`:
    `receptor.check_relief_steps` (True = `interactions.OPTIMISE_STEPS`); it needs a `receptor`, and with it `overlay`,
    implies `interaction_scores` and is refused with a finisher likewise.  `optimise_pose="flexible"` (64 trials) and
    `optimise_pose=("flexible", n)`, n in 1..1024, ask for `interactions.optimise_pose_flexible`; `optimise_pose="search"`
    (8 starts, 64 trials), `("search", S)` and `("search", S, n)`, S in 1..64, for `interactions.search_pose`, whose walk is
    the flexible one (`_optimise_pose_value` reads all of them); every other string or tuple is refused.
    `interaction_scores="contacts"` and `("contacts", t)`, t a real number in [0, 1], are `interaction_scores=True` plus the
    contact fingerprint (`contacts.parse_option`; `o.contacts`, `o.min_contact_recovery` from here on); they need the
    receptor's residue identities: a PDB-format string, or a pocket found on one."""
    o.interaction_scores, o.contacts, o.min_contact_recovery = mcg_contacts.parse_option(o.interaction_scores)
    _args.check_flag("interaction_scores", o.interaction_scores)
    if o.max_interaction_score is not None:
        mcg_interactions.check_threshold("max_interaction_score", o.max_interaction_score)
    _args.check_rank_by(o.rank_by)
    optimise_steps, flexible = 0, False
    if o.optimise_pose is not False:
        budget, flexible, _ = _optimise_pose_value(o.optimise_pose)
        optimise_steps = mcg_receptor.check_relief_steps(budget, "optimise_pose", lowest=1,
                                                         if_true=mcg_interactions.OPTIMISE_STEPS)
        if finisher is not None:
            raise ValueError(mcg_interactions.OPTIMISE_REFUSAL_WITH_FINISHER)
        if o.receptor is None:
            raise ValueError("optimise_pose needs a receptor: it moves the posed molecules to where their interaction "
                             "score with it is lower")
    interact = o.interaction_scores or o.max_interaction_score is not None or optimise_steps > 0
    if o.rank_by == "interaction" and not interact:
        raise ValueError("rank_by='interaction' needs interaction_scores (or max_interaction_score): it ranks by the "
                         "interaction score")
    if interact and finisher is not None:
        raise ValueError(mcg_interactions.REFUSAL_WITH_FINISHER)
    if interact and o.receptor is None:
        raise ValueError("interaction_scores needs a receptor: it scores the posed molecules against it")
    if o.contacts and not isinstance(o.receptor, str):
        raise ValueError(mcg_contacts.REFUSAL_WITHOUT_RESIDUES)
    return interact, optimise_steps, flexible


_RECEPTOR_WITH_SHAPE = ("receptor cannot be combined with reference_shape: the receptor check needs the reference's "
                        "atoms")


def _pocket_receptor(o):
    """The `pocket.Pocket` of a call whose `reference_shape` is one, else None.  A pocket brings its own receptor, which
    every receptor option of the call then reads (`o.receptor` is set to it here); a `receptor=` beside it is refused like
    one beside any other `reference_shape`."""
    from . import pocket as mcg_pocket
    if not isinstance(o.reference_shape, mcg_pocket.Pocket):
        return None
    if o.receptor is not None:
        raise ValueError(_RECEPTOR_WITH_SHAPE + " (a Pocket brings its own receptor)")
    o.receptor = o.reference_shape.receptor
    return o.reference_shape


def _mesh_reference(o) -> dict:
    """`reference_shape`: a watertight mesh in place of the reference conformer (`mesh.load_mesh`), or a `pocket.Pocket`,
    whose mesh it is; the request then carries its `cheminformatics.SolidReference` (host side only: nothing is launched
    here), whether or not an option is on.  `max_atoms_outside` needs it, and `overlay`.  A plain mesh refuses `receptor`
    and `max_receptor_clashes`; a pocket's receptor options are read like a conformer call's."""
    solid = None
    if o.reference_shape is not None:
        if (o.reference_conformer is not None and o.reference_conformer is not False) or o.reference_context is not None:
            raise ValueError("reference_shape cannot be combined with reference_conformer or reference_context: pass "
                             "one reference")
        _args.check_real("shape_density", o.shape_density, 0.0, open_low=True)
        if o.refine_overlay is not False:
            raise ValueError("refine_overlay cannot be combined with reference_shape: the ascent's objective is the "
                             "overlap with the reference's atoms, and a mesh has none")
        if o.pocket is None and (o.receptor is not None or o.max_receptor_clashes is not None):
            raise ValueError(_RECEPTOR_WITH_SHAPE)
        solid = cheminformatics.solid_reference(o.reference_shape)
    if o.max_atoms_outside is not None:
        cheminformatics.check_max_atoms_outside(o.max_atoms_outside)
        if solid is None:
            raise ValueError("max_atoms_outside needs a reference_shape")
        if not o.overlay:
            raise ValueError("max_atoms_outside needs overlay=True: molecules that are not posed into the mesh are not "
                             "in its coordinates")
    return dict(reference=solid, max_atoms_outside=o.max_atoms_outside)


def _receptor_flags(o) -> dict:
    """`max_receptor_clashes` needs a `receptor`.  `relieve_clashes`: `receptor.check_relief_steps` (True =
    `receptor.RELIEF_STEPS`); it needs a `receptor`, and with it `overlay`.  The receptor a `pocket.Pocket` brings counts
    as one; a pocket call without a receptor option and without `overlay` simply does not read it."""
    if o.max_receptor_clashes is not None:
        mcg_receptor.check_max_receptor_clashes(o.max_receptor_clashes)
        if o.receptor is None:
            raise ValueError("max_receptor_clashes needs a receptor")
    relief_steps = 0
    if o.relieve_clashes is not False:
        relief_steps = mcg_receptor.check_relief_steps(o.relieve_clashes, "relieve_clashes", lowest=1,
                                                       if_true=mcg_receptor.RELIEF_STEPS)
        if o.receptor is None:
            raise ValueError("relieve_clashes needs a receptor: it moves the posed molecules out of their contacts with it")
    asked = (o.pocket is None or o.max_receptor_clashes is not None or relief_steps > 0 or o.interaction_scores
             or o.max_interaction_score is not None or o.optimise_pose is not False)
    if o.receptor is not None and not o.overlay and asked:       # a pocket's receptor: only once an option reads it
        raise ValueError("receptor needs overlay=True: molecules that are not posed onto the reference are not in "
                         "the receptor's frame")
    return dict(max_receptor_clashes=o.max_receptor_clashes, relief_steps=relief_steps)


def _shape_fields(o, custom_finisher, solid) -> dict:
    """The shape options; {} for a call that neither scores shape nor poses.  `top_k` / `min_shape_tanimoto` /
    `max_pairwise_tanimoto` imply the shape score; `max_pairwise_tanimoto` and `refine_overlay`
    (`cheminformatics.check_refine_steps`, True = 64) need `overlay`.  Without a mesh the request's reference is the
    `ConformerReference` of the reference conformer."""
    refine_steps = 0
    if o.refine_overlay is not False:
        refine_steps = cheminformatics.check_refine_steps(o.refine_overlay, "refine_overlay", lowest=1, if_true=64)
        if not o.overlay:
            raise ValueError("refine_overlay needs overlay=True: it refines the pose onto the reference")
    scoring = o.shape_scores or not (o.top_k is None and o.min_shape_tanimoto is None and o.max_pairwise_tanimoto is None)
    if not (scoring or o.overlay):
        return {}
    if o.max_pairwise_tanimoto is not None:
        cheminformatics.check_max_pairwise_tanimoto(o.max_pairwise_tanimoto)
        if not o.overlay:
            raise ValueError("max_pairwise_tanimoto needs overlay=True: molecules that are not posed onto the reference "
                             "share no frame to compare them in")
    what = "shape scores" if not o.overlay else "overlay"
    if o.top_k is not None:
        cheminformatics.check_top_k(o.top_k)
    if o.min_shape_tanimoto is not None:
        cheminformatics.check_min_shape_tanimoto(o.min_shape_tanimoto)
    if solid is None and (o.reference_conformer is None or o.reference_conformer is False):
        raise ValueError(f"a reference conformer is needed for {what}; a bare reference_context has no "
                         "coordinates")
    if custom_finisher:
        raise ValueError(f"{what} cannot be combined with a custom finisher: its results carry no coordinates "
                         "this package can read")
    fields = dict(overlay=bool(o.overlay), scores_shape=bool(scoring), top_k=o.top_k, refine_steps=refine_steps,
                  min_shape_tanimoto=o.min_shape_tanimoto, max_pairwise_tanimoto=o.max_pairwise_tanimoto)
    if solid is None:
        fields["reference"] = cheminformatics.ConformerReference(o.gen._reference_coord(o.reference_conformer))
    return fields


def _receptor_fields(o, reference, interact, optimise_steps, flexible=False, starts=0) -> dict:
    """The receptor of a posed call, loaded and checked to be clear of the reference conformer (a pocket has no atoms, and
    is empty space by construction: nothing to check); where the call scores interactions it is also typed, sorted and
    given its tile spheres here (`interactions.prepare_receptor`: host work, one warning where atoms lie outside the
    residue templates); a (coords, atomic_numbers, types) triple carries its own types."""
    typed = isinstance(o.receptor, (tuple, list)) and len(o.receptor) == 3      # (coords, atomic_numbers, types)
    rec = mcg_receptor.load_receptor((o.receptor[0], o.receptor[1]) if typed else o.receptor)
    if o.pocket is None:
        mcg_receptor.check_clear_of_reference(rec[0], reference.coords)
    if not interact:
        return dict(receptor=rec)
    grouped = {}
    if o.contacts:                                # typed and sorted once: the score reads the same atoms in the same order
        grouped = dict(scores_contacts=True, contact_receptor=mcg_contacts.prepare_receptor(o.receptor))
    typed_receptor = grouped["contact_receptor"].typed if grouped else mcg_interactions.prepare_receptor(o.receptor)
    return dict(grouped, receptor=rec, scores_interactions=True, max_interaction_score=o.max_interaction_score,
                rank_by=o.rank_by, typed_receptor=typed_receptor, optimise_steps=optimise_steps,
                optimise_flexible=bool(flexible and optimise_steps),
                optimise_starts=int(starts) if optimise_steps else 0)


def _reference_graph(o, missing: str, max_atoms: int, placed: Optional[str] = None, conformer=None):
    """The reference's heavy-atom graph (`fingerprint.mol_graph`) of `reference_graph`, else of a reference conformer with
    bonds; ValueError(`missing`) where there is neither.  `placed` ("features", "charges"): the graph is laid onto the
    atoms of `conformer`, the request's `ConformerReference` (None with a `reference_shape`: refused likewise), and
    must have as many heavy atoms, at most `max_atoms`; the result is then (atomic numbers, bond codes, coords)."""
    src = o.reference_graph
    if src is None and hasattr(o.reference_conformer, "GetAtoms") and hasattr(o.reference_conformer, "GetBonds"):
        src = o.reference_conformer
    if src is None or (placed is not None and conformer is None):
        raise ValueError(missing)
    z, bonds = mcg_fp.mol_graph(src)
    if placed is None:
        if not 1 <= len(z) <= max_atoms:
            raise ValueError(f"the reference graph must have 1 to {max_atoms} heavy atoms, got {len(z)}")
        return z, bonds
    coords = conformer.coords
    if not 1 <= len(z) <= max_atoms or len(z) != int(coords.shape[0]):
        raise ValueError(f"the reference graph has {len(z)} heavy atoms, the reference conformer "
                         f"{int(coords.shape[0])}: the {placed} are placed on the conformer's atoms, in the "
                         f"graph's order (at most {max_atoms})")
    return z, bonds, coords


def _contact_fields(o, conformer) -> dict:
    """The reference of the contact step: the reference conformer typed by its graph (`reference_graph`, else a reference
    conformer with bonds), whose fingerprint against the same receptor - one more launch of the same kernel, behind the
    generation - the rows are compared with.  Without a graph (a bare conformer, a `reference_shape`, a pocket) there is
    no recovery: "contacts" still reports the fingerprints, `("contacts", t)` is refused."""
    graph = None
    try:
        graph = _reference_graph(o, mcg_contacts.REFUSAL_WITHOUT_GRAPH, mcg_contacts.MAX_ATOMS, "contact types", conformer)
    except ValueError:
        if o.min_contact_recovery is not None or o.reference_graph is not None:
            raise
    return dict(ref_contact_graph=graph, min_contact_recovery=o.min_contact_recovery)


def _electrostatic_fields(o, esp, scores_shape, conformer) -> dict:
    """The reference's charge points are `reference_charges` (`electrostatics.load_reference_charges`) or are computed,
    behind the generation, from the reference's graph (`reference_graph`, else a reference conformer with bonds) on the
    reference conformer's coordinates, its hydrogens placed by the same kernel.  `rank_by="electrostatic"` needs the shape
    and the electrostatic score."""
    if o.rank_by == "electrostatic" and not (esp and scores_shape):
        raise ValueError("rank_by='electrostatic' needs shape scores (shape_scores, top_k, min_shape_tanimoto or "
                         "max_pairwise_tanimoto) and electrostatic_scores: it ranks by their sum")
    if not esp:
        return {}
    fields = dict(scores_electrostatics=True, min_electrostatic_tanimoto=o.min_electrostatic_tanimoto, rank_by=o.rank_by)
    if o.reference_charges is not None:
        return dict(fields, ref_charge_points=mcg_esp.load_reference_charges(o.reference_charges))
    return dict(fields, ref_charge_graph=_reference_graph(
        o, "electrostatic scores need the reference's charges: pass reference_charges= (a sequence "
        "of (charge, (x, y, z)) in the reference's coordinates - the only way with a "
        "reference_shape) or the reference's molecular graph (reference_graph=, or a reference "
        "conformer with bonds)", mcg_esp.MAX_ATOMS, "charges", conformer))


def _pharmacophore_fields(o, scores_shape, conformer) -> dict:
    """`pharmacophore_scores` (implied by `min_pharmacophore_tanimoto`) needs `overlay`; the reference's features are
    `reference_pharmacophore` (`pharmacophore.load_reference_features`) or are perceived, behind the generation, from the
    reference's graph (`reference_graph`, else a reference conformer with bonds) at the reference conformer's coordinates.
    `rank_by="combo"` needs the shape and the pharmacophore score."""
    pharm = o.pharmacophore_scores or o.min_pharmacophore_tanimoto is not None
    if o.reference_pharmacophore is not None and not pharm:
        raise ValueError("reference_pharmacophore is only read with pharmacophore_scores or min_pharmacophore_tanimoto")
    if o.rank_by == "combo" and not (pharm and scores_shape):
        raise ValueError("rank_by='combo' needs shape scores (shape_scores, top_k, min_shape_tanimoto or "
                         "max_pairwise_tanimoto) and pharmacophore_scores: it ranks by their sum")
    if not pharm:
        return {}
    if not o.overlay:
        raise ValueError("pharmacophore_scores needs overlay=True: molecules that are not posed onto the reference are "
                         "not in the coordinates of its features")
    fields = dict(scores_pharmacophore=True, min_pharmacophore_tanimoto=o.min_pharmacophore_tanimoto, rank_by=o.rank_by)
    if o.reference_pharmacophore is not None:
        return dict(fields, ref_features=mcg_pharm.load_reference_features(o.reference_pharmacophore))
    return dict(fields, ref_pharm_graph=_reference_graph(
        o, "pharmacophore scores need the reference's features: pass reference_pharmacophore= (a "
        "sequence of (type, (x, y, z)) in the reference's coordinates - the only way with a "
        "reference_shape) or the reference's molecular graph (reference_graph=, or a reference "
        "conformer with bonds)", mcg_pharm.MAX_ATOMS, "features", conformer))


def _substructure_fields(o, custom_finisher) -> dict:
    """`require_substructures` / `exclude_substructures` / `substructure_counts`: each None or an iterable of pattern
    strings (`substructure.parse`), `substructure.Pattern`s or graph sources (`substructure.from_graph`); they are
    compiled here, together (`compile_substructures`: host work), and an entry that cannot be read or breaks a limit is a
    ValueError naming its list and position; refused with a custom finisher, through RDKit's the Mols' own graphs are
    read."""
    patterns, n_required, n_excluded = compile_substructures(o.require_substructures, o.exclude_substructures,
                                                             o.substructure_counts)
    if patterns is None:
        return {}
    if custom_finisher:
        raise ValueError(mcg_sub.REFUSAL_WITH_FINISHER)
    return dict(substructures=patterns, n_required=n_required, n_excluded=n_excluded)


def _chemistry_fields(o, custom_finisher, excluded, graph_read: bool) -> dict:
    """The chemical options: `max_chemical_tanimoto` implies the chemical score, which needs the reference's graph
    (`_reference_graph`).  `unique`: False, True or "exact" - one row per exact identity (`canonical.identity_bytes`)
    instead of per `graph_key` -, "scaffold" or "framework" - one row per scaffold / generic framework
    (`scaffold.murcko_scaffolds`); these read the Mols' own graphs through RDKit's finisher and are refused with a custom one.
    `excluded`: the graphs of `exclude_graphs` as `read_excluded` read them.  `graph_read`: whether the pharmacophore or
    the electrostatic family already reads `reference_graph` - one that no option reads is refused."""
    if o.max_chemical_tanimoto is not None:
        mcg_fp.check_threshold("max_chemical_tanimoto", o.max_chemical_tanimoto)
    if o.max_pairwise_chemical_tanimoto is not None:
        mcg_fp.check_threshold("max_pairwise_chemical_tanimoto", o.max_pairwise_chemical_tanimoto)
    scoring = o.chemical_scores or o.max_chemical_tanimoto is not None
    if o.reference_graph is not None and not scoring and not graph_read:
        raise ValueError("reference_graph is only read with chemical_scores, max_chemical_tanimoto or pharmacophore "
                         "scores without reference_pharmacophore (or electrostatic scores without reference_charges)")
    chemical = scoring or o.unique or o.max_pairwise_chemical_tanimoto is not None
    if (chemical or excluded is not None) and custom_finisher:
        raise ValueError("chemical scores cannot be combined with a custom finisher: its results carry no graph this "
                         "package can read")
    fields = {} if excluded is None else dict(excluded_graphs=tuple(excluded))
    if not chemical:
        return fields
    graph = None
    if scoring:
        graph = _reference_graph(
            o, "chemical scores need the reference's molecular graph: pass reference_graph= (a Mol, a "
            "GeneratedMolecule or an (atomic_numbers, bond_orders) pair) or a reference conformer "
            "with bonds; coordinates and a bare reference_context have none", mcg_fp.MAX_GRAPH_ATOMS)
    return dict(fields, ref_graph=graph, scores_chemistry=bool(scoring), max_chemical_tanimoto=o.max_chemical_tanimoto,
                unique=o.unique, max_pairwise_chemical_tanimoto=o.max_pairwise_chemical_tanimoto)


def compile_substructures(require, exclude, counts):
    """(`substructure.Compiled` or None, n_required, n_excluded): the patterns of the three substructure options - each None
    or what `substructure.compile_patterns` takes - compiled together, in that order, so that one matching call serves all
    three.  Host work only.  ValueError naming the option and the position of an entry that cannot be read."""
    lists = [() if arg is None else mcg_sub.compile_patterns(arg, where=name).patterns
             for name, arg in (("require_substructures", require), ("exclude_substructures", exclude),
                               ("substructure_counts", counts))]
    if not any(lists):
        return None, 0, 0
    return mcg_sub.compile_patterns([p for part in lists for p in part]), len(lists[0]), len(lists[1])


def substructures(gen, req: Request, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor):
    """The substructure step of padded graphs, ONE `_match_substructures` call with every pattern of the request: (its
    result, per row (counts, status) over the patterns as host lists - what `select` reads)."""
    out = gen._match_substructures(atomic_numbers, bond_orders, n_nodes, req.substructures)
    return out, list(zip(out["count"].cpu().tolist(), out["status"].cpu().tolist()))


def read_excluded(exclude_graphs) -> List[tuple]:
    """The heavy-atom graphs (`fingerprint.mol_graph`) of an `exclude_graphs` argument - an iterable of `GeneratedMolecule`,
    Mols or (atomic_numbers, bond_orders) pairs whose exact identities the call drops -, host side only: the graphs are
    only read here; the entries label them (`label_excluded`, one `_canonical_order` launch per 16 384) behind their own
    argument checks, directly in front of the generation, where one without a canonical order is refused.  ValueError naming
    the position of an entry that is unreadable or has more than `canonical.MAX_ATOMS` heavy atoms, and for an argument
    that is no iterable of graphs."""
    if isinstance(exclude_graphs, (str, bytes)) or not hasattr(exclude_graphs, "__iter__"):
        raise ValueError("exclude_graphs must be an iterable of GeneratedMolecule records, Mols or (atomic_numbers, "
                         f"bond_orders) pairs, got {type(exclude_graphs).__name__}")
    graphs = []
    for k, obj in enumerate(exclude_graphs):
        try:
            z, bonds = mcg_fp.mol_graph(obj)
        except ValueError as e:
            raise ValueError(f"exclude_graphs[{k}] is unreadable: {e}") from None
        if len(z) > mcg_canonical.MAX_ATOMS:
            raise ValueError(f"exclude_graphs[{k}] has {len(z)} heavy atoms; a canonical order takes at most "
                             f"{mcg_canonical.MAX_ATOMS}")
        graphs.append((z, bonds))
    return graphs


def identities(gen, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor):
    """The canonical step of padded graphs, one `_canonical_order` call: (its result, per row the exact identity as (key,
    `canonical.identity_bytes`), None for a row that has no canonical order - it is not proven equal to anything)."""
    canon = gen._canonical_order(atomic_numbers, bond_orders, n_nodes)
    keys = [k & 0xFFFFFFFFFFFFFFFF for k in canon["key"].cpu().tolist()]
    exact = mcg_canonical.identity_bytes(atomic_numbers, bond_orders, n_nodes, ordered=canon)
    return canon, [None if e is None else (k, e) for k, e in zip(keys, exact)]


def excluded_identities(gen, graphs: List[tuple]) -> frozenset:
    """The exact identities of the `read_excluded` graphs, by the kernel that labels the generated rows, in chunks of
    `canonical.MAX_BATCH`; ValueError naming the position of one that has no canonical order."""
    out = set()
    for lo in range(0, len(graphs), mcg_canonical.MAX_BATCH):
        canon, exact = identities(gen, *mcg_fp.pad_graphs(graphs[lo: lo + mcg_canonical.MAX_BATCH]))
        for k, (e, status) in enumerate(zip(exact, canon["status"].cpu().tolist())):
            if e is None:
                raise ValueError(f"exclude_graphs[{lo + k}] has no canonical order: its labelling ended with "
                                 f"{mcg_canonical.describe_status(status)}")
            out.add(e)
    return frozenset(out)


def label_excluded(gen, req: Request) -> Request:
    """`req` with the exact identities of its `exclude_graphs` (`excluded_identities`: device work, through
    `_canonical_order`); `req` itself where the call excludes nothing.  The generation entries call it behind every
    argument check of their own, directly in front of the generation; ValueError naming the position of a graph that has
    no canonical order."""
    if req.excluded_graphs is None:
        return req
    return dataclasses.replace(req, exclude=excluded_identities(gen, list(req.excluded_graphs)))


def stereo_identities(gen, coords, atomic_numbers, bond_orders, n_nodes):
    """The stereo step of padded, embedded graphs, one `_stereo_order` call: (its result, per row the stereo identity as
    (`stereo_key`, `stereo.stereo_identity_bytes`), None for a row that has no stereo order - it is not proven equal to
    anything)."""
    found = gen._stereo_order(coords, atomic_numbers, bond_orders, n_nodes)
    keys = [k & 0xFFFFFFFFFFFFFFFF for k in found["stereo_key"].cpu().tolist()]
    exact = mcg_stereo.stereo_identity_bytes(coords, atomic_numbers, bond_orders, n_nodes, ordered=found)
    return found, [None if e is None else (k, e) for k, e in zip(keys, exact)]


def select_exact(exact: List[Optional[tuple]], order: List[int]) -> List[int]:
    """Positions to keep so that every exact identity occurs once: the rows are grouped by their 64-bit key, and a row is
    dropped only where its identity bytes equal those of a row that comes before it in `order` (positions, best first).  A
    row without an identity (None: no canonical order) is always kept.  The result is in the input's order."""
    groups, keep = {}, []
    for i in order:
        if exact[i] is not None:
            key, body = exact[i]
            seen = groups.setdefault(key, [])
            if body in seen:
                continue
            seen.append(body)
        keep.append(i)
    return sorted(keep)


@dataclasses.dataclass
class Rows:
    """The rows one call may return, as parallel lists: what `select` filters and selects from, on either path."""
    item: List                                    # the `GeneratedMolecule` record or the finished Mol
    sample_id: List[int]
    measured: List[Measured]
    row: List[int]                                # index into the device tensors behind the pair matrices
    exact: Optional[List[Optional[tuple]]] = None     # `identities` per row, where the call compares exact identities
    sub: Optional[List[tuple]] = None                 # `substructures` per row, where the call matches patterns
    stereo: Optional[List[Optional[tuple]]] = None    # `stereo_identities` per row, with `unique="stereo"`
    scaffold: Optional[List[Optional[tuple]]] = None  # `scaffold.murcko_scaffolds`' identity per row, with `unique="scaffold"`
    #                                                   / `"framework"`

    def take(self, keep: List[int]) -> "Rows":
        """The rows at the positions `keep`, in that order."""
        return Rows(*(None if col is None else [col[i] for i in keep] for col in vars(self).values()))


def select(rows: Rows, req: Request, shape_pair, chem_pair) -> List:
    """The items of `rows` a call returns: the rows with at most `max_receptor_clashes` clashing atoms (one without
    contacts - its pose failed - does not pass), then those with at most `max_atoms_outside` atoms outside the mesh (one
    without a count - its pose failed - does not pass), then those with a chemical Tanimoto below `max_chemical_tanimoto` (NaN
    does not pass), then those with a pharmacophore Tanimoto of at least `min_pharmacophore_tanimoto` (NaN and None do not
    pass), then those with an electrostatic Tanimoto of at least `min_electrostatic_tanimoto` (NaN and None do not pass),
    then those with an interaction score of at most `max_interaction_score` (NaN and None do not pass),
    then those with a contact recovery of at least the t of `interaction_scores=("contacts", t)` (NaN and None do not pass),
    then `require_substructures` - the rows in which every required pattern is PROVEN present (count >= 1) - and
    `exclude_substructures` - the rows in which no excluded pattern is proven present; a row whose search for a pattern
    ended with BUDGET before it found an embedding is undetermined: not proven to contain it, so `require` drops it and
    `exclude` keeps it, and one warning per call names how many such rows there were -,
    then `exclude_graphs` - the rows whose exact identity is one of the excluded graphs' (a row without a canonical order is
    not proven equal to anything and stays) -, then `unique` - of the rows with one graph key (`unique="exact"`: with one
    exact identity, `select_exact`; `unique="stereo"`: with one stereo identity, the same walk; `unique="scaffold"` /
    `"framework"`: with one scaffold / framework identity, the same walk again - all acyclic rows share the empty scaffold,
    and a row whose scaffold has no canonical order always stays) the first in ranking order
    (`cheminformatics.ranking_key` of `Request.ranking_score`: by shape score where the call scores shape - plus the
    pharmacophore score with `rank_by="combo"`, the electrostatic score with `rank_by="electrostatic"`; by minus the
    interaction score with `rank_by="interaction"` - else the lowest sample id), still in the
    input's order - then the threshold (always on the shape score alone), the sphere exclusion at `max_pairwise_tanimoto` and at
    `max_pairwise_chemical_tanimoto` in one walk, and `top_k` (`cheminformatics.select_diverse`).  `shape_pair(rows)` /
    `chem_pair(rows)`: the [n,n] pair matrices of the surviving rows, each called only when its threshold is set."""
    def at_most(field: str, limit: int) -> List[int]:
        values = [getattr(m, field) for m in rows.measured]
        return [i for i, v in enumerate(values) if v is not None and v <= limit]
    if req.max_receptor_clashes is not None:
        rows = rows.take(at_most("receptor_clashes", req.max_receptor_clashes))
    if req.max_atoms_outside is not None:
        rows = rows.take(at_most("atoms_outside", req.max_atoms_outside))
    if req.max_chemical_tanimoto is not None:
        rows = rows.take([i for i, m in enumerate(rows.measured) if m.chemical_tanimoto < req.max_chemical_tanimoto])
    if req.min_pharmacophore_tanimoto is not None:
        rows = rows.take([i for i, m in enumerate(rows.measured) if m.pharmacophore_tanimoto is not None
                          and m.pharmacophore_tanimoto >= req.min_pharmacophore_tanimoto])
    if req.min_electrostatic_tanimoto is not None:
        rows = rows.take([i for i, m in enumerate(rows.measured) if m.electrostatic_tanimoto is not None
                          and m.electrostatic_tanimoto >= req.min_electrostatic_tanimoto])
    if req.max_interaction_score is not None:
        rows = rows.take([i for i, m in enumerate(rows.measured) if m.interaction_score is not None
                          and m.interaction_score <= req.max_interaction_score])
    if req.min_contact_recovery is not None:
        rows = rows.take([i for i, m in enumerate(rows.measured) if m.contact_recovery is not None
                          and m.contact_recovery >= req.min_contact_recovery])
    if req.n_required or req.n_excluded:
        need, last = req.n_required, req.n_required + req.n_excluded
        undetermined = sum(1 for c, st in rows.sub if any(st[p] != 0 and c[p] == 0 for p in range(last)))
        if undetermined:
            warnings.warn(f"substructure matching: {undetermined} molecule(s) left undetermined - the search for a required "
                          f"or excluded pattern ended with BUDGET ({mcg_sub.NODE_BUDGET} nodes from one root) before it "
                          "found an embedding; require_substructures drops such a row, exclude_substructures keeps it")
        rows = rows.take([i for i, (c, _) in enumerate(rows.sub) if all(c[p] >= 1 for p in range(need))
                          and not any(c[p] >= 1 for p in range(need, last))])
    if req.excluded_graphs is not None:
        if req.exclude is None:
            raise RuntimeError("the request's exclude_graphs were not labelled: call label_excluded before the selection")
        rows = rows.take([i for i, e in enumerate(rows.exact) if e is None or e not in req.exclude])
    if req.unique:
        order = sorted(range(len(rows.item)), key=lambda i: cheminformatics.ranking_key(
            req.ranking_score(rows.measured[i]), rows.sample_id[i]))
        if req.unique == "exact":
            rows = rows.take(select_exact(rows.exact, order))
        elif req.unique == "stereo":                  # the same walk over (stereo_key, stereo identity bytes)
            rows = rows.take(select_exact(rows.stereo, order))
        elif req.needs_scaffold:                      # ... and over (scaffold key, scaffold identity bytes)
            rows = rows.take(select_exact(rows.scaffold, order))
        else:
            rows = rows.take(mcg_fp.select_unique([m.graph_key for m in rows.measured], order))
    if not req.selects_by_shape and req.max_pairwise_chemical_tanimoto is None:
        return rows.item
    threshold = req.min_shape_tanimoto
    if req.rank_by != "shape" and threshold is not None:          # the walk ranks by the sum: the shape threshold goes first
        rows = rows.take([i for i, m in enumerate(rows.measured) if m.shape_tanimoto >= threshold])
        threshold = None
    keep = cheminformatics.select_diverse(
        [req.ranking_score(m) for m in rows.measured], rows.sample_id,
        shape_pair(rows) if req.max_pairwise_tanimoto is not None else None,
        req.max_pairwise_tanimoto, req.top_k, threshold,
        chem_pair(rows) if req.max_pairwise_chemical_tanimoto is not None else None, req.max_pairwise_chemical_tanimoto)
    return [rows.item[i] for i in keep]


def fingerprints(gen, req: Request, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor):
    """The chemical step of padded graphs, one fingerprint launch: (fingerprints [B,64], graph keys [B] int64, chemical
    Tanimoto [B] to the reference's graph or None when the call does not score)."""
    fp, key, _ = gen._graph_fingerprints(atomic_numbers, bond_orders, n_nodes)
    sim = None
    if req.scores_chemistry:
        ref_fp = gen._graph_fingerprints(*mcg_fp.pad_graphs([req.ref_graph]))[0][0]
        sim = gen._chem_tanimoto(fp, ref_fp.to(fp.device))
    return fp, key, sim


def pharmacophore(gen, req: Request, coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor,
                  n_nodes: torch.Tensor):
    """The pharmacophore step of posed, padded molecules: (Tanimoto [B] fp32, matches [B] int32), by one perceive and one
    score launch over the rows.  The reference's features are the request's, or are perceived here - one more perceive
    launch - from its graph at the reference conformer's coordinates; ValueError where that reference has no feature or
    more rings than are kept."""
    feats = req.ref_features
    if feats is None:
        z, bonds, xyz = req.ref_pharm_graph
        types, rings, count = gen._pharm_perceive(*mcg_fp.pad_graphs([(z, bonds)]))
        if int(count[0]) > mcg_pharm.MAX_RINGS:
            raise ValueError(f"the reference has {int(count[0])} aromatic rings; at most {mcg_pharm.MAX_RINGS} are kept")
        feats = mcg_pharm.load_reference_features(mcg_pharm.feature_points(xyz.unsqueeze(0), types, rings, count)[0])
    return gen._pharm_score(feats, coords, n_nodes, *gen._pharm_perceive(atomic_numbers, bond_orders, n_nodes))


def hydrogens(gen, req: Request, res: dict, placed: Optional[dict] = None) -> dict:
    """The hydrogen step of the rows a rank returns (`add_hydrogens`): the explicit hydrogens of the RETURNED coordinates -
    relaxed, posed, refined, relieved - so they need no transform of their own; one perceive and one placement launch
    over the rows (`_add_hydrogens`).  The per-sample tensors by the names `handoff.measured_from_tensors` reads:
    `hydrogen_coords`, `hydrogen_parents`, `hydrogens_unplaced` (-1 where the row has a non-finite coordinate) and - with
    a receptor - `receptor_hydrogen_clashes`: the hydrogens overlapping a receptor heavy atom by `receptor.CLASH_OVERLAP`
    at hydrogen's van der Waals radius, by the heavy atoms' own kernel (`_receptor_coords`) over the hydrogen columns in
    chunks of its 64-atom width; -1 where posing failed.  `placed`: the `_add_hydrogens` result of the same rows, where
    the electrostatic step has already made it."""
    out = placed if placed is not None else gen._add_hydrogens(res["x"], res["elements"], res["bond"], res["n_nodes"])
    count = out["n_hydrogens"]
    values = dict(hydrogen_coords=out["coords"], hydrogen_parents=out["parents"],
                  hydrogens_unplaced=torch.where(count < 0, torch.full_like(count, -1), out["unplaced"]))
    if req.receptor is not None:
        xyz = out["coords"]
        clashes = torch.zeros_like(count)
        for lo in range(0, int(xyz.shape[1]), mcg_receptor.MAX_LIGAND_ATOMS):
            chunk = xyz[:, lo: lo + mcg_receptor.MAX_LIGAND_ATOMS].contiguous()
            n_chunk = (count - lo).clamp(0, int(chunk.shape[1]))
            ones = torch.ones(chunk.shape[0], chunk.shape[1], dtype=torch.int32, device=xyz.device)
            clashes = clashes + mcg_receptor.clash_summary(gen._receptor_coords(req.receptor, chunk, n_chunk, ones))[0]
        posed = torch.isfinite(res["pose"]).all(dim=1).to(clashes.device) & (count >= 0)
        values["receptor_hydrogen_clashes"] = torch.where(posed, clashes, torch.full_like(clashes, -1))
    return values


def reference_charge_points(gen, req: Request):
    """The reference's charge points (xyz [P,3], charge [P]; host) of a call that scores electrostatics: the request's, or
    - one perceive, one placement and one charge launch - those of the reference's graph on the reference conformer's
    coordinates, its hydrogens placed by the kernel that places the candidates'.  ValueError where that reference holds
    an element without charge parameters."""
    if req.ref_charge_points is not None:
        return req.ref_charge_points
    z, bonds, xyz = req.ref_charge_graph
    zs, bs, nn = mcg_fp.pad_graphs([(z, bonds)])
    perceived = gen._pharm_perceive(zs, bs, nn)
    x = xyz.to(torch.float32).unsqueeze(0)
    placed = gen._add_hydrogens(x, zs, bs, nn, perceived=perceived)
    charges = gen._peoe_charges(zs, bs, nn, perceived=perceived)
    if int(charges["status"][0]) != 0:
        raise ValueError("the reference holds an element without charge parameters (electrostatics.py has rows for H, C, "
                         "N, O, F, P, S, Cl, Br): pass reference_charges=")
    pts, q, count = mcg_esp.charge_points(x.to(placed["coords"].device), charges, placed)
    k = int(count[0])
    return mcg_esp.load_reference_charges((pts[0, :k], q[0, :k]))


def electrostatics(gen, req: Request, res: dict, placed: Optional[dict] = None, perceived=None) -> dict:
    """The electrostatic step of the rows a rank returns (`electrostatic_scores`, `partial_charges`), on the RETURNED
    coordinates and graphs: one charge launch over the rows (`_peoe_charges`) and - with the scores - the charge points of
    the rows with their placed hydrogens (`placed`: the `_add_hydrogens` result of the same rows) and the overlap launches
    against the reference's (`_esp_score`).  The per-sample tensors by the names `handoff.measured_from_tensors` reads:
    `electrostatic_tanimoto` (NaN where posing failed or the row holds an element without parameters) and - with
    `partial_charges` - `partial_charges` / `hydrogen_charges` [B,W], +inf at and beyond a row's atoms."""
    charges = gen._peoe_charges(res["elements"], res["bond"], res["n_nodes"], perceived=perceived)
    values = {}
    if req.partial_charges:
        q = charges["q"]
        real = torch.arange(q.shape[1], device=q.device).view(1, -1) < charges["n_nodes"].to(q.device).view(-1, 1)
        beyond = torch.full_like(q, float("inf"))
        values.update(partial_charges=torch.where(real, q, beyond), hydrogen_charges=torch.where(real, charges["q_h"], beyond))
    if req.scores_electrostatics:
        x = res["x"].to(placed["coords"].device)
        pts, q, count = mcg_esp.charge_points(x, charges, placed)
        sim = gen._esp_score(reference_charge_points(gen, req), pts, q, count)
        posed = torch.isfinite(res["pose"]).all(dim=1).to(sim.device)         # a failed pose is not in the reference's frame
        values["electrostatic_tanimoto"] = torch.where(posed, sim, torch.full_like(sim, float("nan")))
    return values


def interactions(gen, req: Request, res: dict) -> dict:
    """The interaction step of the rows a rank returns (`interaction_scores`), on the RETURNED coordinates - relaxed,
    posed, refined, relieved - and graphs: one `_interaction_scores` call over the rows against the request's typed
    receptor.  The per-sample tensors by the names `handoff.measured_from_tensors` reads: `interaction_score` [B],
    `interaction_terms` [B,6] (G1, G2, REP, HYD, HB, n_rot), `receptor_hbonds` [B] (-1 where posing failed or the row has
    a non-finite coordinate: the record gets None throughout) and `interaction_atom_scores` [B,N], +inf at and beyond a
    row's atoms."""
    out = gen._interaction_scores(req.typed_receptor, res["x"], res["n_nodes"], res["elements"], res["bond"])
    score, hbonds, atoms = out["score"], out["hbonds"], out["atom_scores"]
    dev = score.device
    posed = torch.isfinite(res["pose"]).all(dim=1).to(dev) & (hbonds >= 0)    # a failed pose is not in the receptor's frame
    real = torch.arange(atoms.shape[1], device=dev).view(1, -1) < res["n_nodes"].to(dev).reshape(-1, 1)
    values = dict(interaction_score=torch.where(posed, score, torch.full_like(score, float("nan"))),
                  interaction_terms=torch.cat([out["terms"][:, :5], out["n_rot"].to(dev, torch.float32).view(-1, 1)], dim=1),
                  receptor_hbonds=torch.where(posed, hbonds, torch.full_like(hbonds, -1)),
                  interaction_atom_scores=torch.where(real, atoms, torch.full_like(atoms, float("inf"))))
    if req.optimise_steps:
        # `optimise_rows` carried W of the pose the walk started from; E divides it as the kernel does: one rounded
        # product, one sum, one division - so an unmoved row's two scores have the same bits
        den = 1.0 + torch.tensor(mcg_interactions.ROTOR_WEIGHT, dtype=torch.float32, device=dev) * \
            out["n_rot"].to(dev, torch.float32).clamp(min=0)
        before = res["interaction_score_before"].to(dev, torch.float32) / den
        unmoved = res["pose_trials_kept"].to(dev) == 0                            # the pose scored above IS the start
        if "pose_best_start" in res:                                              # ... unless another start of the search won
            unmoved = unmoved & ~(res["pose_best_start"].to(dev) > 0)
        values["interaction_score_before"] = torch.where(unmoved, values["interaction_score"], before)
    return values


def reference_contacts(gen, req: Request):
    """The reference fingerprint (groups, kinds as host lists) of a call whose request carries the reference's graph: the
    reference conformer's heavy atoms against the call's grouped receptor, by the kernel that fingerprints the rows - one
    `_contact_fingerprint` call; None without the graph.  ValueError where that fingerprint cannot be formed."""
    if req.ref_contact_graph is None:
        return None
    z, bonds, xyz = req.ref_contact_graph
    zs, bs, nn = mcg_fp.pad_graphs([(z, bonds)])
    out = gen._contact_fingerprint(req.contact_receptor, xyz.to(torch.float32).unsqueeze(0), nn, zs, bs)
    if int(out["status"][0]) != mcg_contacts.OK:
        raise ValueError("the reference conformer's contact fingerprint could not be formed: status "
                         f"{mcg_contacts.STATUS_NAMES[int(out['status'][0])]}")
    k = int(out["n_groups"][0])
    return out["groups"][0, :k].cpu().tolist(), out["kinds"][0, :k].cpu().tolist()


def contacts(gen, req: Request, res: dict) -> dict:
    """The contact step of the rows a rank returns (`interaction_scores="contacts"`), on the RETURNED coordinates - relaxed,
    posed, refined, relieved, optimised - and graphs: one `_contact_fingerprint` call over the rows against the request's
    grouped receptor and, where the request carries the reference's graph, one for the reference conformer
    (`reference_contacts`).  The per-sample tensors by the names `handoff.measured_from_tensors` reads: `contact_status` [B]
    (-1 where posing failed: the record gets None throughout), `contact_groups` / `contact_kinds` [B,256],
    `contact_atom_kinds` [B,N] (255 at and beyond a row's atoms), with a reference `contact_recovery` / `contact_tanimoto` [B]
    fp64, and the two values the records share, `contact_labels` and `contact_reference`."""
    ref = reference_contacts(gen, req)
    out = gen._contact_fingerprint(req.contact_receptor, res["x"], res["n_nodes"], res["elements"], res["bond"], reference=ref)
    status, atoms = out["status"], out["atom_kinds"]
    dev = status.device
    posed = torch.isfinite(res["pose"]).all(dim=1).to(dev)                    # a failed pose is not in the receptor's frame
    real = torch.arange(atoms.shape[1], device=dev).view(1, -1) < res["n_nodes"].to(dev).reshape(-1, 1)
    values = dict(contact_status=torch.where(posed, status, torch.full_like(status, -1)), contact_groups=out["groups"],
                  contact_kinds=out["kinds"], contact_atom_kinds=torch.where(real, atoms, torch.full_like(atoms, 255)),
                  contact_labels=req.contact_receptor.group_labels, contact_reference=None)
    if ref is not None:
        values.update(contact_recovery=out["recovery"], contact_tanimoto=out["tanimoto"],
                      contact_reference=(tuple(ref[0]), tuple(ref[1]), mcg_contacts.DEFAULT_KINDS))
    return values


def _index(rows: Rows, device) -> torch.Tensor:
    return torch.tensor(rows.row, dtype=torch.long, device=device)


def compose_pose(pose: torch.Tensor, rotation: torch.Tensor, translation: torch.Tensor) -> torch.Tensor:
    """[B,12]: the pose (Q, d) followed by the rigid move (R, t) as one transform, (Q R, d R + t), so that
    x @ (Q R) + (d R + t) = (x @ Q + d) @ R + t.  `pose` [B,12] rotation row-major then translation, `rotation` [B,3,3],
    `translation` [B,3]; every product written out in a fixed order."""
    Q, d = pose[:, :9].reshape(-1, 3, 3), pose[:, 9:]
    QR = (Q[:, :, 0:1] * rotation[:, 0:1, :] + Q[:, :, 1:2] * rotation[:, 1:2, :]) + Q[:, :, 2:3] * rotation[:, 2:3, :]
    dR = (d[:, 0:1] * rotation[:, 0, :] + d[:, 1:2] * rotation[:, 1, :]) + d[:, 2:3] * rotation[:, 2, :]
    return torch.cat([QR.reshape(-1, 9), dR + translation], dim=1)


def relieve_rows(gen, req: Request, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                 pose: torch.Tensor, tanimoto: torch.Tensor) -> dict:
    """The clash relief of posed, padded rows (`relieve_clashes`), shared by both paths: the clash count of the pose as it
    came (`_receptor_coords`), one `_relieve` call over all rows and - for the rows it moved - the composed pose and the
    shape Tanimoto of the pose as placed (`_score_placed`).  `pose` [B,12] (a row with a non-finite entry: posing failed,
    the row is not in the receptor's frame and is left alone), `tanimoto` [B] the pose's score.  Returns tensors on the
    device of the relief's result: `coords`, `pose`, `overlay_tanimoto` (an unmoved row keeps every bit of what came in),
    `moved` [B] bool, `rotation` / `translation` of the move itself, `relief_rmsd` (0 where nothing moved, NaN where
    posing failed) and `receptor_clashes_before` (-1 where posing failed)."""
    before = mcg_receptor.clash_summary(gen._receptor_coords(req.receptor, coords, n_nodes, atomic_numbers))[0]
    out = gen._relieve(req.receptor, coords, n_nodes, atomic_numbers, req.relief_steps)
    dev = out["coords"].device
    x, pose, tanimoto = coords.to(dev, torch.float32), pose.to(dev, torch.float32), tanimoto.to(dev, torch.float32)
    posed = torch.isfinite(pose).all(dim=1)
    moved = out["moved"].to(dev) & posed
    width = x.shape[1]
    new_x = torch.where(moved.view(-1, 1, 1), out["coords"][:, :width], x)
    rescored = gen._score_placed(req.reference, new_x, n_nodes).to(dev)
    before = before.to(dev)
    return dict(coords=new_x, moved=moved, rotation=out["rotation"], translation=out["translation"],
                pose=torch.where(moved.view(-1, 1), compose_pose(pose, out["rotation"], out["translation"]), pose),
                overlay_tanimoto=torch.where(moved, rescored, tanimoto),
                relief_rmsd=torch.where(posed, torch.where(moved, out["rmsd"], torch.zeros_like(out["rmsd"])),
                                        torch.full_like(out["rmsd"], float("nan"))),
                receptor_clashes_before=torch.where(posed, before, torch.full_like(before, -1)))


FLEX_RECORD_FIELDS = ("pose_torsions", "pose_torsion_angles", "pose_conformer_rmsd", "intramolecular_clash_before",
                      "intramolecular_clash")     # what `optimise_pose="flexible"` adds to a record
SEARCH_RECORD_FIELDS = ("pose_starts", "pose_best_start")      # what `optimise_pose="search"` adds beside them


def optimise_rows(gen, req: Request, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                  bond_orders: torch.Tensor, pose: torch.Tensor, tanimoto: torch.Tensor,
                  row_ids: Optional[torch.Tensor] = None, sample_seed: Optional[int] = None) -> dict:
    """The pose optimisation of posed, padded rows (`optimise_pose`): one `_optimise_pose` call over all rows against the
    request's typed receptor and - for the rows it moved - the composed pose and the shape Tanimoto of the pose as placed
    (`_score_placed`).  `pose` [B,12] (a row with a non-finite entry: posing failed, the row is not in the receptor's frame
    and is left alone), `tanimoto` [B] the pose's score.  Returns tensors on the device of the walk's result: `coords`,
    `pose`, `overlay_tanimoto` (an unmoved row keeps every bit of what came in), `moved` [B] bool, `rotation` /
    `translation` of the move itself, `pose_optimisation_rmsd` (0 where nothing moved, NaN where posing failed),
    `pose_trials_kept` (-1 where posing failed) and `interaction_score_before`: W, the weighted sum, of the pose the walk
    started from (NaN where posing failed) - `interactions` divides it by the rotor term behind the gather, where n_rot is
    counted.  With `req.optimise_flexible` the walk is `_optimise_pose_flex` (torsions turn too): `rotation` / `translation` /
    `pose` stay the rigid part of the move, and the dict gains `pose_torsions` (-1 where posing failed),
    `pose_torsion_angles` [B,16], `pose_conformer_rmsd`, `intramolecular_clash_before` and `intramolecular_clash` (NaN
    there).  With `req.optimise_starts` the stage is `_search_pose`: that walk from so many keyed starts per row, keyed by
    `sample_seed` (None: 0) and the rows' sample ids `row_ids` (None: 0..B-1; in a sharded call the global ids, so a
    molecule gets the same starts on any number of GPUs); `rotation` / `translation` are then the start's rigid part
    followed by the walk's, and the dict gains `pose_starts` and `pose_best_start` (-1 where posing failed or no start has
    a finite objective)."""
    starts = getattr(req, "optimise_starts", 0)       # (a request-like object from before the search has no such field)
    if starts:
        out = gen._search_pose(req.typed_receptor, coords, n_nodes, atomic_numbers, bond_orders, starts, req.optimise_steps,
                               0 if sample_seed is None else sample_seed, row_ids)
    else:
        walk = gen._optimise_pose_flex if req.optimise_flexible else gen._optimise_pose
        out = walk(req.typed_receptor, coords, n_nodes, atomic_numbers, bond_orders, req.optimise_steps)
    dev = out["coords"].device
    x, pose, tanimoto = coords.to(dev, torch.float32), pose.to(dev, torch.float32), tanimoto.to(dev, torch.float32)
    kept = out["kept"].to(dev)
    posed = torch.isfinite(pose).all(dim=1) & (kept >= 0)
    moved = out["moved"].to(dev) & posed
    width = x.shape[1]
    new_x = torch.where(moved.view(-1, 1, 1), out["coords"][:, :width], x)
    rescored = gen._score_placed(req.reference, new_x, n_nodes).to(dev)
    nan = torch.full_like(out["rmsd"], float("nan"))
    flex = {}
    if req.optimise_flexible:
        used = out["torsions"].to(dev)
        flex = dict(pose_torsions=torch.where(posed, used, torch.full_like(used, -1)),
                    pose_torsion_angles=torch.where(moved.view(-1, 1), out["torsion_angles"],
                                                    torch.zeros_like(out["torsion_angles"])),
                    pose_conformer_rmsd=torch.where(posed, torch.where(moved, out["conformer_rmsd"], torch.zeros_like(nan)),
                                                    nan),
                    intramolecular_clash_before=torch.where(posed, out["clash_before"], nan),
                    intramolecular_clash=torch.where(posed, torch.where(moved, out["clash_after"], out["clash_before"]),
                                                     nan))
    if starts:
        best = out["best_start"].to(dev)
        flex.update(pose_starts=torch.where(posed, torch.full_like(best, starts), torch.full_like(best, -1)),
                    pose_best_start=torch.where(posed, best, torch.full_like(best, -1)))
    return dict(flex, coords=new_x, moved=moved, rotation=out["rotation"], translation=out["translation"],
                pose=torch.where(moved.view(-1, 1), compose_pose(pose, out["rotation"], out["translation"]), pose),
                overlay_tanimoto=torch.where(moved, rescored, tanimoto),
                interaction_score_before=torch.where(posed, out["weighted_before"], nan),
                pose_optimisation_rmsd=torch.where(posed, torch.where(moved, out["rmsd"], torch.zeros_like(nan)), nan),
                pose_trials_kept=torch.where(posed, kept, torch.full_like(kept, -1)))


# ----------------------------------------------------------------------------------------------- without a finisher
def measure_tensors(gen, req: Request, res: dict, row_ids: Optional[torch.Tensor] = None,
                    sample_seed: Optional[int] = None) -> dict:
    """Stages 1-3 on one shard's result tensors.  `res` with `x` posed and the per-sample tensors `overlay_tanimoto`,
    `pose`, `shape_tanimoto`, `receptor_clashes` (-1 where posing failed), `receptor_max_overlap` (NaN there), - posed
    into a mesh - `atoms_outside` (of the returned coordinates: counted again behind a relief or an optimisation) and -
    relieved - `relief_rmsd` (NaN where posing failed) and `receptor_clashes_before`
    (-1 there) and - optimised - `interaction_score_before`, `pose_optimisation_rmsd` (NaN where posing failed) and
    `pose_trials_kept` (-1 there) added, as far as the call asked: the spellings `handoff.measured_from_tensors` reads,
    which cross the tensor gather.  `row_ids` (the rows' sample ids, default 0..B-1) and `sample_seed` key the starts of
    `optimise_pose="search"`; nothing else reads them."""
    if req.overlay:
        ov = gen._pose(req.reference, res["x"], res["n_nodes"], req.refine_steps)
        res = dict(res, x=ov["coords"], overlay_tanimoto=ov["tanimoto"],
                   pose=torch.cat([ov["rotation"].reshape(-1, 9), ov["translation"].reshape(-1, 3)], dim=1))
        if "atoms_outside" in ov:
            res["atoms_outside"] = ov["atoms_outside"]
    if req.relief_steps:
        rel = relieve_rows(gen, req, res["x"], res["n_nodes"], res["elements"], res["pose"], res["overlay_tanimoto"])
        res = dict(res, x=rel["coords"], pose=rel["pose"], overlay_tanimoto=rel["overlay_tanimoto"],
                   relief_rmsd=rel["relief_rmsd"], receptor_clashes_before=rel["receptor_clashes_before"])
    if req.optimise_steps:
        opt = optimise_rows(gen, req, res["x"], res["n_nodes"], res["elements"], res["bond"], res["pose"],
                            res["overlay_tanimoto"], row_ids, sample_seed)
        res = dict(res, x=opt["coords"], pose=opt["pose"], overlay_tanimoto=opt["overlay_tanimoto"],
                   interaction_score_before=opt["interaction_score_before"],
                   pose_optimisation_rmsd=opt["pose_optimisation_rmsd"], pose_trials_kept=opt["pose_trials_kept"])
        res.update({k: opt[k] for k in FLEX_RECORD_FIELDS + SEARCH_RECORD_FIELDS if k in opt})
    if "atoms_outside" in res and (req.relief_steps or req.optimise_steps):
        # a pocket's receptor stages moved the rows after the pose counted them: count the returned coordinates
        again = gen._atoms_outside(req.reference, res["x"], res["n_nodes"])
        res["atoms_outside"] = torch.where(res["atoms_outside"].to(again.device) < 0, torch.full_like(again, -1), again)
    if req.scores_shape:
        res = dict(res, shape_tanimoto=gen._score(req.reference, res["x"], res["n_nodes"]))
    if req.receptor is not None:
        clashes, worst = mcg_receptor.clash_summary(
            gen._receptor_coords(req.receptor, res["x"], res["n_nodes"], res["elements"]))
        posed = torch.isfinite(res["pose"]).all(dim=1).to(clashes.device)
        res = dict(res, receptor_clashes=torch.where(posed, clashes, torch.full_like(clashes, -1)),
                   receptor_max_overlap=torch.where(posed, worst, torch.full_like(worst, float("nan"))))
    return res


def return_records(gen, req: Request, res: dict, row_ids: Optional[torch.Tensor], optimise_geometry: bool) -> List:
    """What a call returns without a finisher, from the (gathered, measured) result tensors of the rows this rank returns
    (sample ids `row_ids`, default 0..B-1): stages 4-6.  The `GeneratedMolecule` records (one D2H, timed as
    `last_host_assembly_ms`) pass the validity proxy, then `select`; the pair matrices are taken from the posed rows and
    from their fingerprints, by the records' batch rows."""
    from .conformer_generator import _finish      # per call: that module imports this one, and tests replace it there
    values = {f.name: res.get(f.name) for f in dataclasses.fields(Measured)}
    fp = None
    if req.needs_fingerprints:
        fp, key, sim = fingerprints(gen, req, res["elements"], res["bond"], res["n_nodes"])
        values.update(chemical_tanimoto=sim, graph_key=key if req.tags_graph_keys else None)
    exact = None
    if req.needs_identity:
        canon, exact = identities(gen, res["elements"], res["bond"], res["n_nodes"])
    elif req.smiles:
        canon = gen._canonical_order(res["elements"], res["bond"], res["n_nodes"])
    if req.smiles:
        values.update(canonical_order=canon["order"], canonical_status=canon["status"])
    stereo = None
    if req.needs_stereo:                          # one more launch: the returned coordinates, the parent graph
        found, stereo = stereo_identities(gen, res["x"], res["elements"], res["bond"], res["n_nodes"])
        if req.smiles == "isomeric":
            values.update(stereo_order=found["order"], stereo_status=found["status"], stereo_descriptors=found["stereo"],
                          n_stereo_defined=found["counts"][:, 0] + found["counts"][:, 1],
                          n_stereo_undefined=found["counts"][:, 2])
    scaffolds = None
    if req.needs_scaffold:                        # the returned graph alone: no coordinates
        found = gen._ring_scaffolds(res["elements"], res["bond"], res["n_nodes"], req.unique == "framework")
        scaffolds = found["identity"]
        values.update(mcg_scaffold.record_fields(found, with_smiles=bool(req.smiles)))
    sub = None
    if req.substructures is not None:
        matched, sub = substructures(gen, req, res["elements"], res["bond"], res["n_nodes"])
        values.update(substructure_counts=matched["count"], substructure_status=matched["status"],
                      substructure_first=matched["first"], substructure_patterns=req.substructures.patterns)
    if req.scores_pharmacophore:
        sim, hits = pharmacophore(gen, req, res["x"], res["elements"], res["bond"], res["n_nodes"])
        posed = torch.isfinite(res["pose"]).all(dim=1).to(sim.device)         # a failed pose is not in the reference's frame
        values.update(pharmacophore_tanimoto=torch.where(posed, sim, torch.full_like(sim, float("nan"))),
                      pharmacophore_matches=torch.where(posed, hits, torch.full_like(hits, -1)))
    if req.scores_interactions:
        values.update(interactions(gen, req, res))
    if req.scores_contacts:
        values.update(contacts(gen, req, res))
    placed = perceived = None
    if req.needs_charges:                         # perceived once for the placement and the charges
        perceived = gen._pharm_perceive(res["elements"], res["bond"], res["n_nodes"])
    if req.scores_electrostatics:                 # placed once: the hydrogens of `add_hydrogens` are these
        placed = gen._add_hydrogens(res["x"], res["elements"], res["bond"], res["n_nodes"], perceived=perceived)
    if req.add_hydrogens:
        values.update(hydrogens(gen, req, res, placed))
    if req.needs_charges:
        values.update(electrostatics(gen, req, res, placed, perceived))
    if gen.device.type == "cuda":
        # (the D2H copies below would wait for the call's stream anyway: keep that out of the figure.  The call's stream only -
        #  a device-wide synchronise would also wait for whatever the caller runs on other streams beside the generation.)
        torch.cuda.current_stream(gen.device).synchronize()
    t0 = time.perf_counter()
    mols = molecules_from_tensors(res["x"], res["elements"], res["bond"], res["n_nodes"], res["valid"],
                                  sample_ids=row_ids, **values)
    gen.last_host_assembly_ms = (time.perf_counter() - t0) * 1e3      # D2H of the result tensors + record views
    kept, gen.last_valid_fraction = _finish(mols, optimise_geometry, use_rdkit=False)    # no finisher: the proxy
    if not req.removes:
        return kept
    rows = Rows(kept, [m.sample_id for m in kept], [m._measured for m in kept], [m.batch_row for m in kept],
                None if exact is None else [exact[m.batch_row] for m in kept],
                None if sub is None else [sub[m.batch_row] for m in kept],
                None if stereo is None or req.unique != "stereo" else [stereo[m.batch_row] for m in kept],
                None if scaffolds is None else [scaffolds[m.batch_row] for m in kept])

    def shape_pair(left: Rows):
        x = res["x"]
        idx = _index(left, x.device)
        return gen._pair(req.reference, x.index_select(0, idx),
                         res["n_nodes"].reshape(-1).to(x.device).index_select(0, idx))
    return select(rows, req, shape_pair, lambda left: gen._chem_pair(fp.index_select(0, _index(left, fp.device))))


# ----------------------------------------------------------------------------------------------- through a finisher
class Finished(NamedTuple):
    """One sample of a shard behind its finisher: the one value per sample that crosses the object gather."""
    mol: object                                   # the finished Mol; None = dropped
    measured: Measured


def _heavy_coords(mols: List):
    """(padded [B, max n, 3], n_nodes [B]) of Mols' heavy-atom conformer positions."""
    return cheminformatics.padded_coords([cheminformatics.mol_heavy_coords(m) for m in mols])


def score_mols(gen, reference, mols: List) -> List[Optional[float]]:
    """Shape Tanimoto of finished Mols' heavy-atom conformer positions against `reference` (None where a molecule was
    dropped), in ONE batched device call (`_score`)."""
    live = [k for k, m in enumerate(mols) if m is not None]
    out: List[Optional[float]] = [None] * len(mols)
    if live:
        for k, v in zip(live, gen._score(reference, *_heavy_coords([mols[k] for k in live])).cpu().tolist()):
            out[k] = float(v)
    return out


def _heavy_numbers(mols: List, width: int) -> torch.Tensor:
    """[B, width] int64: the heavy atoms' `GetAtomicNum()` of each Mol, zero padded."""
    z = torch.zeros(len(mols), width, dtype=torch.long)
    for j, m in enumerate(mols):
        heavy = [a.GetAtomicNum() for a in m.GetAtoms() if a.GetAtomicNum() != 1]
        z[j, : len(heavy)] = torch.tensor(heavy, dtype=torch.long)
    return z


def _relieve_mols(gen, req: Request, mols: List, measured: List[Measured]) -> None:
    """The clash relief of the posed Mols (`relieve_rows` on their heavy atoms, one batched call): a moved Mol has every
    conformer position, hydrogens included, moved by the relief's transform (`cheminformatics.apply_pose`), and its
    `Measured` gets the composed pose and the rescored `overlay_tanimoto`; every posed Mol's gets `relief_rmsd` and
    `receptor_clashes_before`."""
    live = [k for k, m in enumerate(mols) if m is not None and measured[k].pose is not None]
    if not live:
        return
    coords, n = _heavy_coords([mols[k] for k in live])
    rel = relieve_rows(gen, req, coords, n, _heavy_numbers([mols[k] for k in live], coords.shape[1]),
                       torch.stack([measured[k].pose for k in live]),
                       torch.tensor([measured[k].overlay_tanimoto for k in live], dtype=torch.float32))
    rel = {k: v.cpu() for k, v in rel.items()}
    for j, k in enumerate(live):
        m = measured[k]
        m.relief_rmsd, m.receptor_clashes_before = float(rel["relief_rmsd"][j]), int(rel["receptor_clashes_before"][j])
        if bool(rel["moved"][j]):
            cheminformatics.apply_pose(mols[k], rel["rotation"][j], rel["translation"][j])
            m.pose, m.overlay_tanimoto = rel["pose"][j].clone(), float(rel["overlay_tanimoto"][j])
            if hasattr(mols[k], "SetDoubleProp"):
                mols[k].SetDoubleProp("overlay_tanimoto", m.overlay_tanimoto)
    if any(measured[k].atoms_outside is not None for k in live):      # a pocket's relief: count the relieved atoms again
        again = gen._atoms_outside(req.reference, rel["coords"], n).cpu().tolist()
        for j, k in enumerate(live):
            if measured[k].atoms_outside is not None:
                measured[k].atoms_outside = int(again[j])


def _contact_mols(gen, rec: tuple, mols: List, posed: List[bool]) -> List[Optional[tuple]]:
    """(receptor_clashes, receptor_max_overlap) of posed Mols' heavy atoms (elements from `GetAtomicNum()`), in ONE
    batched device call; None where a Mol was dropped or its pose failed (it is not in the receptor's frame)."""
    live = [k for k, m in enumerate(mols) if m is not None and posed[k]]
    out: List[Optional[tuple]] = [None] * len(mols)
    if live:
        coords, n = _heavy_coords([mols[k] for k in live])
        z = _heavy_numbers([mols[k] for k in live], coords.shape[1])
        clashes, worst = mcg_receptor.clash_summary(gen._receptor_coords(rec, coords, n, z))
        for j, (c, w) in enumerate(zip(clashes.cpu().tolist(), worst.cpu().tolist())):
            out[live[j]] = (int(c), float(w))
    return out


def measure_finished(gen, req: Request, done: List, res: Optional[dict] = None) -> List[Finished]:
    """Stages 1-3 on one shard's finished Mols (None = dropped), each in ONE batched device call: pose, every conformer
    position moved (`cheminformatics.pose_mols`), then - `relieve_clashes` - the posed Mols moved out of their receptor
    contacts (`_relieve_mols`), then score (`score_mols`), then the receptor contacts of the posed Mols.  Per sample the
    Mol with its `Measured`: None where the call did not ask, the Mol was dropped or - contacts, relief and atoms outside
    the mesh - its pose failed.  `res`: the shard's result tensors; where the call relaxed, its
    `strain_before` / `strain_after` join every sample's values."""
    measured = [Measured() for _ in done]
    live = [k for k, m in enumerate(done) if m is not None]
    if req.overlay:
        ov = {}                                   # the result of the one batched call `pose_mols` makes, if it makes one

        def pose(ref, coords, n):
            ov.update(gen._pose(ref, coords, n, req.refine_steps))
            return ov
        for m, p in zip(measured, cheminformatics.pose_mols(req.reference, done, overlay_fn=pose)):
            if p is not None:                     # (score, rotation, translation), host; no pose where posing failed
                m.overlay_tanimoto = p[0]
                m.pose = None if p[1] is None else torch.cat([p[1].reshape(9), p[2]])     # owns its 12 values
        if "atoms_outside" in ov:
            counts = measured_from_tensors(dict(atoms_outside=ov["atoms_outside"]), len(live))
            for k, c in zip(live, counts):
                measured[k].atoms_outside = c.atoms_outside
    if req.relief_steps:
        _relieve_mols(gen, req, done, measured)
    if req.scores_shape:
        for m, score in zip(measured, score_mols(gen, req.reference, done)):
            m.shape_tanimoto = score
    if req.receptor is not None:
        contacts = _contact_mols(gen, req.receptor, done, [m.pose is not None for m in measured])
        for m, c in zip(measured, contacts):
            m.receptor_clashes, m.receptor_max_overlap = c if c is not None else (None, None)
    if res is not None and "strain_before" in res:
        for m, e0, e1 in zip(measured, res["strain_before"].cpu().tolist(), res["strain_after"].cpu().tolist()):
            m.strain_before, m.strain_after = e0, e1
    return [Finished(mol, m) for mol, m in zip(done, measured)]


def return_finished(gen, req: Request, samples: List[Finished], row_ids: Optional[torch.Tensor],
                    sample_seed: Optional[int]) -> List:
    """What a call returns through a finisher, from the (gathered) `measure_finished` values of the rows this rank returns
    (sample ids `row_ids`, default 0..B-1): stages 4-6.  The chemical step reads the live Mols' own graphs
    (`fingerprint.mol_graph`) in one batched device call.  The Mols get their properties here, behind the object gather,
    which does not carry them: `sample_id` (seeded calls) and what `rdkit_finish.tag_measured` writes.  Then `select`, the
    shape pair matrix taken from the surviving Mols' posed heavy atoms."""
    from . import rdkit_finish
    mols = [s.mol for s in samples]
    ids = list(range(len(mols))) if row_ids is None else row_ids.tolist()
    if sample_seed is not None:
        rdkit_finish.tag_sample_ids(mols, ids)
    gen.last_host_assembly_ms = 0.0
    live = [i for i, m in enumerate(mols) if m is not None]
    gen.last_valid_fraction = len(live) / len(mols) if mols else 0.0
    if not req.measures and not req.relax_steps:  # nothing was measured: nothing to tag or select by
        return [mols[i] for i in live]
    rows = Rows([mols[i] for i in live], [ids[i] for i in live], [samples[i].measured for i in live],
                list(range(len(live))))
    fp = None
    if req.needs_fingerprints and live:
        fp, key, sim = fingerprints(gen, req, *mcg_fp.pad_graphs([mcg_fp.mol_graph(m) for m in rows.item]))
        chem = measured_from_tensors(dict(chemical_tanimoto=sim, graph_key=key if req.tags_graph_keys else None), len(live))
        for m, c in zip(rows.measured, chem):
            m.chemical_tanimoto, m.graph_key = c.chemical_tanimoto, c.graph_key
    if req.needs_identity:                        # the live Mols' own graphs, like the fingerprints
        rows.exact = identities(gen, *mcg_fp.pad_graphs([mcg_fp.mol_graph(m) for m in rows.item]))[1] if live else []
    if req.needs_scaffold:                        # likewise
        rows.scaffold = gen._ring_scaffolds(*mcg_fp.pad_graphs([mcg_fp.mol_graph(m) for m in rows.item]),
                                            req.unique == "framework")["identity"] if live else []
    if req.substructures is not None:             # likewise the live Mols' own graphs
        rows.sub = []
        if live:
            matched, rows.sub = substructures(gen, req, *mcg_fp.pad_graphs([mcg_fp.mol_graph(m) for m in rows.item]))
            found = measured_from_tensors(dict(substructure_counts=matched["count"], substructure_status=matched["status"],
                                               substructure_first=matched["first"],
                                               substructure_patterns=req.substructures.patterns), len(live))
            for m, c in zip(rows.measured, found):
                m.substructure_counts, m.substructure_status = c.substructure_counts, c.substructure_status
                m.substructure_first, m.substructure_patterns = c.substructure_first, c.substructure_patterns
    posed = [i for i, m in enumerate(rows.measured) if m.pose is not None]
    if req.scores_pharmacophore and posed:        # the live, posed Mols' heavy atoms and their own graphs
        z, bonds, nn = mcg_fp.pad_graphs([mcg_fp.mol_graph(rows.item[i]) for i in posed])
        sim, hits = pharmacophore(gen, req, _heavy_coords([rows.item[i] for i in posed])[0], z, bonds, nn)
        scored = measured_from_tensors(dict(pharmacophore_tanimoto=sim, pharmacophore_matches=hits), len(posed))
        for i, c in zip(posed, scored):
            rows.measured[i].pharmacophore_tanimoto = c.pharmacophore_tanimoto
            rows.measured[i].pharmacophore_matches = c.pharmacophore_matches
    rdkit_finish.tag_measured(rows.item, rows.measured)
    if not req.measures:
        return rows.item

    def chem_pair(left: Rows):
        if fp is None:                            # nothing left to compare
            return torch.zeros(0, 0)
        return gen._chem_pair(fp.index_select(0, _index(left, fp.device)))
    return select(rows, req, lambda left: gen._pair(req.reference, *_heavy_coords(left.item)), chem_pair)
