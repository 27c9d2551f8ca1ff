"""What a generation call does between "the shard's result tensors / finished Mols exist" and "the list it returns":
the opt-in measuring, filtering and selecting of `MLConformerGenerator.generate_conformers*` (whose docstring says what
each option means).  The generator generates, parses its keywords into one `Request` (`parse_request`) and hands over.

Stages, in this order:
  BEFORE the gather, on the rank that generated the shard, one batched device call each (`measure_tensors` on the result
  tensors where no finisher runs, `measure_finished` on the finished Mols' heavy atoms where one does):
    1. pose onto the reference (`overlay`, refined with `refine_overlay`) - a conformer, or the solid of a
       `reference_shape` mesh, which also counts the posed atoms outside it;
    2. shape score of the RETURNED coordinates (`shape_scores`, or implied by a shape selection);
    3. receptor contacts of the returned coordinates (`receptor`).
  BEHIND the gather, on the rows a rank returns (`return_records` / `return_finished`):
    4. chemical fingerprints, graph keys and the Tanimoto to the reference's graph: one launch over the rows, one for
       the reference (`fingerprints`);
    5. the values are attached - keyword arguments of `molecules_from_tensors`, or `rdkit_finish.tag_*` on the Mols,
       which lose their properties in the object gather - and validity is taken (`last_valid_fraction`);
    6. `select`, written once for both paths: `max_receptor_clashes`, `max_atoms_outside`, `max_chemical_tanimoto`,
       `unique`, then the
       threshold / sphere exclusion / `top_k` walk of `cheminformatics.select_diverse`.  The two pair matrices are
       computed only when their threshold is set, over the rows that survived the filters.
A call with no option on takes none of these steps: its records / live Mols are returned as they come.

The device work goes through the generator's seams (`_pose_coords`, `_pose_coords_refined`, `_score_coords`,
`_pair_coords`, `_receptor_coords`, `_graph_fingerprints`, `_chem_tanimoto`, `_chem_pair`, and with a `reference_shape`
`_pose_solid`, `_score_solid`, `_pair_solid` in place of the first, third and fourth), looked up on the instance at the
time of the call."""
from __future__ import annotations

import dataclasses
import numbers
import time
from typing import List, Optional, Union

import torch

from . import cheminformatics
from . import fingerprint as mcg_fp
from . import geometry as mcg_geometry
from . import host_pool
from . import receptor as mcg_receptor
from .handoff import molecules_from_tensors


@dataclasses.dataclass(frozen=True)
class Request:
    """The options of one generation call (`parse_request`); `Request()` is the call that asked for none."""
    ref_coord: Optional[torch.Tensor] = None      # the reference's heavy-atom coordinates [n,3] fp32, host (shape options)
    overlay: bool = False
    scores_shape: bool = False                    # `shape_scores`, or implied by any of the three selection options
    top_k: Optional[int] = None
    min_shape_tanimoto: Optional[float] = None
    max_pairwise_tanimoto: Optional[float] = None
    refine_steps: int = 0                         # `refine_overlay`: ascent steps of the refined pose, 0 = not refined
    receptor: Optional[tuple] = None              # (coords [R,3] fp32, atomic numbers [R]) of its heavy atoms, host
    max_receptor_clashes: Optional[int] = None
    ref_graph: Optional[tuple] = None             # (atomic numbers, bond codes [n,n] int8) of the reference, when it scores
    scores_chemistry: bool = False                # `chemical_scores`, or implied by `max_chemical_tanimoto`
    max_chemical_tanimoto: Optional[float] = None
    unique: bool = False
    max_pairwise_chemical_tanimoto: Optional[float] = None
    ref_solid: Optional[object] = None            # `cheminformatics.SolidReference` of a `reference_shape` call
    max_atoms_outside: Optional[int] = None
    relax_steps: int = 0                          # `relax_geometry`: trial steps of the relaxation, 0 = not relaxed

    @property
    def selects_by_shape(self) -> bool:
        return not (self.top_k is None and self.min_shape_tanimoto is None and self.max_pairwise_tanimoto is None)

    @property
    def needs_fingerprints(self) -> bool:
        return self.scores_chemistry or self.unique or self.max_pairwise_chemical_tanimoto is not None

    @property
    def tags_graph_keys(self) -> bool:
        return self.scores_chemistry or self.unique

    @property
    def measures(self) -> bool:
        """Whether any option is on (a receptor needs the pose, a selection implies its score)."""
        return self.overlay or self.scores_shape or self.needs_fingerprints

    @property
    def removes(self) -> bool:
        """Whether the call filters or selects, i.e. may return fewer molecules than are valid."""
        return (self.max_receptor_clashes is not None or self.max_chemical_tanimoto is not None or self.unique
                or self.selects_by_shape or self.max_pairwise_chemical_tanimoto is not None
                or self.max_atoms_outside is not None)


def parse_request(gen, reference_conformer, shape_scores: bool = False, top_k: Optional[int] = None,
                  min_shape_tanimoto: Optional[float] = None, overlay: bool = False,
                  max_pairwise_tanimoto: Optional[float] = None, refine_overlay: Union[bool, int] = False, receptor=None,
                  max_receptor_clashes: Optional[int] = None, chemical_scores=False, reference_graph=None,
                  max_chemical_tanimoto: Optional[float] = None, unique=False,
                  max_pairwise_chemical_tanimoto: Optional[float] = None, reference_shape=None,
                  shape_density: float = 0.02, max_atoms_outside: Optional[int] = None,
                  reference_context=None, relax_geometry: Union[bool, int] = False) -> Request:
    """The public option keywords of a generation entry of `gen` as a `Request`: the shape options first, then the chemical
    ones (`top_k` / `min_shape_tanimoto` / `max_pairwise_tanimoto` imply the shape score, `max_chemical_tanimoto` the
    chemical one).  `reference_shape`: a watertight mesh in place of the reference conformer (`mesh.load_mesh`); the
    request then carries its `cheminformatics.SolidReference` (host side only: nothing is launched here), whether or not an
    option is on.  `relax_geometry`: `geometry.check_steps`; it works with every other option and every finisher.
    Every refusal happens here, before any device work."""
    relax_steps = mcg_geometry.check_steps(relax_geometry)
    custom_finisher = isinstance(getattr(gen, "finisher", None), host_pool.TaskRef)
    shape = {}
    solid = None
    if reference_shape is not None:
        if (reference_conformer is not None and reference_conformer is not False) or reference_context is not None:
            raise ValueError("reference_shape cannot be combined with reference_conformer or reference_context: pass "
                             "one reference")
        if isinstance(shape_density, bool) or not isinstance(shape_density, numbers.Real) or not (
                0.0 < float(shape_density) < float("inf")):
            raise ValueError(f"shape_density must be a positive real number, got {shape_density!r}")
        if refine_overlay is not False:
            raise ValueError("refine_overlay cannot be combined with reference_shape: the ascent's objective is the "
                             "overlap with the reference's atoms, and a mesh has none")
        if receptor is not None or max_receptor_clashes is not None:
            raise ValueError("receptor cannot be combined with reference_shape: the receptor check needs the reference's "
                             "atoms")
        solid = cheminformatics.solid_reference(reference_shape)
    if max_atoms_outside is not None:
        cheminformatics.check_max_atoms_outside(max_atoms_outside)
        if solid is None:
            raise ValueError("max_atoms_outside needs a reference_shape")
        if not overlay:
            raise ValueError("max_atoms_outside needs overlay=True: molecules that are not posed into the mesh are not "
                             "in its coordinates")
    solid_kw = dict(ref_solid=solid, max_atoms_outside=max_atoms_outside, relax_steps=relax_steps)
    if max_receptor_clashes is not None:
        mcg_receptor.check_max_receptor_clashes(max_receptor_clashes)
        if receptor is None:
            raise ValueError("max_receptor_clashes needs a receptor")
    if receptor is not None and not overlay:
        raise ValueError("receptor needs overlay=True: molecules that are not posed onto the reference are not in "
                         "the receptor's frame")
    refine_steps = 0
    if refine_overlay is not False:
        refine_steps = cheminformatics.check_refine_steps(refine_overlay, "refine_overlay", lowest=1, if_true=64)
        if not overlay:
            raise ValueError("refine_overlay needs overlay=True: it refines the pose onto the reference")
    scoring = shape_scores or top_k is not None or min_shape_tanimoto is not None or max_pairwise_tanimoto is not None
    if scoring or overlay:
        if max_pairwise_tanimoto is not None:
            cheminformatics.check_max_pairwise_tanimoto(max_pairwise_tanimoto)
            if not overlay:
                raise ValueError("max_pairwise_tanimoto needs overlay=True: molecules that are not posed onto the reference "
                                 "share no frame to compare them in")
        what = "shape scores" if not overlay else "overlay"
        if top_k is not None:
            cheminformatics.check_top_k(top_k)
        if min_shape_tanimoto is not None:
            cheminformatics.check_min_shape_tanimoto(min_shape_tanimoto)
        if solid is None and (reference_conformer is None or reference_conformer is False):
            raise ValueError(f"a reference conformer is needed for {what}; a bare reference_context has no "
                             "coordinates")
        if custom_finisher:
            raise ValueError(f"{what} cannot be combined with a custom finisher: its results carry no coordinates "
                             "this package can read")
        ref_coord = None
        if solid is None:
            ref_coord = gen._reference_coord(reference_conformer)
            cheminformatics.check_reference_atoms(int(ref_coord.shape[0]))
        rec = None
        if receptor is not None:
            rec = mcg_receptor.load_receptor(receptor)
            mcg_receptor.check_clear_of_reference(rec[0], ref_coord)
        shape = dict(ref_coord=ref_coord, overlay=bool(overlay), scores_shape=bool(scoring), top_k=top_k,
                     min_shape_tanimoto=min_shape_tanimoto, max_pairwise_tanimoto=max_pairwise_tanimoto,
                     refine_steps=refine_steps, receptor=rec, max_receptor_clashes=max_receptor_clashes)

    mcg_fp.check_flag("chemical_scores", chemical_scores)
    mcg_fp.check_flag("unique", unique)
    if max_chemical_tanimoto is not None:
        mcg_fp.check_threshold("max_chemical_tanimoto", max_chemical_tanimoto)
    if max_pairwise_chemical_tanimoto is not None:
        mcg_fp.check_threshold("max_pairwise_chemical_tanimoto", max_pairwise_chemical_tanimoto)
    scoring = chemical_scores or max_chemical_tanimoto is not None
    if reference_graph is not None and not scoring:
        raise ValueError("reference_graph is only read with chemical_scores or max_chemical_tanimoto")
    if not (scoring or unique or max_pairwise_chemical_tanimoto is not None):
        return Request(**shape, **solid_kw)
    if custom_finisher:
        raise ValueError("chemical scores cannot be combined with a custom finisher: its results carry no graph this "
                         "package can read")
    graph = None
    if scoring:
        src = reference_graph
        if src is None and hasattr(reference_conformer, "GetAtoms") and hasattr(reference_conformer, "GetBonds"):
            src = reference_conformer
        if src is None:
            raise ValueError("chemical scores need the reference's molecular graph: pass reference_graph= (a Mol, a "
                             "GeneratedMolecule or an (atomic_numbers, bond_orders) pair) or a reference conformer "
                             "with bonds; coordinates and a bare reference_context have none")
        graph = mcg_fp.mol_graph(src)
        if not 1 <= len(graph[0]) <= mcg_fp.MAX_GRAPH_ATOMS:
            raise ValueError(f"the reference graph must have 1 to {mcg_fp.MAX_GRAPH_ATOMS} heavy atoms, got "
                             f"{len(graph[0])}")
    return Request(ref_graph=graph, scores_chemistry=bool(scoring), max_chemical_tanimoto=max_chemical_tanimoto,
                   unique=bool(unique), max_pairwise_chemical_tanimoto=max_pairwise_chemical_tanimoto, **shape,
                   **solid_kw)


@dataclasses.dataclass
class Rows:
    """The rows one call may return, as parallel lists: what `select` filters and selects from, on either path."""
    item: List                                    # the `GeneratedMolecule` record or the finished Mol
    sample_id: List[int]
    shape: List[Optional[float]]                  # shape Tanimoto; None where the call does not score shape
    contacts: List[Optional[tuple]]               # (receptor_clashes, receptor_max_overlap); None: not measured
    chem: List[Optional[float]]                   # chemical Tanimoto to the reference's graph
    key: List[Optional[int]]                      # graph identity key
    row: List[int]                                # index into the device tensors behind the pair matrices
    outside: Optional[List[Optional[int]]] = None # atoms outside the mesh; None where not measured (the column: no mesh)

    def take(self, keep: List[int]) -> "Rows":
        """The rows at the positions `keep`, in that order."""
        return Rows(*(None if col is None else [col[i] for i in keep] for col in vars(self).values()))


def select(rows: Rows, req: Request, shape_pair, chem_pair) -> List:
    """The items of `rows` a call returns: the rows with at most `max_receptor_clashes` clashing atoms (one without
    contacts - its pose failed - does not pass), then those with at most `max_atoms_outside` atoms outside the mesh (one
    without a count - its pose failed - does not pass), then those with a chemical Tanimoto below `max_chemical_tanimoto` (NaN
    does not pass), then `unique` - of the rows with one graph key the first in ranking order
    (`cheminformatics.ranking_key`: by shape score where the call scores shape, else the lowest sample id), still in the
    input's order - then the threshold, the sphere exclusion at `max_pairwise_tanimoto` and at
    `max_pairwise_chemical_tanimoto` in one walk, and `top_k` (`cheminformatics.select_diverse`).  `shape_pair(rows)` /
    `chem_pair(rows)`: the [n,n] pair matrices of the surviving rows, each called only when its threshold is set."""
    if req.max_receptor_clashes is not None:
        rows = rows.take([i for i, c in enumerate(rows.contacts) if c is not None and c[0] <= req.max_receptor_clashes])
    if req.max_atoms_outside is not None:
        counts = rows.outside if rows.outside is not None else [None] * len(rows.item)
        rows = rows.take([i for i, c in enumerate(counts) if c is not None and c <= req.max_atoms_outside])
    if req.max_chemical_tanimoto is not None:
        rows = rows.take([i for i, s in enumerate(rows.chem) if s < req.max_chemical_tanimoto])
    if req.unique:
        order = sorted(range(len(rows.item)),
                       key=lambda i: cheminformatics.ranking_key(rows.shape[i], rows.sample_id[i]))
        rows = rows.take(mcg_fp.select_unique(rows.key, order))
    if not req.selects_by_shape and req.max_pairwise_chemical_tanimoto is None:
        return rows.item
    keep = cheminformatics.select_diverse(
        rows.shape, rows.sample_id, shape_pair(rows) if req.max_pairwise_tanimoto is not None else None,
        req.max_pairwise_tanimoto, req.top_k, req.min_shape_tanimoto,
        chem_pair(rows) if req.max_pairwise_chemical_tanimoto is not None else None, req.max_pairwise_chemical_tanimoto)
    return [rows.item[i] for i in keep]


def _pose_fn(gen, req: Request):
    """The posing seam of the call: `_pose_coords`, `_pose_coords_refined` when it asked for refinement, or `_pose_solid`
    when its reference is a mesh (the first argument, the reference's coordinates, is then None and not read)."""
    if req.ref_solid is not None:
        return lambda ref, coords, n: gen._pose_solid(req.ref_solid, coords, n)
    if req.refine_steps > 0:
        return lambda ref, coords, n: gen._pose_coords_refined(ref, coords, n, req.refine_steps)
    return gen._pose_coords


def fingerprints(gen, req: Request, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor):
    """The chemical step of padded graphs, one fingerprint launch: (fingerprints [B,64], graph keys [B] int64, chemical
    Tanimoto [B] to the reference's graph or None when the call does not score)."""
    fp, key, _ = gen._graph_fingerprints(atomic_numbers, bond_orders, n_nodes)
    sim = None
    if req.scores_chemistry:
        ref_fp = gen._graph_fingerprints(*mcg_fp.pad_graphs([req.ref_graph]))[0][0]
        sim = gen._chem_tanimoto(fp, ref_fp.to(fp.device))
    return fp, key, sim


def _score_fn(gen, req: Request):
    """The scoring seam of the call, as f(coords, n_nodes): `_score_coords`, or `_score_solid` when its reference is a mesh."""
    if req.ref_solid is not None:
        return lambda coords, n: gen._score_solid(req.ref_solid, coords, n)
    return lambda coords, n: gen._score_coords(req.ref_coord, coords, n)


def _pair_fn(gen, req: Request):
    """The pair-matrix seam of the call, as f(coords, n_nodes): `_pair_coords`, or `_pair_solid`."""
    if req.ref_solid is not None:
        return lambda coords, n: gen._pair_solid(req.ref_solid, coords, n)
    return lambda coords, n: gen._pair_coords(req.ref_coord, coords, n)


def _index(rows: Rows, device) -> torch.Tensor:
    return torch.tensor(rows.row, dtype=torch.long, device=device)


# ----------------------------------------------------------------------------------------------- without a finisher
def measure_tensors(gen, req: Request, res: dict) -> dict:
    """Stages 1-3 on one shard's result tensors.  `res` with `x` posed and the per-sample tensors `overlay_tanimoto`,
    `pose` [B,12] (rotation row-major, then translation; NaN where posing failed), `shape_tanimoto`, `receptor_clashes`
    (-1 where posing failed), `receptor_max_overlap` (NaN there) and - posed into a mesh - `atoms_outside` (-1 where posing
    failed) added, as far as the call asked."""
    if req.overlay:
        ov = _pose_fn(gen, req)(req.ref_coord, res["x"], res["n_nodes"])
        res = dict(res, x=ov["coords"], overlay_tanimoto=ov["tanimoto"],
                   pose=torch.cat([ov["rotation"].reshape(-1, 9), ov["translation"].reshape(-1, 3)], dim=1))
        if req.ref_solid is not None:
            res["atoms_outside"] = ov["atoms_outside"]
    if req.scores_shape:
        res = dict(res, shape_tanimoto=_score_fn(gen, req)(res["x"], res["n_nodes"]))
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
    chem_kw, fp = {}, None
    if req.needs_fingerprints:
        fp, key, sim = fingerprints(gen, req, res["elements"], res["bond"], res["n_nodes"])
        chem_kw = dict(chemical_tanimoto=sim, graph_key=key if req.tags_graph_keys else None)
    if gen.device.type == "cuda":
        torch.cuda.synchronize(gen.device)        # (the D2H copies below would wait anyway: keep that out of the figure)
    t0 = time.perf_counter()
    mols = molecules_from_tensors(res["x"], res["elements"], res["bond"], res["n_nodes"], res["valid"],
                                  sample_ids=row_ids, shape_tanimoto=res.get("shape_tanimoto"),
                                  overlay_tanimoto=res.get("overlay_tanimoto"), pose=res.get("pose"),
                                  receptor_clashes=res.get("receptor_clashes"),
                                  receptor_max_overlap=res.get("receptor_max_overlap"),
                                  atoms_outside=res.get("atoms_outside"), strain_before=res.get("strain_before"),
                                  strain_after=res.get("strain_after"), **chem_kw)
    gen.last_host_assembly_ms = (time.perf_counter() - t0) * 1e3      # D2H of the result tensors + record views
    kept, gen.last_valid_fraction = _finish(mols, optimise_geometry, use_rdkit=False)    # no finisher: the proxy
    if not req.removes:
        return kept
    rows = Rows(kept, [m.sample_id for m in kept], [m.shape_tanimoto for m in kept],
                [m.receptor_contacts for m in kept], [m.chemical_tanimoto for m in kept], [m.graph_key for m in kept],
                [m.batch_row for m in kept], [m.atoms_outside for m in kept])

    def shape_pair(left: Rows):
        x = res["x"]
        idx = _index(left, x.device)
        return _pair_fn(gen, req)(x.index_select(0, idx), res["n_nodes"].reshape(-1).to(x.device).index_select(0, idx))
    return select(rows, req, shape_pair, lambda left: gen._chem_pair(fp.index_select(0, _index(left, fp.device))))


# ----------------------------------------------------------------------------------------------- through a finisher
def _heavy_coords(mols: List):
    """(padded [B, max n, 3], n_nodes [B]) of Mols' heavy-atom conformer positions."""
    return cheminformatics.padded_coords([cheminformatics.mol_heavy_coords(m) for m in mols])


def score_mols(gen, ref_coord: torch.Tensor, mols: List, score_fn=None) -> List[Optional[float]]:
    """Shape Tanimoto of finished Mols' heavy-atom conformer positions (None where a molecule was dropped), in ONE
    batched device call.  `score_fn(coords, n_nodes)`: what scores them (default: `_score_coords` against `ref_coord`)."""
    if score_fn is None:
        score_fn = lambda coords, n: gen._score_coords(ref_coord, coords, n)      # noqa: E731
    live = [k for k, m in enumerate(mols) if m is not None]
    out: List[Optional[float]] = [None] * len(mols)
    if live:
        for k, v in zip(live, score_fn(*_heavy_coords([mols[k] for k in live])).cpu().tolist()):
            out[k] = float(v)
    return out


def _contact_mols(gen, rec: tuple, mols: List, poses: List) -> List[Optional[tuple]]:
    """(receptor_clashes, receptor_max_overlap) of posed Mols' heavy atoms (elements from `GetAtomicNum()`), in ONE
    batched device call; None where a Mol was dropped or its pose failed (it is not in the receptor's frame)."""
    live = [k for k, m in enumerate(mols) if m is not None and poses[k] is not None and poses[k][1] is not None]
    out: List[Optional[tuple]] = [None] * len(mols)
    if live:
        coords, n = _heavy_coords([mols[k] for k in live])
        z = torch.zeros(coords.shape[0], coords.shape[1], dtype=torch.long)
        for j, k in enumerate(live):
            heavy = [a.GetAtomicNum() for a in mols[k].GetAtoms() if a.GetAtomicNum() != 1]
            z[j, : len(heavy)] = torch.tensor(heavy, dtype=torch.long)
        clashes, worst = mcg_receptor.clash_summary(gen._receptor_coords(rec, coords, n, z))
        for j, (c, w) in enumerate(zip(clashes.cpu().tolist(), worst.cpu().tolist())):
            out[live[j]] = (int(c), float(w))
    return out


def measure_finished(gen, req: Request, done: List, res: Optional[dict] = None) -> List[tuple]:
    """Stages 1-3 on one shard's finished Mols (None = dropped), each in ONE batched device call: pose, every conformer
    position moved (`cheminformatics.pose_mols`), then score (`score_mols`), then the receptor contacts of the posed
    Mols.  Per sample (Mol, shape Tanimoto, (overlay_tanimoto, rotation, translation), (receptor_clashes,
    receptor_max_overlap), atoms outside the mesh), None where the call did not ask, the Mol was dropped or - the last
    two - its pose failed: the one value per sample that crosses the object gather.  `res`: the shard's result tensors;
    where the call relaxed (`strain_before` / `strain_after` in it) a sixth value follows, that pair as floats."""
    none = [None] * len(done)
    extra = ()
    if res is not None and "strain_before" in res:
        extra = (list(zip(res["strain_before"].cpu().tolist(), res["strain_after"].cpu().tolist())),)
    pose_fn, counts = _pose_fn(gen, req), []
    if req.overlay and req.ref_solid is not None:
        def pose_fn(ref, coords, n, _solid=pose_fn):        # the one batched call of `pose_mols`: keep its counts
            ov = _solid(ref, coords, n)
            counts.extend(ov["atoms_outside"].cpu().tolist())
            return ov
    poses = cheminformatics.pose_mols(req.ref_coord, done, overlay_fn=pose_fn) if req.overlay else none
    outside = list(none)
    for c, k in zip(counts, [k for k, m in enumerate(done) if m is not None]):
        outside[k] = None if c < 0 else int(c)
    scores = score_mols(gen, req.ref_coord, done, _score_fn(gen, req)) if req.scores_shape else none
    contacts = _contact_mols(gen, req.receptor, done, poses) if req.receptor is not None else none
    return list(zip(done, scores, poses, contacts, outside, *extra))


def return_finished(gen, req: Request, samples: List[tuple], row_ids: Optional[torch.Tensor],
                    sample_seed: Optional[int]) -> List:
    """What a call returns through a finisher, from the (gathered) `measure_finished` values of the rows this rank returns
    (sample ids `row_ids`, default 0..B-1): stages 4-6.  The Mols get their properties here, behind the object gather,
    which does not carry them - `sample_id` (seeded calls), `overlay_tanimoto`, `shape_tanimoto`, `receptor_clashes`,
    `receptor_max_overlap`, `atoms_outside`, `strain_before` / `strain_after` (a call that relaxed), and from the chemical
    step, which reads the live Mols' own graphs
    (`fingerprint.mol_graph`) in one batched device call, the double property `chemical_tanimoto` and the string property
    `graph_key` (the unsigned 64-bit key in decimal: it does not fit an int property).  Then `select`, the shape pair
    matrix taken from the surviving Mols' posed heavy atoms."""
    from . import rdkit_finish
    mols = [s[0] for s in samples]
    ids = list(range(len(mols))) if row_ids is None else row_ids.tolist()
    if sample_seed is not None:
        rdkit_finish.tag_sample_ids(mols, ids)
    gen.last_host_assembly_ms = 0.0
    live = [i for i, m in enumerate(mols) if m is not None]
    gen.last_valid_fraction = len(live) / len(mols) if mols else 0.0
    if req.relax_steps:
        strain = [samples[i][5] if len(samples[i]) > 5 else None for i in live]
        rdkit_finish.tag_scores([mols[i] for i in live], "strain_before", [None if s is None else s[0] for s in strain])
        rdkit_finish.tag_scores([mols[i] for i in live], "strain_after", [None if s is None else s[1] for s in strain])
    if not req.measures:
        return [mols[i] for i in live]
    rows = Rows([mols[i] for i in live], [ids[i] for i in live], [samples[i][1] for i in live],
                [samples[i][3] for i in live], [None] * len(live), [None] * len(live), list(range(len(live))),
                [samples[i][4] if len(samples[i]) > 4 else None for i in live])
    overlays = [None if samples[i][2] is None else samples[i][2][0] for i in live]
    rdkit_finish.tag_scores(rows.item, "overlay_tanimoto", overlays)
    rdkit_finish.tag_scores(rows.item, "shape_tanimoto", rows.shape)
    rdkit_finish.tag_contacts(rows.item, rows.contacts)
    rdkit_finish.tag_atoms_outside(rows.item, rows.outside)
    fp = None
    if req.needs_fingerprints and live:
        fp, key, sim = fingerprints(gen, req, *mcg_fp.pad_graphs([mcg_fp.mol_graph(m) for m in rows.item]))
        rows.key = [int(k) & 0xFFFFFFFFFFFFFFFF for k in key.cpu().tolist()]
        if req.scores_chemistry:
            rows.chem = [float(v) for v in sim.cpu().tolist()]
            rdkit_finish.tag_scores(rows.item, "chemical_tanimoto", rows.chem)
        if req.tags_graph_keys:
            rdkit_finish.tag_graph_keys(rows.item, rows.key)

    def chem_pair(left: Rows):
        if fp is None:                            # nothing left to compare
            return torch.zeros(0, 0)
        return gen._chem_pair(fp.index_select(0, _index(left, fp.device)))
    return select(rows, req, lambda left: _pair_fn(gen, req)(*_heavy_coords(left.item)), chem_pair)
