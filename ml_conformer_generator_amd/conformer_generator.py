"""`MLConformerGenerator` - drop-in for the reference class on the denoising hot path.

Same constructor kwargs, method names, argument order and errors as
`mlconfgen.MLConformerGenerator` (conformer_generator.py:19-399).  Differences, all
forced by the scope of this build:
  * `device` must be a ROCm GPU (default cuda:0): there is no CPU path;
  * `edm_weights` / `adj_mat_seer_weights` may also be an in-memory state dict;
  * the RDKit-owned stages BEFORE the GCN run as the native hand-off of `handoff.py` (one HIP launch).  Its two
    RDKit-owned decisions - canonical-SMILES atom order and 1-order connectivity (`canonicalise`, mol_utils.py:110-126) -
    are inputs of that launch, supplied by `atom_order_provider`: "auto" (default) = RDKit's where RDKit imports
    (`rdkit_order.rdkit_provider`, the reference's own call sequence), else the labelled substitutes (generation order,
    covalent-radius rule); a callable = the caller's own; None = the substitutes.  AdjMatSeer depends on the atom
    order, so with a trained checkpoint the substitutes predict different bonds than the reference.  The returned
    molecules carry their atoms in the order the GCN saw them, like the reference's `canonicalised_samples`;
  * RETURN TYPE: where RDKit imports, `generate_conformers` returns `List[Chem.Mol]` like the
    reference - the HIP path's molecules go through `rdkit_finish.finish` (the reference's
    `standardize_mol` sequence incl. MMFF when `optimise_geometry`; untested offline, RDKit is
    absent here); without RDKit it returns `GeneratedMolecule` records filtered by the labelled
    valence / single-fragment PROXY, and `optimise_geometry=True` cannot be honoured (one
    warning per process).  An RDKit Mol is accepted as reference conformer / fixed fragment;
  * `n_host_workers` (default min(32, this rank's share of the host cores); 0 = serial): the two RDKit stages - canonical order + connectivity
    before the GCN, `redefine_bonds` + `standardize_mol` (MMFF) behind it - are fanned out over a pool of fresh worker
    processes (`host_pool.py`) and pipelined against the GPU per group of molecules; the reference runs them one molecule
    at a time on the calling thread (conformer_generator.py:343-366).  Same per-molecule code, same results, same order;
    the workers are started in the background BEFORE the sampler is launched, and every task has a deadline
    (`task_timeout_s`, default 60 s per chunk of <= 8 molecules; None = none): a worker stuck inside RDKit is killed and
    replaced and its molecules are dropped like any other the gate rejects (utils/standardizer.py:108-109), with a warning;
  * `cpu_affinity` (default None = leave the process alone; "auto" = pin this process - torch's threads and the host
    pool's workers, which inherit the mask - to the cores of its GPU's NUMA node, shared between the ranks of the node:
    `affinity.py`, sysfs only, no HIP call; or an explicit list of cores);
  * `generate_conformers_sharded(...)`: the same call, batch-sharded over the ranks of an
    initialised `torch.distributed` group (one process per GPU, one gather at the end);
  * `sample_seed` (opt-in, every generation entry): molecule i's size and every noise draw are a function of
    (sample_seed, i) alone - the same molecule in any batch, at any row, on any rank.  Seeded calls
    consume neither the CPU nor the device torch RNG.  Default (None): the reference's torch draw order, unchanged;
  * opt-in keywords of every generation entry, all off by default (nothing changes); their meaning is stated once, in
    `generate_conformers`' docstring, and what they do behind the generation lives in `postprocess.py`:
      `shape_scores`, `top_k`, `min_shape_tanimoto`: score every returned molecule's shape against the reference; select;
      `overlay`, `refine_overlay`: pose every returned molecule onto the reference conformer; refine that pose;
      `max_pairwise_tanimoto`: a shape-diverse selection of the posed molecules;
      `receptor`, `max_receptor_clashes`: steric contacts of the posed molecules with a receptor; a filter on them;
      `relieve_clashes`: the posed molecules nudged, as rigid bodies, out of their clashes with the receptor first;
      `chemical_scores`, `reference_graph`, `max_chemical_tanimoto`: chemical similarity to the reference; a filter;
      `unique`, `max_pairwise_chemical_tanimoto`: one molecule per graph; a chemically diverse selection;
      `pharmacophore_scores`, `reference_pharmacophore`, `min_pharmacophore_tanimoto`, `rank_by`: does the posed molecule
      keep the reference's interaction pattern - the overlap of its pharmacophore features with the reference's; a
      filter; ranking by shape + pharmacophore score;
      `electrostatic_scores`, `reference_charges`, `min_electrostatic_tanimoto`, `partial_charges`: does the posed molecule
      present the reference's charge distribution - partial charges by electronegativity equalisation and the Tanimoto
      of their Coulomb overlap with the reference's; a filter; `rank_by="electrostatic"`;
      `interaction_scores`, `max_interaction_score`: does the posed molecule interact with the receptor - an empirical
      interaction score with its terms, a hydrogen-bond count and per-atom contributions; a filter;
      `rank_by="interaction"`;
  * `reference_shape`, `shape_density` (every generation entry): a watertight triangle mesh - an STL file, a (vertices,
    faces) pair - as the reference, what the reference's notebook does with `trimesh` (`mesh.py`, no `trimesh` needed);
    the shape options then score, pose and select against the solid, and `max_atoms_outside` filters on the posed atoms
    that lie outside it; or a `pocket.Pocket` (`pocket.find_pocket(receptor, center)`: the cavity of a receptor at a place
    on it, found on the GPU), whose mesh it is and whose own receptor every receptor option of the call then reads;
  * `relax_geometry` (every generation entry; off by default): every generated molecule's heavy atoms are relaxed on the
    GPU, right behind the bond write-back, on the package's OWN restrained valence force field (`geometry.py`; NOT MMFF94),
    and everything downstream reads the relaxed coordinates.  Independent of `optimise_geometry`, whose meaning and
    warning are unchanged;
  * `standardize` (every generation entry; off by default; records path only): every generated graph is standardised on
    the GPU, right behind the bond write-back and before the relaxation - largest fragment, valence / aromatic-bridge
    checks, a Kekule form (`standardize.py`: the package's OWN definition, NOT RDKit's FragmentParent / Kekulize /
    SanitizeMol) - and everything downstream reads the parent fragment; validity is then that stage's verdict instead of
    the proxy's.
"""
from __future__ import annotations

import contextlib
import os
import time
import warnings
from typing import List, Optional, Union

import torch

from . import _lib
from . import cheminformatics
from . import seeding
from .adj_mat_seer import AdjMatSeer
from .config import (ATOM_DECODER, CONTEXT_NORMS, DIMENSION, MAX_N_NODES, MIN_N_NODES, NOISE_PRECISION,
                     NUM_BOND_TYPES)
from .egnn import EGNNDynamics
from .elements import class_z_from_decoder
from .equivariant_diffusion import EquivariantDiffusion, PredefinedNoiseSchedule
from . import distributed as mcg_dist
from . import host_pool
from . import postprocess
from . import rdkit_order
from . import receptor as mcg_receptor
from . import canonical as mcg_canonical
from . import stereo as mcg_stereo
from . import scaffold as mcg_scaffold
from . import substructure as mcg_sub
from . import fingerprint as mcg_fp
from . import geometry as mcg_geometry
from . import electrostatics as mcg_esp
from . import hydrogens as mcg_hydrogens
from . import interactions as mcg_interactions
from . import pharmacophore as mcg_pharm
from . import standardize as mcg_standardize
from .handoff import (GeneratedMolecule, assemble_molecules, bond_writeback_hip, molecules_from_tensors,
                      prepare_adj_mat_seer_input_hip)
from .mol_utils import (get_context_shape, ifm_get_xh_from_fragment, ifm_merge_hip,
                        ifm_prepare_gen_fragment_context, parse_molblock_heavy_atoms, prepare_edm_input,
                        prepare_fragment)

try:  # RDKit is optional on this path
    from rdkit import Chem  # type: ignore
    HAVE_RDKIT = True
except Exception:  # noqa: BLE001
    Chem = None
    HAVE_RDKIT = False


_WARNED_NO_MMFF = [False]


def _finish(mols: List, optimise_geometry: bool, use_rdkit: Optional[bool] = None):
    """(returned list, valid fraction): the reference's RDKit gate where RDKit exists (serial form; the generator's own
    route is the staged, pooled `rdkit_finish.FinishStage`), else the proxy filter."""
    if not mols:
        return [], 0.0
    if HAVE_RDKIT if use_rdkit is None else use_rdkit:
        from . import rdkit_finish
        done = rdkit_finish.finish(mols, optimise_geometry)
        kept = [m for m in done if m is not None]
        return kept, len(kept) / len(mols)
    if optimise_geometry and not _WARNED_NO_MMFF[0]:
        _WARNED_NO_MMFF[0] = True
        warnings.warn("ml_conformer_generator_amd: RDKit is not installed - optimise_geometry=True (MMFF94) is NOT applied and "
                      "validity is the labelled valence / single-fragment proxy; pass optimise_geometry=False to silence this",
                      RuntimeWarning, stacklevel=4)
    kept = [m for m in mols if m.valid]
    return kept, len(kept) / len(mols)


def _load_state_dict(src, device) -> dict:
    if isinstance(src, dict):
        return src["state_dict"] if "state_dict" in src else src
    return torch.load(src, map_location="cpu")["state_dict"]      # conformer_generator.py:90-102


class MLConformerGenerator(torch.nn.Module):
    def __init__(self, diffusion_steps: int = 100, device: Optional[torch.device] = None,
                 dimension: int = DIMENSION, num_bond_types: int = NUM_BOND_TYPES,
                 min_n_nodes: int = MIN_N_NODES, max_n_nodes: int = MAX_N_NODES,
                 context_norms: dict = CONTEXT_NORMS, atom_decoder: dict = ATOM_DECODER,
                 edm_weights: Union[str, dict] = "./edm_moi_chembl_15_39.pt",
                 adj_mat_seer_weights: Union[str, dict] = "./adj_mat_seer_chembl_15_39.pt",
                 compute_dtype: str = "f32", atom_order_provider="auto", n_host_workers: Optional[int] = None,
                 finisher="auto", task_timeout_s: Optional[float] = host_pool.DEFAULT_TASK_TIMEOUT_S, cpu_affinity=None):
        """The reference's constructor (conformer_generator.py:29-113) plus the options of this package.

        `atom_decoder` {class index 0..7: element symbol} decides which element each generated atom becomes, as in the
        reference (`samples_to_rdkit_mol` writes atom_decoder[argmax(h)], utils/mol_utils.py:41-45): the atomic numbers the
        GCN embeds, the covalent-radius connectivity, the validity proxy, an atom-order provider's input and the returned
        molecules all follow it.  Any element of `config.ELEMENTS` (B C N O F Si P S Cl As Se Br) may be named, two classes
        may name the same one.  Refused with ValueError, here, before any device work: other keys than exactly 0..7,
        hydrogen (every count of this API is heavy atoms), an unknown symbol and Z >= 36 (outside the GCN's element
        embedding, where the reference fails later with an IndexError).  The radii and valences of the non-default
        elements feed only the labelled substitutes (covalent-radius connectivity, validity proxy); they are literature
        values, not pinned against RDKit.  A `fixed_fragment` keeps the reference's FIXED class encoding
        (`elements_decoder` of sorted PERMITTED_ELEMENTS, utils/molgraph.py:10,236-252), not `atom_decoder` - the
        reference's own behaviour.  `dimension` and `num_bond_types` other than the defaults are refused."""
        super().__init__()
        class_z = class_z_from_decoder(atom_decoder)        # a bad decoder fails before anything else is set up
        _lib.lib()       # fail loudly if the HIP library is not built
        device = torch.device("cuda:0" if device is None else device)
        if device.type != "cuda":
            raise ValueError("ml_conformer_generator_amd runs the hot path on an MI355X only; "
                             f"device={device} is not supported (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        # placement first: threads and worker processes created from here on inherit it (affinity.py; sysfs only)
        self.cpu_affinity = None
        if cpu_affinity is not None:
            from . import affinity
            cpus = affinity.rank_cpus(int(os.environ.get("LOCAL_RANK", "0") or 0),
                                      int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1),
                                      device.index) if cpu_affinity == "auto" else list(cpu_affinity)
            self.cpu_affinity = affinity.pin(cpus)
        self.dimension = dimension
        self.context_norms = {k: torch.tensor(v) for k, v in context_norms.items()}
        self.atom_decoder = atom_decoder
        self.class_z = class_z           # atomic number of each atom class: what the device hand-off decodes with
        self.min_n_nodes, self.max_n_nodes = min_n_nodes, max_n_nodes

        net_dynamics = EGNNDynamics(in_node_nf=9, context_node_nf=3, hidden_nf=420, device=device)
        generative_model = EquivariantDiffusion(dynamics=net_dynamics, in_node_nf=8, timesteps=1000,
                                                noise_precision=NOISE_PRECISION)
        adj_mat_seer = AdjMatSeer(dimension=dimension, n_hidden=2048, embedding_dim=64, num_embeddings=36,
                                  num_bond_types=num_bond_types, device=device)
        generative_model.load_state_dict(_load_state_dict(edm_weights, device))
        net_dynamics.set_precision(compute_dtype)      # opt-in: "bf16" reduced-precision operands, "f32x6" split-operand fp32
        adj_mat_seer.load_state_dict(_load_state_dict(adj_mat_seer_weights, device))
        self.generative_model = generative_model
        self.set_diffusion_steps(diffusion_steps)
        self.adj_mat_seer = adj_mat_seer
        # (atomic_numbers, coords[n,3]) -> (order, connectivity) | None per molecule: see rdkit_order.py
        self.atom_order_provider = rdkit_order.default_provider() if atom_order_provider == "auto" else atom_order_provider
        # RDKit finish behind the GCN (`redefine_bonds` + `standardize_mol`): "auto" = RDKit's where RDKit imports, else None
        # (the labelled proxy filter); a `host_pool.TaskRef` = the caller's chunk function; None = the proxy filter
        self.finisher = ("rdkit" if HAVE_RDKIT else None) if finisher == "auto" else finisher
        # host fan-out of the two RDKit stages (host_pool.py): worker PROCESSES, created at first use; 0 = this thread
        self.n_host_workers = host_pool.default_workers() if n_host_workers is None else int(n_host_workers)
        if self.cpu_affinity and n_host_workers is None:
            self.n_host_workers = max(1, min(self.n_host_workers, len(self.cpu_affinity)))     # one worker per pinned core at most
        self.task_timeout_s = task_timeout_s      # deadline of one host task (a chunk of molecules); None = none
        self._finish_stage = None    # rdkit_finish.FinishStage of the shard generated last (consumed by the callers)
        self.last_host_order_ms = None    # wall time from the first order task to the last group's hand-off launch
        self.last_host_finish_ms = None   # wall time spent waiting for finish results after the last group was submitted
        self.last_batch = None       # tensors of the most recent generation (x, h, n_nodes, bond)
        self.last_order = None
        self.last_valid_fraction = None   # share of the last batch that passed the validity proxy
        self.last_noise_seed = None       # device-generator seed of the last sharded call on this rank
        self.last_host_assembly_ms = None # host time of the last call's D2H + molecule records (0.0 through a finisher)
        self._timing = None          # bench.py: {"sampler_start", "sampler_end"} events recorded around the sampler

    def set_diffusion_steps(self, diffusion_steps: int) -> None:
        """Re-wire the noise schedule to `diffusion_steps` denoising steps, exactly as the reference's constructor does
        (conformer_generator.py:105-113); weights, plans and captured graphs are untouched."""
        gm = self.generative_model
        gm.gamma = PredefinedNoiseSchedule(timesteps=diffusion_steps, precision=NOISE_PRECISION)
        gm.time_steps = torch.flip(torch.arange(0, diffusion_steps), dims=[0])
        gm.T = diffusion_steps
        self.diffusion_steps = diffusion_steps

    # ------------------------------------------------------------------ EDM stage
    @torch.no_grad()
    def edm_tensors(self, reference_context: torch.Tensor, n_samples: int = 100, max_n_nodes: int = 32,
                    min_n_nodes: int = 25, resample_steps: int = 0, fixed_fragment=None,
                    inertial_fragment_matching: bool = True, blend_power: int = 3, ifm_diffusion_level: int = 50,
                    sizes: Optional[torch.Tensor] = None, sample_seed: Optional[int] = None,
                    sample_ids: Optional[torch.Tensor] = None):
        """Tensor form of `edm_samples` (conformer_generator.py:125-266): x[B,N,3], h[B,N,8], node_mask.
        `sizes`: molecule sizes drawn by the caller (the sharded path) instead of here.
        `sample_seed` in [0, 2^64): row b is sample `sample_ids[b]` (default arange(n_samples)) of the keyed stream - its
        size (unless `sizes` is given) and every noise draw of every sampler run depend on (sample_seed, sample_ids[b])
        only, and neither torch generator is consumed.  `sample_ids` regenerates chosen molecules;
        it needs a `sample_seed`.  A recorded noise tape (`generative_model.noise_fn`) and a seed are refused."""
        gm = self.generative_model
        if sample_seed is None:
            if sample_ids is not None:
                raise ValueError("sample_ids needs a sample_seed")
            keyed = lambda run: contextlib.nullcontext()              # noqa: E731
        else:
            seeding.check_seed(sample_seed)
            if gm.noise_fn is not None:
                raise ValueError("a recorded noise tape (noise_fn) and a sample_seed cannot be combined")
            sample_ids = seeding.check_sample_ids(torch.arange(n_samples) if sample_ids is None else sample_ids, n_samples)
            ids_dev = sample_ids.to(self.device)                      # the call's one H2D copy of the ids
            keyed = lambda run: gm.keyed(sample_seed, ids_dev, run)   # noqa: E731
        min_n_nodes = max(min_n_nodes, self.min_n_nodes)            # :156-160
        max_n_nodes = min(max_n_nodes, self.max_n_nodes)
        node_mask, edge_mask, batch_context = prepare_edm_input(
            n_samples=n_samples, reference_context=reference_context, context_norms=self.context_norms,
            min_n_nodes=min_n_nodes, max_n_nodes=max_n_nodes, device=self.device, sizes=sizes,
            sample_seed=sample_seed, sample_ids=sample_ids)
        ev = self._timing
        if ev is not None:
            ev["sampler_start"].record()
        if fixed_fragment is None:
            with keyed(0):
                x, h = gm(node_mask, edge_mask, batch_context, resample_steps)
        elif inertial_fragment_matching:
            # generate the complementary fragments separately, then merge (:179-240)
            n_nodes = torch.sum(node_mask, dim=1).to(torch.long)
            ff_x, ff_h = ifm_get_xh_from_fragment(fixed_fragment, self.device)
            f_nm, f_em, f_ctx, shift, rotation = ifm_prepare_gen_fragment_context(
                fixed_fragment_x=ff_x, reference_context=reference_context, n_nodes=n_nodes,
                context_norms=self.context_norms, max_n_nodes=max_n_nodes, min_n_nodes=min_n_nodes,
                device=self.device)
            with keyed(0):
                xg, hg = gm(f_nm, f_em, f_ctx, resample_steps)
            # inverse_coord_transform + ifm_prepare_fragments_for_merge: one HIP launch on the device outputs
            z_known, fixed_mask = ifm_merge_hip(ff_x, ff_h, xg, hg, shift, rotation, self.device, max_n_nodes)
            with keyed(1):
                x, h = gm.merge_fragments(node_mask=node_mask, edge_mask=edge_mask, fixed_mask=fixed_mask,
                                          context=batch_context, z_known=z_known, diffusion_level=ifm_diffusion_level,
                                          resample_steps=resample_steps, blend_power=blend_power)
        else:
            z_known, fixed_mask = prepare_fragment(n_samples=n_samples, fixed_fragment=fixed_fragment,
                                                   max_n_nodes=max_n_nodes, min_n_nodes=min_n_nodes,
                                                   device=self.device)
            with keyed(0):
                x, h = gm.inpaint(node_mask, edge_mask, batch_context, z_known, fixed_mask, resample_steps, blend_power)
        if ev is not None:
            ev["sampler_end"].record()
        return x, h, node_mask

    @torch.no_grad()
    def edm_samples(self, reference_context: torch.Tensor, n_samples: int = 100, max_n_nodes: int = 32,
                    min_n_nodes: int = 25, resample_steps: int = 0, fixed_fragment=None,
                    inertial_fragment_matching: bool = True, blend_power: int = 3, ifm_diffusion_level: int = 50,
                    sample_seed: Optional[int] = None):
        """Samples without bonds (conformer_generator.py:125-266): `List[Chem.Mol]` through `samples_to_rdkit_mol`'s XYZ
        route where RDKit imports (`rdkit_finish.samples`, untested offline), else `GeneratedMolecule` records.  Atoms in
        generation order, as in the reference (canonicalisation happens later, in `generate_conformers`).
        `sample_seed`: as in `edm_tensors`; the Mols then carry the int property `sample_id`."""
        x, h, node_mask = self.edm_tensors(reference_context, n_samples, max_n_nodes, min_n_nodes, resample_steps,
                                           fixed_fragment, inertial_fragment_matching, blend_power,
                                           ifm_diffusion_level, sample_seed=sample_seed)
        n_nodes = node_mask.sum(1).reshape(-1).to(torch.long)
        el, _, _ = prepare_adj_mat_seer_input_hip(x, h, n_nodes, self.dimension, class_z=self.class_z)
        no_bonds = torch.zeros(x.shape[0], self.dimension, self.dimension, dtype=torch.int8, device=x.device)
        mols = assemble_molecules(x, el, no_bonds, n_nodes)
        for m in mols:
            m.valid = True          # no bonds yet: the connectivity proxy does not apply
        if HAVE_RDKIT:
            from . import rdkit_finish
            return rdkit_finish.samples(mols, self._executor(),
                                        sample_ids=None if sample_seed is None else range(len(mols)))
        return mols

    # ------------------------------------------------------------------ full pipeline
    @staticmethod
    def _reference_coord(reference_conformer) -> torch.Tensor:
        """Heavy-atom coordinates [n,3] fp32 of a reference conformer (RDKit Mol, mol block or tensor)."""
        if HAVE_RDKIT and not isinstance(reference_conformer, (str, torch.Tensor)):
            mol = Chem.RemoveHs(reference_conformer)                           # :302-307
            return torch.tensor(mol.GetConformer().GetPositions(), dtype=torch.float32)
        if isinstance(reference_conformer, str):
            return parse_molblock_heavy_atoms(reference_conformer)[0]
        return torch.as_tensor(reference_conformer, dtype=torch.float32)

    def _reference_context(self, reference_conformer, reference_context, n_atoms, reference=None,
                           shape_density: float = 0.02):
        if isinstance(reference, cheminformatics.SolidReference):          # a mesh: the notebook's principal_inertia_components at `density`, with n_atoms
            if not n_atoms:
                raise ValueError(
                    "Reference Number of Atoms should be provided, when generating samples using context.")
            from . import mesh as mcg_mesh
            return mcg_mesh.mesh_context(reference.mesh, shape_density), n_atoms
        if reference_conformer is not None and reference_conformer is not False:
            ref_coord = self._reference_coord(reference_conformer)
            ref_n_atoms = int(ref_coord.shape[0])
            ref_coord = ref_coord - torch.mean(ref_coord, dim=0)              # :310-311
            ref_context, _ = get_context_shape(ref_coord)
            return ref_context, ref_n_atoms
        if reference_context is not None:
            if not n_atoms:
                raise ValueError(
                    "Reference Number of Atoms should be provided, when generating samples using context.")
            return reference_context, n_atoms
        raise ValueError(
            "Either a reference RDkit Mol object or context as torch.Tensor should be provided for generation.")

    # device seams of the opt-in stages: `postprocess.py` calls them through the instance, the host tests stub them there
    # the chemical step
    def _graph_fingerprints(self, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor):
        """(fingerprint [B,64] int32, graph key [B] int64, set bits [B]) of padded graphs (`fingerprint.graph_fingerprints`,
        unchecked: the codes come from the bond write-back or from `mol_graph`)."""
        return mcg_fp.graph_fingerprints(atomic_numbers, bond_orders, n_nodes, self.device, check=False)

    def _chem_tanimoto(self, fp: torch.Tensor, ref_fp: torch.Tensor) -> torch.Tensor:
        """Tanimoto [B] of fingerprints against the reference's (`fingerprint.fingerprint_tanimoto`)."""
        return mcg_fp.fingerprint_tanimoto(fp, ref_fp)

    def _chem_pair(self, fp: torch.Tensor) -> torch.Tensor:
        """[B,B] pairwise Tanimoto of fingerprints (`fingerprint.pairwise_fingerprint_tanimoto`)."""
        return mcg_fp.pairwise_fingerprint_tanimoto(fp)

    # the canonical step
    def _canonical_order(self, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor) -> dict:
        """The exact canonical labelling of padded graphs: `order`, `status`, `leaves`, `key` (`canonical.canonical_order`,
        unchecked: the codes come from the bond write-back or from `mol_graph`; device tensors)."""
        return mcg_canonical.canonical_order(atomic_numbers, bond_orders, n_nodes, self.device, check=False)

    def _stereo_order(self, coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor,
                      n_nodes: torch.Tensor) -> dict:
        """The stereo identity of padded, embedded graphs: `order`, `status`, `leaves`, `key`, `stereo`, `stereo_key`,
        `counts` (`stereo.stereo_order`, one launch per 16 384 rows)."""
        return mcg_stereo.stereo_order(coords, atomic_numbers, bond_orders, n_nodes, self.device, check=False)

    # the scaffold step
    def _ring_scaffolds(self, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor,
                        generic: bool) -> dict:
        """The rings and the scaffold (`generic`: the framework) of padded graphs (`scaffold.murcko_scaffolds`, unchecked:
        the codes come from the bond write-back or from `mol_graph`; device tensors, `identity` a host list): one launch
        of each entry of `scaffold.py`, and the sub-graphs' canonical labelling through `_canonical_order`."""
        return mcg_scaffold.murcko_scaffolds(atomic_numbers, bond_orders, n_nodes, self.device, generic, check=False,
                                             canonical_order=self._canonical_order)

    # the substructure step
    def _match_substructures(self, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor,
                             compiled) -> dict:
        """Every pattern of `compiled` (`substructure.compile_patterns`) matched against padded graphs: `count`, `status`,
        `first`, `covered` (`substructure.match_substructures`, unchecked: the codes come from the bond write-back or from
        `mol_graph`; device tensors).  The hydrogens (`hydrogens.implicit_counts`, host) are counted only where a pattern
        constrains them."""
        return mcg_sub.match_substructures(atomic_numbers, bond_orders, n_nodes, compiled, device=self.device, check=False)

    # the pharmacophore step
    def _pharm_perceive(self, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor):
        """(types [B,W] uint8, ring masks [B,32] int64, ring counts [B]) of padded graphs
        (`pharmacophore.perceive_features`)."""
        return mcg_pharm.perceive_features(atomic_numbers, bond_orders, n_nodes, self.device)

    def _pharm_score(self, reference_features, coords: torch.Tensor, n_nodes: torch.Tensor, types: torch.Tensor,
                     ring_mask: torch.Tensor, n_rings: torch.Tensor):
        """(Tanimoto [B] fp32, matches [B] int32) of posed, padded molecules' perceived features against the reference's
        (`pharmacophore.score_features`)."""
        out = mcg_pharm.score_features(reference_features, coords, n_nodes, types, ring_mask, n_rings, self.device)
        return out["tanimoto"], out["matches"]

    # the hydrogen step
    def _add_hydrogens(self, coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor,
                       n_nodes: torch.Tensor, perceived=None) -> dict:
        """The explicit hydrogens of padded heavy-atom coordinates and graphs (`hydrogens.add_hydrogens`, unchecked: the
        elements come from the validated decoder, the codes from the bond write-back; device tensors); `perceived`: a
        `_pharm_perceive` result for the same graphs, when the electrostatic step has one."""
        return mcg_hydrogens.add_hydrogens(coords, atomic_numbers, bond_orders, n_nodes, self.device, check=False,
                                           perceived=perceived)

    # the electrostatic step
    def _peoe_charges(self, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor,
                      perceived=None):
        """The partial charges of padded graphs (`electrostatics.partial_charges`, unchecked: the generator's own graphs);
        `perceived`: a `_pharm_perceive` result for the same graphs."""
        return mcg_esp.partial_charges(atomic_numbers, bond_orders, n_nodes, self.device, check=False, perceived=perceived)

    def _esp_score(self, reference_points, points: torch.Tensor, charges: torch.Tensor, n_points: torch.Tensor):
        """Electrostatic Tanimoto [B] fp32 of posed charge points against the reference's
        (`electrostatics.electrostatic_tanimoto`)."""
        return mcg_esp.electrostatic_tanimoto(reference_points, points, charges, n_points, self.device)["tanimoto"]

    # the interaction step
    def _interaction_scores(self, receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                            bond_orders: torch.Tensor) -> dict:
        """The interaction scores of posed, padded molecules with the call's typed receptor - a
        `interactions.prepare_receptor` result - (`interactions.interaction_scores`, unchecked: the generator's own
        graphs; device tensors)."""
        return mcg_interactions.interaction_scores(receptor, coords, n_nodes, atomic_numbers, bond_orders,
                                                   device=self.device, check=False)

    def _contact_fingerprint(self, receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                             bond_orders: torch.Tensor, reference=None) -> dict:
        """The contact fingerprints of posed, padded molecules with the call's grouped receptor - a
        `contacts.prepare_receptor` result - and, with `reference` (groups, kinds), their comparison with it
        (`contacts.contact_fingerprint`, device tensors)."""
        from . import contacts as mcg_contacts
        return mcg_contacts.contact_fingerprint(receptor, coords, n_nodes, atomic_numbers, bond_orders, reference=reference,
                                                device=self.device)

    def _optimise_pose(self, receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                       bond_orders: torch.Tensor, steps: int) -> dict:
        """Padded posed heavy-atom coordinates moved as rigid bodies downhill on the interaction score with the call's
        typed receptor - a `interactions.prepare_receptor` result - (`interactions.optimise_pose`, device tensors)."""
        return mcg_interactions.optimise_pose(receptor, coords, n_nodes, atomic_numbers, bond_orders, steps,
                                              device=self.device)

    def _optimise_pose_flex(self, receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                            bond_orders: torch.Tensor, steps: int) -> dict:
        """`_optimise_pose` with the rotatable bonds turned beside the rigid move and the intramolecular guard
        (`interactions.optimise_pose_flexible`, device tensors)."""
        return mcg_interactions.optimise_pose_flexible(receptor, coords, n_nodes, atomic_numbers, bond_orders, steps,
                                                       device=self.device)

    def _search_pose(self, receptor, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                     bond_orders: torch.Tensor, starts: int, steps: int, seed: int, sample_ids) -> dict:
        """`_optimise_pose_flex` from `starts` keyed starts per molecule, the best kept (`interactions.search_pose`, device
        tensors): the starts are keyed by `seed` and the rows' `sample_ids` (None: 0..B-1)."""
        return mcg_interactions.search_pose(receptor, coords, n_nodes, atomic_numbers, bond_orders, starts, steps,
                                            seed=seed, sample_ids=sample_ids, device=self.device)

    # the standardisation step
    def _standardize(self, coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor,
                     n_nodes: torch.Tensor) -> dict:
        """The standardised form of padded heavy-atom graphs - largest fragment, checks, Kekule form
        (`standardize.standardize_graphs`, unchecked: the codes come from the bond write-back; device tensors)."""
        return mcg_standardize.standardize_graphs(coords, atomic_numbers, bond_orders, n_nodes, self.device, check=False)

    # the geometry step
    def _relax_coords(self, coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor,
                      n_nodes: torch.Tensor, steps: int) -> dict:
        """Padded heavy-atom coordinates relaxed on the package's own force field (`geometry.relax_geometry`, unchecked:
        the elements come from the validated decoder, the codes from the bond write-back; device tensors)."""
        return mcg_geometry.relax_geometry(coords, atomic_numbers, bond_orders, n_nodes, steps, self.device, check=False)

    # the shape step
    def _score(self, reference, coords: torch.Tensor, n_nodes: torch.Tensor) -> torch.Tensor:
        """Shape Tanimoto [B] (device) of padded heavy-atom coordinates against the call's reference object
        (`cheminformatics.shape_scores`)."""
        return cheminformatics.shape_scores(reference, coords, n_nodes, self.device)[0]

    def _pose(self, reference, coords: torch.Tensor, n_nodes: torch.Tensor, refine_steps: int = 0) -> dict:
        """Padded heavy-atom coordinates posed onto the call's reference object, the pose refined when `refine_steps` > 0
        (`cheminformatics.shape_overlay`, device tensors; a solid's result also holds `atoms_outside`)."""
        return cheminformatics.shape_overlay(reference, coords, n_nodes, self.device, refine_steps=refine_steps)

    def _pair(self, reference, coords: torch.Tensor, n_nodes: torch.Tensor) -> torch.Tensor:
        """[B,B] pairwise shape Tanimoto (device) of padded heavy-atom coordinates posed onto the call's reference object
        (`cheminformatics.pairwise_shape_tanimoto`)."""
        return cheminformatics.pairwise_shape_tanimoto(reference, coords, n_nodes, self.device)

    def _receptor_coords(self, rec: tuple, coords: torch.Tensor, n_nodes: torch.Tensor,
                         atomic_numbers: torch.Tensor) -> torch.Tensor:
        """Per-atom receptor overlap [B,N] (device) of padded posed heavy-atom coordinates (`receptor.receptor_overlap`)."""
        return mcg_receptor.receptor_overlap(rec, coords, n_nodes, atomic_numbers, self.device)

    def _relieve(self, rec: tuple, coords: torch.Tensor, n_nodes: torch.Tensor, atomic_numbers: torch.Tensor,
                 steps: int) -> dict:
        """Padded posed heavy-atom coordinates moved out of their contacts with the receptor
        (`receptor.relieve_clashes`, device tensors)."""
        return mcg_receptor.relieve_clashes(rec, coords, n_nodes, atomic_numbers, steps, device=self.device)

    def _score_placed(self, reference, coords: torch.Tensor, n_nodes: torch.Tensor) -> torch.Tensor:
        """Shape Tanimoto [B] (device) of padded heavy-atom coordinates as placed in the reference's coordinates
        (`cheminformatics.shape_tanimoto_placed`)."""
        return cheminformatics.shape_tanimoto_placed(reference, coords, n_nodes, self.device)

    def _atoms_outside(self, reference, coords: torch.Tensor, n_nodes: torch.Tensor) -> torch.Tensor:
        """[B] int32 (device): the atoms of padded heavy-atom coordinates, placed in the mesh's own coordinates, that lie
        outside the call's solid reference (`cheminformatics.mesh_atoms_outside`; -1 for a non-finite row)."""
        dev = self.device
        return cheminformatics.mesh_atoms_outside(reference.on(dev)["triangles_own"], coords.to(dev),
                                                  n_nodes.to(dev), dev)

    def _executor(self):
        """Where the poolable host tasks run: the process-wide `HostPool` with `n_host_workers` workers and this generator's
        task deadline (workers created at the first submit or by `prestart`), or this thread."""
        return host_pool.shared_pool(self.n_host_workers, getattr(self, "task_timeout_s", host_pool.DEFAULT_TASK_TIMEOUT_S))

    def _generate_shard(self, ref_context, ref_n_atoms: int, variance: int, sizes: Optional[torch.Tensor],
                        n_samples: int, resample_steps, fixed_fragment, inertial_fragment_matching, blend_power,
                        ifm_diffusion_level, optimise_geometry: bool = True, sample_seed: Optional[int] = None,
                        sample_ids: Optional[torch.Tensor] = None, relax_steps: int = 0, standardize: bool = False):
        """Sampler -> hand-off -> GCN -> bond write-back + validity proxy for `n_samples` molecules on THIS device.
        Returns per-sample DEVICE tensors (dim 0 = n_samples; n_samples may be 0 for an empty shard).
        `relax_steps` > 0 (`relax_geometry`): every group's coordinates are relaxed right behind its bond write-back
        (`_relax_coords`, one launch per group, all rows); the relaxed coordinates are what `x`, the finisher's records and
        everything downstream hold, and `strain_before` / `strain_after` [n_samples] join the returned tensors.
        `standardize`: every group's graphs are standardised right behind its bond write-back and BEFORE the relaxation
        (`_standardize`, one launch per group, all rows): `x`, `elements`, `bond`, `n_nodes` and everything downstream
        are the parent fragment's, `valid` is the standardisation's verdict (status 0) instead of the proxy's flag, and
        `atoms_removed`, `n_fragments` [n_samples], `atom_map` [n_samples,42] and `kekule_bond_orders` [n_samples,42,42]
        join the returned tensors.  `last_batch` keeps what the hand-off and the GCN wrote and gains `standardized`, the
        stage's own result.
        `sample_seed`, `sample_ids`: the keyed stream of `edm_tensors`; `sample_ids` (default arange) also names the
        records handed to the finisher.

        With an atom-order provider and / or a finisher (RDKit's where RDKit imports) the part behind the sampler is a
        pipeline over groups of molecules (conformer_generator.py:343-366 runs it one molecule at a time): every order
        task of the batch is submitted to the host pool as soon as x, h are on the host; the hand-off + GCN + write-back
        of group g is launched when ITS order results are in; its records are copied back and its finish tasks submitted
        while the pool still works on the order of the later groups.  `self._finish_stage` then holds the pending finish
        (consumed by `generate_conformers*`)."""
        N = min(ref_n_atoms + variance, self.max_n_nodes)
        D = self.dimension
        dev = self.device
        self._finish_stage = None
        self.last_host_order_ms = self.last_host_finish_ms = None
        provider, finisher = self.atom_order_provider, getattr(self, "finisher", None)
        staged = provider is not None or finisher is not None
        executor = self._executor() if staged else None
        if executor is not None:
            # worker start-up (~0.3 s for 32 interpreters, plus `import rdkit` in each) hides under the sampler launched below
            tasks = [rdkit_order.provider_task(provider)[0]] if provider is not None and rdkit_order.provider_task(provider) else []
            if finisher == "rdkit":
                tasks.append(host_pool.FINISH_TASK)
            elif isinstance(finisher, host_pool.TaskRef):
                tasks.append(finisher)
            executor.prestart(tasks)
        if n_samples == 0:
            if finisher is not None:      # an empty shard still takes part in the object gather of the finished molecules
                from . import rdkit_finish
                self._finish_stage = rdkit_finish.FinishStage(finisher, optimise_geometry, executor)
            strain = dict(strain_before=torch.zeros(0, device=dev), strain_after=torch.zeros(0, device=dev)) \
                if relax_steps else {}
            std_out = {}
            if standardize:
                i32 = dict(dtype=torch.int32, device=dev)
                std_out = dict(atoms_removed=torch.zeros(0, **i32), n_fragments=torch.zeros(0, **i32),
                               atom_map=torch.zeros(0, D, **i32),
                               kekule_bond_orders=torch.zeros(0, D, D, dtype=torch.int8, device=dev))
            return dict(x=torch.zeros(0, N, 3, device=dev), elements=torch.zeros(0, D, dtype=torch.int8, device=dev),
                        bond=torch.zeros(0, D, D, dtype=torch.int8, device=dev),
                        n_nodes=torch.zeros(0, dtype=torch.int32, device=dev),
                        valid=torch.zeros(0, dtype=torch.uint8, device=dev), **strain, **std_out)
        x, h, node_mask = self.edm_tensors(
            reference_context=ref_context, n_samples=n_samples, min_n_nodes=ref_n_atoms - variance,
            max_n_nodes=ref_n_atoms + variance, resample_steps=resample_steps, fixed_fragment=fixed_fragment,
            inertial_fragment_matching=inertial_fragment_matching, blend_power=blend_power,
            ifm_diffusion_level=ifm_diffusion_level, sizes=sizes, sample_seed=sample_seed, sample_ids=sample_ids)
        n_nodes = node_mask.sum(1).reshape(-1).to(torch.long)
        ids = list(range(n_samples)) if sample_ids is None else [int(i) for i in torch.as_tensor(sample_ids).tolist()]
        groups = rdkit_order.launch_groups(n_samples) if staged else [(0, n_samples)]
        t0 = time.perf_counter()
        # host: RDKit's (or the caller's) order + connectivity - every task of the batch goes out now
        stage = (rdkit_order.OrderStage(provider, x, h, n_nodes, executor, groups, self.class_z)
                 if provider is not None else None)
        fin = None
        if finisher is not None:
            from . import rdkit_finish
            fin = rdkit_finish.FinishStage(finisher, optimise_geometry, executor)
        parts, orders, std_parts = [], [], []
        for g, (lo, hi) in enumerate(groups):
            order = conn = built = None
            if stage is not None:
                order, conn, built = stage.result(g)
            ng = n_nodes[lo:hi]
            # atoms, distances, connectivity AND coordinates come out in the order the GCN sees (canonicalised_samples)
            el, dm, am, x_out = prepare_adj_mat_seer_input_hip(x[lo:hi], h[lo:hi], ng, D, order=order, connectivity=conn,
                                                               with_coords=True, class_z=self.class_z)
            bond = self.adj_mat_seer.bond_orders(el, dm, am)
            sym, valid = bond_writeback_hip(bond, el, ng)
            if standardize:                                   # all rows; from here on the molecule is its parent fragment
                std = self._standardize(x_out, el, sym, ng)
                std_parts.append((x_out, el, std))
                x_out, sym, valid = std["coords"], std["bond_orders"], std["valid"]
                el, ng = std["atomic_numbers"].to(el.dtype), std["n_nodes"].to(ng.dtype)
            if built is not None and not all(built):          # `MolFromXYZBlock` returned None: the reference drops it
                valid = valid & torch.tensor(built, dtype=torch.bool, device=valid.device)
            extra = ()
            if relax_steps:                                   # all rows, valid or not: the finisher judges for itself
                rel = self._relax_coords(x_out, el, sym, ng, relax_steps)
                extra = (x_out, rel["energy_before"], rel["energy_after"])
                x_out = rel["coords"]
            parts.append((x_out, el, bond, sym, valid) + extra)
            orders.append(order if order is not None else [None] * (hi - lo))
            if fin is not None:                               # this group's records -> the pool, behind the order tasks
                fin.add(molecules_from_tensors(x_out, el.to(torch.int8), sym, ng.to(torch.int32), valid.to(torch.uint8),
                                               sample_ids=ids[lo:hi]))
        if stage is not None:
            self.last_host_order_ms = (time.perf_counter() - t0) * 1e3
        cat = (lambda k: parts[0][k]) if len(parts) == 1 else (lambda k: torch.cat([p[k] for p in parts], dim=0))
        x_out, el, bond, sym, valid = (cat(k) for k in range(5))
        self._finish_stage = fin
        self.last_batch = dict(x=x, h=h, n_nodes=n_nodes, elements=el, bond=bond, x_ordered=x_out)     # tensors only
        strain = {}
        if relax_steps:           # `x_ordered` stays what the hand-off wrote; the relaxed coordinates are a key of their own
            self.last_batch.update(x_ordered=cat(5), x_relaxed=x_out)
            strain = dict(strain_before=cat(6), strain_after=cat(7))
        n_out, std_out = n_nodes, {}
        if standardize:           # `x_ordered`, `elements` stay what the hand-off wrote; the stage's result is a key of its own
            scat = (lambda pick: pick(std_parts[0])) if len(std_parts) == 1 else \
                (lambda pick: torch.cat([pick(p) for p in std_parts], dim=0))
            full = {k: scat(lambda p, k=k: p[2][k]) for k in std_parts[0][2]}
            self.last_batch.update(x_ordered=scat(lambda p: p[0]), elements=scat(lambda p: p[1]), standardized=full)
            n_out = full["n_nodes"]
            std_out = dict(atoms_removed=full["atoms_removed"], n_fragments=full["n_fragments"], atom_map=full["atom_map"],
                           kekule_bond_orders=full["kekule_orders"])
        flat = [o for grp in orders for o in grp]
        self.last_order = None if all(o is None for o in flat) else flat    # per-molecule atom orders (None: generation order)
        return dict(x=x_out, elements=el.to(torch.int8), bond=sym, n_nodes=n_out.to(torch.int32),
                    valid=valid.to(torch.uint8), **strain, **std_out)

    def _collect_finish(self, n_samples: int) -> List:
        """The pending finish of the shard generated last -> its `n_samples` per-sample results (None = dropped)."""
        stage, self._finish_stage = getattr(self, "_finish_stage", None), None
        done = []
        if stage is not None:
            t0 = time.perf_counter()
            done = stage.results()
            self.last_host_finish_ms = (time.perf_counter() - t0) * 1e3
        if len(done) != n_samples:
            raise ValueError(f"the finish returned {len(done)} results for a shard of {n_samples}")
        return done

    @torch.no_grad()
    def generate_conformers(self, reference_conformer=None, n_samples: int = 10, variance: int = 2,
                            reference_context: torch.Tensor = None, n_atoms: int = None,
                            optimise_geometry: bool = True, resample_steps: int = 0, fixed_fragment=None,
                            inertial_fragment_matching: bool = True, blend_power: int = 3,
                            ifm_diffusion_level: int = 50, sample_seed: Optional[int] = None, shape_scores: bool = False,
                            top_k: Optional[int] = None, min_shape_tanimoto: Optional[float] = None,
                            overlay: bool = False, max_pairwise_tanimoto: Optional[float] = None,
                            refine_overlay: Union[bool, int] = False, receptor=None,
                            max_receptor_clashes: Optional[int] = None, chemical_scores: bool = False,
                            reference_graph=None, max_chemical_tanimoto: Optional[float] = None,
                            unique: Union[bool, str] = False,
                            max_pairwise_chemical_tanimoto: Optional[float] = None, reference_shape=None,
                            shape_density: float = 0.02, max_atoms_outside: Optional[int] = None,
                            relax_geometry: Union[bool, int] = False, pharmacophore_scores: bool = False,
                            reference_pharmacophore=None, min_pharmacophore_tanimoto: Optional[float] = None,
                            rank_by: str = "shape", relieve_clashes: Union[bool, int] = False,
                            add_hydrogens: bool = False, standardize: bool = False,
                            electrostatic_scores: bool = False, reference_charges=None,
                            min_electrostatic_tanimoto: Optional[float] = None, partial_charges: bool = False,
                            smiles: bool = False, exclude_graphs=None, require_substructures=None,
                            exclude_substructures=None, substructure_counts=None,
                            interaction_scores: bool = False,
                            max_interaction_score: Optional[float] = None,
                            optimise_pose: Union[bool, int] = False) -> List:
        """Generate molecules from a reference shape (conformer_generator.py:268-368).
        Returns the VALID molecules only (invalid ones are dropped, as in the reference): `List[Chem.Mol]` through the
        reference's standardisation (+ MMFF94 when `optimise_geometry`) where RDKit imports, else `GeneratedMolecule`
        records that pass the labelled valence / single-fragment proxy of `mcg_bond_writeback` (no MMFF: warned once).
        Each record says which sample it is (`GeneratedMolecule.sample_id`).  `sample_seed`: the keyed stream of
        `edm_tensors` - sample i is the same molecule whatever `n_samples`; the Mols carry the int property `sample_id`.
        `shape_scores=True`: every returned molecule carries the shape Tanimoto of its RETURNED heavy-atom coordinates
        against the reference (`GeneratedMolecule.shape_tanimoto`, the Mols' double property `shape_tanimoto`) - what
        `evaluate_samples(reference, [mol])` reports, computed on the GPU (`cheminformatics.shape_scores`); sample order.
        `min_shape_tanimoto` / `top_k` (either implies scoring): keep the molecules scoring >= the threshold, then the k
        best, in descending score order (ties: lower sample id); `last_valid_fraction` is taken before this selection.
        `overlay=True`: every returned molecule is posed onto the reference conformer, in the coordinates the reference
        was given in, by a proper rigid transform (a rotation, never a mirror) found on the GPU from the principal shape
        frames and the four-orientation search (`cheminformatics.shape_overlay`).  Records: `coords` are the posed
        coordinates, `pose` = (rotation, translation) with returned = generated @ rotation + translation, and
        `overlay_tanimoto` the shape Tanimoto of that pose (a molecule whose pose failed keeps its generated coordinates,
        `pose` None, `overlay_tanimoto` NaN).  Mols: every conformer position, hydrogens included, moved by the pose of
        the heavy atoms; double property `overlay_tanimoto`.  With scoring the molecules are posed first, then scored:
        `shape_tanimoto` stays the score of the RETURNED coordinates, and since `evaluate_samples` takes the reference's
        frame with whatever handedness LAPACK gives it, it can differ from the un-posed call's score for the same
        molecule; `overlay_tanimoto` is the score of the proper pose.
        `max_pairwise_tanimoto` (needs `overlay=True`; implies scoring): a shape-diverse selection.  After the threshold,
        the molecules are walked in ranking order and one is kept unless its shape Tanimoto, as posed, with an already
        kept molecule is >= the value (`cheminformatics.pairwise_shape_tanimoto` on the GPU, `select_diverse`); then
        `top_k`.
        `refine_overlay` (needs `overlay=True`): True (64 steps) or a step budget 1..1024.  Each molecule's pose is
        refined on the GPU: from each of the four principal-frame starts a rigid-body ascent of the Gaussian overlap with
        the reference, the best refined candidate kept where its shape Tanimoto is strictly better than the start's
        (`cheminformatics.shape_overlay(refine_steps=...)`).  `pose` and `overlay_tanimoto` describe the returned pose;
        ranking and selection are unchanged, and the pair matrix of `max_pairwise_tanimoto` reads the refined poses.
        `receptor` (needs `overlay=True`): the receptor the reference ligand was taken from - an RDKit Mol, a PDB-format
        string or a (coords, atomic_numbers) pair (`receptor.load_receptor`), in the reference's coordinates.  The
        returned (posed, possibly refined) heavy atoms are measured against its heavy atoms on the GPU
        (`receptor.receptor_overlap`; DESIGN.md section 6, "Receptor clashes"): records carry `receptor_clashes` (atoms
        overlapping a receptor atom by >= 0.6 A) and `receptor_max_overlap` (A), the Mols the int / double properties of
        the same names; None (no property) where posing failed.  `max_receptor_clashes=k`: drop the molecules with more
        than k clashing atoms, and those whose pose failed, before the threshold / diversity / `top_k` selection.
        `relieve_clashes` (needs a `receptor`): True (32 trials) or a trial budget 1..1024.  Right behind the pose and its
        refinement every posed molecule is nudged, as a rigid body, out of its contacts with the receptor on the GPU
        (`receptor.relieve_clashes`; DESIGN.md section 6, "Clash relief"): a downhill walk on the summed squared contact
        depth - the package's OWN procedure, not a docking score and not a force field: no attraction, no trade of shape
        against fit; it stops at the first clash-free pose it finds, within 2 A of where the pose put the centroid.  The
        relieved coordinates are what shape scoring, receptor contacts, pharmacophore scores and the pair matrices read,
        and what is returned.  For a molecule it moved, `pose` is the composed transform (returned = generated @ rotation
        + translation still holds) and `overlay_tanimoto` the shape Tanimoto of the pose as placed, on the reference's own
        grid; the Mols are moved with every conformer position, hydrogens included.  An unmoved molecule keeps every bit.
        Records carry `relief_rmsd` (A the heavy atoms moved; 0.0 where nothing moved) and `receptor_clashes_before` (the
        clash count of the pose before the relief), the Mols the double / int properties of those names; None (no
        property) in a call without it and where posing failed.  `receptor_clashes` / `receptor_max_overlap` keep their
        meaning: the contacts of the returned coordinates.
        `chemical_scores=True`: the chemical half of `evaluate_samples`, RDKit-free.  Every returned molecule carries
        `chemical_tanimoto` - the Tanimoto of its chemical fingerprint with the reference graph's - and `graph_key`, the
        unsigned 64-bit identity key of its molecular graph (records: the properties of those names; Mols: the double
        property `chemical_tanimoto` and the STRING property `graph_key`, the key in decimal).  The fingerprint is this
        package's own Morgan-type fingerprint (radius 2, 2 048 bits, bond types on, chirality off; `fingerprint.py`,
        DESIGN.md section 6): a labelled SUBSTITUTE for RDKit's, not bit-compatible with it, computed on the GPU from the
        returned heavy-atom graphs.  Equal keys: the same graph, up to what colour refinement can tell apart and hash
        collisions.  The reference's graph is `reference_graph` (a Mol, a `GeneratedMolecule` or an (atomic_numbers,
        bond_orders) pair: `fingerprint.mol_graph`), else `reference_conformer` where it is a Mol with bonds.  No
        aromaticity is perceived: both sides must use one convention (generated aromatic bonds carry code 4).
        `max_chemical_tanimoto=t` (implies the score): drop the molecules whose `chemical_tanimoto` is >= t, or NaN;
        1.0 drops exactly those whose fingerprint equals the reference's.
        `unique=True`: of the molecules with equal `graph_key` keep one - the first in ranking order where the call
        scores shape (descending `shape_tanimoto`, ties to the lower sample id, NaN last), else the lowest sample id.
        `max_pairwise_chemical_tanimoto=t`: sphere exclusion on the pairwise fingerprint Tanimoto
        (`fingerprint.pairwise_fingerprint_tanimoto`), in the same walk as `max_pairwise_tanimoto` - a molecule is
        excluded if either matrix reaches its threshold against an already kept one; the walk is in ranking order, or
        in sample order where the call does not score shape.
        `reference_shape` (instead of `reference_conformer` / `reference_context`; needs `n_atoms`): a watertight triangle
        mesh as the reference - a path, bytes or file object holding a binary or ASCII STL, a (vertices, faces) pair or
        an object with `.vertices` and `.faces` (`mesh.load_mesh`; no `trimesh`).  The context is the solid's principal
        inertia components at `shape_density` (`mesh.mesh_context`: the reference notebook's
        `principal_inertia_components` with `density = 0.02`); generation itself is unchanged.  `shape_scores`, `overlay`,
        `top_k`, `min_shape_tanimoto` and `max_pairwise_tanimoto` then work as with a conformer, the solid standing in for
        it: its density is the indicator function of its inside (generalized winding number |w| > 0.5) on the grid of its
        own principal frame - this package's own definition, the reference scores molecules against molecules only
        (`cheminformatics.shape_scores_solid`, `shape_overlay_solid`, `pairwise_shape_tanimoto_solid`; DESIGN.md section 6,
        "Solid references").  The pose is in the mesh's own coordinates, and posed records / Mols carry `atoms_outside` (the
        int property of that name): the heavy atoms of the pose outside the mesh; None (no property) where posing failed.
        `max_atoms_outside=k` (needs `overlay=True` and `reference_shape`): drop the molecules with more than k atoms
        outside, and those whose pose failed, beside `max_receptor_clashes`.
        `reference_shape=pocket`, a `pocket.Pocket` from `pocket.find_pocket` ("Pockets from the
        receptor"): the pocket's mesh is the solid, and `max_receptor_clashes`, `relieve_clashes`, `interaction_scores`,
        `max_interaction_score`, `rank_by="interaction"`, `optimise_pose` and the `receptor_hydrogen_clashes` of
        `add_hydrogens` read the pocket's own receptor (they need `overlay=True` as with a `receptor`); `receptor=` beside
        it stays refused.
        `relax_geometry`: True (200 steps) or a step budget 1..4096.  Every generated molecule's heavy atoms are relaxed on
        the GPU right behind the bond write-back, one launch per group of molecules (`geometry.relax_geometry`; DESIGN.md
        section 6, "Relaxed geometry"), on the package's OWN restrained valence force field - NOT MMFF94, heavy atoms
        only: harmonic bond, 1-3 distance and one-sided non-bonded terms under the reference's position restraint (flat to
        0.2 A, then 800 kcal/mol/A^2, `standardize_mol`), so no atom ends far from where the sampler put it.  The
        relaxed coordinates are what everything behind it reads - the records handed to a finisher (RDKit's MMFF94, where
        RDKit imports and `optimise_geometry` asks for it, then starts from them; the two are independent), posing,
        scoring, receptor and mesh contacts - and what is returned.  Records carry `strain_before` / `strain_after`, the
        force field's energy (kcal/mol by its constants) before and after, the Mols the double properties of those
        names; None (no property) in a call that did not relax.  `last_batch["x_ordered"]` keeps the unrelaxed
        coordinates, `last_batch["x_relaxed"]` holds the relaxed ones.  `optimise_geometry` and its warning mean what
        they meant.
        `pharmacophore_scores=True` (needs `overlay=True`): does the posed molecule keep the reference's interaction pattern?
        Every returned molecule carries `pharmacophore_tanimoto` - the Tanimoto of the Gaussian overlap of its
        pharmacophore features (donor, acceptor, cation, anion, hydrophobe, aromatic ring), as posed, with the
        reference's - and `pharmacophore_matches`, the reference features that have one of its features of the same type
        within 1.5 A (records: the properties of those names; Mols: the double / int properties); None (no property)
        where posing failed.  The features are this package's OWN definition (`pharmacophore.py`, DESIGN.md section 6,
        "Pharmacophore overlap"), perceived on the GPU from the returned heavy-atom graphs: not RDKit's feature factory
        and not a vendor's colour score.  The reference's features are `reference_pharmacophore` - a sequence of (type,
        (x, y, z)) in the reference's coordinates, types "donor", "acceptor", "cation", "anion", "hydrophobe", "ring"
        (`pharmacophore.load_reference_features`; the only way with a `reference_shape` or a reference without bonds) -
        or are perceived from `reference_graph`, else from `reference_conformer` where it is a Mol with bonds, at the
        reference conformer's heavy-atom coordinates, in the graph's atom order.  No aromaticity is perceived: a ring
        feature needs code-4 bonds.
        `min_pharmacophore_tanimoto=t` (implies the score): drop the molecules whose `pharmacophore_tanimoto` is below t,
        NaN or missing.
        `rank_by="combo"` (needs a shape score and the pharmacophore score; default "shape"): `unique`, the diversity walk
        and `top_k` rank by `shape_tanimoto + pharmacophore_tanimoto` instead of `shape_tanimoto`; `min_shape_tanimoto`
        still thresholds the shape score alone.
        `add_hydrogens=True`: every returned record carries its explicit hydrogens - `hydrogen_coords` ([nH,3] fp32),
        `hydrogen_parents` (the heavy atom of each, ascending) and `hydrogens_unplaced` (hydrogens the count rule gives to
        atoms the placement has no direction for; 0 for an ordinary molecule) - placed on the GPU by the package's OWN
        definition, NOT RDKit's AddHs (`hydrogens.add_hydrogens`; DESIGN.md section 6, "Explicit hydrogens"): the count
        from the bond codes plus one aromatic N-H per 5-ring, ideal directions by the parent's hybridisation at rcov + 0.31
        A, terminal groups turned to the torsion that keeps them clear of the other atoms; no charges, no tautomer search.
        It runs last of the measuring stages, behind the gather, beside the pharmacophore step, on the rows a rank returns
        and on the RETURNED coordinates - relaxed, posed, refined, relieved - so the hydrogens are in the frame of `coords`
        and need no transform; it removes no molecule and changes no other value.  `to_molblock(hydrogens=True)` /
        `to_xyz_block(hydrogens=True)` write the all-atom molecule.  With a `receptor` the records also carry
        `receptor_hydrogen_clashes`: the hydrogens overlapping a receptor heavy atom by >= 0.6 A at the radius 1.20 A, by
        the kernel of the heavy-atom contacts; None where posing failed; `receptor_clashes` / `receptor_max_overlap` keep
        their heavy-atom meaning and no filter reads the hydrogens.  All of these are None in a call without the option,
        and the three hydrogen fields where the molecule has a non-finite coordinate.
        `standardize=True` (records path only): every generated graph is standardised on the GPU right behind the bond
        write-back and BEFORE `relax_geometry`, as the reference takes the fragment parent before MMFF
        (`standardize.standardize_graphs`; DESIGN.md section 6, "Standardised graphs") - by the package's OWN definition,
        NOT RDKit's FragmentParent / Kekulize / SanitizeMol: the largest connected fragment is kept (ties: the larger sum
        of atomic numbers, then the lowest atom index), its atoms in their order; it is valid when no atom exceeds the
        proxy's maximum valence (aromatic bonds counted as their sigma bond), no aromatic bond lies outside a ring and
        its aromatic bonds have a Kekule form, found by a fixed-order search within a step budget.  No charges, no
        normalisation, no tautomers.  The returned molecules ARE the parent fragments - coordinates, elements, bonds and
        everything measured downstream - and validity is this verdict instead of the proxy's: a molecule with a stray atom
        beside a good fragment is kept, one whose aromatic bonds admit no Kekule form is dropped.  Records carry
        `atoms_removed`, `n_fragments`, `atom_map` (each atom's index in the graph as generated) and
        `kekule_bond_orders`; `to_molblock(kekulize=True)` writes the Kekule form.  `last_batch` keeps what the hand-off
        and the GCN wrote and gains `standardized`.  All of these are None in a call without the option.
        `electrostatic_scores=True` (needs `overlay=True`; records path only): does the posed molecule present the
        reference's charge distribution?  Every returned record carries `electrostatic_tanimoto` - the Tanimoto of the
        Coulomb overlap of Gaussian-smeared partial charges on its heavy atoms and placed hydrogens, as posed, with the
        reference's, in [-1/3, 1]; NaN where posing failed and where the molecule holds an element without charge
        parameters.  The charges are this package's OWN definition (`electrostatics.py`, DESIGN.md section 6,
        "Electrostatic similarity"): iterative electronegativity equalisation on the returned heavy-atom graph with the
        hydrogens of `add_hydrogens`' count rule - NOT RDKit's Gasteiger charges, not a vendor's electrostatic score; no
        formal charges, no protonation states.  The reference's charge points are `reference_charges` - a sequence of
        (charge, (x, y, z)) in the reference's coordinates (`electrostatics.load_reference_charges`; the only way with a
        `reference_shape` or a reference without bonds) - or are computed from `reference_graph`, else from
        `reference_conformer` where it is a Mol with bonds, at the reference conformer's heavy-atom coordinates with its
        hydrogens placed by the same kernel.  The step runs behind the gather, beside the pharmacophore step; with
        `add_hydrogens` the hydrogens are placed once for both.
        `min_electrostatic_tanimoto=t` (implies the score; t in [-1, 1]): drop the molecules whose
        `electrostatic_tanimoto` is below t, NaN or missing, right behind `min_pharmacophore_tanimoto`.
        `rank_by="electrostatic"` (needs a shape score and the electrostatic score): `unique`, the diversity walk and
        `top_k` rank by `shape_tanimoto + electrostatic_tanimoto`; `min_shape_tanimoto` still thresholds shape alone.
        `partial_charges=True` (records path only; needs no reference and no pose): every returned record carries
        `partial_charges` ([n] fp32, the heavy atoms) and `hydrogen_charges` ([n] fp32, the charge of EACH hydrogen of
        that atom, 0 where it has none); NaN where the molecule holds an element without parameters.
        `to_xyz_block(charges=True)` writes them as a fifth column.  All of these are None in a call without the option.
        `smiles=True` (records path only): every returned record carries `canonical_order` - its exact canonical atom
        order, found on the GPU by a partition-refinement search per molecule (`canonical.canonical_order`; DESIGN.md
        section 6, "Canonical graphs and SMILES") - `canonical_status` and `smiles`, the canonical SMILES the host writes
        from it on first read (`smiles.write_smiles`).  The package's OWN definition: valid OpenSMILES, NOT RDKit's
        canonical SMILES, no string equality with any toolkit; no charges, and no stereochemistry unless asked for
        (`smiles="isomeric"`, below).  Equal strings mean the
        same graph, so "unique within the batch" and "novel against a known set" can be counted on them.  A graph the
        labelling refuses (an atom with more than 8 neighbours, more than 4 096 leaves) has `canonical_status` != 0 and
        None for the other two; `to_smiles(canonical=False)` still writes it in its own atom order.  The "[nH]" of an
        imidazole-type ring may sit on the other N than the hydrogen `add_hydrogens` placed on the same record.
        `unique="exact"`: as `unique=True` - same place in the order of stages, same ranking - but a molecule is dropped
        only where its exact identity (`canonical.identity_bytes`) equals that of a better-ranked one: two different
        graphs that share a `graph_key` (cubane and the 8-ring with its four diagonals do) are both kept.  A molecule
        without a canonical order is never dropped.  It reads the Mols' own graphs through RDKit's finisher.
        `smiles="isomeric"` (records path only): everything `smiles=True` gives, unchanged, and - from one more launch on
        the returned coordinates (`stereo.stereo_order`; DESIGN.md section 6, "Stereo identity") - `stereo_order`,
        `stereo_status`, `stereo_descriptors` (per atom 4 tet + db, in the record's order and relative to it),
        `n_stereo_defined` and `n_stereo_undefined`; `smiles` and `to_smiles()` then write the isomeric string ("@" / "@@",
        "/" / "\\"), `to_smiles(isomeric=False)` the other.  The package's OWN definition: NOT RDKit's stereo perception,
        no CIP labels; tetrahedral C / Si and C=C / C=N / N=N only.  `unique="stereo"` (records path only): as
        `unique="exact"`, but a molecule is dropped only where its stereo identity (`stereo.stereo_identity_bytes`)
        equals that of a better-ranked one - both enantiomers of a chiral molecule stay, which the reflection-equivariant
        sampler makes equally often.  `exclude_graphs` stays at constitution level.
        `unique="scaffold"` / `unique="framework"`: as `unique="exact"` - same place in the order of stages, same ranking,
        the Mols' own graphs through RDKit's finisher - but one molecule per ring framework stays: a molecule is dropped
        where its scaffold - ring, linker and doubly bonded exo atoms, elements and bond codes kept - or, with
        "framework", its generic framework - ring and linker atoms, all carbon, all single - has the identity of a
        better-ranked molecule's (`scaffold.murcko_scaffolds`; DESIGN.md section 6, "Rings and scaffolds": the package's OWN
        definitions, NOT RDKit's ring perception or MurckoScaffold).  All acyclic molecules share the empty scaffold; a
        scaffold without a canonical order is never dropped.  On the records path every returned record carries `n_rings`,
        `n_ring_systems`, `min_ring_size`, `max_ring_size`, `ring_sizes`, `ring_systems`, `scaffold_atoms`, `scaffold_key`,
        `scaffold_status` and - with `smiles` - `scaffold_smiles`, read off the record's own returned graph (with
        `standardize` the parent fragment's); `scaffold.of_records` writes them onto records without a selection.
        `exclude_graphs=`: an iterable of `GeneratedMolecule` records, Mols or (atomic_numbers, bond_orders) pairs
        (`fingerprint.mol_graph`: their heavy atoms).  They are read with the other arguments and labelled by the same
        kernel directly in front of the generation, behind every refusal of the call, and a generated molecule whose
        exact identity equals one of them is dropped, in front of `unique`.
        `require_substructures=` / `exclude_substructures=` / `substructure_counts=`: each an iterable of patterns - strings
        in a small, labelled subset of SMARTS (`substructure.parse`: "c1ccccc1", "C(=O)[Cl,Br]", "[nH]", "*@*"),
        `substructure.Pattern`s, or graphs (`GeneratedMolecule`, Mol, (atomic_numbers, bond_orders) pair: the piece with
        exact elements and bond codes, `substructure.from_graph` - the check that a `fixed_fragment` survived the bond
        network); `substructure.CATALOGUE` is a short list of unwanted groups.  All of them are matched against the
        returned molecules' graphs (with `standardize` the parent fragment's) in ONE launch of a subgraph-monomorphism search
        on the GPU (`substructure.match_substructures`; DESIGN.md section 6, "Substructure patterns": the package's OWN
        definition, NOT RDKit's `HasSubstructMatch`).  A molecule stays only if every required pattern is proven present
        (count >= 1) and no excluded one is; a search that hits its node budget before it finds an embedding leaves the
        row undetermined - `require` drops it, `exclude` keeps it, one warning names how many.  Records carry
        `substructure_patterns` (the three lists in that order) and, per pattern, `substructure_counts`,
        `substructure_status` and `substructure_first` (the atoms of the first embedding); through RDKit's finisher the
        Mols' own graphs are read and the counts are set as the space-separated property `substructure_counts` (that path
        is not tested where RDKit is absent).  All None in a call without the options, which launches nothing new.
        `interaction_scores=True` (needs a `receptor`, and with it `overlay=True`; records path only): does the posed
        molecule interact with the pocket?  Every returned record carries `interaction_score` - an empirical interaction
        score E of its returned coordinates (relaxed, posed, refined, relieved) with the typed receptor, negative is
        better -, `interaction_terms` (the five sums G1, G2, REP, HYD, HB and `n_rot`), `receptor_hbonds` (the donor /
        acceptor pairs at hydrogen-bond distance, an exact integer) and `interaction_atom_scores` (each atom's weighted
        contribution); all None where posing failed.  THE PACKAGE'S OWN DEFINITION (`interactions.py`, DESIGN.md section
        6, "Receptor interactions"): the functional form of the AutoDock Vina scoring function on the package's own
        heavy-atom typing, intermolecular terms only - NOT AutoDock Vina's output, not a binding free energy, no search.
        The receptor's atoms are typed by `receptor.load_typed_receptor` - a residue-template table for a PDB string, the
        element rules for a (coords, atomic_numbers) pair or a Mol, or the explicit third element of a (coords,
        atomic_numbers, types) triple - once per call; one warning counts the N, O and metal atoms outside the table.  The
        step runs behind the gather, beside the pharmacophore step, in one launch.
        `interaction_scores="contacts"` does everything `True` does plus the contact fingerprint: WHICH residues the
        returned coordinates touch, with which kind of contact.  Every record also carries `residue_contacts` - a tuple
        of (label, kind names) such as ("A:SER195", ("contact", "hbond_donor")) -, `contact_groups`, `contact_kinds`,
        `contact_atom_kinds` and `contact_status`, and - where the call has the reference's graph (`reference_graph=`, or a
        reference conformer with bonds) - `contact_recovery`, `contact_tanimoto`, `contacts_recovered` and
        `contacts_missed` against the fingerprint of the reference conformer with the same receptor.
        `interaction_scores=("contacts", t)`, t in [0, 1], also keeps only the molecules with `contact_recovery >= t` (NaN
        and None do not pass); it is refused without the reference's graph.  Both need the receptor's residues: a
        PDB-format string, or a `reference_shape` pocket found on one; any other receptor form is refused - call
        `contacts.contact_fingerprint(groups=...)` on the returned coordinates instead.  THE PACKAGE'S OWN DEFINITION
        (`contacts.py`, DESIGN.md section 6, "Receptor contacts"): NOT ProLIF, PLIP or SIFt output; heavy atoms only; no
        ionic, aromatic or metal kinds.
        `optimise_pose` (needs a `receptor` and `overlay=True`; records path only; implies `interaction_scores`): True (64
        trials) or a trial budget 1..1024.  Directly behind the pose, its refinement and the clash relief, every posed
        molecule is moved as a rigid body to where that interaction score is lower (`interactions.optimise_pose`;
        DESIGN.md section 6, "Optimised pose"): a downhill accept / reject walk along the score's net force and torque, the
        centroid held within 2 A of where it started.  THE PACKAGE'S OWN PROCEDURE: not a docking run, not AutoDock Vina's
        local optimisation; rigid body only - no torsions, no intramolecular term, no hydrogens, no global search.  The
        optimised coordinates are what everything behind it reads and what is returned; `pose` is the composed transform
        and `overlay_tanimoto` the shape Tanimoto of the pose as placed; an unmoved molecule keeps every bit.  Records
        carry `interaction_score_before` (E of the pose the walk started from), `pose_optimisation_rmsd` (A the heavy
        atoms moved; 0.0 where nothing moved) and `pose_trials_kept`; None in a call without it and where posing failed.
        `optimise_pose="flexible"` (64 trials) or `("flexible", n)`, n in 1..1024: the same stage, with up to 16 rotatable
        bonds turned beside the rigid move and an intramolecular guard (`interactions.optimise_pose_flexible`; DESIGN.md
        section 6, "Flexible pose" - the package's own procedure likewise).  `pose` stays the rigid part of the move: it
        maps `x_relaxed` to the returned coordinates only up to `pose_conformer_rmsd`.  Records also carry `pose_torsions`,
        `pose_torsion_angles`, `pose_conformer_rmsd`, `intramolecular_clash_before` and `intramolecular_clash`; None in
        every other call.
        `optimise_pose="search"` (8 starts, 64 trials), `("search", S)` or `("search", S, n)`, S in 1..64: the flexible walk
        from S starts per molecule, the best result kept (`interactions.search_pose`; DESIGN.md section 6, "Pose search" -
        the package's own bounded multi-start, not a docking run and not AutoDock Vina's Monte Carlo search).  Start 0 is
        the pose as it came; the others are keyed by `sample_seed` (0 without one) and the sample id, so a molecule gets
        the same starts in any batch and on any number of GPUs; the result is never worse, by the walk's own objective,
        than `"flexible"` alone.  `pose` is the start's rigid part followed by the walk's.  Records carry the flexible
        fields and `pose_starts`, `pose_best_start` (0: the pose as it came won); None in every other call.
        `max_interaction_score=t` (implies the score; t a finite real number): keep the molecules with E <= t; NaN and
        missing do not pass; right behind `min_electrostatic_tanimoto`.
        `rank_by="interaction"` (needs the score): `unique`, the diversity walk and `top_k` rank by -E;
        `min_shape_tanimoto` still thresholds the shape score.
        Order of the stages: validity, `max_receptor_clashes`, `max_atoms_outside`, `max_chemical_tanimoto`,
        `min_pharmacophore_tanimoto`, `min_electrostatic_tanimoto`, `max_interaction_score`, `require_substructures`,
        `exclude_substructures`,
        `exclude_graphs`, `unique`, then the selection (threshold, exclusion, `top_k`).  The filters only remove molecules.
        Refused with ValueError before any device work: a chemical option that is not a bool / a real number in (0, 1],
        a chemical score without a reference graph, a `reference_graph` that `fingerprint.mol_graph` refuses or that has no
        or more than 64 heavy atoms, scoring or posing without a reference conformer, a reference
        outside 3..64 heavy atoms, top_k < 1, a threshold outside [0, 1], max_pairwise_tanimoto outside (0, 1] or without
        overlay, refine_overlay other than True or an integer in 1..1024 or without overlay, a receptor without overlay,
        one `load_receptor` refuses or one that holds the reference (a reference heavy atom within 0.5 A of a receptor
        heavy atom), max_receptor_clashes other than an integer >= 0 or without a receptor, relieve_clashes other than
        False, True or an integer in 1..1024 or without a receptor, optimise_pose other than False, True, an integer in
        1..1024, "flexible", ("flexible", n), "search", ("search", S) or ("search", S, n), without a receptor or on a generator with a finisher, a custom finisher, a
        `reference_shape` together with another reference, with `refine_overlay` or with a `receptor` (a `Pocket` brings
        its own; a plain mesh with any receptor option), or without
        `n_atoms`, a mesh `load_mesh` refuses ("The mesh needs to be watertight."), a `shape_density` that is not a positive
        real number, max_atoms_outside other than an integer >= 0, without a `reference_shape` or without overlay, and
        relax_geometry other than False, True or an integer in 1..4096 (a float, None, 0, a negative or larger number),
        pharmacophore_scores that is not a bool, without overlay or without a source of the reference's features, a
        `reference_pharmacophore` that `load_reference_features` refuses or that no option reads, a reference graph whose
        heavy-atom count differs from the reference conformer's, min_pharmacophore_tanimoto outside [0, 1], and a
        `rank_by` other than "shape", "combo", "electrostatic" or "interaction", or "combo" / "electrostatic" without both of
        its scores or "interaction" without its score, interaction_scores that is not a bool, without a receptor or on a
        generator with a finisher, a receptor whose types `load_typed_receptor` refuses, max_interaction_score that is not a
        finite real number,
        electrostatic_scores or partial_charges that is not a bool or on a generator with a finisher, electrostatic scores
        without overlay or without a source of the reference's charges, a `reference_charges` that
        `load_reference_charges` refuses or that no option reads, min_electrostatic_tanimoto outside [-1, 1], and add_hydrogens that is not a bool or on
        a generator with a finisher, RDKit's or a custom one (on Mols use `Chem.AddHs(mol, addCoords=True)`), and standardize
        that is not a bool or on a generator with a finisher (RDKit's finisher runs `standardize_mol` itself), smiles that
        is neither a bool nor "isomeric" or on a generator with a finisher, a unique other than True, False, "exact",
        "stereo", "scaffold" or "framework" ("stereo" on a generator with a finisher), and an
        `exclude_graphs` entry that is unreadable, has more than 64 heavy atoms or has no canonical order (the message
        names its position), a substructure option that is no iterable of patterns or holds an entry that cannot be read
        or has more than 32 query atoms (the message names the list, the position and, for a string, the character), and a
        substructure option on a generator with a custom finisher.  A reference
        graph in which no feature is found is refused where it is perceived, behind the generation."""
        if sample_seed is not None:
            seeding.check_seed(sample_seed)
        req = postprocess.entry_request(self, locals())      # every option under its own name
        ref_context, ref_n_atoms = self._reference_context(reference_conformer, reference_context, n_atoms, req.reference,
                                                           shape_density)
        req = postprocess.label_excluded(self, req)      # `exclude_graphs`: the first device work, behind every check above
        keyed = () if sample_seed is None else (sample_seed, None)   # unseeded: the positional call of before
        relax = dict(relax_steps=req.relax_steps) if req.relax_steps else {}
        if req.standardize:
            relax["standardize"] = True
        res = self._generate_shard(ref_context, ref_n_atoms, variance, None, n_samples, resample_steps, fixed_fragment,
                                   inertial_fragment_matching, blend_power, ifm_diffusion_level, optimise_geometry, *keyed,
                                   **relax)
        if getattr(self, "finisher", None) is None:
            return postprocess.return_records(self, req, postprocess.measure_tensors(self, req, res, None, sample_seed),
                                              None, optimise_geometry)
        done = self._collect_finish(n_samples)    # finished per group while the later groups were still on their way
        return postprocess.return_finished(self, req, postprocess.measure_finished(self, req, done, res), None,
                                           sample_seed)

    @torch.no_grad()
    def generate_conformers_sharded(self, reference_conformer=None, n_samples: int = 10, variance: int = 2,
                                    reference_context: torch.Tensor = None, n_atoms: int = None,
                                    optimise_geometry: bool = True, resample_steps: int = 0, fixed_fragment=None,
                                    inertial_fragment_matching: bool = True, blend_power: int = 3,
                                    ifm_diffusion_level: int = 50, group=None, seed: Optional[int] = None,
                                    gather: str = "all", balance: str = "cost",
                                    sample_seed: Optional[int] = None, shape_scores: bool = False,
                                    top_k: Optional[int] = None, min_shape_tanimoto: Optional[float] = None,
                                    overlay: bool = False, max_pairwise_tanimoto: Optional[float] = None,
                                    refine_overlay: Union[bool, int] = False, receptor=None,
                                    max_receptor_clashes: Optional[int] = None, chemical_scores: bool = False,
                                    reference_graph=None, max_chemical_tanimoto: Optional[float] = None,
                                    unique: Union[bool, str] = False,
                                    max_pairwise_chemical_tanimoto: Optional[float] = None, reference_shape=None,
                                    shape_density: float = 0.02, max_atoms_outside: Optional[int] = None,
                                    relax_geometry: Union[bool, int] = False, pharmacophore_scores: bool = False,
                                    reference_pharmacophore=None, min_pharmacophore_tanimoto: Optional[float] = None,
                                    rank_by: str = "shape", relieve_clashes: Union[bool, int] = False,
                                    add_hydrogens: bool = False, standardize: bool = False,
                                    electrostatic_scores: bool = False, reference_charges=None,
                                    min_electrostatic_tanimoto: Optional[float] = None,
                                    partial_charges: bool = False, smiles: bool = False,
                                    exclude_graphs=None, require_substructures=None, exclude_substructures=None,
                                    substructure_counts=None, interaction_scores: bool = False,
                                    max_interaction_score: Optional[float] = None,
                                    optimise_pose: Union[bool, int] = False) -> List:
        """`generate_conformers` for `n_samples` molecules in TOTAL, sharded over the ranks of the initialised
        `torch.distributed` group (one process per GPU, each with its own generator instance / weight replica;
        SURVEY.md section 8e).  The global size vector is drawn once on rank 0 and broadcast; every rank derives the same
        assignment of molecules to ranks from it (`distributed.assign_shards`: `balance="cost"` = longest-processing-time
        on the edge count n(n-1), "count" = contiguous equal-count slices) and generates its own; ONE all-gather of the
        result tensors at the end gives every rank the full batch, in SAMPLE order.  `seed`: per-rank noise seed `seed + rank` for the
        device generator; None (default) = a base seed drawn on rank 0 and broadcast, so that ranks NEVER share a noise
        stream (every process starts its device generator from the same constant).  A rank whose shard fails makes
        every rank raise `distributed.ShardError`.  `gather="rank0"`: only rank 0 of the group receives (and returns) the
        whole batch - one `gather` instead of the all-gather - and every other rank returns its own shard's molecules.
        Where a finisher runs (RDKit's), every rank finishes ITS OWN shard in its own host pool and the finished Mols are
        gathered as objects.  Without an initialised group this is `generate_conformers`.
        `sample_seed` (instead of `seed`): the keyed stream of `edm_tensors` - every rank computes the keyed sizes of all
        `n_samples` itself (no broadcast), generates its shard with the shard's global indices as `sample_ids` and seeds
        no generator, so sample i is the same molecule on any world size and under either `balance`.
        `shape_scores`, `top_k`, `min_shape_tanimoto`, `overlay`, `max_pairwise_tanimoto`, `refine_overlay`, `receptor`,
        `max_receptor_clashes`, `chemical_scores`, `reference_graph`, `max_chemical_tanimoto`, `unique`,
        `max_pairwise_chemical_tanimoto`, `reference_shape`, `shape_density`, `max_atoms_outside`, `relax_geometry`,
        `pharmacophore_scores`, `reference_pharmacophore`, `min_pharmacophore_tanimoto`, `rank_by`, `relieve_clashes`,
        `electrostatic_scores`, `reference_charges`, `min_electrostatic_tanimoto`, `partial_charges` (behind the gather, on
        the rows a rank returns, like the hydrogens), `smiles`, `unique="exact"`, `unique="scaffold"` / `"framework"` (perceived
        behind the gather, on the rows a rank returns, like the canonical order), `exclude_graphs` (labelled behind the
        gather, on the rows a rank returns, beside the fingerprints; every rank labels the excluded graphs itself),
        `require_substructures`, `exclude_substructures`, `substructure_counts` (matched behind the gather, on the rows a
        rank returns; every rank compiles the patterns itself),
        `interaction_scores`, `max_interaction_score` (scored behind the gather, on the rows a rank returns; every rank
        types and sorts the receptor itself), `optimise_pose` (on each rank's own shard, before the gather, directly behind
        the relief; its per-sample tensors travel with the rest),
        `add_hydrogens` (placed behind the gather, on the rows a rank returns), `standardize` (on each rank's own shard,
        before the gather; its per-sample tensors travel with the rest, one collective each): as in
        `generate_conformers` (every rank loads the mesh and computes its occupancy itself).  The fingerprints are computed behind the gather,
        on the rows a rank returns: with gather="all" uniqueness and chemical diversity hold over the whole batch, with
        gather="rank0" within each other rank's own shard, like the rest of the selection.
        Every rank poses, relieves, scores and measures the receptor contacts of ITS OWN shard on its own GPU before the gather
        (posed coordinates, poses, scores and contacts travel as per-sample result tensors, or next to the finished
        Mols).  The selection runs on the rows a rank
        returns: with gather="all" every rank selects from the whole batch (the pair matrix of the whole batch on its own
        GPU) and returns the same list; with gather="rank0" every other rank selects within its own shard."""
        if gather not in ("all", "rank0"):
            raise ValueError("gather must be 'all' or 'rank0'")
        if sample_seed is not None:
            if seed is not None:
                raise ValueError("pass either seed (per-rank device generator) or sample_seed (keyed stream), not both")
            seeding.check_seed(sample_seed)
        req = postprocess.entry_request(self, locals())      # every option under its own name
        ref_context, ref_n_atoms = self._reference_context(reference_conformer, reference_context, n_atoms, req.reference,
                                                           shape_density)
        lo_n = max(ref_n_atoms - variance, self.min_n_nodes)
        hi_n = min(ref_n_atoms + variance, self.max_n_nodes)
        req = postprocess.label_excluded(self, req)      # `exclude_graphs`: the first device work, behind every check above
        # decided from the configuration, not from what this rank's shard happened to produce: every rank takes the same
        # path through the collectives (an EMPTY shard has no stage of its own making)
        finishing = getattr(self, "finisher", None) is not None
        finished: List = []       # `postprocess.measure_finished` of this rank's shard, where a finisher runs

        def run_shard(sizes_shard, index):
            keyed = () if sample_seed is None else (sample_seed, index)
            relax = dict(relax_steps=req.relax_steps) if req.relax_steps else {}
            if req.standardize:
                relax["standardize"] = True
            res = self._generate_shard(ref_context, ref_n_atoms, variance, sizes_shard, int(index.numel()), resample_steps,
                                       fixed_fragment, inertial_fragment_matching, blend_power, ifm_diffusion_level,
                                       optimise_geometry, *keyed, **relax)
            if not finishing:
                # on this rank's GPU, gathered with the rest; the shard's global sample ids key the starts of a pose search
                return postprocess.measure_tensors(self, req, res, index, sample_seed)
            # collected HERE, in front of the status exchange: a finish that raises on one rank (a dead worker, a custom
            # finisher's exception, a result-count mismatch) makes EVERY rank raise ShardError instead of leaving the
            # others parked in the object gather
            done = self._collect_finish(int(index.numel()))
            finished[:] = postprocess.measure_finished(self, req, done, res)
            return res

        def seed_device(s):
            self.last_noise_seed = s          # this rank's noise stream (base seed + rank)
            if self.device.type == "cuda":
                with torch.cuda.device(self.device):
                    torch.cuda.manual_seed(s)

        dst = 0 if gather == "rank0" else None
        if sample_seed is None:
            draw_sizes, seed_fn = (lambda: mcg_dist.draw_global_sizes(n_samples, lo_n, hi_n, group)), seed_device
        else:       # identical on every rank by construction: no broadcast, and no generator is seeded
            draw_sizes, seed_fn = (lambda: mcg_dist.keyed_global_sizes(n_samples, lo_n, hi_n, sample_seed)), None
        _, res, shards = mcg_dist.sharded_generate(
            n_samples, draw_sizes, run_shard, group=group,
            seed=seed, seed_fn=seed_fn, gather_dst=dst, balance=balance, gather_tensors=not finishing)
        self.last_shards = shards
        # the sample ids of the rows this rank returns: the whole batch in sample order, or (gather="rank0", rank > 0)
        # its own shard
        _, rank = mcg_dist.world_and_rank(group)
        row_ids = shards[rank] if (dst is not None and rank != dst and len(shards) > 1) else None
        if not finishing:
            return postprocess.return_records(self, req, res, row_ids, optimise_geometry)
        samples = mcg_dist.gather_objects(finished, shards, group, dst)   # the Mols travel as objects, with their scores
        return postprocess.return_finished(self, req, samples, row_ids, sample_seed)

    forward = generate_conformers      # `__call__`: the same signature, defaults and `no_grad` by construction
