"""MI355X-native denoising hot path of mlconfgen (EGNN sampler + AdjMatSeer GCN).

Drop-in for `mlconfgen.MLConformerGenerator` on that path; all per-step
arithmetic runs in hand-written HIP kernels (gfx950) behind the C-ABI declared in
`include/mlconfgen_hip.h`.  There is no CPU fallback: constructing the generator
without the built library raises.
"""
from .config import (ATOM_DECODER, CONTEXT_NORMS, DIMENSION, MAX_N_NODES,
                     MIN_N_NODES, NUM_BOND_TYPES)

_FINGERPRINT = ("graph_fingerprints", "fingerprint_tanimoto", "pairwise_fingerprint_tanimoto", "mol_graph", "select_unique")
_MESH = ("load_mesh", "mass_properties", "mesh_context", "solid_frame")
_GEOMETRY = ("relax_geometry", "strain_energy")
_PHARMACOPHORE = ("perceive_features", "feature_points", "pharmacophore_tanimoto", "load_reference_features")
_RECEPTOR = ("relieve_clashes",)
_POCKET = ("find_pocket", "Pocket")

__all__ = ["MLConformerGenerator", "evaluate_samples", "ATOM_DECODER", "CONTEXT_NORMS", "DIMENSION",
           "MAX_N_NODES", "MIN_N_NODES", "NUM_BOND_TYPES", *_FINGERPRINT, *_MESH, *_GEOMETRY, *_PHARMACOPHORE,
           *_RECEPTOR, *_POCKET]


def __getattr__(name):
    # the reference exports `MLConformerGenerator` and `evaluate_samples` from the package root (mlconfgen/__init__.py)
    if name == "MLConformerGenerator":
        from .conformer_generator import MLConformerGenerator
        return MLConformerGenerator
    if name == "evaluate_samples":
        from .cheminformatics import evaluate_samples
        return evaluate_samples
    if name in _FINGERPRINT:             # chemical fingerprints and graph keys (fingerprint.py: a substitute for RDKit's)
        from . import fingerprint
        return getattr(fingerprint, name)
    if name in _MESH:                    # watertight meshes as reference shapes (mesh.py: host side, no trimesh)
        from . import mesh
        return getattr(mesh, name)
    if name in _GEOMETRY:                # restrained relaxation on the package's own force field (geometry.py: not MMFF94)
        from . import geometry
        return getattr(geometry, name)
    if name in _PHARMACOPHORE:           # pharmacophore features and their overlap (pharmacophore.py: the package's own)
        from . import pharmacophore
        return getattr(pharmacophore, name)
    if name in _RECEPTOR:                # clash relief of posed molecules (receptor.py: the package's own procedure)
        from . import receptor
        return getattr(receptor, name)
    if name in _POCKET:                  # a receptor's pocket as a `reference_shape` (pocket.py: the package's own)
        from . import pocket
        return getattr(pocket, name)
    raise AttributeError(name)
