"""Standardised molecular graphs on the GPU ("Standardised graphs"): the largest fragment of a
generated graph, the checks that make it a molecule, and a Kekule form of its aromatic bonds - the three stages the
reference runs on RDKit Mols in `standardize_mol` (FragmentParent, Kekulize, SanitizeMol), for the records path that has
no RDKit.

THE PACKAGE'S OWN, LABELLED DEFINITION: not RDKit's `FragmentParent` / `Kekulize` / `SanitizeMol` - no formal charges are
assigned, no normalisation transforms are applied, no tautomers, no stereo; no agreement with RDKit is claimed.

Inputs per molecule, as `hydrogens.add_hydrogens` takes them: fp32 coords, atomic numbers, symmetric bond codes (0 none,
1, 2, 3, 4 aromatic), n <= 64 atoms.  Any other code, the diagonal and everything at or beyond n reads as no bond (the
matrix is read through its lower triangle).
Fragments  the connected components of the bond graph over the n real atoms.  The PARENT is the component with the most
         atoms; ties go to the larger sum of atomic numbers, then to the component that holds the lowest atom index.  Kept
         atoms keep their relative order: new index = rank among the kept.  Coordinates are copied bit for bit.
Checks   on the parent, collected in `status` (a bit set; 0 = valid):
         EMPTY (1)            n = 0.
         OVER_VALENCE (2)     a kept atom's bonds exceed `2 * max_valence[Z]` of csrc/mcg_elements.h (the validity proxy's
                              table) in half-bonds, the codes 1/2/3/4 counting 2/4/6/2.  An aromatic bond counts its
                              sigma bond here and NOT the proxy's 3: with 3, furan's oxygen (two aromatic bonds: 3 > 2),
                              every ring-fusion carbon (three: 4.5 > 4) and 2-pyridone's carbonyl carbon would be
                              over-valent and no fused aromatic could be valid.  The pi electron is the Kekule search's
                              business: it gives an atom a double bond only where v0 has room for it.
         AROMATIC_BRIDGE (4)  some code-4 bond is a bridge of the parent's bond graph: removing it disconnects its ends,
                              so it lies in no ring.
         NOT_KEKULIZABLE (8), SEARCH_BUDGET (16): the Kekule search below; it runs only when bits 1, 2 and 4 are clear.
         A row with a non-finite coordinate is standardised like any other: the coordinates play no part in the verdict.
Kekule form   with the v0 table of `pharmacophore.py` / `hydrogens.VALENCE` (any other Z: 0): for an atom, sigma = the sum
         of the orders of its code-1/2/3 bonds + its number of code-4 bonds, free = v0 - sigma.  An atom is ELIGIBLE if it
         has a code-4 bond and free >= 1; an eligible atom is OPTIONAL if Z is 7, 15 or 33, else REQUIRED.  Eligible edges
         are the code-4 bonds between two eligible atoms.  The search runs independently on each connected component of
         the eligible graph:
           pick the highest-index eligible atom a that is neither matched nor skipped; none: the component succeeds.
           Try its unmatched, unskipped eligible neighbours in descending index: match the pair, recurse, undo on failure.
           Then, if a is optional, mark it skipped and recurse; undo on failure.  Otherwise fail.
         Every entry into this procedure costs one step; a component that exceeds KEKULE_BUDGET = 16384 steps stops and
         sets SEARCH_BUDGET; a component that fails sets NOT_KEKULIZABLE.  No pruning changes the step count.
         `kekule_orders`: the parent's codes with each code-4 bond replaced by 2 where its ends are a matched pair and by
         1 otherwise; all zero when status != 0.  By construction no atom exceeds v0 on its formerly aromatic bonds.
         Highest-first leaves the LOWEST-index N of pyrrole, imidazole and benzimidazole without a double bond: the N to
         which `hydrogens.py` gives its aromatic N-H.
Known departures from RDKit: `LargestFragmentChooser` counts hydrogens too and breaks ties by SMILES; RDKit kekulizes a
5-ring N only with an explicit `[nH]`, where this search simply leaves an N unmatched; RDKit's valence model (charges,
hypervalent states) is not reproduced.
A molecule's outputs have the same bits whatever the batch, its row and the padded widths.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import _args, _lib

MAX_ATOMS = 64                  # include/mlconfgen_hip.h MCG_STANDARDIZE_MAX_ATOMS
MAX_BATCH = 16384               # MCG_STANDARDIZE_MAX_B
KEKULE_BUDGET = 16384           # MCG_STANDARDIZE_KEKULE_BUDGET
EMPTY, OVER_VALENCE, AROMATIC_BRIDGE, NOT_KEKULIZABLE, SEARCH_BUDGET = 1, 2, 4, 8, 16
STATUS_NAMES = {EMPTY: "EMPTY", OVER_VALENCE: "OVER_VALENCE", AROMATIC_BRIDGE: "AROMATIC_BRIDGE",
                NOT_KEKULIZABLE: "NOT_KEKULIZABLE", SEARCH_BUDGET: "SEARCH_BUDGET"}
REFUSAL_WITH_FINISHER = ("standardize cannot be combined with a finisher (RDKit's or a custom one): it standardises the "
                         "GeneratedMolecule records; RDKit's finisher already runs standardize_mol on its Mols")


def describe_status(status: int) -> List[str]:
    """The names of the bits set in a `status` value, ascending; [] for a valid molecule."""
    status = int(status)
    if status < 0 or status >= 2 * SEARCH_BUDGET:
        raise ValueError(f"not a standardisation status: {status}")
    return [name for bit, name in STATUS_NAMES.items() if status & bit]


@torch.no_grad()
def standardize_graphs(coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor,
                       n_nodes: torch.Tensor, device=None, check: bool = True) -> Dict[str, torch.Tensor]:
    """The standardised form of B molecular graphs by this module's definition (NOT RDKit's): one
    `mcg_standardize_graphs` launch per 16384 rows.  `coords` [B,N,3] fp32, `atomic_numbers` [B, >= W], `bond_orders`
    [B,W,W] (symmetric codes 0 none / 1 / 2 / 3 / 4 aromatic), `n_nodes` [B] real atoms each, at most min(N, W); W <= 64.
    Device tensors:
      coords [B,N,3]          the parent's coordinates, compacted, copied bit for bit, zero beyond its atoms
      atomic_numbers [B,W]    int32, likewise
      bond_orders [B,W,W]     int8: the parent's codes, compacted
      n_nodes [B]             int32: the parent's atom count
      kekule_orders [B,W,W]   int8: the codes with every aromatic bond written 1 or 2; all zero where status != 0
      atom_map [B,W]          int32: the old index of each new atom, -1 beyond the parent
      n_fragments [B], atoms_removed [B]   int32
      status [B]              int32 bit set (`describe_status`), valid [B] bool = status == 0
    ValueError before the kernel: shapes that do not fit, W > 64, float graph tensors, atom counts outside
    [0, min(N, W)], and with `check=True` (one device reduction, one host read) a code outside 0..4, a matrix that is not
    symmetric or an atomic number < 1 on a real atom."""
    x = torch.as_tensor(coords)
    if x.dim() != 3 or x.shape[2] != 3 or not x.dtype.is_floating_point:
        raise ValueError(f"coords must be floating point [B,N,3], got {list(x.shape)} of type {x.dtype}")
    too_wide = f"graphs of at most {MAX_ATOMS} atoms are standardised"
    width = torch.as_tensor(bond_orders).shape[1:2]
    if width and int(width[0]) > MAX_ATOMS:      # named before the rest of the shape is looked at
        raise ValueError(f"{too_wide}, got a width of {int(width[0])}")
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS, too_wide, counts=False)
    N = int(x.shape[1])
    if int(x.shape[0]) != B:
        raise ValueError(f"coords holds {int(x.shape[0])} molecules, bond_orders {B}")
    _args.check_n_nodes(n_nodes, B, min(N, W))
    dev = _args.resolve_device(device, x)
    launches = B > 0 and N > 0 and W > 0           # the kernel writes every element of every output
    fill = torch.empty if launches else torch.zeros
    out = {"coords": fill(B, N, 3, dtype=torch.float32, device=dev),
           "atomic_numbers": fill(B, W, dtype=torch.int32, device=dev),
           "bond_orders": fill(B, W, W, dtype=torch.int8, device=dev),
           "n_nodes": fill(B, dtype=torch.int32, device=dev),
           "kekule_orders": fill(B, W, W, dtype=torch.int8, device=dev),
           "atom_map": torch.empty(B, W, dtype=torch.int32, device=dev) if launches else
           torch.full((B, W), -1, dtype=torch.int32, device=dev),
           "n_fragments": fill(B, dtype=torch.int32, device=dev),
           "atoms_removed": fill(B, dtype=torch.int32, device=dev),
           "status": fill(B, dtype=torch.int32, device=dev) if launches else
           torch.full((B,), EMPTY, dtype=torch.int32, device=dev)}
    if launches:
        xd = x.to(dev, torch.float32).contiguous()
        zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
        if check:
            _args.check_graphs(zd, bd, nn, W)
        for lo in range(0, B, MAX_BATCH):
            rows = slice(lo, min(lo + MAX_BATCH, B))
            _lib.check(_lib.lib().mcg_standardize_graphs(
                _lib.dptr(xd[rows]), _lib.dptr(zd[rows]), _lib.dptr(bd[rows]), _lib.dptr(nn[rows]), rows.stop - lo, N, W,
                _lib.dptr(out["coords"][rows]), _lib.dptr(out["atomic_numbers"][rows]), _lib.dptr(out["bond_orders"][rows]),
                _lib.dptr(out["kekule_orders"][rows]), _lib.dptr(out["atom_map"][rows]), _lib.dptr(out["n_nodes"][rows]),
                _lib.dptr(out["n_fragments"][rows]), _lib.dptr(out["atoms_removed"][rows]), _lib.dptr(out["status"][rows]),
                _lib.current_stream_ptr(dev)), "mcg_standardize_graphs")
    out["valid"] = out["status"] == 0
    return out
