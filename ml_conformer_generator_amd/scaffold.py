"""Rings and scaffolds of molecular graphs, on the GPU ("Rings and scaffolds"): which ring framework
a molecule has - the identity behind `unique="scaffold"` / `unique="framework"` and the ring fields of a record.

THE PACKAGE'S OWN, LABELLED DEFINITIONS: not RDKit's ring perception, no SSSR, and NOT RDKit's `MurckoScaffold`; no
agreement with any toolkit is claimed.  On the heavy-atom graph (symmetric bond codes 0 none / 1 / 2 / 3 / 4 aromatic, n <=
64 atoms), exact and independent of the atom numbering:
  ring bond    (a, j) iff j is reachable from a with that bond left out.
  ring atom    an atom with a ring bond.
  ring system  a connected component of the ring-bond sub-graph - fused, bridged and spiro rings are ONE system - labelled
               by its lowest atom index; a non-ring atom has -1.
  n_rings      ring bonds - ring atoms + ring systems, the cyclomatic number (cubane 5, naphthalene 2).
  ring size    of a ring bond: the shortest path between its ends with the bond left out, plus 1 - the smallest cycle
               through it; of an atom: the smallest over its ring bonds, 0 for a non-ring atom; `min_ring_size` /
               `max_ring_size` of the molecule: the smallest / largest over its ring bonds, 0 / 0 when acyclic.
               `max_ring_size` is "the largest ring one cannot avoid": a 14-membered macrocycle 14, bicyclo[2.2.2]octane 6.
  linker atom  remove, as long as one exists, every atom with fewer than two remaining neighbours; the non-ring atoms
               that remain: the atoms on paths between ring systems.  An acyclic fragment leaves nothing.
  exo atom     an atom outside ring and linker joined to a ring or linker atom by a code-2 bond (a ring C=O, a linker S=O).
  scaffold     ring + linker + exo atoms, elements and bond codes kept: the Bemis-Murcko framework with the doubly bonded
               first shell.
  framework    ring + linker atoms, every atom written as carbon and every bond as code 1: the generic graph framework.
The identity of a scaffold is `canonical.identity_bytes` of its graph; the empty scaffold (an acyclic molecule) has the
fixed identity `EMPTY_IDENTITY`, so all acyclic molecules share one scaffold; a scaffold without a canonical order
(`canonical.STATUS_DEGREE` / `STATUS_BUDGET`) has none and is not proven equal to anything.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _args, _lib
from . import canonical as mcg_canonical

MAX_ATOMS = 64                  # include/mlconfgen_hip.h MCG_SCAFFOLD_MAX_ATOMS
MAX_BATCH = 16384               # MCG_SCAFFOLD_MAX_B
MASK_RING, MASK_LINKER, MASK_EXO, MASK_SCAFFOLD = 0, 1, 2, 3          # the columns of `masks`
COUNT_NAMES = ("n_rings", "n_ring_systems", "min_ring_size", "max_ring_size", "ring_atoms", "linker_atoms", "exo_atoms",
               "ring_bonds")    # the columns of `counts`
MODE_KEEP, MODE_GENERIC = 0, 1  # `induced_subgraph`: elements and codes kept / Z = 6 and code 1
EMPTY_IDENTITY = (0, b"")       # the (key, identity bytes) of the empty scaffold
UNIQUE_VALUES = ("scaffold", "framework")                             # the values of `unique` this module serves


def _padded(atomic_numbers, bond_orders, n_nodes, device, check: bool, what: str):
    """(z, bonds, counts on the device as the kernels read them, B, W, the device); a width of 0 becomes the kernels'
    smallest, 1, with no atom in it."""
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS,
                                           f"{what} molecules of at most {MAX_ATOMS} atoms")
    dev = _args.resolve_device(device, bonds)
    if W == 0:
        z, bonds, W = torch.zeros(B, 1, dtype=torch.int32), torch.zeros(B, 1, 1, dtype=torch.int8), 1
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
    if check and B:
        _args.check_graphs(zd, bd, nn, W)
    return zd, bd, nn, B, W, dev


@torch.no_grad()
def ring_perception(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                    check: bool = True) -> Dict[str, torch.Tensor]:
    """The rings of B molecular graphs by this module's definitions, `mcg_ring_scaffold` launches over chunks of
    `MAX_BATCH` rows: `atomic_numbers` [B, >= W], `bond_orders` [B,W,W], `n_nodes` [B]; the diagonal and everything at or
    beyond a molecule's atom count is ignored, whatever it holds.  Device tensors, named after the kernel's outputs:
      ring_nb [B,W]      int64 holding the unsigned bit pattern: bit j of entry a set iff (a, j) is a ring bond; 0 beyond
                         the row's atoms
      ring_size [B,W]    int32: the atom's ring size, 0 for a non-ring atom and beyond the row's atoms
      ring_system [B,W]  int32: the atom's ring-system label, -1 for a non-ring atom and beyond the row's atoms
      masks [B,4]        int64 bit patterns: the ring, linker, exo and scaffold atoms (`MASK_*`)
      counts [B,8]       int32: `COUNT_NAMES`
    Every output is exact: the same bits whatever the batch, the row and the padded width.  A width of 0 is taken as 1.
    ValueError before the kernel as `canonical.canonical_order` raises them."""
    zd, bd, nn, B, W, dev = _padded(atomic_numbers, bond_orders, n_nodes, device, check, "ring perception takes")
    out = dict(ring_nb=torch.zeros(B, W, dtype=torch.int64, device=dev),
               ring_size=torch.zeros(B, W, dtype=torch.int32, device=dev),
               ring_system=torch.full((B, W), -1, dtype=torch.int32, device=dev),
               masks=torch.zeros(B, 4, dtype=torch.int64, device=dev),
               counts=torch.zeros(B, 8, dtype=torch.int32, device=dev))
    for lo in range(0, B, MAX_BATCH):
        hi = min(B, lo + MAX_BATCH)
        _lib.check(_lib.lib().mcg_ring_scaffold(_lib.dptr(zd[lo:hi]), _lib.dptr(bd[lo:hi]), _lib.dptr(nn[lo:hi]), hi - lo, W,
                                                _lib.dptr(out["ring_nb"][lo:hi]), _lib.dptr(out["ring_size"][lo:hi]),
                                                _lib.dptr(out["ring_system"][lo:hi]), _lib.dptr(out["masks"][lo:hi]),
                                                _lib.dptr(out["counts"][lo:hi]), _lib.current_stream_ptr(dev)),
                   "mcg_ring_scaffold")
    return out


@torch.no_grad()
def induced_subgraph(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, mask: torch.Tensor,
                     mode: int = MODE_KEEP, device=None) -> Dict[str, torch.Tensor]:
    """The sub-graph each row's `mask` [B] (int64 bit pattern: bit a keeps atom a) induces, `mcg_induced_subgraph`: the
    kept atoms in ascending index, compacted to the front.  Device tensors: `atomic_numbers` [B,W] int32, `bond_orders`
    [B,W,W] int8 (zero behind the kept atoms; a value that is no bond code is written as 0), `n` [B] int32, `atom_map`
    [B,W] int32 (the source index of each kept atom, -1 behind them).  `mode`: `MODE_KEEP`, or `MODE_GENERIC` - every
    kept atom carbon, every bond code 1."""
    if mode not in (MODE_KEEP, MODE_GENERIC):
        raise ValueError(f"mode must be {MODE_KEEP} (elements and codes kept) or {MODE_GENERIC} (generic), got {mode!r}")
    zd, bd, nn, B, W, dev = _padded(atomic_numbers, bond_orders, n_nodes, device, False, "sub-graphs are taken of")
    mask = torch.as_tensor(mask)
    if mask.numel() != B or mask.dtype != torch.int64:
        raise ValueError(f"mask must hold {B} int64 bit patterns, got {list(mask.shape)} of type {mask.dtype}")
    md = mask.reshape(B).to(dev).contiguous()
    out = dict(atomic_numbers=torch.zeros(B, W, dtype=torch.int32, device=dev),
               bond_orders=torch.zeros(B, W, W, dtype=torch.int8, device=dev),
               n=torch.zeros(B, dtype=torch.int32, device=dev),
               atom_map=torch.full((B, W), -1, dtype=torch.int32, device=dev))
    for lo in range(0, B, MAX_BATCH):
        hi = min(B, lo + MAX_BATCH)
        _lib.check(_lib.lib().mcg_induced_subgraph(_lib.dptr(zd[lo:hi]), _lib.dptr(bd[lo:hi]), _lib.dptr(nn[lo:hi]),
                                                   _lib.dptr(md[lo:hi]), int(mode), hi - lo, W,
                                                   _lib.dptr(out["atomic_numbers"][lo:hi]),
                                                   _lib.dptr(out["bond_orders"][lo:hi]), _lib.dptr(out["n"][lo:hi]),
                                                   _lib.dptr(out["atom_map"][lo:hi]), _lib.current_stream_ptr(dev)),
                   "mcg_induced_subgraph")
    return out


def identities_of(sub: Dict[str, torch.Tensor], ordered: Dict[str, torch.Tensor]) -> List[Optional[tuple]]:
    """Per row the identity of a compacted scaffold graph as (key, identity bytes): `EMPTY_IDENTITY` for the empty
    scaffold, None where the graph has no canonical order - such a row is not proven equal to anything.  The bytes are
    `canonical.identity_of` of the graph relabelled into its canonical order (one gather on the device, one D2H copy per
    tensor), cut out of the host arrays row by row: n, each Z as two bytes (low first), the lower-triangle codes."""
    status = ordered["status"].cpu().tolist()
    keys = [k & 0xFFFFFFFFFFFFFFFF for k in ordered["key"].cpu().tolist()]
    counts = sub["n"].cpu().tolist()
    zc, bc = mcg_canonical.relabel(sub["atomic_numbers"], sub["bond_orders"], ordered["order"])
    zc, bc = zc.cpu().numpy().astype("<u2"), bc.cpu().numpy().astype(np.uint8)
    below = {}                                         # n -> the lower triangle's indices, row by row
    out: List[Optional[tuple]] = []
    for b, (st, k, n) in enumerate(zip(status, keys, counts)):
        if st == mcg_canonical.STATUS_EMPTY:
            out.append(EMPTY_IDENTITY)
        elif st != 0:
            out.append(None)
        else:
            i, j = below.setdefault(n, np.tril_indices(n, -1))
            out.append((k, bytes([n]) + zc[b, :n].tobytes() + bc[b][i, j].tobytes()))
    return out


@torch.no_grad()
def murcko_scaffolds(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                     generic: bool = False, check: bool = True, perceived: Optional[Dict[str, torch.Tensor]] = None,
                     canonical_order=None) -> dict:
    """The scaffold (`generic=True`: the framework) of B molecular graphs by this module's definitions, without leaving the
    device: one `ring_perception` (or `perceived`, a result for the same graphs), one `induced_subgraph` of the scaffold
    mask (the ring + linker mask in mode `MODE_GENERIC`), one `canonical.canonical_order` launch on the sub-graphs
    (`canonical_order`: a callable (z, bonds, n) -> that dict in its place).  Returns the compacted graphs
    `atomic_numbers` [B,W], `bond_orders` [B,W,W], `n` [B], `atom_map` [B,W] (`induced_subgraph`), their canonical `order`
    [B,W] / `status` [B] / `key` [B], `identity` - per row (key, identity bytes), `EMPTY_IDENTITY` for an acyclic molecule,
    None for a scaffold without a canonical order - and `perceived`."""
    _args.check_flag("generic", generic)
    if perceived is None:
        perceived = ring_perception(atomic_numbers, bond_orders, n_nodes, device, check)
    masks = perceived["masks"]
    mask = (masks[:, MASK_RING] | masks[:, MASK_LINKER]) if generic else masks[:, MASK_SCAFFOLD]
    sub = induced_subgraph(atomic_numbers, bond_orders, n_nodes, mask.contiguous(),
                           MODE_GENERIC if generic else MODE_KEEP, masks.device)
    if canonical_order is None:
        ordered = mcg_canonical.canonical_order(sub["atomic_numbers"], sub["bond_orders"], sub["n"], masks.device,
                                                check=False)
    else:
        ordered = canonical_order(sub["atomic_numbers"], sub["bond_orders"], sub["n"])
    return dict(sub, order=ordered["order"], status=ordered["status"], key=ordered["key"],
                identity=identities_of(sub, ordered), perceived=perceived)


def smiles_of(scaffolds: dict) -> List[Optional[str]]:
    """Per row of a `murcko_scaffolds` result the canonical SMILES of its scaffold graph (`smiles.write_smiles` on the
    graph in its canonical order): "" for the empty scaffold, None where it has no canonical order.  Host work."""
    from . import smiles as mcg_smiles
    zc, bc = mcg_canonical.relabel(scaffolds["atomic_numbers"], scaffolds["bond_orders"], scaffolds["order"])
    zc, bc = zc.cpu(), bc.cpu()
    out: List[Optional[str]] = []
    for b, (st, n) in enumerate(zip(scaffolds["status"].cpu().tolist(), scaffolds["n"].cpu().tolist())):
        if st == mcg_canonical.STATUS_EMPTY:
            out.append("")
        elif st != 0:
            out.append(None)
        else:
            out.append(mcg_smiles.write_smiles(zc[b, :n], bc[b, :n, :n]))
    return out


@torch.no_grad()
def scaffold_smiles(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                    generic: bool = False, check: bool = True) -> List[Optional[str]]:
    """One string per row: the canonical SMILES of its scaffold (`generic=True`: its framework) - `murcko_scaffolds`, then
    `smiles_of`.  The empty string stands for the empty scaffold; None: the scaffold has no canonical order."""
    return smiles_of(murcko_scaffolds(atomic_numbers, bond_orders, n_nodes, device, generic, check))


def record_fields(scaffolds: dict, with_smiles: bool = False) -> Dict[str, object]:
    """The per-sample values of `handoff.Measured`'s ring and scaffold fields from a `murcko_scaffolds` result, as
    `handoff.measured_from_tensors` reads them: `n_rings` / `n_ring_systems` / `min_ring_size` / `max_ring_size` [B],
    `ring_sizes` / `ring_systems` [B,W], `scaffold_atoms` [B,W] (the `atom_map`: the kept atoms ascending, -1 behind
    them), `scaffold_key` [B] int64 (0 for the empty scaffold and where there is no order), `scaffold_status` [B] and -
    `with_smiles` - `scaffold_smiles`, a host list."""
    p = scaffolds["perceived"]
    counts = p["counts"]
    out = dict(n_rings=counts[:, 0], n_ring_systems=counts[:, 1], min_ring_size=counts[:, 2], max_ring_size=counts[:, 3],
               ring_sizes=p["ring_size"], ring_systems=p["ring_system"], scaffold_atoms=scaffolds["atom_map"],
               scaffold_key=scaffolds["key"], scaffold_status=scaffolds["status"])
    if with_smiles:
        out["scaffold_smiles"] = smiles_of(scaffolds)
    return out


def of_records(records: Sequence, generic: bool = False, device=None) -> List:
    """Annotates `GeneratedMolecule` records after the fact - for callers who want the ring and scaffold fields without a
    selection: one `murcko_scaffolds` pass over the records' own graphs, the fields of `record_fields` (with the string)
    written onto each record's values.  Returns the records; a record of more than `MAX_ATOMS` atoms is a ValueError."""
    from . import fingerprint as mcg_fp
    from .handoff import _UNMEASURED, Measured, measured_from_tensors
    records = list(records)
    if not records:
        return records
    graphs = [mcg_fp.mol_graph(m) for m in records]
    for k, (z, _) in enumerate(graphs):
        if len(z) > MAX_ATOMS:
            raise ValueError(f"records[{k}] has {len(z)} heavy atoms; ring perception takes at most {MAX_ATOMS}")
    z, bonds, n = mcg_fp.pad_graphs(graphs)
    found = murcko_scaffolds(z, bonds, n, device, generic, check=False)
    for m, values in zip(records, measured_from_tensors(record_fields(found, with_smiles=True), len(records))):
        if m._measured is _UNMEASURED:                 # the shared "nothing measured" value is never written to
            m._measured = Measured()
        for k in _RECORD_FIELDS:
            setattr(m._measured, k, getattr(values, k))
    return records


_RECORD_FIELDS = ("n_rings", "n_ring_systems", "min_ring_size", "max_ring_size", "ring_sizes", "ring_systems",
                  "scaffold_atoms", "scaffold_key", "scaffold_status", "scaffold_smiles")


def group_by_scaffold(identities: Sequence[Optional[tuple]]) -> List[List[int]]:
    """The positions of `identities` (`murcko_scaffolds`' `identity`) grouped by scaffold, as a list of index lists in
    first-seen order - for a caller's own "at most k per scaffold" policy.  A None (no canonical order) is a group of its
    own: it is not proven equal to anything."""
    groups: List[List[int]] = []
    seen: Dict[tuple, int] = {}
    for i, ident in enumerate(identities):
        if ident is None:
            groups.append([i])
            continue
        at = seen.setdefault(tuple(ident), len(groups))
        if at == len(groups):
            groups.append([])
        groups[at].append(i)
    return groups
