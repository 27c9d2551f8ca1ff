"""Exact canonical labelling of molecular graphs, on the GPU ("Canonical graphs and SMILES"): which
molecule a graph is, whatever its atom numbering - the identity behind `unique="exact"`, `exclude_graphs=` and the
canonical SMILES of a record (`smiles.py` writes the string from the graph in this order).

THE PACKAGE'S OWN, LABELLED DEFINITION: not RDKit's canonical atom ranking, and no agreement with any toolkit is claimed.
On the heavy-atom graph (atomic numbers Z, symmetric bond codes 0 none / 1 / 2 / 3 / 4 aromatic, n <= 64 atoms):
  colour      key0(a) = (Z, degree, twice the bond-order sum with aromatic 1.5); rank(a) = the number of atoms with a
              smaller key; tied atoms share a rank - a cell.
  refinement  key(a) = (rank(a), the (rank(j), code(a,j)) pairs of a's neighbours ascending), compared lexicographically,
              ranked again; repeated until the number of distinct ranks stops growing.  Integers only: nothing is hashed.
  search      all cells singletons: a leaf.  Else the target cell is the non-singleton cell of smallest rank r; for each
              member v in ascending input index: v keeps r, the other members get r + 1, refine, recurse.  The twin rule,
              the only pruning: v is skipped if an already tried member u is its twin - Z(u) = Z(v) and code(u,w) =
              code(v,w) for every w other than u and v (swapping twins is an automorphism).
  certificate of a leaf, order[k] the atom of rank k: Z(order[0..n-1]), then code(order[i], order[j]) for i = 1..n-1,
              j = 0..i-1.  The canonical order is the leaf with the lexicographically smallest certificate, the first
              such leaf on ties (equal certificates are automorphic images).
  refusals    per row, in `status`: EMPTY (n = 0), DEGREE (an atom with more than MAX_DEGREE = 8 neighbours), BUDGET (a
              branch was still unexplored behind the LEAF_BUDGET = 4 096th leaf; `leaves` is then 4 096).  Such a row has
              no canonical order (-1 throughout) and the key 0.
Two graphs have equal `identity_bytes` if and only if they are isomorphic (elements and bond codes included).  `key` is
64 bits of the certificate hashed under the fingerprint's two seeds: for grouping only, never for a decision.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _args, _lib

MAX_ATOMS = 64                 # include/mlconfgen_hip.h MCG_CANONICAL_MAX_ATOMS
MAX_BATCH = 16384               # MCG_CANONICAL_MAX_B
MAX_DEGREE = 8                  # MCG_CANONICAL_MAX_DEGREE
LEAF_BUDGET = 4096              # MCG_CANONICAL_LEAF_BUDGET
STATUS_EMPTY, STATUS_DEGREE, STATUS_BUDGET = 1, 2, 4
STATUS_NAMES = {STATUS_EMPTY: "EMPTY", STATUS_DEGREE: "DEGREE", STATUS_BUDGET: "BUDGET"}
REFUSAL_WITH_FINISHER = ("smiles cannot be combined with a finisher (RDKit's or a custom one): the canonical order and the "
                         "string go onto the GeneratedMolecule records; on RDKit Mols use Chem.MolToSmiles(mol)")


def describe_status(status: int) -> str:
    """"ok" for 0, else the names of the set bits of a `status` word, joined with "|"."""
    status = int(status)
    if status == 0:
        return "ok"
    names = [name for bit, name in STATUS_NAMES.items() if status & bit]
    rest = status & ~sum(STATUS_NAMES)
    return "|".join(names + ([f"0x{rest:x}"] if rest else []))


@torch.no_grad()
def canonical_order(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                    check: bool = True) -> Dict[str, torch.Tensor]:
    """The canonical atom order of B molecular graphs by this module's definition, `mcg_canonical_order` launches over
    chunks of `MAX_BATCH` rows: `atomic_numbers` [B, >= W], `bond_orders` [B,W,W] (symmetric codes 0 none / 1 / 2 / 3 / 4
    aromatic), `n_nodes` [B] real atoms each; the diagonal and everything at or beyond a molecule's atom count is
    ignored, whatever it holds.  Device tensors:
      order [B,W]   int32: position k holds the input index of the atom of canonical rank k; -1 beyond the row's atoms,
                    and throughout a row whose status is not 0
      status [B]    int32: 0, or STATUS_EMPTY / STATUS_DEGREE / STATUS_BUDGET (`describe_status`)
      leaves [B]    int32: the leaves the search visited (a function of the graph alone, whatever its numbering)
      key [B]       int64 holding the unsigned bit pattern: 64 bits of the certificate, 0 where status is not 0
    Every output is exact: the same bits whatever the batch, the row and the padded width; `leaves`, `key` and the
    relabelled graph do not depend on the atom numbering.
    ValueError before the kernel: W > 64, shapes that do not fit, atom counts outside [0, W], and with `check=True` (one
    device reduction, `fingerprint`'s) a code outside 0..4, a matrix that is not symmetric over the real atoms, an atomic
    number < 1 on a real atom."""
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS,
                                           f"canonical orders take molecules of at most {MAX_ATOMS} atoms")
    dev = _args.resolve_device(device, bonds)
    if W == 0:                                  # no atoms anywhere: B empty graphs at the kernel's smallest width
        z, bonds, W = torch.zeros(B, 1, dtype=torch.int32), torch.zeros(B, 1, 1, dtype=torch.int8), 1
        order = torch.full((B, 0), -1, dtype=torch.int32, device=dev)
    else:
        order = torch.full((B, W), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    leaves = torch.zeros(B, dtype=torch.int32, device=dev)
    key = torch.zeros(B, dtype=torch.int64, device=dev)
    out = dict(order=order, status=status, leaves=leaves, key=key)
    if B == 0:
        return out
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
    if check:
        _args.check_graphs(zd, bonds.to(dev), nn, W)
    wide = order if order.shape[1] == W else torch.full((B, W), -1, dtype=torch.int32, device=dev)
    for lo in range(0, B, MAX_BATCH):
        hi = min(B, lo + MAX_BATCH)
        _lib.check(_lib.lib().mcg_canonical_order(_lib.dptr(zd[lo:hi]), _lib.dptr(bd[lo:hi]), _lib.dptr(nn[lo:hi]), hi - lo,
                                                  W, _lib.dptr(wide[lo:hi]), _lib.dptr(status[lo:hi]),
                                                  _lib.dptr(leaves[lo:hi]), _lib.dptr(key[lo:hi]),
                                                  _lib.current_stream_ptr(dev)), "mcg_canonical_order")
    return out


def relabel(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, order: torch.Tensor
            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(z* [B,W] int32, bonds* [B,W,W] int8): the graphs with new atom k = old atom order[b, k], zero where order is -1;
    two gathers on the tensors' device.  The diagonal of bonds* is zero."""
    order = torch.as_tensor(order)
    dev = order.device
    B, W = int(order.shape[0]), int(order.shape[1])
    z = torch.as_tensor(atomic_numbers)[:, :W].to(dev, torch.int32)
    bonds = torch.as_tensor(bond_orders).to(dev, torch.int8)
    if W == 0:
        return z.reshape(B, 0), bonds.reshape(B, 0, 0)
    real = order >= 0
    idx = order.clamp(min=0).to(torch.long)
    zc = torch.where(real, z.gather(1, idx), torch.zeros_like(z))
    rows = bonds.gather(1, idx.unsqueeze(2).expand(B, W, W))
    both = rows.gather(2, idx.unsqueeze(1).expand(B, W, W))
    pair = real.unsqueeze(1) & real.unsqueeze(2) & ~torch.eye(W, dtype=torch.bool, device=dev).unsqueeze(0)
    return zc, torch.where(pair, both, torch.zeros_like(both))


@torch.no_grad()
def canonical_graphs(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                     check: bool = True, ordered: Optional[Dict[str, torch.Tensor]] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(z* [B,W] int32, bonds* [B,W,W] int8) on the device: the graphs relabelled into canonical order (`canonical_order`,
    then `relabel`) - equal for isomorphic graphs.  A row whose status is not 0 is all zero.  `ordered`: a
    `canonical_order` result for the same graphs, when the caller already has it."""
    out = ordered if ordered is not None else canonical_order(atomic_numbers, bond_orders, n_nodes, device, check)
    return relabel(atomic_numbers, bond_orders, out["order"])


def identity_of(z: List[int], codes: List[List[int]]) -> bytes:
    """The identity bytes of ONE graph already in canonical order: n, each Z as two bytes (low first), then the
    lower-triangle codes row by row."""
    n = len(z)
    return bytes([n]) + b"".join(bytes([v & 255, (v >> 8) & 255]) for v in z) + \
        bytes(codes[i][j] for i in range(1, n) for j in range(i))


@torch.no_grad()
def identity_bytes(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                   check: bool = True, ordered: Optional[Dict[str, torch.Tensor]] = None) -> List[Optional[bytes]]:
    """One `bytes` per row: the exact identity of its graph - n, Z* and the lower-triangle codes of the canonical graph
    (`identity_of`).  Equal bytes if and only if the graphs are isomorphic.  None for a row whose status is not 0: it is
    not proven equal to anything.  One D2H copy per tensor."""
    out = ordered if ordered is not None else canonical_order(atomic_numbers, bond_orders, n_nodes, device, check)
    zc, bc = relabel(atomic_numbers, bond_orders, out["order"])
    status = out["status"].cpu().tolist()
    counts = torch.as_tensor(n_nodes).reshape(-1).cpu().tolist()
    zc, bc = zc.cpu().tolist(), bc.cpu().tolist()
    return [identity_of(zc[b][: counts[b]], bc[b]) if status[b] == 0 else None for b in range(len(status))]
