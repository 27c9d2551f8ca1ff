"""Exact stereo identity of embedded molecular graphs, on the GPU ("Stereo identity"): which
STEREOISOMER a set of coordinates is, whatever its atom numbering and whatever proper rigid motion it went through - the
identity behind `unique="stereo"` and the isomeric SMILES of a record (`smiles="isomeric"`; `smiles.py` writes the marks).

THE PACKAGE'S OWN, LABELLED DEFINITION: not RDKit's stereo perception, no CIP R/S labels, no string equality with any
toolkit.  On the heavy-atom coordinates (fp32) and the graph of `canonical.py`:
  tetrahedral   an atom is a candidate when Z is 6 or 14, every bond has code 1, the heavy degree is 4 - or 3, the fourth
                valence then being the one implicit hydrogen - and its neighbours do not include two terminal twins (two
                degree-1 atoms of equal Z bonded to it with the same code).  With the neighbours in ascending input
                index, chi = det[(n1-n4),(n2-n4),(n3-n4)] over the product of the three lengths (degree 3: of the three
                unit vectors n_i - a); s = sign chi; UNDEFINED (s = 0) where |chi| < 0.1 or a vector has no length.
  double bond   a code-2 bond a=b is a candidate when both ends have Z 6 or 7, no other bond that is not code 1, one or
                two further heavy neighbours and no two terminal twins.  c = the cosine of the dihedral of each
                substituent pair about the axis (perpendicular components, normalised); UNDEFINED where a |c| < 0.1, a
                perpendicular component vanishes, or two substituents of one end do not lie on opposite sides of every
                substituent of the other end.  Ring bonds are not excluded: in a small ring the descriptor is a constant.
  descriptors   at a labelling L (a leaf of the search): tet(a) = 0, or 1 / 2 by the sign of s(a) x the parity of the
                permutation that sorts a's neighbours by L (the implicit H last); db = 0, or 1 where the lowest-L
                substituents of the two ends are cis, 2 where trans, stored at the end of larger L.  The stereo vector:
                v[k] = 4 tet + db of the atom at position k.
  identity      the lexicographically smallest (certificate, v) - the certificate is `canonical.py`'s and compared
                first, so: the smallest v over ALL labellings whose certificate is that search's minimal one (they are
                one labelling's images under every automorphism of the graph).
  search        `canonical.py`'s, except that a leaf whose certificate equals the best one wins if its v is smaller, and
                that the twin rule skips only TERMINAL twins (twins of degree <= 1: swapping them moves no descriptor;
                swapping the two CH2 of a 1,3-disubstituted cyclobutane does).  `leaves` therefore differs from the
                graph search's; limits, refusals and status bits are the same.
Two embedded molecules have equal `stereo_identity_bytes` if and only if some graph isomorphism carries every defined
descriptor of one onto the other's: a centre with two interchangeable substituents has the same value in the molecule and
its mirror image, meso forms equal their mirror image, pseudo-asymmetric and ring cis / trans cases are told apart.
`stereo_key` is 64 bits of (certificate, v): for grouping only, never for a decision.  Deliberately out: CIP labels,
N / P / S centres, allenes and axes, charges.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _args, _lib
from . import canonical as mcg_canonical

MAX_ATOMS = mcg_canonical.MAX_ATOMS
MAX_BATCH = mcg_canonical.MAX_BATCH
THRESHOLD = 0.1                 # |chi| and |cos| below it: undefined - part of the definition
REFUSAL_UNIQUE_WITH_FINISHER = ('unique="stereo" cannot be combined with a finisher (RDKit\'s or a custom one): the stereo '
                                "identity is read from the GeneratedMolecule records' coordinates; on RDKit Mols use "
                                "Chem.AssignStereochemistryFrom3D(mol) and compare isomeric SMILES or InChI")


@torch.no_grad()
def stereo_order(coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor,
                 device=None, check: bool = True) -> Dict[str, torch.Tensor]:
    """The stereo identity of B embedded molecules by this module's definition, `mcg_stereo_order` launches over chunks of
    `MAX_BATCH` rows: `coords` [B, N, 3] floating point (read as fp32, for real atoms only; N may be smaller than W
    where no molecule has more than N atoms), `atomic_numbers`, `bond_orders` [B,W,W], `n_nodes` as `canonical.canonical_order` takes them.  Device tensors:
      order [B,W], status [B], leaves [B], key [B]   as `canonical.canonical_order` returns them; `key` is the GRAPH key and
                    equals that function's wherever both have status 0; `leaves` counts this search's leaves
      stereo [B,W]  int8: v in canonical position order (4 tet + db of the atom order[b, k]); 0 beyond the row's atoms
                    and throughout a row whose status is not 0
      stereo_key [B] int64 holding the unsigned bit pattern: 64 bits of (certificate, v), 0 where status is not 0
      counts [B,3]  int32: defined tetrahedral descriptors, defined double bonds, undefined candidates
    Every integer output is exact and the same whatever the batch, the row and the padded width; `stereo`, `stereo_key`
    and `leaves` depend neither on the atom numbering nor on a proper rigid motion of the coordinates (away from the 0.1
    threshold).  ValueError before the kernel: `canonical_order`'s, coordinates that are not [B, N, 3] floats, an atom
    count above N."""
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS,
                                           f"stereo orders take molecules of at most {MAX_ATOMS} atoms")
    x = torch.as_tensor(coords)
    if x.dim() != 3 or x.shape[0] != B or x.shape[2] != 3 or not x.dtype.is_floating_point:
        raise ValueError(f"coords must be floating point [B, N, 3] = [{B}, N, 3], got {list(x.shape)} of type {x.dtype}")
    if x.shape[1] < W:                          # a generation's coordinates are as wide as its largest molecule only
        _args.check_n_nodes(n_nodes, B, int(x.shape[1]))
        x = torch.cat([x, x.new_zeros(B, W - x.shape[1], 3)], dim=1)
    dev = _args.resolve_device(device, bonds, x)
    wide = max(W, 1)
    out = dict(order=torch.full((B, W), -1, dtype=torch.int32, device=dev),
               status=torch.zeros(B, dtype=torch.int32, device=dev), leaves=torch.zeros(B, dtype=torch.int32, device=dev),
               key=torch.zeros(B, dtype=torch.int64, device=dev), stereo=torch.zeros(B, W, dtype=torch.int8, device=dev),
               stereo_key=torch.zeros(B, dtype=torch.int64, device=dev),
               counts=torch.zeros(B, 3, dtype=torch.int32, device=dev))
    if B == 0:
        return out
    if W == 0:                                  # no atoms anywhere: B empty graphs at the kernel's smallest width
        z, bonds = torch.zeros(B, 1, dtype=torch.int32), torch.zeros(B, 1, 1, dtype=torch.int8)
        x = torch.zeros(B, 1, 3)
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, wide, dev)
    xd = x[:, :wide].to(dev, torch.float32).contiguous()
    if check:
        _args.check_graphs(zd, bonds.to(dev), nn, wide)
    order = out["order"] if W else torch.full((B, 1), -1, dtype=torch.int32, device=dev)
    stereo = out["stereo"] if W else torch.zeros(B, 1, dtype=torch.int8, device=dev)
    for lo in range(0, B, MAX_BATCH):
        hi = min(B, lo + MAX_BATCH)
        _lib.check(_lib.lib().mcg_stereo_order(
            _lib.dptr(xd[lo:hi]), _lib.dptr(zd[lo:hi]), _lib.dptr(bd[lo:hi]), _lib.dptr(nn[lo:hi]), hi - lo, wide,
            _lib.dptr(order[lo:hi]), _lib.dptr(out["status"][lo:hi]), _lib.dptr(out["leaves"][lo:hi]),
            _lib.dptr(out["key"][lo:hi]), _lib.dptr(stereo[lo:hi]), _lib.dptr(out["stereo_key"][lo:hi]),
            _lib.dptr(out["counts"][lo:hi]), _lib.current_stream_ptr(dev)), "mcg_stereo_order")
    return out


@torch.no_grad()
def stereo_identity_bytes(coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor,
                          n_nodes: torch.Tensor, device=None, check: bool = True,
                          ordered: Optional[Dict[str, torch.Tensor]] = None) -> List[Optional[bytes]]:
    """One `bytes` per row: the exact stereo identity - `canonical.identity_of` of the graph in this search's order, then
    the n bytes of v.  Equal bytes if and only if some graph isomorphism carries every defined descriptor of one molecule
    onto the other's.  None for a row whose status is not 0.  `ordered`: a `stereo_order` result for the same rows."""
    out = ordered if ordered is not None else stereo_order(coords, atomic_numbers, bond_orders, n_nodes, device, check)
    zc, bc = mcg_canonical.relabel(atomic_numbers, bond_orders, out["order"])
    status = out["status"].cpu().tolist()
    counts = torch.as_tensor(n_nodes).reshape(-1).cpu().tolist()
    zc, bc, v = zc.cpu().tolist(), bc.cpu().tolist(), out["stereo"].cpu().tolist()
    return [mcg_canonical.identity_of(zc[b][: counts[b]], bc[b]) + bytes(v[b][: counts[b]]) if status[b] == 0 else None
            for b in range(len(status))]


def own_order_descriptors(order, stereo, bond_orders) -> List[int]:
    """v of ONE molecule - which is in canonical position order and relative to the canonical labelling L - as one
    value 4 tet + db per atom IN THE MOLECULE'S OWN ORDER AND RELATIVE TO IT: tet 1 / 2 is the handedness of the atom's
    neighbours taken in ascending own index (the implicit H last), db 1 cis / 2 trans of the lowest-indexed substituents
    of the two ends, stored at the end of larger index - what `smiles.write_smiles(..., stereo=)` reads for a graph in
    this order.  `order[k]`: the atom of canonical rank k; `stereo[k]`: its v; `bond_orders` [n,n] in the molecule's own
    order.  Integers only: tet flips with the parity between the two neighbour orders, db once per end whose lowest
    substituent differs between them (two substituents of one end lie on opposite sides)."""
    order = [int(a) for a in order]
    n = len(order)
    codes = torch.as_tensor(bond_orders)[:n, :n].tolist()
    L = [0] * n
    for k, a in enumerate(order):
        L[a] = k
    out = [0] * n
    for k, a in enumerate(order):
        v = int(stereo[k])
        tet, db = v >> 2, v & 3
        nb = [j for j in range(n) if j != a and codes[a][j] != 0]
        if tet:
            odd = sum(1 for i in range(len(nb)) for j in range(i) if L[nb[j]] > L[nb[i]]) & 1
            out[a] += 4 * (3 - tet if odd else tet)
        if db:
            b = next(j for j in nb if codes[a][j] == 2)
            for c, other in ((a, b), (b, a)):
                subs = [j for j in range(n) if j != c and j != other and codes[c][j] != 0]
                if min(subs, key=lambda j: L[j]) != subs[0]:
                    db = 3 - db
            out[max(a, b)] += db
    return out
