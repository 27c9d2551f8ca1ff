"""Chemical fingerprints and graph identity keys of molecular graphs, on the GPU ("Chemical
fingerprints").

A LABELLED SUBSTITUTE: the fingerprint is a circular, Morgan-type fingerprint with the parameters of the reference's
`evaluate_samples` (radius 2, 2 048 bits, bond types on, chirality off), but by this package's OWN definition - it is not
bit-compatible with RDKit's Morgan fingerprint (RDKit's atom invariants need implicit hydrogens and its own hash).
`cheminformatics.evaluate_samples` keeps RDKit's own fingerprints where RDKit imports.

Definition, on the heavy-atom graph (atomic numbers Z, symmetric bond codes 0 none / 1 / 2 / 3 / 4 aromatic), with H =
MurmurHash3_x86_32 over uint32 words and SEED = 0x6d636731:
  inv_0(a) = H([0, Z(a), degree, twice the bond-order sum (aromatic 1.5), size of the smallest ring through a or 0]);
  inv_r(a) = H([r, inv_{r-1}(a), then the neighbours' (bond code, inv_{r-1}) pairs in ascending order]);
  fingerprint: bit inv_r(a) & 2047 for every atom and r = 0, 1, 2, as 64 uint32 words (bit k: word k >> 5, position k & 31);
  graph key:   the n invariants after K = max(n - 1, 2) rounds, sorted, hashed with n under two seeds into 64 bits.
Isomorphic graphs always get equal keys and fingerprints, whatever the atom numbering.  The converse can fail: two
different graphs that colour refinement cannot tell apart, or a hash collision, share a key (cubane's skeleton and the
Wagner graph do); `canonical.py` has the exact identity.
Tanimoto of two fingerprints: popcount(A & B) / popcount(A | B) in fp32; NaN where either has no bit set (no atoms).

No aromaticity is perceived: a reference graph and the generated graphs must use ONE convention (the generator emits
code 4 for aromatic bonds; an RDKit-sanitised reference Mol reports 1.5 for them, which is read as code 4).
"""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple

import torch

from . import _args, _lib

FP_WORDS = 64                   # include/mlconfgen_hip.h MCG_FP_WORDS: 2 048 bits
MAX_GRAPH_ATOMS = 64            # csrc/mcg_fingerprint.hip FP_MAXW: one lane and one 64-bit neighbour mask per atom
MAX_PAIR_BATCH = 16384          # MCG_SHAPE_PAIR_MAX_B: the [B,B] fp32 matrix stays within 1 GB
_BOND_CODE = {1.0: 1, 2.0: 2, 3.0: 3, 1.5: 4}


# ----------------------------------------------------------------------------------------------- graphs
def mol_graph(obj) -> Tuple[List[int], torch.Tensor]:
    """(atomic_numbers, bond_orders [n,n] int8) of the HEAVY atoms of `obj`: a `GeneratedMolecule`; an RDKit Mol or any
    stand-in with `GetAtoms()` / `GetBonds()` (atoms `GetAtomicNum`; bonds `GetBeginAtomIdx`, `GetEndAtomIdx`,
    `GetBondTypeAsDouble` 1, 2, 3, 1.5 -> codes 1, 2, 3, 4; hydrogens and their bonds are dropped); or an
    `(atomic_numbers, bond_orders)` pair (hydrogens dropped likewise).  No aromaticity perception: a Kekule reference and
    an aromatic generated molecule are different graphs.  ValueError: any other object, another bond type, a bond matrix
    that is not square, symmetric and of codes 0..4, an atomic number < 1."""
    from .handoff import GeneratedMolecule
    if isinstance(obj, GeneratedMolecule):
        z, bonds = [int(v) for v in obj.atomic_numbers], torch.as_tensor(obj.bond_orders).to(torch.int8)
    elif hasattr(obj, "GetAtoms") and hasattr(obj, "GetBonds"):
        z = [int(a.GetAtomicNum()) for a in obj.GetAtoms()]
        bonds = torch.zeros(len(z), len(z), dtype=torch.int8)
        for bnd in obj.GetBonds():
            i, j, order = int(bnd.GetBeginAtomIdx()), int(bnd.GetEndAtomIdx()), float(bnd.GetBondTypeAsDouble())
            if order not in _BOND_CODE:
                raise ValueError(f"bond {i}-{j}: bond type {order!r} is not single, double, triple or aromatic")
            bonds[i, j] = bonds[j, i] = _BOND_CODE[order]
    elif isinstance(obj, (tuple, list)) and len(obj) == 2:
        try:
            z = [int(v) for v in torch.as_tensor(obj[0]).reshape(-1).tolist()]
            bonds = torch.as_tensor(obj[1])
        except (TypeError, RuntimeError, ValueError) as e:
            raise ValueError(f"(atomic_numbers, bond_orders): unreadable: {e}") from None
        if bonds.dim() != 2 or tuple(bonds.shape) != (len(z), len(z)) or bonds.dtype.is_floating_point or \
                bonds.dtype == torch.bool:
            raise ValueError(f"(atomic_numbers [n], bond_orders [n,n]): integer bond codes [{len(z)},{len(z)}] are needed, "
                             f"got {list(bonds.shape)} of type {bonds.dtype}")
        bonds = bonds.cpu().to(torch.int64)
        if bonds.numel() and (int(bonds.min()) < 0 or int(bonds.max()) > 4 or not torch.equal(bonds, bonds.t())):
            raise ValueError("bond_orders must be symmetric with codes 0 none / 1 / 2 / 3 / 4 aromatic")
        bonds = bonds.to(torch.int8)
    else:
        raise ValueError("a molecular graph is a GeneratedMolecule, a Mol with GetAtoms() / GetBonds() or an "
                         f"(atomic_numbers, bond_orders) pair, got {type(obj).__name__}")
    if any(v < 1 for v in z):
        raise ValueError(f"atomic numbers must be >= 1, got {min(z)}")
    heavy = [k for k, v in enumerate(z) if v != 1]
    if len(heavy) != len(z):
        idx = torch.tensor(heavy, dtype=torch.long)
        z, bonds = [z[k] for k in heavy], bonds.index_select(0, idx).index_select(1, idx)
    return z, bonds.contiguous()


def pad_graphs(graphs: Sequence[Tuple[List[int], torch.Tensor]]):
    """`mol_graph` results -> (atomic_numbers [B,W] int32, bond_orders [B,W,W] int8, n_nodes [B] int32) on the host, W the
    largest atom count (at least 1)."""
    n = [len(z) for z, _ in graphs]
    W = max(n + [1])
    zs = torch.zeros(len(graphs), W, dtype=torch.int32)
    bonds = torch.zeros(len(graphs), W, W, dtype=torch.int8)
    for b, (z, bo) in enumerate(graphs):
        zs[b, : n[b]] = torch.tensor(z, dtype=torch.int32)
        bonds[b, : n[b], : n[b]] = bo
    return zs, bonds, torch.tensor(n, dtype=torch.int32)


# ----------------------------------------------------------------------------------------------- device
@torch.no_grad()
def graph_fingerprints(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                       check: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(fingerprint [B,64] int32, graph key [B] int64, set bits [B] int32) on the device, of B molecular graphs:
    `atomic_numbers` [B, >= W], `bond_orders` [B,W,W] (symmetric codes 0 none / 1 / 2 / 3 / 4 aromatic), `n_nodes` [B]
    real atoms each; the diagonal and everything at or beyond a molecule's atom count is ignored, whatever it holds.
    One `mcg_graph_fingerprint` launch (this module's docstring: the definition, and that it is a substitute for RDKit's
    Morgan fingerprint, not that fingerprint).  The int32 / int64 tensors hold the unsigned bit patterns; a key as a
    Python int: `int(k) & (2**64 - 1)`.  Equal keys mean isomorphic graphs up to what colour refinement can tell apart
    and hash collisions; isomorphic graphs always have equal keys.  Every output is exact: the same bits whatever the
    batch, the row, the padded width and the atom numbering.
    ValueError before the kernel: W > 64, shapes that do not fit, atom counts outside [0, W]
    (`cheminformatics.check_n_nodes`), and with `check=True` (one device reduction) a code outside 0..4, a matrix that is
    not symmetric over the real atoms, an atomic number < 1 on a real atom."""
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_GRAPH_ATOMS,
                                           f"graph fingerprints take molecules of at most {MAX_GRAPH_ATOMS} atoms")
    dev = _args.resolve_device(device, bonds)
    fp = torch.zeros(B, FP_WORDS, dtype=torch.int32, device=dev)
    key = torch.empty(B, dtype=torch.int64, device=dev)
    pop = torch.zeros(B, dtype=torch.int32, device=dev)
    if B == 0:
        return fp, key, pop
    if W == 0:                                  # no atoms anywhere: B empty graphs at the kernel's smallest width
        z, bonds, W = torch.zeros(B, 1, dtype=torch.int32), torch.zeros(B, 1, 1, dtype=torch.int8), 1
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
    if check:
        _args.check_graphs(zd, bonds.to(dev), nn, W)
    _lib.check(_lib.lib().mcg_graph_fingerprint(_lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nn), B, W, _lib.dptr(fp),
                                                _lib.dptr(key), _lib.dptr(pop), _lib.current_stream_ptr(dev)),
               "mcg_graph_fingerprint")
    return fp, key, pop


def _fp_tensor(fp, dev=None) -> torch.Tensor:
    f = torch.as_tensor(fp)
    if f.dim() not in (1, 2) or f.shape[-1] != FP_WORDS or f.dtype != torch.int32:
        raise ValueError(f"a fingerprint is [..., {FP_WORDS}] int32, got {list(f.shape)} of type {f.dtype}")
    return f if dev is None else f.to(dev)


@torch.no_grad()
def fingerprint_tanimoto(fp: torch.Tensor, ref_fp: torch.Tensor) -> torch.Tensor:
    """[B] fp32 on the device: the Tanimoto of every fingerprint `fp` [B,64] against the one fingerprint `ref_fp` [64]
    (`mcg_fingerprint_tanimoto`): popcount(A & B) / popcount(A | B), one fp32 division; NaN where either has no bit."""
    f = _fp_tensor(fp)
    if f.dim() != 2:
        raise ValueError(f"fp must be [B, {FP_WORDS}], got {list(f.shape)}")
    dev = _args.resolve_device(None, f)
    f = f.to(dev).contiguous()
    ref = _fp_tensor(ref_fp, dev).reshape(-1).contiguous()
    if ref.numel() != FP_WORDS:
        raise ValueError(f"ref_fp must be one fingerprint of {FP_WORDS} words, got {list(ref.shape)}")
    B = int(f.shape[0])
    out = torch.empty(B, device=dev)
    if B == 0:
        return out
    _lib.check(_lib.lib().mcg_fingerprint_tanimoto(_lib.dptr(f), _lib.dptr(ref), B, _lib.dptr(out),
                                                   _lib.current_stream_ptr(dev)), "mcg_fingerprint_tanimoto")
    return out


@torch.no_grad()
def pairwise_fingerprint_tanimoto(fp: torch.Tensor) -> torch.Tensor:
    """[B,B] fp32 on the device: the Tanimoto of every pair of the fingerprints `fp` [B,64]
    (`mcg_fingerprint_pair_tanimoto`).  Exactly symmetric, the diagonal exactly 1; a molecule without atoms has a NaN row
    and column and changes no other entry.  ValueError for more than `MAX_PAIR_BATCH` fingerprints."""
    f = _fp_tensor(fp)
    if f.dim() != 2:
        raise ValueError(f"fp must be [B, {FP_WORDS}], got {list(f.shape)}")
    B = int(f.shape[0])
    if B > MAX_PAIR_BATCH:
        raise ValueError(f"the pair matrix takes at most {MAX_PAIR_BATCH} fingerprints, got {B}")
    dev = _args.resolve_device(None, f)
    f = f.to(dev).contiguous()
    out = torch.empty(B, B, device=dev)
    if B == 0:
        return out
    _lib.check(_lib.lib().mcg_fingerprint_pair_tanimoto(_lib.dptr(f), B, _lib.dptr(out), _lib.current_stream_ptr(dev)),
               "mcg_fingerprint_pair_tanimoto")
    return out


# ----------------------------------------------------------------------------------------------- host
def select_unique(keys: Sequence[int], order: Sequence[int]) -> List[int]:
    """Positions to keep so that every graph key occurs once: of the positions sharing a key, the one that comes first
    in `order` (a sequence of positions, best first; positions it does not name are not kept).  The result is in the
    input's order."""
    seen, keep = set(), []
    for i in order:
        if keys[i] not in seen:
            seen.add(keys[i])
            keep.append(i)
    return sorted(keep)


# (name, value): `max_chemical_tanimoto`, `max_pairwise_chemical_tanimoto` - the rule of `max_pairwise_tanimoto`
check_threshold = functools.partial(_args.check_real, low=0.0, high=1.0, open_low=True)
check_flag = _args.check_flag
