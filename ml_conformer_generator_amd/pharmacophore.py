"""Pharmacophore features of molecular graphs and their overlap with a reference's, on the GPU (DESIGN.md section 6,
"Pharmacophore overlap"): does a posed molecule keep the reference's interaction pattern - a donor where the reference has
one, an acceptor, a charge, an aromatic ring?

THE PACKAGE'S OWN, LABELLED DEFINITION: not RDKit's feature factory and not any vendor's colour force field; no agreement
with either is claimed.

Perception reads the heavy-atom graph alone - atomic numbers z, symmetric bond codes (1 / 2 / 3 / 4 aromatic, anything
else no bond), n <= 64 atoms - and no coordinates, so it is exact integer work.  Per atom: deg (bonded atoms), v2 (twice
the bond-order sum: codes 1 2 3 4 add 2 4 6 3), narom (code-4 bonds; aromatic = narom >= 1), nH = max(0, (2 v0(Z) - v2)
// 2) with v0: B 3, C 4, N 3, O 2, F 1, Si 4, P 3, S 2, Cl 1, As 3, Se 2, Br 1, I 1; any other element carries no feature.
Aromatic rings: the simple cycles of 5 or 6 ring-eligible atoms (2 <= narom <= 3, deg <= 4) joined all round by code-4
  bonds; a ring is the 64-bit mask of its members (one ring per member set), the rings are listed in ascending order of
  the mask as an unsigned integer, at most MAX_RINGS = 32 are kept - a molecule with more reports its true count and gets
  NaN scores.  A Kekule ring (codes 1 and 2 alternating) has no ring feature: aromaticity is not perceived.
Types (per-atom bits; an atom may carry several):
  D donor (1):      a non-aromatic N or O with nH >= 1; or an aromatic N of degree 2 in an aromatic 5-ring without an O, S
                    or Se member and without an aromatic N of degree 3 (pyrrole, indole, both N of imidazole; not the N
                    of oxazole, thiazole, N-methylimidazole).
  A acceptor (2):   an O without an aromatic bond and with v2 <= 4; a non-aromatic N with a code-2 or code-3 bond and v2 <=
                    6; an aromatic N of degree 2 - unless it is a donor by the rule above and none of the rings that make
                    it one holds a second aromatic N of degree 2 (pyrrole: D alone; imidazole's two N, being tautomers:
                    D and A).
  P cation (4):     a non-aromatic N with deg >= 1 whose bonds are all code 1, with no aromatic neighbour and no
                    neighbour that has a code-2 bond to O or S (amines, amidine and guanidine N; not amides, sulfonamides,
                    anilines).
  N anion (8):      a C, S or P with a code-2 bond to an O of degree 1 and a code-1 bond to an O of degree 1 (carboxylic,
                    sulfonic, phosphoric acids); the feature sits on the central atom.
  H hydrophobe (16): a non-aromatic C all of whose neighbours are C (none counts); Cl, Br, I.
  R ring:           one feature per aromatic ring at the centroid of its members - an fp32 sum in ascending atom index,
                    then one fp32 division by the member count.
The feature set of a molecule at given coordinates: per atom in ascending index its types in ascending bit order, each at
the atom, then the ring centroids in list order.
Overlap  O(A, B) = sum over the six types t, i in A_t, j in B_t of exp(-KAPPA |a_i - b_j|^2), KAPPA = 0.5 / A^2 (a
unit-width Gaussian), all weights 1, no cut-off.
Score    T(R, M) = O(R,M) / (O(R,R) + O(M,M) - O(R,M)), in [0, 1] since the Gaussian kernel is positive definite.
Matches  the reference features that have a candidate feature of their type at d2 <= 2.25 (1.5 A), d2 = dx*dx + dy*dy +
         dz*dz in fp32 without contraction.
A candidate without features scores T = 0, matches = 0; one with a non-finite coordinate on a real atom scores NaN,
matches = -1, the other rows unaffected; a reference without features is refused on the host.
"""
from __future__ import annotations

import functools
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _args, _lib

TYPE_NAMES = ("donor", "acceptor", "cation", "anion", "hydrophobe", "ring")       # type index 0..5; atom bit 1 << index
RING_TYPE = 5
KAPPA = 0.5
MATCH_DISTANCE = 1.5
MAX_RINGS = 32                  # include/mlconfgen_hip.h MCG_PHARM_MAX_RINGS
MAX_FEATURES = 352              # MCG_PHARM_MAX_FEATURES: 64 atoms x 5 atom types + MAX_RINGS
MAX_ATOMS = 64                  # one lane and one mask bit per atom

Features = Tuple[torch.Tensor, torch.Tensor]      # (xyz [F,3] fp32, type index [F] uint8), host


# ----------------------------------------------------------------------------------------------- device
@torch.no_grad()
def perceive_features(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(types [B,W] uint8, ring masks [B,32] int64, ring counts [B] int32) on the device, of B molecular graphs:
    `atomic_numbers` [B, >= W], `bond_orders` [B,W,W] (symmetric codes 1 / 2 / 3 / 4 aromatic, anything else no bond),
    `n_nodes` [B]; the diagonal and everything at or beyond a molecule's atom count is ignored, whatever it holds.  One
    `mcg_pharm_perceive` launch (this module's docstring: the definition).  The int64 masks hold the unsigned bit
    patterns (bit k = atom k), ascending as unsigned integers, zero beyond the count; a count above `MAX_RINGS` is the
    true count, with the first `MAX_RINGS` masks.  Exact: the same bits whatever the batch, the row and the padded width.
    ValueError before the kernel: W > 64, shapes that do not fit, atom counts outside [0, W]."""
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS,
                                           f"pharmacophore features take molecules of at most {MAX_ATOMS} atoms")
    dev = _args.resolve_device(device, bonds)
    if W == 0:                                  # no atoms anywhere: B empty graphs at the kernel's smallest width
        z, bonds, W = torch.zeros(B, 1, dtype=torch.int32), torch.zeros(B, 1, 1, dtype=torch.int8), 1
    types = torch.zeros(B, W, dtype=torch.uint8, device=dev)
    rings = torch.zeros(B, MAX_RINGS, dtype=torch.int64, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    if B == 0:
        return types, rings, count
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
    _lib.check(_lib.lib().mcg_pharm_perceive(_lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nn), B, W, _lib.dptr(types),
                                             _lib.dptr(count), _lib.dptr(rings), _lib.current_stream_ptr(dev)),
               "mcg_pharm_perceive")
    return types, rings, count


@torch.no_grad()
def reference_self_overlap(reference_features: Features, device=None) -> torch.Tensor:
    """O(R,R) [1] fp64 on the device: the reference's feature list run through `mcg_pharm_score` as a one-row batch against
    itself - the kernel and the summation order of every other overlap."""
    xyz, typ = reference_features
    dev = _args.resolve_device(device)
    out = _score_launch(None, None, None, None, None, 1, 1, 1, xyz.to(dev), typ.to(dev), None, dev, False)
    return out["o_mm"]


def _score_launch(coords, nn, types, rings, count, B, N, W, ref_xyz, ref_type, o_rr, dev, per_type: bool) -> dict:
    out = dict(o_rm=torch.empty(B, dtype=torch.float64, device=dev), o_mm=torch.empty(B, dtype=torch.float64, device=dev),
               tanimoto=torch.empty(B, dtype=torch.float32, device=dev),
               matches=torch.empty(B, dtype=torch.int32, device=dev))
    if per_type:
        out["per_type"] = torch.empty(B, 6, dtype=torch.float64, device=dev)
    if B == 0:
        return out
    ref_xyz, ref_type = ref_xyz.to(torch.float32).contiguous(), ref_type.to(torch.uint8).contiguous()
    _lib.check(_lib.lib().mcg_pharm_score(_lib.dptr(coords), _lib.dptr(nn), _lib.dptr(types), _lib.dptr(rings),
                                          _lib.dptr(count), B, N, W, _lib.dptr(ref_xyz), _lib.dptr(ref_type),
                                          int(ref_type.numel()), _lib.dptr(o_rr), _lib.dptr(out["o_rm"]),
                                          _lib.dptr(out["o_mm"]), _lib.dptr(out["tanimoto"]), _lib.dptr(out["matches"]),
                                          _lib.dptr(out.get("per_type")), _lib.current_stream_ptr(dev)),
               "mcg_pharm_score")
    return out


@torch.no_grad()
def score_features(reference_features: Features, coords: torch.Tensor, n_nodes: torch.Tensor, types: torch.Tensor,
                   ring_mask: torch.Tensor, n_rings: torch.Tensor, device=None, per_type: bool = False) -> dict:
    """The overlap of B posed molecules' features with the reference's: dict of `o_rm`, `o_mm` [B] fp64, `tanimoto` [B]
    fp32, `matches` [B] int32 and - `per_type=True` - `per_type` [B,6] fp64 (the six parts of `o_rm`), on the device.
    `coords` [B,N,3] fp32 in the reference's coordinates; `types` [B,W], `ring_mask` [B,32], `n_rings` [B] as
    `perceive_features` returns them.  Two launches of `mcg_pharm_score`: the reference against itself (O(R,R)), then the
    rows.  A row with a non-finite coordinate on a real atom or more than `MAX_RINGS` rings: NaN, matches -1.  Every
    output has the same bits whatever the batch, the row and the widths N and W."""
    xyz, typ = load_reference_features(reference_features)
    c = torch.as_tensor(coords)
    t = torch.as_tensor(types)
    if c.dim() != 3 or c.shape[2] != 3 or not 1 <= c.shape[1] <= MAX_ATOMS:
        raise ValueError(f"coords must be [B, 1..{MAX_ATOMS}, 3], got {list(c.shape)}")
    B, N = int(c.shape[0]), int(c.shape[1])
    if t.dim() != 2 or t.shape[0] != B or not 1 <= t.shape[1] <= MAX_ATOMS or t.dtype != torch.uint8:
        raise ValueError(f"types must be [B, 1..{MAX_ATOMS}] uint8 with B = {B}, got {list(t.shape)} of type {t.dtype}")
    W = int(t.shape[1])
    r = torch.as_tensor(ring_mask)
    k = torch.as_tensor(n_rings)
    if tuple(r.shape) != (B, MAX_RINGS) or r.dtype != torch.int64 or k.numel() != B:
        raise ValueError(f"ring_mask must be [B, {MAX_RINGS}] int64 and n_rings [B], got {list(r.shape)} of type "
                         f"{r.dtype} and {list(k.shape)}")
    _args.check_n_nodes(n_nodes, B, min(N, W))
    dev = _args.resolve_device(device, c)
    xyz, typ = xyz.to(dev), typ.to(dev)
    o_rr = reference_self_overlap((xyz, typ), dev)
    return _score_launch(c.to(dev, torch.float32).contiguous(),
                         torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous(), t.to(dev).contiguous(),
                         r.to(dev).contiguous(), k.to(dev, torch.int32).reshape(B).contiguous(), B, N, W, xyz, typ, o_rr,
                         dev, per_type)


@torch.no_grad()
def pharmacophore_tanimoto(reference_features, coords: torch.Tensor, atomic_numbers: torch.Tensor,
                           bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(tanimoto [B] fp32, matches [B] int32) on the device of B posed molecules against the reference's features
    (`load_reference_features`): one `perceive_features` launch, then `score_features`.  `coords` [B,N,3] in the
    reference's coordinates, the graphs as in `perceive_features`."""
    types, rings, count = perceive_features(atomic_numbers, bond_orders, n_nodes, device)
    out = score_features(reference_features, coords, n_nodes, types, rings, count, types.device)
    return out["tanimoto"], out["matches"]


# ----------------------------------------------------------------------------------------------- host
def feature_points(coords: torch.Tensor, types: torch.Tensor, ring_mask: torch.Tensor, n_rings: torch.Tensor
                   ) -> List[List[Tuple[str, Tuple[float, float, float]]]]:
    """Per molecule the host-side list of (type name, (x, y, z)) in the order of the definition: per atom in ascending
    index its types in ascending bit order, then the kept rings at their fp32 centroids.  `coords` [B,N,3], the rest as
    `perceive_features` returns it.  For the reference, and for inspection."""
    c = torch.as_tensor(coords).detach().cpu().to(torch.float32)
    t = torch.as_tensor(types).cpu().tolist()
    masks = torch.as_tensor(ring_mask).cpu().tolist()
    counts = torch.as_tensor(n_rings).cpu().reshape(-1).tolist()
    out = []
    for b in range(c.shape[0]):
        feats = []
        for a, bits in enumerate(t[b][: c.shape[1]]):
            for k in range(RING_TYPE):
                if bits >> k & 1:
                    feats.append((TYPE_NAMES[k], tuple(c[b, a].tolist())))
        for m in masks[b][: min(max(counts[b], 0), MAX_RINGS)]:
            members = [k for k in range(min(MAX_ATOMS, c.shape[1])) if (m & 0xFFFFFFFFFFFFFFFF) >> k & 1]
            if members:
                acc = torch.zeros(3)
                for k in members:
                    acc = acc + c[b, k]
                feats.append((TYPE_NAMES[RING_TYPE], tuple((acc / torch.tensor(float(len(members)))).tolist())))
        out.append(feats)
    return out


def load_reference_features(obj) -> Features:
    """A reference's feature points as (xyz [F,3] fp32, type index [F] uint8) on the host, from a sequence of (type,
    (x, y, z)) - type names "donor", "acceptor", "cation", "anion", "hydrophobe", "ring" - or from an earlier result of
    this function.  ValueError: an unknown type name, a point that is not three finite numbers, an empty list, more than
    `MAX_FEATURES` features."""
    if isinstance(obj, tuple) and len(obj) == 2 and torch.is_tensor(obj[0]) and torch.is_tensor(obj[1]):
        xyz, typ = obj[0].detach().cpu().to(torch.float32).reshape(-1, 3), obj[1].detach().cpu().to(torch.uint8).reshape(-1)
        if xyz.shape[0] != typ.shape[0] or (typ.numel() and int(typ.max()) > RING_TYPE):
            raise ValueError("reference features: xyz [F,3] and type indices [F] in 0..5 are needed")
    else:
        try:
            items = list(obj)
        except TypeError:
            raise ValueError(f"reference features are a sequence of (type, (x, y, z)), got {type(obj).__name__}") from None
        names, points = [], []
        for k, item in enumerate(items):
            try:
                name, point = item
                point = [float(v) for v in point]
            except (TypeError, ValueError):
                raise ValueError(f"reference feature {k} is not a (type, (x, y, z)) pair: {item!r}") from None
            if name not in TYPE_NAMES:
                raise ValueError(f"reference feature {k}: unknown type {name!r}; the types are {', '.join(TYPE_NAMES)}")
            if len(point) != 3:
                raise ValueError(f"reference feature {k}: a point is three numbers, got {len(point)}")
            names.append(TYPE_NAMES.index(name))
            points.append(point)
        xyz = torch.tensor(points, dtype=torch.float32).reshape(-1, 3)
        typ = torch.tensor(names, dtype=torch.uint8)
    if typ.numel() == 0:
        raise ValueError("the reference has no pharmacophore features: nothing to score against")
    if typ.numel() > MAX_FEATURES:
        raise ValueError(f"a reference has at most {MAX_FEATURES} features, got {typ.numel()}")
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError("reference feature points must be finite")
    return xyz.contiguous(), typ.contiguous()


def select_score(shape: Optional[float], pharmacophore: Optional[float]) -> Optional[float]:
    """The ranking value of `rank_by="combo"`: shape Tanimoto + pharmacophore Tanimoto; NaN where either is NaN or
    missing (such a molecule ranks last)."""
    if shape is None or pharmacophore is None:
        return math.nan
    return shape + pharmacophore


check_threshold = functools.partial(_args.check_real, low=0.0, high=1.0)      # (name, value): `min_pharmacophore_tanimoto`
check_flag = _args.check_flag
check_rank_by = _args.check_rank_by
