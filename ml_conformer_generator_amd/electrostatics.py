"""Partial charges of molecular graphs and the electrostatic similarity of posed molecules to a reference, on the GPU
("Electrostatic similarity"): does a posed molecule present the reference's charge distribution - the
third check of ligand-based screening beside shape (`cheminformatics`) and colour (`pharmacophore.py`).

THE PACKAGE'S OWN, LABELLED DEFINITION: not RDKit's `ComputeGasteigerCharges` and not any vendor's electrostatic score; no
agreement with either is claimed.  No formal charges, no protonation states: a carboxylic acid is neutral, an amine is
neutral.  It reuses two definitions the package already has: the hydrogen count and the parent class of `hydrogens.py`.

Charges  read the heavy-atom graph alone - atomic numbers, symmetric bond codes (1 / 2 / 3 / 4 aromatic, anything else no
         bond), n <= 64 atoms - and no coordinates.
  Counts     per heavy atom nH is exactly `hydrogens.implicit_counts` (the pharmacophore perception's count plus the one
             aromatic N-H per 5-ring) and the class linear / planar / tetrahedral exactly the "Parent" rule of `hydrogens.py`.
  Parameters chi(q) = a + b q + c q^2 with (a, b, c), the Gasteiger-Marsili values as the literature gives them:
               H   7.17, 6.24, -0.56
               C   tetrahedral 7.98, 9.18, 1.88;  planar 8.79, 9.32, 1.51;  linear 10.39, 9.45, 0.73
               N   tetrahedral 11.54, 10.82, 1.36;  planar 12.87, 11.15, 0.85;  linear 15.68, 11.70, -0.27
               O   tetrahedral 14.18, 12.92, 1.39;  planar and linear 17.07, 13.79, 0.47
               F   14.66, 13.85, 2.31     Cl  11.00, 9.69, 1.35     Br  10.08, 8.47, 1.16     P  8.90, 8.24, 0.96
               S   tetrahedral 10.14, 9.13, 1.38;  planar and linear 10.88, 9.49, 1.33;  with two or more code-2 bonds
                   to O, whatever its class, 12.00, 10.81, 1.20
             chi+ = a + b + c, and 20.02 for H.  The table is the package's own; the tests pin it only to itself.  A
             molecule with a real atom of any other element (B, Si, As, Se, I, any Z without a row) is not charged: NaN in
             every charge of the row and status 1, the other rows unaffected.
  Iteration  all charges start at 0; steps k = 1..6 with damping 0.5^k, Jacobi style: every chi is taken from the charges
             of step k - 1.  Every bond code 1..4 counts once per pair, whatever its order.  For a bond i-j, f_ij = (chi_j -
             chi_i) / (chi+_i if chi_j > chi_i, else chi+_j).  Each atom adds, in fp32 and in ascending neighbour index, the
             f_ij of its neighbours, then nH * f_iH for its hydrogens, which share one charge q_H,i that moves by -f_iH; all
             updates are multiplied by 0.5^k: q_i += 0.5^k (sum), q_H,i -= 0.5^k f_iH.
  Outputs    q [B,W] the heavy atoms, q_h [B,W] the charge of EACH hydrogen of that atom (0 where nH = 0), nh [B,W] int32,
             status [B]; 0 at and beyond a row's atoms.  A row has the same bits whatever the batch, its row and the padded
             width.  Checked on the CPU: methane C -0.0776, H +0.0194; water O -0.4105, H +0.2052; ethanol O -0.3953,
             hydroxyl H +0.2094; every molecule's charges sum to 0.
Points   a molecule's charge points are its heavy atoms, in order, with q; then its placed hydrogens in `add_hydrogens`'
         output order, each with its parent's q_h.  A hydrogen that the count rule gives but the placement has no direction
         for adds its charge to its parent's point (the total stays 0).  At most 256 points: 64 heavy + 192 hydrogens.
Overlap  E(A,B) = sum_i sum_j qa_i qb_j K(|a_i - b_j|), the Coulomb energy between unit-normalised Gaussian charges of width
         0.5 A: K(r) = erf(MU r) / r with MU = 1.0 / A; for r < 1e-3, K(r) = MU (2 / sqrt pi) (1 - (MU r)^2 / 3); r^2 = dx dx
         + dy dy + dz dz in fp32 without contraction.  MU = 1.0 is a decision, not a measurement: at 0.5 / A the self-overlap
         of neutral molecules cancels to under 1 % of the sum of its terms' magnitudes (measured on the `hydrogens_cases`
         fixtures), at 1.0 it is 3-34 %.  The kernel is positive definite.
Score    T(R,M) = E(R,M) / (E(R,R) + E(M,M) - E(R,M)), in [-1/3, 1]; 0 where the denominator is below 1e-12 (nothing is
         charged).  E(M,M) is the full double sum, i = j included.  Each term is computed in fp32 (`erff`); thread t owns
         candidate point t, adds its terms in fp64 in ascending index of the other side, and the threads' sums are added in
         fp64 by one binary tree over t; the three sums are rounded to fp32 once and T is computed from them in fp32.  E(R,R)
         comes from the same kernel with the reference as its own candidate row, so T(A,A) is 1 to the last bit or two.  A
         candidate with a non-finite coordinate on a real point, or with status 1, scores NaN, the other rows unaffected; a
         reference with no point, with status 1 or with E(R,R) < 1e-12 is refused on the host.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Tuple

import torch

from . import _args, _lib
from . import pharmacophore as mcg_pharm

MAX_ATOMS = 64                  # include/mlconfgen_hip.h MCG_CHARGES_MAX_ATOMS
MAX_BATCH = 16384               # MCG_CHARGES_MAX_B and MCG_ESP_MAX_B
MAX_POINTS = 256                # MCG_ESP_MAX_POINTS: 64 heavy atoms + 3 x 64 hydrogens
MU = 1.0                        # 1 / angstrom
EMPTY = 1e-12                   # a Tanimoto denominator, or a reference's self-overlap, below this: nothing is charged
REFUSAL_WITH_FINISHER = ("electrostatic_scores and partial_charges cannot be combined with a finisher (RDKit's or a custom "
                         "one): they read the placed hydrogens of the GeneratedMolecule records")

ChargePoints = Tuple[torch.Tensor, torch.Tensor]  # (xyz [P,3] fp32, charge [P] fp32), host


# ----------------------------------------------------------------------------------------------- device
@torch.no_grad()
def partial_charges(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, device=None,
                    check: bool = True, perceived=None) -> Dict[str, torch.Tensor]:
    """The partial charges of B molecular graphs by this module's definition (NOT RDKit's Gasteiger charges): one
    `pharmacophore.perceive_features` launch (`perceived`: its result for the same graphs, when the caller has it), then
    one `mcg_charges_peoe` launch.  `atomic_numbers` [B, >= W], `bond_orders` [B,W,W] (symmetric codes 0 none / 1 / 2 / 3 /
    4 aromatic), `n_nodes` [B]; W <= 64.  Device tensors:
      q [B,W]      fp32: the heavy atoms' charges
      q_h [B,W]    fp32: the charge of EACH hydrogen of that atom, 0 where it has none
      nh [B,W]     int32: its hydrogens (`hydrogens.implicit_counts`)
      status [B]   int32: 1 for a row with a real atom of an element without parameters - NaN in its q and q_h
      n_nodes [B]  int32: the atom counts as given (what `charge_points` reads)
    the per-atom ones 0 at and beyond a row's atoms.  More than 16384 molecules go through in launches of 16384 rows.
    ValueError before the kernels: shapes that do not fit, W > 64, atom counts outside [0, W], and with `check=True` (one
    device reduction, one host read) a code outside 0..4, a matrix that is not symmetric, an atomic number < 1 on a real
    atom."""
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS,
                                           f"partial charges take molecules of at most {MAX_ATOMS} atoms")
    dev = _args.resolve_device(device, bonds)
    launches = B > 0 and W > 0                      # the kernel writes every element of every output
    fill = torch.empty if launches else torch.zeros
    out = {"q": fill(B, W, dtype=torch.float32, device=dev), "q_h": fill(B, W, dtype=torch.float32, device=dev),
           "nh": fill(B, W, dtype=torch.int32, device=dev), "status": fill(B, dtype=torch.int32, device=dev),
           "n_nodes": torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous()}
    if not launches:
        return out
    zd = z[:, :W].to(dev, torch.int32).contiguous()
    bd = bonds.to(dev, torch.int8).contiguous()
    nn = out["n_nodes"]
    if check:
        _args.check_graphs(zd, bd, nn, W)
    types, rings, count = perceived if perceived is not None else mcg_pharm.perceive_features(zd, bd, nn, dev)
    for lo in range(0, B, MAX_BATCH):
        rows = slice(lo, min(lo + MAX_BATCH, B))
        _lib.check(_lib.lib().mcg_charges_peoe(
            _lib.dptr(zd[rows]), _lib.dptr(bd[rows]), _lib.dptr(nn[rows]), _lib.dptr(types[rows]), _lib.dptr(rings[rows]),
            _lib.dptr(count[rows]), rows.stop - lo, W, _lib.dptr(out["q"][rows]), _lib.dptr(out["q_h"][rows]),
            _lib.dptr(out["nh"][rows]), _lib.dptr(out["status"][rows]), _lib.current_stream_ptr(dev)), "mcg_charges_peoe")
    return out


@torch.no_grad()
def charge_points(coords: torch.Tensor, charges: Dict[str, torch.Tensor], hydrogens: Dict[str, torch.Tensor]
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(points [B,PW,3] fp32, charge [B,PW] fp32, n_points [B] int32), on the device of `coords`: per molecule its heavy
    atoms in order with `q`, then its placed hydrogens in `add_hydrogens`' output order, each with its parent's `q_h`; a
    hydrogen the count rule gives but the placement has no direction for adds its charge to its parent's point; zero
    beyond a row's points.  `coords` [B,N,3] the heavy atoms `hydrogens` was placed on, `charges` a `partial_charges`
    result (its `n_nodes` says how many atoms a row has), `hydrogens` an `add_hydrogens` result for the same graphs.  PW is
    the batch's largest count, at least 1.  Plain torch: gathers, one fp32 product and sum per heavy atom."""
    x = torch.as_tensor(coords)
    dev = x.device
    x = x.to(torch.float32)
    q, qh, nh = (charges[k].to(dev) for k in ("q", "q_h", "nh"))
    B, W = int(q.shape[0]), int(q.shape[1])
    if x.dim() != 3 or x.shape[0] != B or x.shape[2] != 3:
        raise ValueError(f"coords must be [B,N,3] with B = {B}, got {list(x.shape)}")
    n = charges["n_nodes"].to(dev, torch.long).reshape(B)
    placed = hydrogens["counts"].to(dev)
    h = hydrogens["n_hydrogens"].to(dev, torch.long).clamp(min=0)
    hx, parents = hydrogens["coords"].to(dev, torch.float32), hydrogens["parents"].to(dev, torch.long)
    if B and int(n.max()) > min(W, int(x.shape[1])):
        raise ValueError(f"n_nodes must lie in [0, {min(W, int(x.shape[1]))}], got up to {int(n.max())}")
    total = n + h
    PW = max(int(total.max()) if B else 0, 1)
    if PW > MAX_POINTS:
        raise ValueError(f"a molecule has at most {MAX_POINTS} charge points, got {PW}")
    p = torch.arange(PW, device=dev).view(1, PW)
    heavy, hyd = p < n.view(B, 1), (p >= n.view(B, 1)) & (p < total.view(B, 1))
    folded = torch.where(nh > placed, q + (nh - placed).to(torch.float32) * qh, q)       # the unplaced ones, on their parent
    a_idx = p.clamp(max=max(W - 1, 0)).expand(B, PW)
    x_idx = p.clamp(max=max(int(x.shape[1]) - 1, 0)).expand(B, PW)
    points = torch.zeros(B, PW, 3, dtype=torch.float32, device=dev)
    charge = torch.zeros(B, PW, dtype=torch.float32, device=dev)
    if W and x.shape[1]:
        points = torch.where(heavy.unsqueeze(2), x.gather(1, x_idx.unsqueeze(2).expand(B, PW, 3)), points)
        charge = torch.where(heavy, folded.gather(1, a_idx), charge)
    if hx.shape[1]:
        h_idx = (p - n.view(B, 1)).clamp(0, int(hx.shape[1]) - 1)
        par = parents.gather(1, h_idx).clamp(0, max(W - 1, 0))
        points = torch.where(hyd.unsqueeze(2), hx.gather(1, h_idx.unsqueeze(2).expand(B, PW, 3)), points)
        charge = torch.where(hyd, qh.gather(1, par), charge)
    return points.contiguous(), charge.contiguous(), total.to(torch.int32)


def _overlap_launch(ref_xyz, ref_q, xyz, q, n_points, e_rr, dev) -> Dict[str, torch.Tensor]:
    B, PW = int(xyz.shape[0]), int(xyz.shape[1])
    out = {k: torch.empty(B, dtype=torch.float32, device=dev) for k in ("cross", "self", "tanimoto")}
    for lo in range(0, B, MAX_BATCH):
        rows = slice(lo, min(lo + MAX_BATCH, B))
        _lib.check(_lib.lib().mcg_esp_overlap(
            _lib.dptr(ref_xyz), _lib.dptr(ref_q), int(ref_q.numel()), _lib.dptr(xyz[rows]), _lib.dptr(q[rows]),
            _lib.dptr(n_points[rows]), rows.stop - lo, PW, MU, _lib.dptr(e_rr), _lib.dptr(out["cross"][rows]),
            _lib.dptr(out["self"][rows]), _lib.dptr(out["tanimoto"][rows]), _lib.current_stream_ptr(dev)),
            "mcg_esp_overlap")
    return out


@torch.no_grad()
def reference_self_overlap(reference_points, device=None) -> torch.Tensor:
    """E(R,R) [1] fp32 on the device: the reference's points run through `mcg_esp_overlap` as a one-row batch against
    themselves - the kernel and the summation order of every other overlap."""
    xyz, q = load_reference_charges(reference_points)
    dev = _args.resolve_device(device)
    xyz, q = xyz.to(dev), q.to(dev)
    count = torch.tensor([int(q.numel())], dtype=torch.int32, device=dev)
    return _overlap_launch(xyz, q, xyz.unsqueeze(0), q.unsqueeze(0), count, None, dev)["self"]


@torch.no_grad()
def electrostatic_tanimoto(reference_points, points: torch.Tensor, charges: torch.Tensor, n_points: torch.Tensor,
                           device=None) -> Dict[str, torch.Tensor]:
    """The electrostatic similarity of B posed molecules' charge points to the reference's: dict of `cross` = E(R,M), `self`
    = E(M,M) and `tanimoto`, [B] fp32 on the device.  `reference_points`: what `load_reference_charges` takes; `points`
    [B,PW,3] fp32 in the reference's coordinates, `charges` [B,PW], `n_points` [B] as `charge_points` returns them, PW <=
    256.  Two launches of `mcg_esp_overlap`: the reference against itself (E(R,R)), then the rows.  A row with a non-finite
    coordinate or charge on a real point: NaN.  Every output has the same bits whatever the batch, the row and PW.
    ValueError before the rows' launch: shapes that do not fit, PW > 256, point counts outside [0, PW], a reference
    `load_reference_charges` refuses or whose E(R,R) is below 1e-12 (one host read)."""
    xyz, q = load_reference_charges(reference_points)
    x, c = torch.as_tensor(points), torch.as_tensor(charges)
    if x.dim() != 3 or x.shape[2] != 3 or not x.dtype.is_floating_point:
        raise ValueError(f"points must be floating point [B,PW,3], got {list(x.shape)} of type {x.dtype}")
    B, PW = int(x.shape[0]), int(x.shape[1])
    if PW > MAX_POINTS:
        raise ValueError(f"electrostatic scores take molecules of at most {MAX_POINTS} charge points, got a width of {PW}")
    if tuple(c.shape) != (B, PW) or not c.dtype.is_floating_point:
        raise ValueError(f"charges must be floating point [B,PW] = [{B}, {PW}], got {list(c.shape)} of type {c.dtype}")
    _args.check_n_nodes(n_points, B, PW)
    dev = _args.resolve_device(device, x)
    xyz, q = xyz.to(dev), q.to(dev)
    e_rr = reference_self_overlap((xyz, q), dev)
    if not float(e_rr[0]) >= EMPTY:
        raise ValueError(f"the reference's electrostatic self-overlap is {float(e_rr[0]):.3e}, below {EMPTY:g}: it carries "
                         "no charge to score against")
    if B == 0 or PW == 0:
        nothing = torch.zeros(B, dtype=torch.float32, device=dev)
        return dict(cross=nothing, self=nothing.clone(), tanimoto=nothing.clone())
    return _overlap_launch(xyz, q, x.to(dev, torch.float32).contiguous(), c.to(dev, torch.float32).contiguous(),
                           torch.as_tensor(n_points).to(dev, torch.int32).reshape(B).contiguous(), e_rr, dev)


# ----------------------------------------------------------------------------------------------- host
def load_reference_charges(obj) -> ChargePoints:
    """A reference's charge points as (xyz [P,3] fp32, charge [P] fp32) on the host, from a sequence of (charge, (x, y,
    z)) in the reference's coordinates, or from an earlier result of this function.  ValueError: an item that is not such a
    pair, a value that is not finite, an empty list, more than `MAX_POINTS` points."""
    if isinstance(obj, tuple) and len(obj) == 2 and torch.is_tensor(obj[0]) and torch.is_tensor(obj[1]):
        xyz, q = obj[0].detach().cpu().to(torch.float32).reshape(-1, 3), obj[1].detach().cpu().to(torch.float32).reshape(-1)
        if xyz.shape[0] != q.shape[0]:
            raise ValueError("reference charges: xyz [P,3] and charges [P] are needed")
    else:
        try:
            items = list(obj)
        except TypeError:
            raise ValueError(f"reference charges are a sequence of (charge, (x, y, z)), got {type(obj).__name__}") from None
        values, pts = [], []
        for k, item in enumerate(items):
            try:
                value, point = item
                if isinstance(value, (bool, str)):
                    raise TypeError
                value, point = float(value), [float(v) for v in point]
            except (TypeError, ValueError):
                raise ValueError(f"reference charge {k} is not a (charge, (x, y, z)) pair: {item!r}") from None
            if len(point) != 3:
                raise ValueError(f"reference charge {k}: a point is three numbers, got {len(point)}")
            values.append(value)
            pts.append(point)
        xyz = torch.tensor(pts, dtype=torch.float32).reshape(-1, 3)
        q = torch.tensor(values, dtype=torch.float32)
    if q.numel() == 0:
        raise ValueError("the reference has no charge points: nothing to score against")
    if q.numel() > MAX_POINTS:
        raise ValueError(f"a reference has at most {MAX_POINTS} charge points, got {q.numel()}")
    if not bool(torch.isfinite(xyz).all()) or not bool(torch.isfinite(q).all()):
        raise ValueError("reference charge points must be finite")
    return xyz.contiguous(), q.contiguous()


def select_score(shape: Optional[float], electrostatic: Optional[float]) -> Optional[float]:
    """The ranking value of `rank_by="electrostatic"`: shape Tanimoto + electrostatic Tanimoto; NaN where either is NaN or
    missing (such a molecule ranks last)."""
    if shape is None or electrostatic is None:
        return math.nan
    return shape + electrostatic


check_threshold = functools.partial(_args.check_real, low=-1.0, high=1.0)     # (name, value): `min_electrostatic_tanimoto`
check_rank_by = _args.check_rank_by
