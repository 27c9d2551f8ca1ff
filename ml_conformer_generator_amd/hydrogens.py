"""Explicit hydrogens of molecular graphs with 3D heavy atoms, on the GPU ("Explicit hydrogens"): how
many hydrogens each heavy atom carries and where they sit, so that the molecules this package returns can be taken
all-atom into a docking programme, a force field, a QM single point or a viewer.

THE PACKAGE'S OWN, LABELLED DEFINITION: not RDKit's `AddHs` - no formal charges, no protonation states, no tautomer search
beyond the one-N rule below; no agreement with RDKit is claimed.  It reuses two definitions the package already has: the
pharmacophore perception's `nH` and ring list (`pharmacophore.py`) and the force field's centre rule (`geometry.py`).

Inputs per molecule: fp32 heavy-atom coordinates, atomic numbers, symmetric bond codes (0 none, 1, 2, 3, 4 aromatic),
n <= 64 atoms.
Count    per atom deg, v2 and nH = max(0, (2 v0(Z) - v2) // 2) exactly as `pharmacophore.py` defines them, with its v0
         table (B 3, C 4, N 3, O 2, F 1, Si 4, P 3, S 2, Cl 1, As 3, Se 2, Br 1, I 1); any other element gets 0.  One
         addition, the aromatic N-H that v2 cannot see: the aromatic rings of 5 members are walked in the list order of
         `mcg_pharm_perceive` (ascending member mask; the first 32 rings of a molecule are listed); if no member of the
         ring has yet received a hydrogen by this rule, its lowest-index member that is an aromatic N of degree 2 carrying
         the perception's donor bit gets nH = 1 (pyrrole, indole, ONE N of imidazole).
Parent   linear: a code-3 bond or at least two code-2 bonds; planar: a code-2 or code-4 bond; planar also: Z is 7 or 8 and
         a bonded neighbour has a code-2 or code-4 bond (amide, aniline, phenol, enol); tetrahedral otherwise.
Length   X-H = rcov(Z) + 0.31 A (the radii of csrc/mcg_elements.h = `config.ELEMENTS`).
Directions, with k heavy neighbours, u_m the unit vectors from the parent to them in ascending neighbour index, h = nH,
perp(a) = normalize(e - (a.e) a) for the coordinate axis e with the smallest |a.e| (ties: x, then y, then z), normalize(0)
= 0, and "degenerate" = a norm below 1e-3:
  tetrahedral  k = 3, h = 1:  -normalize(u1 + u2 + u3); degenerate: normalize((u2 - u1) x (u3 - u1)).
               k = 2, h <= 2: b = -normalize(u1 + u2), n = normalize(u1 x u2); either degenerate: b = perp(u1), n = u1 x b;
                              H_m = cos(54.7356 deg) b +- sin(54.7356 deg) n, +n first.
  planar       k = 2, h = 1:  -normalize(u1 + u2); degenerate: perp(u1).
  linear       k = 1, h = 1:  -u1.
  k = 1, tetrahedral (h <= 3) or planar (h <= 2) - a ROTOR: a = u1, j the neighbour, w the lowest-index neighbour of j
               other than the parent, p = x_w - x_j with its component along a removed (no w, or p degenerate: p =
               perp(a)), e1 = normalize(p), e2 = a x e1,
                 dir_m = cos(t) a + sin(t) (cos(phi_m) e1 + sin(phi_m) e2),
               t the H-X-j angle itself: 109.4712 deg (tetrahedral) or 120 deg (planar); phi_m = 180 deg + 120 deg m +
               delta (tetrahedral) or 180 deg + 180 deg m + delta (planar): at delta = 0 the first hydrogen is anti to w.
  k = 0 in a one-atom molecule: the first h of (1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1) over sqrt 3 (tetrahedral, h <= 4);
               of three directions at 120 deg in the xy-plane from +x (planar, h <= 3); of +x, -x (linear, h <= 2).
  any other (hybridisation, k, h) - an atom without a neighbour in a larger molecule among them: no hydrogen is placed and
               h joins the molecule's `unplaced` count.
Rotor scan   delta is chosen after every non-rotor ("fixed") hydrogen is placed, from 0, 30, ... 330 deg (tetrahedral) or
         0, 180 deg (planar): S(delta) = sum over the rotor's hydrogens of [sum over the heavy atoms other than the parent
         and j of max(0, 2.4 - d)^2 + sum over the fixed hydrogens of max(0, 2.0 - d)^2], in fp32 in one order (hydrogens
         ascending; heavy atoms ascending, then fixed hydrogens in output order).  The smallest S wins, ties go to the
         smallest delta: an unhindered rotor keeps the staggered / anti default.  Rotors do not see each other, so the
         result does not depend on any processing order.  A parent with k = 1 that places no hydrogen is no rotor.
Output   hydrogens in ascending order of the parent, then of m.  A molecule with a non-finite coordinate on a real atom gets
         no hydrogens and the count -1.  A molecule's result has the same bits whatever the batch, its row and the padded
         widths.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import _args, _lib
from . import pharmacophore as mcg_pharm
from .config import ELEMENTS

MAX_ATOMS = 64                  # include/mlconfgen_hip.h MCG_HYDROGENS_MAX_ATOMS
MAX_BATCH = 16384               # MCG_HYDROGENS_MAX_B
XH_MARGIN = 0.31                # angstrom: X-H = rcov(Z) + XH_MARGIN
VALENCE = {5: 3, 6: 4, 7: 3, 8: 2, 9: 1, 14: 4, 15: 3, 16: 2, 17: 1, 33: 3, 34: 2, 35: 1, 53: 1}      # pharmacophore.py's v0
REFUSAL_WITH_FINISHER = ("add_hydrogens cannot be combined with a finisher (RDKit's or a custom one): the hydrogens are "
                         "placed on the GeneratedMolecule records; on RDKit Mols use Chem.AddHs(mol, addCoords=True)")


def slots(width: int) -> int:
    """Hydrogen slots per row the kernel needs for rows of `width` atoms: an atom with a neighbour carries at most 3, a
    one-atom molecule at most 4."""
    return max(4, 3 * int(width))


def _graph_arguments(atomic_numbers, bond_orders, n_nodes):
    """(z, bonds, B, W) of the graph arguments, shapes and dtypes checked; of the counts only that there are B."""
    return _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS,
                                 f"hydrogens are added to molecules of at most {MAX_ATOMS} atoms", counts=False)


def _aromatic_rings(arom: List[List[int]], n: int) -> List[int]:
    """The member masks of the simple cycles of 5 or 6 atoms along `arom` (per atom its ring-eligible aromatic
    neighbours), ascending: the ring list of the pharmacophore perception."""
    found = set()
    for s in range(n):
        stack = [(s,)]
        while stack:
            path = stack.pop()
            last = path[-1]
            if len(path) in (5, 6) and s in arom[last]:
                found.add(sum(1 << a for a in path))
            if len(path) < 6:
                stack.extend(path + (j,) for j in arom[last] if j > s and j not in path)
    return sorted(found)


def implicit_counts(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor) -> torch.Tensor:
    """[B,W] int32 on the host: the hydrogens each heavy atom carries by the count rule of this module's docstring - nH
    from the bond codes, plus the one aromatic N-H per 5-ring - whether or not the placement has a direction for them
    (`add_hydrogens` reports `counts`, the placed ones, and `unplaced`, the rest).  No GPU: integer work in torch, and a
    ring search in Python for the molecules that have an aromatic N of degree 2.  Arguments as `add_hydrogens` takes them;
    the diagonal and everything at or beyond a molecule's atom count is ignored."""
    z, bonds, B, W = _graph_arguments(atomic_numbers, bond_orders, n_nodes)
    nn = torch.as_tensor(n_nodes).detach().cpu().reshape(B).to(torch.long).clamp(0, W)
    z = z[:, :W].detach().cpu().to(torch.long)
    c = bonds.detach().cpu().to(torch.long)
    real = torch.arange(W).view(1, W) < nn.view(B, 1)
    pair = real.unsqueeze(1) & real.unsqueeze(2) & ~torch.eye(W, dtype=torch.bool).unsqueeze(0)
    c = torch.where(pair & (c >= 1) & (c <= 4), c, torch.zeros_like(c))
    v2 = torch.tensor([0, 2, 4, 6, 3])[c].sum(dim=2)
    v0 = torch.zeros(max(VALENCE) + 2, dtype=torch.long)
    v0[list(VALENCE)] = torch.tensor(list(VALENCE.values()))
    nh = torch.div(2 * v0[z.clamp(0, v0.numel() - 1)] - v2, 2, rounding_mode="floor").clamp(min=0) * real
    deg, narom = (c != 0).sum(dim=2), (c == 4).sum(dim=2)
    ring_n = real & (z == 7) & (narom >= 1) & (deg == 2)
    for b in ring_n.any(dim=1).nonzero().reshape(-1).tolist():
        n = int(nn[b])
        zb, cb, degb, naromb = z[b].tolist(), c[b].tolist(), deg[b].tolist(), narom[b].tolist()
        ok = [2 <= naromb[a] <= 3 and degb[a] <= 4 for a in range(n)]
        arom = [[j for j in range(n) if cb[a][j] == 4 and ok[a] and ok[j]] for a in range(n)]
        rings = _aromatic_rings(arom, n)[: mcg_pharm.MAX_RINGS]
        five = [[a for a in range(n) if m >> a & 1] for m in rings if bin(m).count("1") == 5]
        # the perception's donor bit of an aromatic N of degree 2: a 5-ring without O, S, Se and without an aromatic N of degree 3
        donor_ring = [not any(zb[a] in (8, 16, 34) or (zb[a] == 7 and naromb[a] >= 1 and degb[a] == 3) for a in ring)
                      for ring in five]
        donors = {a for ring, good in zip(five, donor_ring) if good for a in ring if bool(ring_n[b, a])}
        given = set()
        for ring in five:
            cand = [a for a in ring if a in donors]
            if cand and not given.intersection(ring):
                given.add(cand[0])
        for a in given:
            nh[b, a] = 1
    return nh.to(torch.int32)


@torch.no_grad()
def add_hydrogens(coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor,
                  device=None, check: bool = True, return_rotors: bool = False, perceived=None) -> Dict[str, torch.Tensor]:
    """The explicit hydrogens of B molecules by this module's definition (NOT RDKit's AddHs): one
    `pharmacophore.perceive_features` launch (`perceived`: its result for the same graphs, when the caller already has
    it), then one `mcg_hydrogens_place` launch.  `coords` [B,N,3] fp32 heavy-atom
    coordinates, `atomic_numbers` [B, >= W], `bond_orders` [B,W,W] (symmetric codes 0 none / 1 / 2 / 3 / 4 aromatic),
    `n_nodes` [B] real atoms each, at most min(N, W); W <= 64.  Device tensors:
      coords [B,Hmax,3]   the hydrogens, in ascending order of their parent, then of m; Hmax is the batch's largest count,
                          rows are zero beyond their own
      parents [B,Hmax]    int32: each hydrogen's heavy atom, -1 beyond the row's count
      counts [B,W]        int32: the hydrogens placed on each heavy atom
      n_hydrogens [B]     int32: the row's count; -1 for a row with a non-finite coordinate on a real atom (no hydrogens)
      unplaced [B]        int32: hydrogens the count rule gives to atoms the definition has no direction for
      rotor_delta [B,W]   (`return_rotors=True`) int32: the torsion offset chosen for a rotor, degrees; -1: not a rotor
    More than 16384 molecules go through in launches of 16384 rows.
    ValueError before the kernels: shapes that do not fit, W > 64, and with `check=True` (device reductions, one
    host read each) a code outside 0..4, a matrix that is not symmetric, an atomic number < 1 or one without a covalent
    radius (`config.ELEMENTS`) on a real atom; atom counts outside [0, min(N, W)] always."""
    x = torch.as_tensor(coords)
    if x.dim() != 3 or x.shape[2] != 3 or not x.dtype.is_floating_point:
        raise ValueError(f"coords must be floating point [B,N,3], got {list(x.shape)} of type {x.dtype}")
    z, bonds, B, W = _graph_arguments(atomic_numbers, bond_orders, n_nodes)
    N = int(x.shape[1])
    if int(x.shape[0]) != B:
        raise ValueError(f"coords holds {int(x.shape[0])} molecules, bond_orders {B}")
    _args.check_n_nodes(n_nodes, B, min(N, W))
    dev = _args.resolve_device(device, x)
    launches = B > 0 and N > 0 and W > 0           # the kernel writes every element of the per-row and per-atom outputs
    fill = torch.empty if launches else torch.zeros
    out = {"coords": torch.zeros(B, 0, 3, dtype=torch.float32, device=dev),
           "parents": torch.zeros(B, 0, dtype=torch.int32, device=dev),
           "counts": fill(B, W, dtype=torch.int32, device=dev),
           "n_hydrogens": fill(B, dtype=torch.int32, device=dev),
           "unplaced": fill(B, dtype=torch.int32, device=dev)}
    if return_rotors:
        out["rotor_delta"] = torch.empty(B, W, dtype=torch.int32, device=dev) if launches else \
            torch.full((B, W), -1, dtype=torch.int32, device=dev)
    if not launches:
        return out
    xd = x.to(dev, torch.float32).contiguous()
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
    if check:
        _args.check_graphs(zd, bd, nn, W)
        _args.check_known_elements(zd, nn, W, "add_hydrogens", ELEMENTS)
    types, rings, count = perceived if perceived is not None else mcg_pharm.perceive_features(zd, bd, nn, dev)
    HW = slots(W)
    h_xyz = torch.empty(B, HW, 3, dtype=torch.float32, device=dev)
    parents = torch.empty(B, HW, dtype=torch.int32, device=dev)
    rotors = out.get("rotor_delta")
    for lo in range(0, B, MAX_BATCH):
        rows = slice(lo, min(lo + MAX_BATCH, B))
        _lib.check(_lib.lib().mcg_hydrogens_place(
            _lib.dptr(xd[rows]), _lib.dptr(zd[rows]), _lib.dptr(bd[rows]), _lib.dptr(nn[rows]), _lib.dptr(types[rows]),
            _lib.dptr(rings[rows]), _lib.dptr(count[rows]), rows.stop - lo, N, W, HW, _lib.dptr(h_xyz[rows]),
            _lib.dptr(parents[rows]), _lib.dptr(out["counts"][rows]), _lib.dptr(out["n_hydrogens"][rows]),
            _lib.dptr(out["unplaced"][rows]), None if rotors is None else _lib.dptr(rotors[rows]),
            _lib.current_stream_ptr(dev)), "mcg_hydrogens_place")
    h_max = max(int(out["n_hydrogens"].max()), 0)
    out["coords"], out["parents"] = h_xyz[:, :h_max].contiguous(), parents[:, :h_max].contiguous()
    return out
