"""Relaxed geometry: the heavy atoms of molecules moved downhill on a small restrained valence force field, on the GPU
("Relaxed geometry").

A LABELLED SUBSTITUTE: the reference cleans generated geometries with RDKit's MMFF94 under a position restraint on every
atom (`standardize_mol`, utils/standardizer.py:72-74).  This module keeps that restraint and replaces the force field by
the package's OWN - it is NOT MMFF94 and claims no parity with it.  Heavy atoms only.

Definition, per molecule (coordinates x, start coordinates x0, atomic numbers, symmetric bond codes 0 none / 1 / 2 / 3 /
4 aromatic; radii `rcov` of `config.ELEMENTS` = csrc/mcg_elements.h):
  E = sum over unordered pairs i < j of 1/2 k_ij (r_ij - d0_ij)^2  +  sum over atoms of the restraint.
  Every pair has exactly one class:
    bond (code o != 0):   k = 600, d0 = rcov_i + rcov_j - s(o), s(1) = 0, s(4) = 0.13, s(2) = 0.18, s(3) = 0.32;
    angle (not bonded, at least one common bonded neighbour j):  k = 150, d0 from the law of cosines on the two bond d0's
      at theta0(j) = 180 deg if j has a triple bond or at least two double bonds, else 120 deg if j has a double or an
      aromatic bond, else 109.47 deg; ring corrections override it: 90 deg if i and k have at least two common neighbours
      (a four-ring), else min(theta0, 108 deg) if a path i - a - b - k exists that avoids j (a five-ring); of several
      centres j the smallest d0 counts;
    non-bonded (every other pair):  one-sided, only where r < d0; k = 100, d0 = rcov_i + rcov_j + 0.9 A.
  Restraint per atom: 1/2 800 max(0, |x_i - x0_i| - 0.2)^2 - the reference's `MMFFAddPositionConstraint(idx, 0.2, 800.0)`.
  Deliberately out: torsions, impropers / planarity, charges, hydrogens, aromaticity perception.
Minimiser: `steps` trial steps x' = x - (s / max_i |g_i|) g from s = 0.02 A; accepted only if E(x') < E(x) (then s *= 1.2,
else s *= 0.5); it stops early only where max_i |g_i| == 0.  Deterministic: a molecule's result has the same bits whatever
the batch, its row and the padded widths.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _args, _lib
from .config import ELEMENTS

MAX_RELAX_ATOMS = 64            # include/mlconfgen_hip.h MCG_RELAX_MAX_ATOMS (= fingerprint.MAX_GRAPH_ATOMS)
MAX_RELAX_STEPS = 4096          # MCG_RELAX_MAX_STEPS
DEFAULT_STEPS = 200             # what `relax_geometry=True` stands for


def check_steps(value) -> int:
    """The `relax_geometry` option as a step budget: False -> 0 (off), True -> 200, an integer in 1..4096 -> itself (an
    integer type, not a bool); anything else is a ValueError."""
    return _args.check_steps("relax_geometry", value, 1, MAX_RELAX_STEPS, if_true=DEFAULT_STEPS, if_false=0)


def _check_molecules(z: torch.Tensor, bonds: torch.Tensor, nn: torch.Tensor, W: int) -> None:
    """The `check=True` half of `relax_geometry`: `_args.check_graphs`, and a covalent radius for every real atom."""
    _args.check_graphs(z, bonds, nn, W)
    _args.check_known_elements(z, nn, W, "relax_geometry", ELEMENTS)


@torch.no_grad()
def relax_geometry(coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor,
                   steps: int = DEFAULT_STEPS, device=None, return_gradient: bool = False,
                   restraint_coords: Optional[torch.Tensor] = None, check: bool = True) -> Dict[str, torch.Tensor]:
    """B molecules relaxed on the package's own restrained force field (this module's docstring: NOT MMFF94), one
    `mcg_geometry_relax` launch.  `coords` [B,N,3] fp32, `atomic_numbers` [B, >= W], `bond_orders` [B,W,W] (symmetric
    codes 0 none / 1 / 2 / 3 / 4 aromatic), `n_nodes` [B] real atoms each, at most min(N, W); W <= 64.  Device tensors:
      coords [B,N,3]        the relaxed coordinates (padded atoms zero; `steps=0`: the input's real atoms bit for bit)
      energy_before [B]     E at `coords`
      energy_after [B]      E at the returned coordinates, <= energy_before
      accepted_steps [B]    int32: the accepted ones of the `steps` trial steps
      max_displacement [B]  the largest distance of an atom from where it started, A
      gradient [B,N,3]      (`return_gradient=True`) dE/dx at the START coordinates
    `restraint_coords` [B,N,3] (default: `coords`): the positions the restraint holds the atoms to - a relaxation
    continued from coordinates that already moved stays restrained to the original ones.
    ValueError before the kernel: shapes that do not fit, W > 64, `steps` outside 0..4096, and with `check=True` (device
    reductions, one host read each) atom counts outside [0, min(N, W)] (unchecked, the kernel clamps them), a code outside
    0..4, a matrix that is not symmetric, an atomic number < 1 or one without a covalent radius (`config.ELEMENTS`) on a
    real atom."""
    x = torch.as_tensor(coords)
    bonds = torch.as_tensor(bond_orders)
    if x.dim() != 3 or x.shape[2] != 3 or not x.dtype.is_floating_point:
        raise ValueError(f"coords must be floating point [B,N,3], got {list(x.shape)} of type {x.dtype}")
    B, N = int(x.shape[0]), int(x.shape[1])
    if bonds.dim() != 3 or bonds.shape[1] != bonds.shape[2] or bonds.shape[0] != B:      # its own words: it knows B already
        raise ValueError(f"bond_orders must be [B,W,W] with B = {B}, got {list(bonds.shape)}")
    z, bonds, _, W = _args.graph_arguments(atomic_numbers, bonds, n_nodes, MAX_RELAX_ATOMS,
                                           f"relax_geometry takes molecules of at most {MAX_RELAX_ATOMS} atoms", counts=None)
    if isinstance(steps, bool) or not isinstance(steps, int) or not (0 <= steps <= MAX_RELAX_STEPS):
        raise ValueError(f"steps must be an integer in 0..{MAX_RELAX_STEPS}, got {steps!r}")
    if restraint_coords is not None and tuple(torch.as_tensor(restraint_coords).shape) != (B, N, 3):
        raise ValueError(f"restraint_coords must have the shape of coords, {[B, N, 3]}")
    if check:
        _args.check_n_nodes(n_nodes, B, min(N, W))
    elif torch.as_tensor(n_nodes).numel() != B:      # unchecked: no host read of device counts; the kernel clamps them
        raise ValueError(f"n_nodes holds {torch.as_tensor(n_nodes).numel()} counts for a batch of {B}")
    dev = _args.resolve_device(device, x)
    out = {"coords": torch.zeros(B, N, 3, dtype=torch.float32, device=dev),
           "energy_before": torch.zeros(B, dtype=torch.float32, device=dev),
           "energy_after": torch.zeros(B, dtype=torch.float32, device=dev),
           "accepted_steps": torch.zeros(B, dtype=torch.int32, device=dev),
           "max_displacement": torch.zeros(B, dtype=torch.float32, device=dev)}
    if return_gradient:
        out["gradient"] = torch.zeros(B, N, 3, dtype=torch.float32, device=dev)
    if B == 0 or N == 0 or W == 0:
        return out
    xd = x.to(dev, torch.float32).contiguous()
    rd = None if restraint_coords is None else torch.as_tensor(restraint_coords).to(dev, torch.float32).contiguous()
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
    if check:
        _check_molecules(zd, bonds.to(dev), nn, W)
    energy = torch.empty(B, 2, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().mcg_geometry_relax_ex(_lib.dptr(xd), _lib.dptr(rd), _lib.dptr(zd), _lib.dptr(bd), _lib.dptr(nn),
                                                B, N, W, steps, _lib.dptr(out["coords"]), _lib.dptr(energy),
                                                _lib.dptr(out.get("gradient")), _lib.dptr(stats),
                                                _lib.current_stream_ptr(dev)), "mcg_geometry_relax")
    out["energy_before"], out["energy_after"] = energy[:, 0].contiguous(), energy[:, 1].contiguous()
    out["accepted_steps"], out["max_displacement"] = stats[:, 0].to(torch.int32), stats[:, 1].contiguous()
    return out


def strain_energy(coords: torch.Tensor, atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor,
                  device=None, return_gradient: bool = False, restraint_coords: Optional[torch.Tensor] = None,
                  check: bool = True) -> Dict[str, torch.Tensor]:
    """`relax_geometry(steps=0)`: the force field's energy (`energy_before` = `energy_after`) and, asked for, its gradient
    at the given coordinates - a measure of how strained each molecule is; nothing moves."""
    return relax_geometry(coords, atomic_numbers, bond_orders, n_nodes, 0, device, return_gradient, restraint_coords, check)
