"""The one place arguments are checked: the refusals the wrappers between a caller and the library share, and the two
idioms (which device, the graph tensors as the kernels read them) they repeat.  A leaf: it imports nothing from the
package, so every module takes it at the top.  Nothing here touches a device except `check_graphs`,
`check_known_elements` (the `check=True` reductions, on tensors that are already there) and `device_graph`."""
from __future__ import annotations

import math
import numbers
import operator
from typing import Optional

import torch


# ----------------------------------------------------------------------------------------------- tensors
def check_n_nodes(n_nodes: torch.Tensor, B: int, N: int) -> None:
    """B atom counts, each in [0, N] (the kernels read them from device memory and cannot report a bad one)."""
    n = torch.as_tensor(n_nodes).reshape(-1)
    if n.numel() != B:
        raise ValueError(f"n_nodes holds {n.numel()} counts for a batch of {B}")
    if B and (int(n.min()) < 0 or int(n.max()) > N):
        raise ValueError(f"n_nodes must lie in [0, {N}] (the padded width), got {int(n.min())}..{int(n.max())}")


def graph_arguments(atomic_numbers, bond_orders, n_nodes, max_atoms: int, too_wide: str, counts: Optional[bool] = True):
    """(z, bonds, B, W) of padded graph arguments - `atomic_numbers` [B, >= W], `bond_orders` [B,W,W], `n_nodes` [B] - their
    shapes and dtypes checked.  `too_wide`: the caller's own words for a width above `max_atoms`, up to ", got a width of".
    `counts`: True - each count in [0, W] (`check_n_nodes`: one host read where the counts are on the device); False -
    only that there are B of them, nothing is read; None - not looked at: the caller has other refusals to make first."""
    bonds = torch.as_tensor(bond_orders)
    z = torch.as_tensor(atomic_numbers)
    if bonds.dim() != 3 or bonds.shape[1] != bonds.shape[2]:
        raise ValueError(f"bond_orders must be [B,W,W], got {list(bonds.shape)}")
    B, W = int(bonds.shape[0]), int(bonds.shape[1])
    if W > max_atoms:
        raise ValueError(f"{too_wide}, got a width of {W}")
    if z.dim() != 2 or z.shape[0] != B or z.shape[1] < W:
        raise ValueError(f"atomic_numbers must be [B, >= W] = [{B}, >= {W}], got {list(z.shape)}")
    if bonds.dtype.is_floating_point or z.dtype.is_floating_point:
        raise ValueError("atomic_numbers and bond_orders must be integer tensors")
    if counts:
        check_n_nodes(n_nodes, B, W)
    elif counts is False and torch.as_tensor(n_nodes).numel() != B:
        raise ValueError(f"n_nodes holds {torch.as_tensor(n_nodes).numel()} counts for a batch of {B}")
    return z, bonds, B, W


def ligand_arguments(coords, n_nodes, atomic_numbers, max_atoms: int, max_batch: int, what: str):
    """(B, N, z) of posed, padded ligand arguments - `coords` [B,N,3], `n_nodes` [B], `atomic_numbers` [B, >= N] or None
    (z is then None) - with the counts in [0, N] and the limits on N and B checked.  `what`: the caller's own words for
    who takes at most so many ("clash relief takes")."""
    B, N = int(coords.shape[0]), int(coords.shape[1])
    check_n_nodes(n_nodes, B, N)
    if N > max_atoms or B > max_batch:
        raise ValueError(f"{what} at most {max_batch} molecules of at most {max_atoms} atoms, got [{B}, {N}]")
    if atomic_numbers is None:
        return B, N, None
    z = torch.as_tensor(atomic_numbers)
    if z.dim() != 2 or z.shape[0] != B or z.shape[1] < N:
        raise ValueError(f"atomic_numbers must be [B, >= N] = [{B}, >= {N}], got {list(z.shape)}")
    return B, N, z


def check_graphs(z: torch.Tensor, bonds: torch.Tensor, nn: torch.Tensor, W: int) -> None:
    """The `check=True` half of the graph wrappers: one device reduction, one host read."""
    real = torch.arange(W, device=z.device).view(1, W) < nn.view(-1, 1)
    pair = real.unsqueeze(1) & real.unsqueeze(2)
    c = bonds.to(torch.int16)
    bad = torch.stack([(pair & ((c < 0) | (c > 4))).any(), (pair & (c != c.transpose(1, 2))).any(),
                       (real & (z < 1)).any()]).cpu().tolist()
    if bad[0]:
        raise ValueError("bond_orders must hold the codes 0 none / 1 / 2 / 3 / 4 aromatic")
    if bad[1]:
        raise ValueError("bond_orders must be symmetric over each molecule's atoms")
    if bad[2]:
        raise ValueError("atomic numbers must be >= 1 on every real atom")


def check_known_elements(z: torch.Tensor, nn: torch.Tensor, W: int, who: str, elements: dict) -> None:
    """Every real atom of `z` [B,W] has a row in `elements` (`config.ELEMENTS`: Z -> (symbol, covalent radius)), else a
    ValueError in the name of `who`: one device reduction, one host read."""
    known = torch.zeros(max(elements) + 2, dtype=torch.bool)         # the last entry, for any other Z: False
    known[list(elements)] = True
    known = known.to(z.device)
    real = torch.arange(W, device=z.device).view(1, W) < nn.view(-1, 1)
    if bool((real & ~known[z.to(torch.long).clamp(min=0, max=known.numel() - 1)]).any()):
        raise ValueError(f"{who} knows the elements {[elements[k][0] for k in sorted(elements)]} only (no covalent "
                         "radius for another Z)")


def resolve_device(device, *tensors) -> torch.device:
    """`device` where it is given, else the device of the first of `tensors` that is on a GPU, else cuda:0.  Constructs a
    `torch.device` and nothing more: no device is touched."""
    if device is None:
        device = next((t.device for t in tensors if t.is_cuda), "cuda:0")
    return torch.device(device)


def device_graph(z: torch.Tensor, bonds: torch.Tensor, n_nodes, B: int, W: int, dev):
    """(atomic numbers [B,W] int32, bond codes [B,W,W] int8, counts [B] int32), contiguous on `dev`: a padded graph as
    the kernels read it."""
    return (z[:, :W].to(dev, torch.int32).contiguous(), bonds.to(dev, torch.int8).contiguous(),
            torch.as_tensor(n_nodes).to(dev, torch.int32).reshape(B).contiguous())


# ----------------------------------------------------------------------------------------------- scalars
def check_flag(name: str, value) -> bool:
    """An on / off option as a bool; anything but True or False is a ValueError."""
    if value is not True and value is not False:
        raise ValueError(f"{name} must be True or False, got {value!r}")
    return value


def check_real(name: str, value, low: Optional[float] = None, high: Optional[float] = None, open_low: bool = False
               ) -> float:
    """A real-number option as a float (not a bool, not NaN), else a ValueError that names `name` and the interval: with
    `high`, in [low, high] - (low, high] with `open_low`; without, any finite number, at least `low` where that is given
    and above it with `open_low` (a positive number: `low` 0)."""
    ok = not isinstance(value, bool) and isinstance(value, numbers.Real)
    if high is not None:
        what = f"a real number in {'(' if open_low else '['}{low:g}, {high:g}]"
        ok = ok and float(value) <= high
    else:
        what = "a finite real number" if low is None else "a positive real number" if open_low else \
            f"a finite real number >= {low:g}"
        ok = ok and math.isfinite(float(value))
    if ok and low is not None:
        ok = float(value) > low if open_low else float(value) >= low
    if not ok:
        raise ValueError(f"{name} must be {what}, got {value!r}")
    return float(value)


def _as_index(value) -> Optional[int]:
    """`value` as an int where it is of an integer type (numpy.int64 ...; not a bool, not a float), else None."""
    try:
        return None if isinstance(value, bool) else int(operator.index(value))
    except TypeError:
        return None


def check_at_least(name: str, value, lowest: int) -> int:
    """An integer option >= `lowest` as an int (any integer type; not a bool, not a float), else ValueError."""
    k = _as_index(value)
    if k is None or k < lowest:
        raise ValueError(f"{name} must be an integer >= {lowest}, got {value!r}")
    return k


def check_steps(name: str, value, lowest: int, highest: int, if_true: Optional[int] = None,
                if_false: Optional[int] = None) -> int:
    """A step budget as an int in `lowest`..`highest` (an integer type, not a bool), else a ValueError that names `name`.
    `if_true` / `if_false`: the budget True / False stands for, where the option accepts it."""
    if value is True and if_true is not None:
        return if_true
    if value is False and if_false is not None:
        return if_false
    k = _as_index(value)
    if k is None or not (lowest <= k <= highest):
        what = "an integer" if if_true is None else "True or an integer step budget"
        raise ValueError(f"{name} must be {'False, ' if if_false is not None else ''}{what} in {lowest}..{highest}, "
                         f"got {value!r}")
    return k


def check_rank_by(value) -> str:
    """`rank_by` as "shape", "combo", "electrostatic" or "interaction", else ValueError."""
    if value not in ("shape", "combo", "electrostatic", "interaction"):
        raise ValueError(f"rank_by must be 'shape', 'combo', 'electrostatic' or 'interaction', got {value!r}")
    return value
