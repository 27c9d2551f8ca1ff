"""The one code rule of the graph kernels ("The shared prologue of the graph kernels"): between two
real atoms a bond code is 1, 2, 3 or 4 and ANY other value is no bond.  Every entry that runs one wave per molecule is
called on a two-row batch - row 0 an ordinary molecule (acetic acid), row 1 a probe - with 0, with each off-range value and
with 1 at one symmetric entry (i, j) of the probe between two otherwise unbonded atoms.  An off-range value must give the
0 call's output buffers byte for byte; code 1 must change row 1 (the entry matters to that kernel) and leave row 0 alone.
Shapes: n = W = 6 with the entry (0, 4), and n = W = 64 with the entry (63, 0) - the last lane and the top mask bit.
Probes: a chain the entry closes to a ring (N at one end of the entry, O at the other), for `mcg_standardize_graphs` two
chains the entry joins.  Buffers are compared as bytes, sentinel fill included: equal means equal."""
import math

import pytest
import torch

from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd.fingerprint import FP_WORDS
from ml_conformer_generator_amd.interactions import FLEX_MAX_TORSIONS as MAX_TORSIONS
from ml_conformer_generator_amd.pharmacophore import MAX_RINGS
from ml_conformer_generator_amd.substructure import MAX_PATTERN_ATOMS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OFF_RANGE = (5, 127, -1, -128)
ENTRY = {6: (0, 4), 64: (63, 0)}                  # n = W -> the probed entry


class _Out:
    """An output buffer of `per_row` bytes per batch row."""

    def __init__(self, per_row):
        self.per_row = per_row


class _Graphs:
    """The two-row batch with `value` at the probed entry, on the device."""

    def __init__(self, W, fragments, value):
        i, j = ENTRY[W]
        chain = [(0, 1), (1, 2), (2, 3), (3, 4), (2, 5)] if W == 6 else [(k, k + 1) for k in range(W - 1)]
        if fragments:
            chain.remove((2, 3) if W == 6 else (31, 32))
        z = torch.zeros(2, W, dtype=torch.int32)
        bonds = torch.zeros(2, W, W, dtype=torch.int8)
        z[0, :4] = torch.tensor([6, 6, 8, 8], dtype=torch.int32)
        for a, b, c in [(0, 1, 1), (1, 2, 2), (1, 3, 1)]:
            bonds[0, a, b] = bonds[0, b, a] = c
        z[1] = 6
        z[1, min(i, j)], z[1, max(i, j)] = 7, 8
        for a, b in chain:
            bonds[1, a, b] = bonds[1, b, a] = 1
        assert int(bonds[1, i, j]) == 0 and int(bonds[1, j, i]) == 0
        bonds[1, i, j] = bonds[1, j, i] = value
        coords = torch.tensor([[1.5 * math.cos(0.9 * k) + 0.05 * k, 1.5 * math.sin(0.9 * k), 0.55 * k] for k in range(W)],
                              dtype=torch.float32).expand(2, W, 3)
        self.z, self.bonds, self.coords = z.to(DEV), bonds.to(DEV), coords.contiguous().to(DEV)
        self.n = torch.tensor([4, W], dtype=torch.int32, device=DEV)
        self.types = torch.zeros(2, W, dtype=torch.uint8, device=DEV)
        self.ring_mask = torch.zeros(2, MAX_RINGS, dtype=torch.int64, device=DEV)
        self.n_rings = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.keep_all = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        # one pattern, N ~ O over a code-1 bond: any degree, any hydrogen count, ring and aromatic flags not asked
        any_count = (255 << 8) | (255 << 24)
        pat_atoms = torch.zeros(1, MAX_PATTERN_ATOMS, 2, dtype=torch.int64)
        pat_atoms[0, 0] = torch.tensor([1 << 7, any_count])
        pat_atoms[0, 1] = torch.tensor([1 << 8, any_count])
        pat_bonds = torch.zeros(1, MAX_PATTERN_ATOMS, MAX_PATTERN_ATOMS, dtype=torch.uint8)
        pat_bonds[0, 1, 0] = 1
        self.pat_n = torch.tensor([2], dtype=torch.int32, device=DEV)
        self.pat_atoms, self.pat_bonds = pat_atoms.to(DEV), pat_bonds.to(DEV)


def _arguments(name, g, W):
    """The entry's arguments in the header's order, without the stream: tensors, integers, None and `_Out`s."""
    HW = max(4, 3 * W)
    graph = [g.z, g.bonds, g.n]
    return {
        "mcg_graph_fingerprint": lambda: graph + [2, W, _Out(4 * FP_WORDS), _Out(8), _Out(4)],
        "mcg_canonical_order": lambda: graph + [2, W, _Out(4 * W), _Out(4), _Out(4), _Out(8)],
        "mcg_stereo_order": lambda: [g.coords] + graph + [2, W, _Out(4 * W), _Out(4), _Out(4), _Out(8), _Out(W), _Out(8),
                                                           _Out(12)],
        "mcg_pharm_perceive": lambda: graph + [2, W, _Out(W), _Out(4), _Out(8 * MAX_RINGS)],
        "mcg_standardize_graphs": lambda: [g.coords] + graph + [2, W, W, _Out(12 * W), _Out(4 * W), _Out(W * W), _Out(W * W),
                                                                 _Out(4 * W), _Out(4), _Out(4), _Out(4), _Out(4)],
        "mcg_geometry_relax": lambda: [g.coords] + graph + [2, W, W, 8, _Out(12 * W), _Out(8), _Out(12 * W), _Out(8)],
        "mcg_hydrogens_place": lambda: [g.coords] + graph + [g.types, g.ring_mask, g.n_rings, 2, W, W, HW, _Out(12 * HW),
                                                              _Out(4 * HW), _Out(4 * W), _Out(4), _Out(4), _Out(4 * W)],
        "mcg_charges_peoe": lambda: graph + [g.types, g.ring_mask, g.n_rings, 2, W, _Out(4 * W), _Out(4 * W), _Out(4 * W),
                                             _Out(4)],
        "mcg_substructure_match": lambda: graph + [None, 2, W, g.pat_n, g.pat_atoms, g.pat_bonds, 1, _Out(4), _Out(4),
                                                   _Out(4 * MAX_PATTERN_ATOMS), _Out(8)],
        "mcg_ring_scaffold": lambda: graph + [2, W, _Out(8 * W), _Out(4 * W), _Out(4 * W), _Out(32), _Out(32)],
        "mcg_induced_subgraph": lambda: graph + [g.keep_all, 0, 2, W, _Out(4 * W), _Out(W * W), _Out(4), _Out(4 * W)],
        "mcg_torsion_tree": lambda: graph + [2, W, _Out(8 * MAX_TORSIONS), _Out(8 * MAX_TORSIONS), _Out(8 * W), _Out(8)],
    }[name]()


ENTRIES = ("mcg_graph_fingerprint", "mcg_canonical_order", "mcg_stereo_order", "mcg_pharm_perceive", "mcg_standardize_graphs",
           "mcg_geometry_relax", "mcg_hydrogens_place", "mcg_charges_peoe", "mcg_substructure_match", "mcg_ring_scaffold",
           "mcg_induced_subgraph", "mcg_torsion_tree")


def _call(name, W, value):
    """One launch of `name` with `value` at the probed entry: its output buffers as host byte tensors [2, per_row]."""
    g = _Graphs(W, name == "mcg_standardize_graphs", value)
    outs, args = [], []
    for x in _arguments(name, g, W):
        if isinstance(x, _Out):
            outs.append(torch.full((2, x.per_row), 0x5a, dtype=torch.uint8, device=DEV))
            x = outs[-1]
        args.append(_lib.dptr(x) if isinstance(x, torch.Tensor) else x)
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr(torch.device(DEV))), name)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("W", sorted(ENTRY))
@pytest.mark.parametrize("name", ENTRIES)
def test_an_off_range_code_is_no_bond(name, W):
    none, bonded = _call(name, W, 0), _call(name, W, 1)
    for value in OFF_RANGE:
        got = _call(name, W, value)
        for k, (x, y) in enumerate(zip(got, none)):
            assert torch.equal(x, y), f"{name}: output {k} with {value} at the entry differs from the output with 0"
    assert any(not torch.equal(x[1], y[1]) for x, y in zip(bonded, none)), f"{name}: the entry does not reach row 1"
    assert all(torch.equal(x[0], y[0]) for x, y in zip(bonded, none)), f"{name}: the probe's entry reached row 0"
