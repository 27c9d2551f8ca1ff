"""Molecules above 42 atoms, host side (no GPU): which regime of the plan builder each shared case falls into, where the
accepted size range ends, and that the pass rule the GPU tests use against the fp64 oracle (a) leaves a correct fp32
evaluation an order of magnitude of room at these sizes and (b) sees one missing edge of a 114-atom molecule.

Cases and expected regimes: tests/large_molecule_cases.py.  GPU half: tests/test_large_molecules_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from large_molecule_cases import (CASES, WEIGHT_RECIPE, WEIGHT_SEED, build_inputs, oracle_per_molecule, span16, span64,
                                  unit_spans)
from parity_tolerance import violation


def _check_tables(sizes, N, cus, edge_mt=1):
    from ml_conformer_generator_amd import _lib
    L = _lib.lib()
    a = np.asarray(sizes, dtype=np.int32)
    info = np.zeros(8, dtype=np.int32)
    opts = _lib.PlanOpts(edge_mt=edge_mt)
    rc = L.mcg_plan_check_tables(len(a), int(N), a.ctypes.data, C.byref(opts), cus, info.ctypes.data)
    return rc, info.tolist(), (L.mcg_last_error().decode() if rc else "")


def test_span_restatement_on_hand_counted_examples():
    """The ten-line restatement itself: one 17-atom molecule owns 16 rows per atom, atom 0 in tile 0 alone, atom 1 in
    tile 1 alone (span 1); 18 atoms -> 17 rows, atom 0 covers rows 0..16 (two tiles).  One-atom molecules own no rows."""
    assert unit_spans([17], 16) == [1] and unit_spans([18], 16) == [2]
    assert unit_spans([1, 2], 16) == [0, 1]
    assert unit_spans([3, 17], 16) == [1, 2]              # 6 rows in front: atom 0's 16 rows now straddle tiles 0 and 1
    assert unit_spans([114], 16) == [8] and unit_spans([114], 64) == [3]


@pytest.mark.parametrize("name", sorted(CASES))
def test_each_case_is_in_the_regime_it_claims(name):
    """`mcg_plan_check_tables` (the plan builder's own host half and its self-check of every table) for devices of 64, 256
    and 304 compute units, against the regime the case states and against the span restatement."""
    c = CASES[name]
    sizes, N = c["sizes"], c["N"]
    assert max(sizes) == N and N > 42
    assert span16(sizes) == c["span16"] and span64(sizes) == c["span64"]
    for cus in ((c["cus"],) if "cus" in c else (64, 256, 304)):
        rc, info, err = _check_tables(sizes, N, cus, edge_mt=1)
        if c["sets"] is None:                                # refused, and the message names the limit
            assert rc != 0 and "115 atoms" in err and f"{N} atoms" in err and "16 rows" in err, (cus, rc, err)
        else:
            assert rc == 0, (cus, err)
            assert info[0] == c["sets"], (cus, info)
            if c["sets"] == 1 and "cus" not in c:            # four-tile units only: units == four-tile units, two rows per atom
                assert info[1] == info[2] > 0 and info[4] == 2 and info[5:] == [0, 0, 0], (cus, info)
                assert c["span16"] > 4                       # ... because quarter-tile units would need more than four
            if c["sets"] == 1 and "cus" in c:                # one mixed set: complete rounds of four-tile units + a quarter-tile tail
                assert 0 < info[2] < info[1] and info[2] % (2 * cus) == 0 and info[4] == 3 and info[5:] == [0, 0, 0], (cus, info)
            if c["sets"] == 2:                               # quarter-tile units (span 4) and, for latency mode 0, four-tile units (span 2)
                assert info[4] == 4 and info[7] == 2 and info[5] > 0 and c["span16"] == 4, (cus, info)
            if c["sets"] == 0:
                assert 5 <= c["span16"] <= 8 and info[1:] == [0] * 7, (cus, info)
        # 64-row units: accepted where no unit holds more than 16 atoms' rows (no molecule below 6 atoms)
        rc4, _, err4 = _check_tables(sizes, N, cus, edge_mt=4)
        if c["edge_mt_wide"] == 4:
            assert rc4 == 0, (cus, err4)
            assert c["span64"] <= 8
    assert (c["sets"] is None) == (c["span16"] > 8)
    # the routes the GPU module will assert are consistent with these spans
    for (mode, variant), r in c["routes"].items():
        wide = mode != "f32" and c["edge_mt_wide"] == 4
        if "pspan" in r:
            assert r["pspan"] == (c["span64"] if wide else c["span16"]), (mode, variant, r)
        if r["edge"] == "Exact":
            assert c["sets"] and r["unit_span"] == (3 if "cus" in c else 4 if c["sets"] == 2 and variant == "auto" else 2)
        elif "unit_span" in r:
            assert r["unit_span"] == 0                       # tables the route does not use are not reported
        if r["agg"] == "GatherP":
            assert r["pspan"] <= 4
        if r["edge"] in ("W64Bf16", "W64X6"):
            assert wide


def _batches(seed, trials, lo=1, hi=113):
    g = torch.Generator().manual_seed(seed)
    for _ in range(trials):
        B = int(torch.randint(1, 6, (1,), generator=g))
        yield torch.randint(lo, hi + 1, (B,), generator=g).tolist()


def test_the_accepted_size_range_ends_at_115_atoms_wherever_the_molecule_stands():
    """16-row tiles: an atom keeps at most eight partial-sum slots, so its n - 1 rows may run through eight tiles.  113 rows
    (n = 114) starting at any row span at most eight.  114 rows (n = 115) do when they start on an EVEN row - and they always
    do: every molecule in front contributes n (n - 1) rows, an even count, and i * 114 is even.  115 rows (n = 116) start on
    every residue mod 16 within one molecule (115 is odd, i runs over 116 values), row 15 included: nine tiles.  Above that
    the row table alone would take a molecule behind some prefixes and not behind others (117 atoms: four residues), so the
    plan builder refuses every molecule above 115 atoms by size.  Pinned here: 114- and 115-atom molecules are accepted at
    every position of every batch, 116-, 117- and 130-atom ones are refused behind any prefix, with a message that names
    the molecule and the limit.  200 seeded batches of mixed sizes, the large molecule at every position."""
    accepted_115 = lucky = 0
    for k, sizes in enumerate(_batches(114, 200)):
        for pos in range(len(sizes) + 1):
            for big in (114, 115):
                s = sizes[:pos] + [big] + sizes[pos:]
                rc, info, err = _check_tables(s, big, [64, 256, 304][k % 3])
                assert rc == 0, (s, err, info)
                # (unit tables only where the large molecule falls into complete rounds of four-tile units, whose 64 rows
                #  its atoms span at most three of, and the quarter-tile tail holds small molecules - case H)
                assert info[0] == 0 or (info[0] == 1 and 0 < info[2] < info[1] and info[4] <= 4), (s, info)
                assert span16(s) <= 8
                accepted_115 += big == 115
        prefix = sizes
        for big in (116, 117, 130):
            s = prefix + [big]
            rc, _, err = _check_tables(s, max(s), 256)
            assert rc != 0 and "up to 115 atoms" in err and f"{big} atoms" in err, (s, rc, err)
            if big == 116:
                assert span16(s) > 8
            lucky += span16(s) <= 8
    assert accepted_115 >= 400
    assert lucky > 0          # e.g. [3, 53, 26, 117]: would fit behind this prefix, is refused like behind every other


def test_64_row_units_take_molecules_up_to_451_atoms():
    """The same argument with R = 64: 7 * 64 + 3 = 451 atoms are accepted wherever they stand, 452 are refused."""
    for sizes in _batches(451, 6, lo=6, hi=300):
        for pos in range(len(sizes) + 1):
            s = sizes[:pos] + [451] + sizes[pos:]
            rc, _, err = _check_tables(s, 451, 256, edge_mt=4)
            assert rc == 0, (s, err)
            assert span64(s) <= 8
        s = sizes + [452]
        rc, _, err = _check_tables(s, 452, 256, edge_mt=4)
        assert rc != 0 and "up to 451 atoms" in err and "64 rows" in err, (s, err)
        assert span64(s) > 8


def test_plan_creation_refuses_an_oversized_molecule_before_touching_a_device():
    """`mcg_plan_create` on this (possibly GPU-less) host: the refusal is a host-side return code with the same text."""
    from ml_conformer_generator_amd import _lib
    L = _lib.lib()
    a = np.asarray(CASES["F"]["sizes"], dtype=np.int32)
    h = C.c_void_p()
    rc = L.mcg_plan_create(len(a), 200, a.ctypes.data, 1, C.byref(h))
    assert rc != 0 and not h.value
    assert b"mcg_plan_create" in L.mcg_last_error() and b"up to 115 atoms" in L.mcg_last_error()


def test_route_hook_refuses_null_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    L = _lib.lib()
    info = (C.c_int32 * 8)(*([-7] * 8))
    assert L.mcg_debug_route(None, None, 0, info) != 0
    assert b"mcg_debug_route" in L.mcg_last_error()
    assert list(info) == [-7] * 8                            # nothing written on refusal
    with pytest.raises(_lib.McgError, match="mcg_debug_route"):
        _lib.debug_route(None, None)


# ---------------------------------------------------------------------------------------------- the pass rule itself

@functools.lru_cache(maxsize=None)
def _oracles(name):
    from conftest import sd_for
    from oracle import egnn_oracle as EO
    c = CASES[name]
    sd = sd_for({"weight_seed": WEIGHT_SEED, "weight_recipe": WEIGHT_RECIPE})
    sd64 = {k: v.double() for k, v in sd.items()}
    t, z, nm, em, ctx = build_inputs(c["sizes"], c["N"], c["seed"])
    ref64 = EO.egnn_dynamics(sd64, t.double(), z.double(), nm.double(), em.double(), ctx.double())
    ref32 = EO.egnn_dynamics(sd, t, z, nm, em, ctx)
    return sd, (t, z, nm, em, ctx), ref32, ref64


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_fp32_oracle_keeps_a_tenth_of_the_tolerance_against_fp64(name):
    """A condition on the INPUTS of the GPU tests, not on the kernels: at these sizes a correct fp32 evaluation (the CPU
    oracle) sits below 0.1 x the stated per-call tolerance of the fp64 value, so `close(out, ref64)` leaves a correct
    kernel ten times the room its own rounding needs.  Measured with these inputs: see the printed figure (0.02 - 0.04)."""
    _, (t, z, nm, em, ctx), ref32, ref64 = _oracles(name)
    assert t.unique().numel() == t.numel() and float(z.abs().max()) > 2.0
    v = violation(ref32, ref64, split=3)
    print(f"LARGE-N host case {name}: fp32 oracle at {v:.4f} x tolerance of fp64")
    assert v < 0.1, v


def test_per_molecule_oracle_is_the_whole_batch_oracle():
    """The GPU module evaluates its fp64 ground truth molecule by molecule (large_molecule_cases.oracle_per_molecule): on
    case C - a 9-atom molecule between 68, 80 and 101 atoms, padded to 101 - it equals the whole-batch fp64 evaluation to
    rounding (1e-12 of the magnitude; the tolerance it serves is 1e-5), and in fp32 it is one more correct fp32 evaluation."""
    sd, (t, z, nm, em, ctx), ref32, ref64 = _oracles("C")
    per64 = oracle_per_molecule({k: v.double() for k, v in sd.items()}, t, z, nm, ctx)
    assert per64.dtype == torch.float64 and float((per64 * (1 - nm)).abs().max()) == 0.0
    assert float((per64 - ref64).abs().max()) <= 1e-12 * float(ref64.abs().max())
    assert violation(oracle_per_molecule(sd, t, z, nm, ctx), ref64, split=3) < 0.1


def test_the_pass_rule_sees_one_missing_edge_of_a_114_atom_molecule():
    """The rule used on the GPU, fed a deliberately wrong ORACLE (no broken kernel): case D with the single edge
    atom 0 <- atom 113 of the 114-atom molecule removed, and with one 16-row tile of atom 0's edges (j = 1..16) removed.
    Floor: 10 x the tolerance.  Measured with these inputs: 210 x and 2 150 x (printed)."""
    from oracle import egnn_oracle as EO
    sd, (t, z, nm, em, ctx), _, ref64 = _oracles("D")
    N = CASES["D"]["N"]
    assert CASES["D"]["sizes"][0] == 114
    for what, js in (("one edge", [113]), ("one 16-row tile", list(range(1, 17)))):
        em_mut = em.clone().reshape(-1, N, N)
        em_mut[0, 0, js] = 0.0                               # row = atom 0 of molecule 0 receives nothing from atoms js
        assert float(em.sum() - em_mut.sum()) == len(js)
        out = EO.egnn_dynamics(sd, t, z, nm, em_mut.reshape(-1, 1), ctx)
        v = violation(out, ref64, split=3)
        print(f"LARGE-N host case D without {what}: {v:.1f} x tolerance")
        assert v >= 10.0, (what, v)
