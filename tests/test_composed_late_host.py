"""The second composed batch (`composed_late_cases`) is one the GPU test (`test_composed_late_gpu.py`) may judge by: shown
here through the restatements alone, on the CPU.  These are conditions on the chosen molecules, the receptor and the trial
budgets, not measurements of the product: where one fails, the molecules change, not the condition."""
import functools

import numpy as np
import torch

import canonical_ref as CR
import composed_cases as CC
import composed_late_cases as LC
import electrostatics_ref as ER
import flex_pose_ref as FP
import hydrogens_ref as HR
import interactions_ref as IR
import pharmacophore_cases as PC
import pharmacophore_ref as PR
import pose_optimise_ref as P
import relief_ref as RR
import scaffold_ref as SFR
import stereo_cases as STC
import stereo_ref as STR
import substructure_cases as SBC
from ml_conformer_generator_amd import interactions as IX
from ml_conformer_generator_amd import receptor as RC
from ml_conformer_generator_amd import substructure as S
from ml_conformer_generator_amd.config import ATOMIC_NUMBERS

KEPT = LC.kept()
NAMES = [it["name"] for it in LC.batch()]
PARENT = {it["name"]: LC.parent(it) for it in KEPT}
LOW, HIGH = LC.STEREO_BAND


def _xyz(x):
    return [tuple(float(v) for v in p) for p in np.asarray(x, dtype=np.float64)]


def test_the_batch_has_its_size_elements_noise_and_a_dropped_row_mid_batch():
    items = LC.batch()
    assert 12 <= len(items) <= 16 and len(set(NAMES)) == len(NAMES)
    assert all(it["mol"][2] <= 20 and it["mol"][2] < LC.WIDTH for it in items)
    assert all(z in ATOMIC_NUMBERS for it in items for z in it["mol"][0])          # what the default decoder can emit
    assert 0 < NAMES.index(LC.DROPPED) < len(NAMES) - 3                            # rows behind it: batch_row != position
    assert PARENT[LC.ONE_ATOM][0][2] == 1 and sum(1 for it in KEPT if PARENT[it["name"]][0][2] < 3) == 2
    for it in items:                                                               # the noise is there, and is fixed
        assert it["xyz"].dtype == np.float32 and it["xyz"].shape == (it["mol"][2], 3)
    again = LC.batch.__wrapped__()
    assert all(np.array_equal(a["xyz"], b["xyz"]) for a, b in zip(items, again))
    clean = dict((name, fx) for name, fx, _ in LC._rows())
    moved = np.concatenate([(it["xyz"] - clean[it["name"]]["xyz"]).ravel() for it in items])
    assert 0.12 < moved.std() < 0.18 and len(moved) >= 150


def test_standardisation_gives_the_intended_statuses_maps_and_fragments():
    std = LC.standardized()
    for it in LC.batch():
        s, (status, atom_map, n_fragments) = std[it["name"]], it["expect"]
        assert (s["status"], s["atom_map"], s["n_fragments"]) == (status, atom_map, n_fragments), it["name"]
        if n_fragments == 2:
            gone = [a for a in range(it["mol"][2]) if a not in atom_map]
            d = np.linalg.norm(it["xyz"][atom_map][:, None].astype(np.float64) - it["xyz"][gone][None], axis=2)
            assert d.min() >= 5.0, (it["name"], d.min())                           # each fragment has its own place
    assert [n for n in NAMES if std[n]["status"] != 0] == [LC.DROPPED]
    shifted = [n for n in NAMES if std[n]["status"] == 0 and std[n]["atom_map"][0] != 0]
    assert shifted == list(LC.SHIFTED) and len(shifted) >= 2                       # the parent BEHIND a smaller fragment
    # in the first of them the parent has a ring with a substituent, a rotatable bond and an atom that carries hydrogens
    mol = PARENT[LC.SHIFTED[0]][0]
    keep = SFR.scaffold(*mol)[3]
    assert 0 < len(keep) < mol[2] and FP.tree(*mol)["used"] >= 1 and max(HR.counts(*mol)) >= 1


def test_stereo_rows_are_defined_undefined_and_a_pair_of_stereoisomers():
    counts = {n: STR.counts(*PARENT[n][0], _xyz(PARENT[n][1])) for n in PARENT}
    assert sum(1 for c in counts.values() if c[0] >= 1) >= 2                       # defined tetrahedral centres
    assert sum(1 for c in counts.values() if c[1] >= 1) >= 1                       # a defined double bond
    assert counts[LC.UNDEFINED] == (0, 0, 1)                                       # an undefined centre
    a, b = (PARENT[n] for n in LC.STEREOISOMERS)
    assert CR.identity_bytes(*a[0]) == CR.identity_bytes(*b[0])                    # `unique="exact"` merges them,
    assert STR.identity_bytes(*a[0], _xyz(a[1])) != STR.identity_bytes(*b[0], _xyz(b[1]))      # `unique="stereo"` does not
    assert counts[LC.STEREOISOMERS[0]] == counts[LC.STEREOISOMERS[1]] == (1, 0, 0)
    again = PARENT[LC.SAME_STEREOISOMER]                                           # ... and merges the same stereoisomer
    assert STR.identity_bytes(*a[0], _xyz(a[1])) == STR.identity_bytes(*again[0], _xyz(again[1]))
    assert not np.array_equal(a[1], again[1])
    # the two hexadienes are one graph and two double-bond isomers
    c, d = PARENT["hexa-2,4-diene"], PARENT["hexa-2,4-diene, cis-trans"]
    assert CR.identity_bytes(*c[0]) == CR.identity_bytes(*d[0])
    assert STR.identity_bytes(*c[0], _xyz(c[1])) != STR.identity_bytes(*d[0], _xyz(d[1]))


def test_torsion_scaffold_and_framework_rows():
    used = {n: FP.tree(*PARENT[n][0])["used"] for n in LC.posed_parents()}
    assert sum(1 for k in used.values() if k >= 1) >= 3 and sum(1 for k in used.values() if k == 0) >= 3
    graph = {n: CR.identity_bytes(*PARENT[n][0]) for n in PARENT}
    murcko = {n: SFR.identity(*PARENT[n][0]) for n in PARENT}
    frame = {n: SFR.identity(*PARENT[n][0], generic=True) for n in PARENT}
    pairs = [(a, b) for a in PARENT for b in PARENT if a < b]
    assert any(murcko[a] == murcko[b] != b"" and graph[a] != graph[b] for a, b in pairs)
    assert any(frame[a] == frame[b] != b"" and murcko[a] != murcko[b] for a, b in pairs)
    assert sum(1 for n in PARENT if murcko[n] == b"") >= 1                         # no ring: the empty scaffold
    # the four identities group the kept rows four different ways
    stereo = {n: STR.identity_bytes(*PARENT[n][0], _xyz(PARENT[n][1])) for n in PARENT}
    assert len({len(set(v.values())) for v in (graph, stereo, murcko, frame)}) == 4


def test_substructure_patterns_are_present_on_some_kept_rows_and_absent_on_others():
    for pattern in LC.REQUIRE + LC.EXCLUDE:
        found = [SBC.reference(PARENT[n][0], S.as_pattern(pattern), nh=HR.counts(*PARENT[n][0]))["count"] for n in PARENT]
        assert any(c >= 1 for c in found) and any(c == 0 for c in found), (pattern, found)
    bounded = [p for p in LC.REQUIRE + LC.EXCLUDE + LC.COUNTS if any(q.hmin > 0 or q.hmax < 255 for q in S.as_pattern(p).atoms)]
    assert bounded                                                                 # the `nh` column of the table
    # ... and that pattern's answer depends on the hydrogens: without them it finds something else on some row
    p = S.as_pattern(bounded[0])
    assert any(SBC.reference(PARENT[n][0], p, nh=HR.counts(*PARENT[n][0]))["count"] !=
               SBC.reference(PARENT[n][0], p, nh=[0] * PARENT[n][0][2])["count"] for n in PARENT)


def test_every_element_of_every_parent_has_charge_parameters():
    for n in PARENT:
        assert ER.charges(*PARENT[n][0])["status"] == 0, n
    z, adj = LC.reference()[1]
    assert ER.charges(list(z), adj.tolist(), len(z))["status"] == 0


def test_every_kept_row_meets_the_stage_tolerances_preconditions():
    """At the parent's input coordinates and at its fp64 pose: the hydrogens' conditions, the stereo decision margins
    `test_stereo_gpu` requires of its fuzz (no |chi| or |cos| in [0.05, 0.2]) and the pharmacophore match-distance margin."""
    fr = CC.reference_features()
    posed = LC.posed_parents()
    assert set(posed) == {n for n in PARENT if PARENT[n][0][2] >= 3}
    placed = 0
    for n, (mol, xyz) in PARENT.items():
        for x in [xyz] + ([posed[n].numpy()] if n in posed else []):
            placed += CC.hydrogen_conditions(mol, x, n)["n_hydrogens"]
            assert all(not (LOW <= m <= HIGH) for m in STR.margins(*mol, _xyz(x))), (n, STR.margins(*mol, _xyz(x)))
        if n in posed:
            x = posed[n].double()
            d0 = torch.cdist(torch.from_numpy(xyz).double(), torch.from_numpy(xyz).double())
            assert float((torch.cdist(x, x) - d0).abs().max()) < 1e-4, n           # the fp64 pose is rigid
            t, rings, _ = PR.perceive(*mol)
            assert PC._margin_ok(fr, PR.features(posed[n].numpy(), t, rings)), n
    assert placed >= 80


@functools.lru_cache(maxsize=None)
def _walks():
    """name -> (the relief's restatement, the rigid walk's, the flexible walk's) from the fp64 pose, each started where the
    one before it ended, against the typed receptor with the budgets of call A."""
    rec = LC.receptor()
    prepared = IX.prepare_receptor(rec)
    y, rj, tj = prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(), prepared.types.numpy()
    rv = RC.vdw_radii(rec[1]).double().numpy()
    out = {}
    for n, x in LC.posed_parents().items():
        mol = PARENT[n][0]
        moved = RR.walk(x.double().numpy(), RC.vdw_radii(torch.tensor(mol[0])).double().numpy(), rec[0].double().numpy(), rv,
                        LC.RELIEF_STEPS)
        start = moved["coords"].astype(np.float32)
        ri, ti = IR.radii(mol[0]), IR.ligand_types(*mol, PR.perceive(*mol)[0])
        rigid = P.run_walk(start, ri, ti, y, rj, tj, LC.OPTIMISE_STEPS, LC.MAX_SHIFT)
        flex = FP.run_walk(start, (ri, ti), (y, rj, tj), np.array(mol[0]), np.array(mol[1]), LC.OPTIMISE_STEPS, LC.MAX_SHIFT)
        out[n] = (moved, rigid, flex)
    return out


def test_the_relief_and_both_walks_move_some_rows_and_leave_others():
    rec = LC.receptor()
    ref_xyz, _ = LC.reference()
    assert float(torch.cdist(rec[0].double(), ref_xyz.double()).min()) > RC.SELF_CONTACT + 0.5
    assert 0 < rec[0].shape[0] <= RC.MAX_RECEPTOR_ATOMS and set(rec[1].tolist()) == {6, 7, 8}
    walks = _walks()
    relieved = [n for n, (m, _, _) in walks.items() if m["accepted"] > 0]
    kept = [n for n, (_, r, _) in walks.items() if r["kept"] > 0]
    none = [n for n, (_, r, _) in walks.items() if r["kept"] == 0]
    turned = [n for n, (_, _, f) in walks.items() if f["kept"] > 0 and np.abs(f["angles"][: f["tree"]["used"]]).max(initial=0) > 0]
    print(f"COMPOSED LATE host: relief moves {relieved}; the rigid walk keeps a trial on {kept}, none on {none}; the flexible "
          f"walk turns a torsion on {turned} (budgets {LC.RELIEF_STEPS}, {LC.OPTIMISE_STEPS})")
    assert len(relieved) >= 2 and len(relieved) < len(walks)
    assert len(kept) >= 2 and len(none) >= 1
    assert len(turned) >= 2
    # a row without a torsion walks as the rigid walk walks it
    for n, (_, r, f) in walks.items():
        if f["tree"]["used"] == 0:
            assert np.array_equal(r["coords"], f["coords"]) and r["kept"] == f["kept"], n
