"""The composed batch of `composed_cases` is one the GPU test (`test_composed_path_gpu.py`) may judge by: shown here
through the restatements alone, on the CPU.  These are conditions on the chosen molecules, not measurements of the
product: where one fails, the molecules change, not the condition."""
import numpy as np
import torch

import composed_cases as CC
import geometry_ref as GR
import pharmacophore_cases as PC
import pharmacophore_ref as PR
from ml_conformer_generator_amd import receptor as RC
from ml_conformer_generator_amd.config import ATOMIC_NUMBERS

KEPT = [it for it in CC.batch() if CC.standardized()[it["name"]]["status"] == 0]


def test_the_batch_is_what_the_issue_asks_for():
    items = CC.batch()
    names = [it["name"] for it in items]
    assert 10 <= len(items) <= 12 and len(set(names)) == len(names)
    assert all(it["mol"][2] <= 24 and it["mol"][2] < CC.WIDTH for it in items)
    assert all(z in ATOMIC_NUMBERS for it in items for z in it["mol"][0])          # what the default decoder can emit
    assert sorted(it["mol"][2] for it in items)[:2] == [1, 2]
    assert 0 < names.index(CC.DROPPED) < len(names) - 3                            # rows behind it: batch_row != position
    for it in items:                                                               # the noise is there, and is fixed
        assert it["xyz"].dtype == np.float32 and it["xyz"].shape == (it["mol"][2], 3)
    again = CC.batch.__wrapped__()
    assert all(np.array_equal(a["xyz"], b["xyz"]) for a, b in zip(items, again))
    clean = dict((name, fx) for name, fx, _ in CC._rows())
    moved = np.concatenate([(it["xyz"] - clean[it["name"]]["xyz"]).ravel() for it in items])
    assert 0.12 < moved.std() < 0.18 and len(moved) >= 150


def test_standardisation_gives_the_intended_statuses_maps_and_fragments():
    std = CC.standardized()
    two = 0
    for it in CC.batch():
        s, (status, atom_map, n_fragments) = std[it["name"]], it["expect"]
        assert (s["status"], s["atom_map"], s["n_fragments"]) == (status, atom_map, n_fragments), it["name"]
        assert s["atoms_removed"] == it["mol"][2] - len(atom_map)
        if n_fragments == 2:
            two += 1
            gone = [a for a in range(it["mol"][2]) if a not in atom_map]
            d = np.linalg.norm(it["xyz"][atom_map][:, None].astype(np.float64) - it["xyz"][gone][None], axis=2)
            assert d.min() >= 5.0, (it["name"], d.min())                           # each fragment has its own place
    assert two >= 2
    assert [it["name"] for it in CC.batch() if std[it["name"]]["status"] != 0] == [CC.DROPPED]
    assert std["propane and ethanol"]["atom_map"][0] != 0                          # a renumbering, not a truncation
    # aromatic five- and six-rings with N and O on them, and Kekule forms that put double bonds somewhere
    rings = {it["name"]: PR.perceive(*CC.parent(it)[0])[1] for it in KEPT}
    assert sum(1 for r in rings.values() for m in r if bin(m).count("1") == 5) >= 2
    assert sum(1 for r in rings.values() for m in r if bin(m).count("1") == 6) >= 5
    assert all(std[k]["doubles"] for k in ("phenol", "imidazole", "indole", "reference molecule", "pyridine"))


def test_every_kept_row_meets_the_conditions_of_the_hydrogen_tolerance():
    placed = 0
    for it in KEPT:
        mol, xyz = CC.parent(it)
        placed += CC.hydrogen_conditions(mol, xyz, it["name"])["n_hydrogens"]
    assert placed >= 40


def test_posed_features_keep_the_margin_to_the_match_distance():
    ref_xyz, _ = CC.reference()
    fr = CC.reference_features()
    assert len(fr) >= 10 and {k for k, _ in fr} >= {0, 1, 2, 3, 4, 5}
    posed = CC.posed_parents()
    assert set(posed) == {it["name"] for it in KEPT if CC.parent(it)[0][2] >= 3}
    with_features = 0
    for it in KEPT:
        mol, xyz = CC.parent(it)
        if it["name"] not in posed:
            continue
        x = posed[it["name"]].double()
        d0 = torch.cdist(torch.from_numpy(xyz).double(), torch.from_numpy(xyz).double())
        assert float((torch.cdist(x, x) - d0).abs().max()) < 1e-4, it["name"]      # the fp64 pose is rigid
        t, rings, _ = PR.perceive(*mol)
        fm = PR.features(posed[it["name"]].numpy(), t, rings)
        with_features += bool(fm)
        assert PC._margin_ok(fr, fm), it["name"]
    assert with_features >= 6
    own = posed["reference molecule"]                  # the reference's own noisy copy lands on it: features will match
    t, rings, _ = PR.perceive(*CC.parent(next(it for it in KEPT if it["name"] == "reference molecule"))[0])
    assert PR.matches(fr, PR.features(own.numpy(), t, rings)) >= 5
    assert float((own.double() - ref_xyz.double()).pow(2).sum(1).mean().sqrt()) < 0.6


def test_the_relaxation_accepts_a_step_on_every_kept_row_of_three_or_more_atoms():
    seen = 0
    for it in KEPT:
        (z, codes, n), xyz = CC.parent(it)
        if n < 3:
            continue
        seen += 1
        out = GR.minimise(xyz, xyz, GR.topology(z, np.array(codes)), CC.RELAX_STEPS)
        assert out["accepted"] >= 1 and out["E"] < out["E_start"], (it["name"], out["accepted"])
    assert seen >= 8


def test_the_carved_pocket_makes_some_posed_rows_clash_and_leaves_one_clean():
    """... and, by the relief's fp64 restatement, some of the clashing rows can be moved clear and one cannot: the call
    then has rows the relief moves and a row `max_receptor_clashes` removes."""
    import relief_ref as RR
    from test_receptor_gpu import _restate
    rec_xyz, rec_z = CC.receptor()
    ref_xyz, _ = CC.reference()
    assert float(torch.cdist(rec_xyz.double(), ref_xyz.double()).min()) > RC.SELF_CONTACT + 1.0
    assert 0 < rec_xyz.shape[0] <= RC.MAX_RECEPTOR_ATOMS

    def count(x, z):
        over = _restate(np.asarray(x, dtype=np.float32)[None], np.array([z]), [len(z)], rec_xyz.numpy(), rec_z.numpy())[0]
        return int((over >= np.float32(RC.CLASH_OVERLAP)).sum())
    rj = RC.vdw_radii(rec_z).double().numpy()
    before, after = {}, {}
    for it in KEPT:
        if it["name"] in CC.posed_parents():
            z, x = CC.parent(it)[0][0], CC.posed_parents()[it["name"]].double().numpy()
            before[it["name"]] = count(x, z)
            moved = RR.walk(x, RC.vdw_radii(torch.tensor(z)).double().numpy(), rec_xyz.double().numpy(), rj, RC.RELIEF_STEPS)
            after[it["name"]] = count(moved["coords"], z)
    print("COMPOSED host: clashes of the fp64 poses with the carved pocket", before, "and behind the fp64 relief", after)
    assert sum(1 for c in before.values() if c > 0) >= 2 and sum(1 for c in before.values() if c == 0) >= 1
    assert sum(1 for k, c in after.items() if c == 0 and before[k] > 0) >= 2 and sum(1 for c in after.values() if c > 0) >= 1
