"""`optimise_pose="flexible"` through the generation entries on the MI355X, in the carved pocket of
`test_pose_optimise_gpu.test_generation_with_optimise_pose`: the three entries return equal records, the new record fields
are set exactly where `pose` is, the score does not rise, and `optimise_pose=True` in the same process still gives the
rigid walk's bits."""
import numpy as np
import pytest
import torch

from ml_conformer_generator_amd import interactions as IX

pytestmark = pytest.mark.gpu

NEW = ("pose_torsions", "pose_torsion_angles", "pose_conformer_rmsd", "intramolecular_clash_before", "intramolecular_clash")


def _flat(m, skip=()):
    return {k: (None if v is None else v.tolist() if torch.is_tensor(v) else v) for k, v in vars(m._measured).items()
            if k not in skip and k != "interaction_atom_scores"}


def _public(m):
    return (_flat(m), None if m.interaction_atom_scores is None else m.interaction_atom_scores.view(torch.int32).tolist(),
            m.coords.view(torch.int32).tolist())


def test_turned_torsions_reach_the_records():
    """The generation test's synthetic molecules have no rotatable bond, so the stage's own code for a molecule that DOES
    turn - `postprocess.optimise_rows`' selections, `handoff.measured_from_tensors`' slicing of the angles - runs here on
    `flex_cases` graphs: posed rows beside one whose pose failed, against the walk's own tensors."""
    import types

    import flex_cases as FC
    import interactions_ref as IR
    from ml_conformer_generator_amd import handoff, postprocess
    dev = torch.device("cuda:0")
    by = FC.by_name()
    pool = [by[k] for k in ("hexane", "toluene", "isopentylbenzene", "folded_heptane", "butane")]
    z, bonds, n, x = FC.padded(pool, 14)
    real = np.arange(14)[None, :, None] < n[:, None, None]
    x = ((x - x.sum(axis=1, keepdims=True) / n[:, None, None] + np.array([0.6, -0.3, 0.2], dtype=np.float32)) * real)
    x = torch.from_numpy(x.astype(np.float32))
    zt, bt, nt = torch.from_numpy(z), torch.from_numpy(bonds), torch.from_numpy(n)
    prepared = IX.prepare_receptor(IR.cases()[2].receptor)
    walk = lambda rec, c, k, e, b, steps: IX.optimise_pose_flexible(rec, c, k, e, b, steps, device=dev)      # noqa: E731
    gen = types.SimpleNamespace(_optimise_pose_flex=walk,
                                _score_placed=lambda ref, c, k: torch.full((c.shape[0],), 0.25, device=dev))
    req = types.SimpleNamespace(optimise_flexible=True, optimise_steps=24, typed_receptor=prepared, reference=None)
    pose = torch.eye(3).reshape(1, 9).repeat(len(pool), 1)
    pose = torch.cat([pose, torch.zeros(len(pool), 3)], dim=1)
    pose[4, 2] = float("nan")                                                    # butane: its pose failed
    out = postprocess.optimise_rows(gen, req, x, nt, zt, bt, pose, torch.full((len(pool),), 0.5))
    direct = {k: v.cpu() for k, v in walk(prepared, x, nt, zt, bt, 24).items()}
    values = {k: out[k] for k in postprocess.FLEX_RECORD_FIELDS + ("pose_trials_kept", "pose_optimisation_rmsd",
                                                                   "interaction_score_before")}
    records = handoff.measured_from_tensors(values, len(pool))
    for row, g in enumerate(pool[:4]):
        m = records[row]
        k = len(g.torsions)
        assert m.pose_torsions == k and m.pose_trials_kept == int(direct["kept"][row]) > 0
        assert m.pose_torsion_angles == direct["torsion_angles"][row, :k].tolist() and len(m.pose_torsion_angles) == k
        assert m.pose_conformer_rmsd == float(direct["conformer_rmsd"][row])
        assert m.intramolecular_clash_before == float(direct["clash_before"][row])
        assert m.intramolecular_clash == float(direct["clash_after"][row])
        assert torch.equal(out["coords"][row].cpu().view(torch.int32), direct["coords"][row].view(torch.int32))
        assert (any(m.pose_torsion_angles) and m.pose_conformer_rmsd > 0) if k else m.pose_conformer_rmsd == 0.0
    assert records[3].intramolecular_clash < records[3].intramolecular_clash_before                # the folded heptane opens
    failed = records[4]
    assert all(getattr(failed, f) is None for f in NEW + ("pose_trials_kept", "pose_optimisation_rmsd"))
    assert torch.equal(out["coords"][4].cpu().view(torch.int32), x[4].view(torch.int32)) and not bool(out["moved"][4])


def test_generation_with_flexible_optimise_pose(monkeypatch):
    from composed_cases import carved_pocket
    from test_receptor_relief_gpu import _posed_setup
    gen, ref, kw, base = _posed_setup(monkeypatch)
    pts, z = carved_pocket(ref, base)
    g = torch.Generator().manual_seed(12)
    z = torch.tensor([6, 6, 7, 8])[torch.randint(0, 4, (len(z),), generator=g)]
    rec = (pts, z, torch.randint(0, 8, (len(z),), generator=g))
    launched = []
    real = gen._optimise_pose_flex
    monkeypatch.setattr(gen, "_optimise_pose_flex", lambda *a, **k: launched.append(1) or real(*a, **k))

    rigid_first = gen.generate_conformers(receptor=rec, optimise_pose=True, **kw)
    assert launched == [] and all(getattr(m, f) is None for m in rigid_first for f in NEW)
    plain = gen.generate_conformers(receptor=rec, interaction_scores=True, **kw)
    got = gen.generate_conformers(receptor=rec, optimise_pose="flexible", **kw)
    assert launched == [1] and [m.sample_id for m in got] == [m.sample_id for m in plain]
    n_turned = 0
    for a, b in zip(plain, got):
        if b.pose is None:
            assert all(getattr(b, f) is None for f in NEW + ("pose_trials_kept",)) and torch.equal(a.coords, b.coords)
            continue
        assert all(getattr(b, f) is not None for f in NEW)                        # set exactly where `pose` is
        assert b.interaction_score <= b.interaction_score_before
        assert np.float32(b.interaction_score_before) == np.float32(a.interaction_score)
        assert 0 <= b.pose_torsions <= IX.FLEX_MAX_TORSIONS and len(b.pose_torsion_angles) == b.pose_torsions
        assert b.intramolecular_clash >= 0 and b.intramolecular_clash_before >= 0 and b.pose_conformer_rmsd >= 0
        if b.pose_trials_kept == 0:
            assert torch.equal(a.coords, b.coords) and b.pose_conformer_rmsd == 0.0
            assert b.intramolecular_clash == b.intramolecular_clash_before and not any(b.pose_torsion_angles)
            continue
        # what was kept lowered W + 0.840 CLASH; E's divisor is the molecule's own constant
        den = 1.0 + IX.ROTOR_WEIGHT * b.interaction_terms["n_rot"]
        assert (b.interaction_score * den + 0.840 * b.intramolecular_clash
                < b.interaction_score_before * den + 0.840 * b.intramolecular_clash_before + 1e-6)
        n_turned += 1 if any(b.pose_torsion_angles) else 0
        if not any(b.pose_torsion_angles):
            assert b.pose_conformer_rmsd == 0.0
        else:
            assert b.pose_conformer_rmsd > 0.0
    print(f"FLEX e2e: {n_turned} of {len(got)} turned a torsion; torsions {[m.pose_torsions for m in got]}; E "
          f"{[None if m.interaction_score_before is None else round(m.interaction_score_before, 3) for m in got]} -> "
          f"{[None if m.interaction_score is None else round(m.interaction_score, 3) for m in got]}; conformer rmsd "
          f"{[None if m.pose_conformer_rmsd is None else round(m.pose_conformer_rmsd, 3) for m in got]}")
    # (the synthetic weights' graphs decide how many torsions there are to turn: where a moved molecule has one, one turned)
    if any(m.pose_torsions and m.pose_trials_kept for m in got if m.pose is not None):
        assert n_turned >= 1
    for entry in ("generate_conformers_sharded", "forward"):
        again = getattr(gen, entry)(receptor=rec, optimise_pose="flexible", **kw)
        assert [_public(m) for m in again] == [_public(m) for m in got], entry
    fewer = gen.generate_conformers(receptor=rec, optimise_pose=("flexible", 2), **kw)
    assert all(m.pose_trials_kept is None or m.pose_trials_kept <= 2 for m in fewer)
    # the rigid option in the same process: today's bits, before and after the flexible calls
    rigid_again = gen.generate_conformers(receptor=rec, optimise_pose=True, **kw)
    assert [_public(m) for m in rigid_again] == [_public(m) for m in rigid_first]
    with pytest.raises(ValueError, match="optimise_pose"):
        gen.generate_conformers(receptor=rec, optimise_pose=("rigid", 8), **kw)
