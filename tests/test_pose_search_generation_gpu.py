"""`optimise_pose="search"` through the generation entries on the MI355X, in the carved pocket of
`test_pose_flex_generation_gpu`: the records carry the search's fields exactly where `pose` is, the interaction score is the
stand-alone score of the returned coordinates, a sample id gets the same bits in two batch sizes and through the three
entries, the search is never worse than the flexible walk alone, and `optimise_pose="flexible"` in the same process is still
`optimise_pose_flexible` on its rows."""
import numpy as np
import pytest
import torch

from ml_conformer_generator_amd import interactions as IX

pytestmark = pytest.mark.gpu

FLEX = ("pose_torsions", "pose_torsion_angles", "pose_conformer_rmsd", "intramolecular_clash_before", "intramolecular_clash")
NEW = ("pose_starts", "pose_best_start")
DEV = torch.device("cuda:0")


def _flat(m):
    return {k: (None if v is None else v.tolist() if torch.is_tensor(v) else v) for k, v in vars(m._measured).items()
            if k != "interaction_atom_scores"}


def _public(m):
    return (_flat(m), None if m.interaction_atom_scores is None else m.interaction_atom_scores.view(torch.int32).tolist(),
            m.coords.view(torch.int32).tolist())


def _alone(m):
    """(coords [1,n,3], n [1], z [1,n], bonds [1,n,n]) of one record's returned molecule."""
    k = len(m.atomic_numbers)
    return (m.coords[None], torch.tensor([k], dtype=torch.int32), torch.tensor([m.atomic_numbers], dtype=torch.int32),
            m.bond_orders[None])


def test_generation_with_a_pose_search(monkeypatch):
    from composed_cases import carved_pocket
    from test_receptor_relief_gpu import _posed_setup
    gen, ref, kw, _ = _posed_setup(monkeypatch)
    kw = dict(kw, sample_seed=7)
    pts, z = carved_pocket(ref, gen.generate_conformers(**kw))                   # carved round this seed's own poses
    g = torch.Generator().manual_seed(12)
    z = torch.tensor([6, 6, 7, 8])[torch.randint(0, 4, (len(z),), generator=g)]
    rec = (pts, z, torch.randint(0, 8, (len(z),), generator=g))
    seen = []
    real = gen._search_pose
    monkeypatch.setattr(gen, "_search_pose", lambda *a: seen.append(a[5:]) or real(*a))

    flexible_first = gen.generate_conformers(receptor=rec, optimise_pose=("flexible", 8), **kw)
    assert seen == [] and all(getattr(m, f) is None for m in flexible_first for f in NEW)
    got = gen.generate_conformers(receptor=rec, optimise_pose=("search", 4, 8), **kw)
    assert len(seen) == 1 and seen[0][:3] == (4, 8, 7) and seen[0][3] is None    # starts, trials, the call's seed, ids 0..B-1
    assert [m.sample_id for m in got] == [m.sample_id for m in flexible_first]
    posed = [m for m in got if m.pose is not None]
    assert len(posed) >= 6
    for m, f in zip(got, flexible_first):
        if m.pose is None:
            assert all(getattr(m, k) is None for k in NEW + FLEX + ("pose_trials_kept",))
            continue
        assert m.pose_starts == 4 and 0 <= m.pose_best_start < 4
        assert all(getattr(m, k) is not None for k in FLEX)
        den = 1.0 + IX.ROTOR_WEIGHT * m.interaction_terms["n_rot"]
        # never worse than the flexible walk alone (start 0 IS that walk), by the walk's own objective
        assert (m.interaction_score * den + 0.840 * m.intramolecular_clash
                <= f.interaction_score * den + 0.840 * f.intramolecular_clash + 1e-6)
        assert np.float32(m.interaction_score_before) == np.float32(f.interaction_score_before)
        if m.pose_best_start == 0:                                               # ... and where it won, its record
            assert _public(m)[1:] == _public(f)[1:]
            assert {k: v for k, v in _flat(m).items() if k not in NEW} == {k: v for k, v in _flat(f).items() if k not in NEW}
    # the interaction score is the stand-alone score of the returned coordinates, bit for bit
    prepared = IX.prepare_receptor(rec)
    for m in posed:
        own = IX.interaction_scores(prepared, *_alone(m), device=DEV)["score"].cpu()
        assert np.float32(m.interaction_score).view(np.uint32) == own.numpy().view(np.uint32)[0], m.sample_id
    print(f"SEARCH e2e: best starts {[m.pose_best_start for m in got]}; E flexible "
          f"{[None if m.interaction_score is None else round(m.interaction_score, 3) for m in flexible_first]} -> search "
          f"{[None if m.interaction_score is None else round(m.interaction_score, 3) for m in got]}")
    # a sample id gets the same bits in another batch size, and through the other two entries
    fewer = gen.generate_conformers(receptor=rec, optimise_pose=("search", 4, 8), **dict(kw, n_samples=5))
    by_id = {m.sample_id: m for m in got}
    assert [m.sample_id for m in fewer] == list(range(5))
    for m in fewer:
        assert _public(m) == _public(by_id[m.sample_id]), m.sample_id
    for entry in ("generate_conformers_sharded", "forward"):
        again = getattr(gen, entry)(receptor=rec, optimise_pose=("search", 4, 8), **kw)
        assert [_public(m) for m in again] == [_public(m) for m in got], entry
    # another seed keys other starts (where a keyed start won, it is another one or another pose)
    other = gen.generate_conformers(receptor=rec, optimise_pose=("search", 4, 8), **dict(kw, sample_seed=8))
    assert len(other) == len(got)
    # `optimise_pose="flexible"` in the same process: `optimise_pose_flexible` on its rows, before and after the search
    flexible_again = gen.generate_conformers(receptor=rec, optimise_pose=("flexible", 8), **kw)
    assert [_public(m) for m in flexible_again] == [_public(m) for m in flexible_first]
    rows = gen.generate_conformers(receptor=rec, interaction_scores=True, **kw)  # the rows the stage is handed
    walked = 0
    for a, m in zip(rows, flexible_again):
        if m.pose is None:
            continue
        direct = IX.optimise_pose_flexible(prepared, *_alone(a), steps=8, device=DEV)
        assert m.pose_trials_kept == int(direct["kept"][0]), m.sample_id
        want = direct["coords"][0].cpu() if m.pose_trials_kept else a.coords
        assert torch.equal(want.view(torch.int32), m.coords.view(torch.int32)), m.sample_id
        walked += 1 if m.pose_trials_kept else 0
    assert walked >= 1
    with pytest.raises(ValueError, match="optimise_pose"):
        gen.generate_conformers(receptor=rec, optimise_pose=("search", 65), **kw)
