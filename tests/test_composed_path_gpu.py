"""The composed post-generation path on the MI355X ("Which coordinates and which graph each returned
value reads"): one `generate_conformers` call with `standardize`, `relax_geometry`, `overlay`, `refine_overlay`,
`receptor`, `relieve_clashes`, `shape_scores`, `pharmacophore_scores`, `chemical_scores` and `add_hydrogens` all on, over
the known molecules of `composed_cases` injected at the sampler and write-back seams.  Every value of every returned
record is recomputed from the record's OWN coordinates and graph through the stage restatements, at the tolerance the
stage's own GPU test states for it - this file introduces no number; then the independence of the options, the three
entries and the selection behind it.  `test_composed_path_host.py` shows, by the restatements alone, that the batch is
one these checks may judge by.

`_finish` is left as it is: with `standardize` a record's validity IS the standardisation's verdict, so it keeps every
record but the one the batch holds for it to drop (asserted).

`shape_tanimoto` is the score of `shape_scores` - the molecule's own principal frame in the best of four orientations,
whatever its pose - so it equals the Tanimoto of the coordinates AS PLACED only where the returned pose is that
alignment.  It is therefore held to the as-placed grid value in the same call without `refine_overlay` and
`relieve_clashes`, where the returned pose is that alignment on every row; in the call with all options it is held to a
stand-alone `shape_scores` of the returned coordinates, and how far it lies from the as-placed value there, and from the
other call's value (the frame's handedness follows the coordinates it is computed from), is printed."""
import dataclasses
import math
import struct

import numpy as np
import pytest
import torch

import composed_cases as CC
import fingerprint_ref as FR
import geometry_ref as GR
import pharmacophore_ref as PR
from ml_conformer_generator_amd import receptor as RC
from ml_conformer_generator_amd.handoff import Measured

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FIELDS = [f.name for f in dataclasses.fields(Measured)]
LEFT_OUT = dict(add_hydrogens=("hydrogen_coords", "hydrogen_parents", "hydrogens_unplaced", "receptor_hydrogen_clashes"),
                chemical_scores=("chemical_tanimoto", "graph_key"),
                pharmacophore_scores=("pharmacophore_tanimoto", "pharmacophore_matches"),
                shape_scores=("shape_tanimoto",))
_DONE = {}


def _options():
    ref_xyz, ref_graph = CC.reference()
    return dict(reference_conformer=ref_xyz, n_samples=len(CC.batch()), variance=2, optimise_geometry=False,
                standardize=True, relax_geometry=CC.RELAX_STEPS, overlay=True, refine_overlay=CC.REFINE_STEPS,
                receptor=CC.receptor(), relieve_clashes=True, shape_scores=True, pharmacophore_scores=True,
                chemical_scores=True, reference_graph=ref_graph, add_hydrogens=True)


def _setup(monkeypatch):
    gen, full, _ = CC.substituted(monkeypatch, CC.batch())
    return gen, full


def _call(monkeypatch, key, entry="generate_conformers", **change):
    """The records of the composed call with `change` applied to its options, computed once per `key`."""
    if key not in _DONE:
        gen, _ = _setup(monkeypatch)
        _DONE[key] = getattr(gen, entry)(**dict(_options(), **change))
    return _DONE[key]


def _word(v):
    """A value by its bits: floats as their fp64 bytes (a NaN equals itself), fp32 tensors as int32."""
    if v is None or isinstance(v, (int, bool, str)):
        return v
    if isinstance(v, float):
        return struct.pack("<d", v)
    if torch.is_tensor(v):
        v = v.contiguous()
        return (str(v.dtype), tuple(v.shape), (v.view(torch.int32) if v.dtype == torch.float32 else v).tolist())
    if isinstance(v, (list, tuple)):
        return [_word(x) for x in v]
    raise TypeError(type(v))


def _bits(m, without=()):
    """Every field of a record by its bits, in the style of `_fields` and `_measured` of the stage tests."""
    out = dict(sample_id=m.sample_id, batch_row=m.batch_row, valid=m.valid, atomic_numbers=m.atomic_numbers,
               coords=_word(m.coords), bond_orders=_word(m.bond_orders))
    for k in FIELDS:
        if k not in without:
            out[k] = _word(getattr(m, k) if k != "pose" else (None if m.pose is None else torch.cat([m.pose[0].reshape(9),
                                                                                                   m.pose[1]])))
    return out


def _graph(m):
    return list(m.atomic_numbers), [[int(v) for v in row] for row in m.bond_orders.tolist()], len(m.atomic_numbers)


def _placed_tanimoto(ref, mols):
    """[len(mols)]: the grid Tanimoto of each record's returned coordinates against the reference, as placed: the
    reference's row of `pairwise_shape_tanimoto` with the reference as row 0."""
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto
    n_ref = int(ref.shape[0])
    x = torch.zeros(len(mols) + 1, max([n_ref] + [len(m.atomic_numbers) for m in mols]), 3)
    x[0, :n_ref] = ref
    for b, m in enumerate(mols):
        x[b + 1, : len(m.atomic_numbers)] = m.coords
    n = torch.tensor([n_ref] + [len(m.atomic_numbers) for m in mols], dtype=torch.int32)
    return pairwise_shape_tanimoto(ref, x, n, DEV).cpu()


class _Worst:
    """The worst error over tolerance per value, printed in the style of the `RELIEF e2e:` lines."""

    def __init__(self):
        self.seen = {}

    def __call__(self, name, err, tol, what):
        ratio = (0.0 if err == 0 else math.inf) if tol == 0 else err / tol
        if ratio >= self.seen.get(name, (-1.0,))[0]:
            self.seen[name] = (ratio, err, tol)
        assert err <= tol, (name, what, err, tol)

    def report(self):
        for name, (ratio, err, tol) in self.seen.items():
            print(f"COMPOSED e2e: {name}: worst error {err:.3e} of tolerance {tol:.3e} ({ratio:.3f})")


def test_every_record_of_the_call_with_all_options_describes_its_own_coordinates_and_graph(monkeypatch):
    from test_hydrogens_gpu import TOL as H_TOL
    from test_receptor_gpu import _restate
    from test_shape_diversity_gpu import REF_ROW_ATOL
    from test_shape_overlay_gpu import _reference_transform
    from oracle.shape_oracle import tanimoto_score as oracle_tanimoto
    from ml_conformer_generator_amd import geometry
    from ml_conformer_generator_amd.cheminformatics import shape_scores

    gen, full = _setup(monkeypatch)
    items, std_ref = CC.batch(), CC.standardized()
    ref_xyz, ref_graph = CC.reference()
    rec_xyz, rec_z = CC.receptor()
    refined = []
    real_pose = gen._pose

    def pose(*a, **k):                                # which rows' refined pose replaced the start, by batch row
        ov = real_pose(*a, **k)
        refined.append(ov["refined"].cpu().tolist() if "refined" in ov else None)
        return ov
    monkeypatch.setattr(gen, "_pose", pose)
    plain = gen.generate_conformers(**dict(_options(), relieve_clashes=False))      # the same call without the relief
    start = gen.generate_conformers(**dict(_options(), relieve_clashes=False, refine_overlay=False))   # ... and unrefined
    refined.clear()
    got = gen.generate_conformers(**_options())
    lb = gen.last_batch
    _DONE["all"], _DONE["no relief"] = got, plain
    assert len(refined) == 1

    kept_rows = [b for b, it in enumerate(items) if std_ref[it["name"]]["status"] == 0]
    dropped = [it["name"] for it in items].index(CC.DROPPED)
    assert [m.sample_id for m in got] == kept_rows == [m.batch_row for m in got]     # the dropped row is absent ...
    assert dropped not in kept_rows and [m.sample_id for m in got][dropped:] == list(range(dropped + 1, len(items)))
    assert [m.sample_id for m in plain] == kept_rows == [m.sample_id for m in start] and all(m.valid for m in got)
    assert gen.last_valid_fraction == len(kept_rows) / len(items)

    # the relaxation, stand-alone, of the standardised tensors: every row, every bit
    std = lb["standardized"]
    assert std["status"].cpu().tolist() == [std_ref[it["name"]]["status"] for it in items]
    alone = geometry.relax_geometry(std["coords"], std["atomic_numbers"], std["bond_orders"], std["n_nodes"], CC.RELAX_STEPS,
                                    DEV, check=False)
    assert torch.equal(alone["coords"].view(torch.int32), lb["x_relaxed"].view(torch.int32))
    x_std, x_rel = std["coords"].cpu(), lb["x_relaxed"].cpu()

    y_r, M_r, t_r = _reference_transform(ref_xyz)
    placed, placed_start = _placed_tanimoto(ref_xyz, got)[0, 1:], _placed_tanimoto(ref_xyz, start)[0, 1:]
    n_max = max(len(m.atomic_numbers) for m in got)
    xs = torch.zeros(len(got), n_max, 3)
    for k, m in enumerate(got):
        xs[k, : len(m.atomic_numbers)] = m.coords
    own_scores = shape_scores(ref_xyz, xs, torch.tensor([len(m.atomic_numbers) for m in got], dtype=torch.int32), DEV)[0].cpu()
    fr = CC.reference_features()
    ref_bits = FR.fingerprint(ref_graph[0], ref_graph[1].tolist(), len(ref_graph[0]))
    worst = _Worst()
    n_moved = n_still = n_matched = n_hydrogens = n_relaxed = 0
    off_pose = off_call = 0.0
    for k, (m, p) in enumerate(zip(got, plain)):
        b, name = m.sample_id, items[m.sample_id]["name"]
        want, n = std_ref[name], len(m.atomic_numbers)
        mol = _graph(m)

        # ---- the standardisation: the restatement of the injected graph, and the injected coordinates at its atom map
        assert (m.atom_map, m.atoms_removed, m.n_fragments) == (want["atom_map"], want["atoms_removed"], want["n_fragments"]), name
        assert m.atomic_numbers == want["atomic_numbers"] and m.bond_orders.tolist() == want["bond_orders"], name
        assert m.kekule_bond_orders.tolist() == want["kekule_orders"], name
        assert torch.equal(x_std[b, :n].view(torch.int32), full["xyz"][b, want["atom_map"]].view(torch.int32)), name
        assert not x_std[b, n:].any() and not x_rel[b, n:].any()

        # ---- the strain energies: the parent's topology, at the standardised and at the relaxed coordinates (rule a)
        topo = GR.topology(*mol[:2])
        for field, x in (("strain_before", x_std[b, :n]), ("strain_after", x_rel[b, :n])):
            ev = GR.evaluate(x.numpy(), x_std[b, :n].numpy(), topo)
            ok, ratio, _ = GR.rule_a(getattr(m, field), ev["grad"], ev)
            worst(field, abs(getattr(m, field) - ev["E"]), GR.C_A * GR.U32 * ev["S_E"], name)
            assert ok, (name, field, ratio)
        assert m.strain_after <= m.strain_before
        n_relaxed += m.strain_after < m.strain_before

        # ---- the pose: from the relaxed coordinates to the returned ones
        if m.pose is None:
            assert torch.equal(m.coords.view(torch.int32), x_rel[b, :n].view(torch.int32)), name
            assert m.relief_rmsd is None and m.receptor_clashes is None and m.receptor_clashes_before is None
            assert m.pharmacophore_tanimoto is None and m.receptor_hydrogen_clashes is None
        else:
            R, t = m.pose
            worst("pose", float((m.coords.double() - (x_rel[b, :n].double() @ R.double() + t.double())).abs().max()), 2e-4, name)
            worst("det R", abs(float(torch.det(R.double())) - 1.0), 1e-5, name)

            # ---- the shape values, at the returned coordinates
            worst("overlay_tanimoto vs placed grid", abs(m.overlay_tanimoto - float(placed[k])), REF_ROW_ATOL, name)
            y = ((m.coords.double() - t_r.double()) @ M_r.double()).to(torch.float32)
            worst("overlay_tanimoto vs fp64 oracle", abs(m.overlay_tanimoto - oracle_tanimoto(y_r, y)), 2e-4, name)
            moved = not torch.equal(m.coords, p.coords)
            s0 = start[k]
            y0 = ((s0.coords.double() - t_r.double()) @ M_r.double()).to(torch.float32)
            worst("shape_tanimoto vs placed grid, unrefined call", abs(s0.shape_tanimoto - float(placed_start[k])), REF_ROW_ATOL, name)
            worst("shape_tanimoto vs fp64 oracle, unrefined call", abs(s0.shape_tanimoto - oracle_tanimoto(y_r, y0)), 2e-4, name)
            off_pose = max(off_pose, abs(m.shape_tanimoto - float(placed[k])))
            off_call = max(off_call, abs(m.shape_tanimoto - s0.shape_tanimoto))

            # ---- the receptor: bit for bit at the returned coordinates; the relief against the call without it
            over = _restate(m.coords[None].numpy(), np.array([m.atomic_numbers]), [n], rec_xyz.numpy(), rec_z.numpy())[0]
            assert m.receptor_clashes == int((over >= np.float32(RC.CLASH_OVERLAP)).sum()), name
            assert m.receptor_max_overlap == float(over.max()), name
            assert m.receptor_clashes <= m.receptor_clashes_before == p.receptor_clashes, name
            assert (m.relief_rmsd > 0) == moved, name
            rmsd = float(((m.coords.double() - p.coords.double()) ** 2).sum(1).mean().sqrt())
            assert m.relief_rmsd == pytest.approx(rmsd, rel=1e-3, abs=1e-5), name
            worst("relief_rmsd", abs(m.relief_rmsd - rmsd), 1e-3 * rmsd + 1e-5, name)
            n_moved += moved
            n_still += not moved

            # ---- the pharmacophore: the reference's features against the returned coordinates and the parent's graph
            ph = PR.score(fr, m.coords.numpy(), *mol)
            worst("pharmacophore_tanimoto", abs(m.pharmacophore_tanimoto - ph["tanimoto"]), PR.SCORE_C * PR.EPS32, name)
            assert m.pharmacophore_matches == ph["matches"], (name, m.pharmacophore_matches, ph["matches"])
            n_matched += m.pharmacophore_matches > 0
        worst("shape_tanimoto vs shape_scores alone", abs(m.shape_tanimoto - float(own_scores[k])), 2e-4, name)

        # ---- the chemistry: the parent's graph, exactly
        bits, key = FR.fingerprint_and_key(*mol)
        assert m.graph_key == key, name
        assert np.float32(m.chemical_tanimoto).view(np.uint32) == FR.tanimoto(bits, ref_bits).view(np.uint32), name

        # ---- the hydrogens: the parent's graph at the returned coordinates, under the conditions of the tolerance
        h = CC.hydrogen_conditions(mol, m.coords.numpy(), name)
        assert m.hydrogen_parents == h["parents"] and m.hydrogens_unplaced == h["unplaced"], name
        assert tuple(m.hydrogen_coords.shape) == (h["n_hydrogens"], 3), name
        if h["n_hydrogens"]:
            worst("hydrogen_coords", float(np.abs(m.hydrogen_coords.numpy().astype(np.float64) - h["coords"]).max()), H_TOL, name)
        if any(c > 0 for c in h["nh"]):
            assert h["n_hydrogens"] > 0 and len(m.hydrogen_parents) > 0, name         # an H-bearing atom: hydrogens
            n_hydrogens += 1
        if m.pose is not None:
            nh = h["n_hydrogens"]
            over = _restate(m.hydrogen_coords[None].numpy(), np.ones((1, nh), dtype=np.int64), [nh], rec_xyz.numpy(),
                            rec_z.numpy())[0] if nh else np.zeros(0, dtype=np.float32)
            assert m.receptor_hydrogen_clashes == int((over >= np.float32(RC.CLASH_OVERLAP)).sum()), name
    worst.report()
    print(f"COMPOSED e2e: shape_tanimoto lies up to {off_pose:.3e} from the as-placed grid value of the refined, relieved pose "
          f"and up to {off_call:.3e} from its value in the unrefined call")
    print(f"COMPOSED e2e: {len(got)} records; clashes {[m.receptor_clashes_before for m in got]} -> "
          f"{[m.receptor_clashes for m in got]}; refined {[bool(refined[0][m.sample_id]) for m in got]}; pharmacophore "
          f"matches {[m.pharmacophore_matches for m in got]}; hydrogens {[len(m.hydrogen_parents) for m in got]}")

    # ---- coverage: the call measured something
    assert sum(1 for m in got if m.atoms_removed > 0) >= 2
    assert n_moved >= 2 and n_still >= 1 and n_matched >= 1
    assert n_hydrogens >= 10 and n_relaxed >= 8
    assert float(RC.vdw_radius(1)) == 1.20                                        # hydrogen's radius in the restatement


def _all(monkeypatch):
    return _call(monkeypatch, "all")


@pytest.mark.parametrize("option", list(LEFT_OUT))
def test_an_option_left_out_changes_no_bit_of_the_other_values(monkeypatch, option):
    full = _all(monkeypatch)
    less = _call(monkeypatch, "without " + option, **{option: False})
    assert len(less) == len(full)
    for a, b in zip(full, less):
        assert all(getattr(b, k) is None for k in LEFT_OUT[option]), (option, a.sample_id)
        assert any(getattr(a, k) is not None for k in LEFT_OUT[option]), (option, a.sample_id)
        assert _bits(a, LEFT_OUT[option]) == _bits(b, LEFT_OUT[option]), (option, a.sample_id)


@pytest.mark.parametrize("entry", ["generate_conformers_sharded", "forward"])
def test_the_three_entries_return_the_same_records(monkeypatch, entry):
    full = _all(monkeypatch)
    other = _call(monkeypatch, entry, entry=entry)
    assert [_bits(m) for m in other] == [_bits(m) for m in full]


def _restated_selection(mols, shape_pair, chem_pair, max_clashes, min_pharm, t_shape, t_chem, top_k):
    """`postprocess.select`'s docstring in plain Python, for the options of the selection test: positions into `mols`,
    in the order the call returns them."""
    def rank(i):
        s = mols[i].shape_tanimoto + mols[i].pharmacophore_tanimoto                  # rank_by="combo"
        return (-s if s == s else math.inf, mols[i].sample_id)
    rows = [i for i, m in enumerate(mols) if m.receptor_clashes is not None and m.receptor_clashes <= max_clashes]
    stages = [list(rows)]
    rows = [i for i in rows if mols[i].pharmacophore_tanimoto is not None and mols[i].pharmacophore_tanimoto >= min_pharm]
    stages.append(list(rows))
    first = {}
    for i in sorted(rows, key=rank):
        first.setdefault(mols[i].graph_key, i)
    rows = [i for i in rows if first[mols[i].graph_key] == i]
    stages.append(list(rows))
    kept = []
    for i in sorted(rows, key=rank):
        if top_k is not None and len(kept) >= top_k:
            break
        if not any((t_shape is not None and shape_pair[i][j] >= t_shape) or (t_chem is not None and chem_pair[i][j] >= t_chem)
                   for j in kept):
            kept.append(i)
    return kept, stages


def test_the_selection_reads_the_rows_it_returns(monkeypatch):
    from test_shape_diversity_gpu import PAIR_ATOL
    from ml_conformer_generator_amd.cheminformatics import pairwise_shape_tanimoto
    mols = _all(monkeypatch)
    ref_xyz, _ = CC.reference()
    B = len(mols)
    shape_pair = _placed_tanimoto(ref_xyz, mols)[1:, 1:].double().numpy()
    prints = [FR.fingerprint(*_graph(m)) for m in mols]
    chem_pair = np.array([[float(FR.tanimoto(prints[i], prints[j])) for j in range(B)] for i in range(B)])

    # thresholds from the records of the call without a selection, each between two of the values it is compared with
    clashes = sorted({m.receptor_clashes for m in mols if m.receptor_clashes is not None})
    max_clashes = clashes[-2] if len(clashes) > 1 else clashes[0]
    rows = [i for i, m in enumerate(mols) if m.receptor_clashes is not None and m.receptor_clashes <= max_clashes]
    assert len(rows) < B
    pharm = sorted({mols[i].pharmacophore_tanimoto for i in rows})
    min_pharm = (pharm[0] + pharm[1]) / 2
    assert all(abs(mols[i].pharmacophore_tanimoto - min_pharm) > PR.SCORE_C * PR.EPS32 for i in rows)
    _, stages = _restated_selection(mols, shape_pair, chem_pair, max_clashes, min_pharm, None, None, None)
    left = stages[-1]
    assert len(stages[1]) < len(stages[0]) and len(left) < len(stages[1])          # the filter, then `unique`, remove a row
    off = sorted({float(shape_pair[i][j]) for i in left for j in left if i < j})
    t_shape = (off[-1] + off[-2]) / 2
    assert all(abs(v - t_shape) > PAIR_ATOL for v in off), (off, t_shape)
    off = sorted({float(chem_pair[i][j]) for i in left for j in left if i < j})
    t_chem = (off[-1] + off[-2]) / 2
    assert all(abs(v - t_chem) > 0 for v in off)
    only_shape = _restated_selection(mols, shape_pair, chem_pair, max_clashes, min_pharm, t_shape, None, None)[0]
    only_chem = _restated_selection(mols, shape_pair, chem_pair, max_clashes, min_pharm, None, t_chem, None)[0]
    both = _restated_selection(mols, shape_pair, chem_pair, max_clashes, min_pharm, t_shape, t_chem, None)[0]
    assert len(only_shape) < len(left) and len(only_chem) < len(left) and len(both) >= 4
    top_k = len(both) - 1
    want = _restated_selection(mols, shape_pair, chem_pair, max_clashes, min_pharm, t_shape, t_chem, top_k)[0]
    assert len(want) == top_k >= 3

    gen, _ = _setup(monkeypatch)
    seen = {}
    real_pair, real_chem = gen._pair, gen._chem_pair

    def pair(ref, x, n):
        seen["pair"] = (x.cpu(), n.cpu().tolist())
        return real_pair(ref, x, n)

    def chem(fp):
        seen["chem"] = real_chem(fp).cpu()
        return seen["chem"]
    monkeypatch.setattr(gen, "_pair", pair)
    monkeypatch.setattr(gen, "_chem_pair", chem)
    got = gen.generate_conformers(max_receptor_clashes=max_clashes, min_pharmacophore_tanimoto=min_pharm, unique=True,
                                  max_pairwise_tanimoto=t_shape, max_pairwise_chemical_tanimoto=t_chem, top_k=top_k,
                                  rank_by="combo", **_options())
    print(f"COMPOSED select: of {B} records {len(stages[0])} pass max_receptor_clashes={max_clashes}, {len(stages[1])} "
          f"min_pharmacophore_tanimoto={min_pharm:.4f}, {len(left)} unique, {len(only_shape)} / {len(only_chem)} the walk at "
          f"{t_shape:.4f} / {t_chem:.4f} alone, {len(both)} both, top_k={top_k}: {[m.sample_id for m in got]}")
    assert [m.sample_id for m in got] == [mols[i].sample_id for i in want]
    assert [_bits(m) for m in got] == [_bits(mols[i]) for i in want]                # and they are the records of that call
    # the pair matrices were taken from the rows that survived the filters: their coordinates, their graphs
    x, n = seen["pair"]
    assert n == [len(mols[i].atomic_numbers) for i in left]
    for r, i in enumerate(left):
        assert torch.equal(x[r, : n[r]].view(torch.int32), mols[i].coords.contiguous().view(torch.int32)), mols[i].sample_id
    assert np.array_equal(seen["chem"].numpy().astype(np.float64), chem_pair[np.ix_(left, left)])
    own = pairwise_shape_tanimoto(ref_xyz, x, torch.tensor(n, dtype=torch.int32), DEV).cpu().double().numpy()
    assert float(np.abs(own - shape_pair[np.ix_(left, left)]).max()) == 0.0       # the same bits whatever the batch
