"""The composed post-generation path on the MI355X for the option families added behind `test_composed_path_gpu.py`
("Which coordinates and which graph each returned value reads"), over the known molecules of
`composed_late_cases` injected at the sampler and write-back seams.

Call A turns on every option that can share a call - the first ten, `electrostatic_scores`, `partial_charges`,
`smiles="isomeric"`, the three substructure options, `interaction_scores` and `optimise_pose=("flexible", n)` - and is made
three more times with the rigid walk, without the walk, and without the walk and the relief: those give the earlier
coordinate sets of every row.  Every value of every record is recomputed from the record's OWN coordinates and graph
through the stage restatements at the tolerance, and under the preconditions, the stage's own GPU test states (this file
introduces no number); the two
walks are held bit for bit to a stand-alone launch on the records of the call without them; and for every value that
reads the returned coordinates the restatement is ALSO evaluated at the three earlier coordinate sets of the same row
(`x_relaxed`, the refined pose, the relieved pose) and must lie further than twice the tolerance from the restatement at
the returned ones on two rows (an integer: differ on one), so that a value computed from stale coordinates cannot pass.
The stereo fields are exempt from that last check, because no stage changes chirality: a rigid move keeps every signed
volume, and a torsion turns one whole side of a bond about it, which moves no neighbour of a centre relative to the
others.  What is asserted instead is that the descriptors are equal at all four coordinate sets.

The ring and scaffold fields come with `unique="scaffold"` / `"framework"` only, which cannot share call A (it removes
rows): they are held to the restatement in two calls of their own that keep the row whose parent sits behind a smaller
fragment, besides `scaffold.of_records` on call A's records and the selection test's calls.
`test_composed_late_host.py` shows, by the restatements alone, that the batch is one these checks may judge by."""
import copy
import dataclasses
import math

import numpy as np
import pytest
import torch

import canonical_ref as CR
import composed_cases as CC
import composed_late_cases as LC
import electrostatics_ref as ER
import fingerprint_ref as FR
import flex_pose_ref as FP
import geometry_ref as GR
import hydrogens_ref as HR
import interactions_ref as IR
import pharmacophore_ref as PR
import scaffold_ref as SFR
import stereo_ref as STR
import substructure_cases as SBC
from test_composed_path_gpu import _Worst, _bits, _graph, _placed_tanimoto, _word
from ml_conformer_generator_amd import interactions as IX
from ml_conformer_generator_amd import receptor as RC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_DONE = {}
UNWORDED = ("substructure_patterns", "interaction_terms")          # what `_bits` cannot spell: compared beside it
LEFT_OUT = dict(
    electrostatic_scores=(dict(electrostatic_scores=False), "all", ("electrostatic_tanimoto",)),
    partial_charges=(dict(partial_charges=False), "all", ("partial_charges", "hydrogen_charges")),
    smiles=(dict(smiles=False), "all", ("canonical_order", "canonical_status", "stereo_order", "stereo_status",
                                        "stereo_descriptors", "n_stereo_defined", "n_stereo_undefined")),
    substructure_counts=(dict(substructure_counts=None), "all", ("substructure_counts", "substructure_status",
                                                                 "substructure_first", "substructure_patterns")),
    interaction_scores=(dict(interaction_scores=False, optimise_pose=False), "relieved",
                        ("interaction_score", "interaction_terms", "receptor_hbonds", "interaction_atom_scores")),
    add_hydrogens=(dict(add_hydrogens=False), "all", ("hydrogen_coords", "hydrogen_parents", "hydrogens_unplaced",
                                                      "receptor_hydrogen_clashes")))
CHANGES = dict(all={}, rigid=dict(optimise_pose=LC.OPTIMISE_STEPS), relieved=dict(optimise_pose=False),
               refined=dict(optimise_pose=False, relieve_clashes=False))


def _options():
    ref_xyz, ref_graph = LC.reference()
    return dict(reference_conformer=ref_xyz, n_samples=len(LC.batch()), variance=2, optimise_geometry=False,
                standardize=True, relax_geometry=LC.RELAX_STEPS, overlay=True, refine_overlay=LC.REFINE_STEPS,
                receptor=LC.receptor(), relieve_clashes=LC.RELIEF_STEPS, shape_scores=True, pharmacophore_scores=True,
                chemical_scores=True, reference_graph=ref_graph, add_hydrogens=True, electrostatic_scores=True,
                partial_charges=True, smiles="isomeric", require_substructures=None, exclude_substructures=None,
                substructure_counts=LC.REQUIRE + LC.EXCLUDE + LC.COUNTS, interaction_scores=True,
                optimise_pose=("flexible", LC.OPTIMISE_STEPS), unique=False)


def _setup(monkeypatch):
    gen, full, _ = CC.substituted(monkeypatch, LC.batch(), width=LC.WIDTH)
    return gen, full


def _call(monkeypatch, key, entry="generate_conformers", **change):
    """The records of call A with `change` applied to its options, computed once per `key`."""
    if key not in _DONE:
        gen, _ = _setup(monkeypatch)
        _DONE[key] = getattr(gen, entry)(**dict(_options(), **dict(CHANGES.get(key, {}), **change)))
        if key == "all":
            _DONE["last_batch"] = {k: v.cpu() if torch.is_tensor(v) else {a: b.cpu() for a, b in v.items() if torch.is_tensor(b)}
                                   for k, v in gen.last_batch.items() if k in ("x_relaxed", "standardized")}
            _DONE["valid fraction"] = gen.last_valid_fraction
    return _DONE[key]


def _late_bits(m, without=()):
    """`_bits` of a record of call A: the two fields it cannot spell - a dict of floats, a tuple of patterns - beside it."""
    out = _bits(m, tuple(without) + UNWORDED)
    if "interaction_terms" not in without:
        t = m.interaction_terms
        out["interaction_terms"] = None if t is None else [(k, _word(float(v))) for k, v in sorted(t.items())]
    if "substructure_patterns" not in without:
        out["substructure_patterns"] = m.substructure_patterns
    out["smiles"] = m.smiles
    return out


def _copies(records):
    """Records that share the originals' tensors but carry values of their own."""
    out = []
    for m in records:
        c = copy.copy(m)
        c._measured = dataclasses.replace(m._measured)
        out.append(c)
    return out


def _xyz(x):
    return [tuple(float(v) for v in p) for p in np.asarray(x, dtype=np.float64)]


class _Context:
    """What the restatements of one call share: the receptor as the kernels walk it, the reference's features and charge
    points."""

    def __init__(self, h_tol, rec=None):
        """`h_tol`: the hydrogens' tolerance (`test_hydrogens_gpu.TOL`); `rec`: another receptor than call A's (a pocket's
        own) - the reference's values are then left out."""
        self.h_tol = h_tol
        from ml_conformer_generator_amd import electrostatics as ES
        from ml_conformer_generator_amd import hydrogens as HY
        from test_shape_overlay_gpu import _reference_transform
        self.rec = LC.receptor() if rec is None else rec
        self.prepared = IX.prepare_receptor(self.rec)
        self.y, self.rj, self.tj = (self.prepared.xyzr[:, :3].numpy(), self.prepared.xyzr[:, 3].numpy(),
                                    self.prepared.types.numpy())
        if rec is not None:
            return
        self.ref_xyz, self.ref_graph = LC.reference()
        self.fr = CC.reference_features()
        self.frame = _reference_transform(self.ref_xyz)
        # the reference's charge points as the product makes them: its own charge and placement kernels on the reference
        z, adj = self.ref_graph
        zz, nn = torch.tensor([list(z)], dtype=torch.int32), torch.tensor([len(z)], dtype=torch.int32)
        ch = ES.partial_charges(zz, adj[None], nn, DEV)
        pts, q, count = ES.charge_points(self.ref_xyz[None].to(DEV), ch, HY.add_hydrogens(self.ref_xyz[None], zz, adj[None], nn, DEV))
        k = int(count[0])
        self.ref_points = (pts[0, :k].cpu().double().numpy(), q[0, :k].cpu().double().numpy())

    def clashes(self, x, z):
        from test_receptor_gpu import _restate
        x = np.asarray(x, dtype=np.float32)
        if not len(x):
            return 0, -math.inf
        over = _restate(x[None], np.array([z]), [len(z)], np.asarray(self.rec[0]), np.asarray(self.rec[1]))[0]
        return int((over >= np.float32(RC.CLASH_OVERLAP)).sum()), float(over.max())

    def interaction_args(self, mol, x):
        z = mol[0]
        return (np.asarray(x, dtype=np.float32), IR.radii(z), IR.ligand_types(*mol, PR.perceive(*mol)[0]), self.y, self.rj,
                self.tj, IR.rotatable_bonds(*mol))

    def placed_oracle(self, x):
        from oracle.shape_oracle import tanimoto_score
        y_r, M_r, t_r = self.frame
        return tanimoto_score(y_r, ((torch.as_tensor(x).double() - t_r.double()) @ M_r.double()).to(torch.float32))

    def readers(self, mol, x, charges, placed=None):
        """name -> (value, tolerance or None for an integer) of every value that reads the coordinates, restated at `x`
        [n,3] fp32 on the parent graph `mol`; `charges`: the record's own (q, q_h); `placed`: hydrogens to use in place of
        the restatement's own placement at `x` (the record's own, at the returned coordinates)."""
        x = np.asarray(x, dtype=np.float32)
        z, n = mol[0], mol[2]
        h = HR.place(*mol, x)
        ph = PR.score(self.fr, x, *mol)
        args = self.interaction_args(mol, x)
        sc, bd = IR.score(*args), IR.bounds(*args)
        cl, worst = self.clashes(x, z)
        hx = np.asarray(h["coords"] if placed is None else placed["coords"], dtype=np.float64).reshape(-1, 3)
        hcl = self.clashes(hx, [1] * len(hx))[0]
        ch = dict(q=charges[0], q_h=charges[1], nh=HR.counts(*mol))
        es = ER.score(self.ref_points, ER.points(n, x, ch, h if placed is None else placed))
        return dict(hydrogen_coords=(np.asarray(h["coords"], dtype=np.float64).reshape(-1, 3), self.h_tol),
                    receptor_hydrogen_clashes=(hcl, None),
                    pharmacophore_tanimoto=(ph["tanimoto"], PR.SCORE_C * PR.EPS32), pharmacophore_matches=(ph["matches"], None),
                    interaction_score=(sc["score"], bd["score"]), interaction_terms=(sc["terms"], bd["terms"]),
                    interaction_atom_scores=(sc["atom_scores"], bd["atom_scores"]), receptor_hbonds=(sc["hbonds"], None),
                    electrostatic_tanimoto=(es["tanimoto"], es["tol_tanimoto"]),
                    receptor_clashes=(cl, None), receptor_max_overlap=(worst, 0.0),
                    overlay_tanimoto=(self.placed_oracle(x), 2e-4)), h


def _gap(a, b, tol):
    """How far two restated values lie apart, in units of the tolerance (inf where the tolerance is 0 and they differ)."""
    a, b, tol = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    if a.shape != b.shape:
        return math.inf
    d = np.abs(a - b)
    r = np.divide(d, tol, out=np.where(d > 0, np.inf, 0.0), where=tol > 0)
    return float(r.max()) if r.size else 0.0


def _standalone(records, flexible):
    """`interactions.optimise_pose` / `optimise_pose_flexible` alone on the records of the call without the walk: host
    tensors by record position."""
    W = LC.WIDTH
    B = len(records)
    x, z, bonds = torch.zeros(B, W, 3), torch.zeros(B, W, dtype=torch.int32), torch.zeros(B, W, W, dtype=torch.int8)
    n = torch.tensor([len(m.atomic_numbers) for m in records], dtype=torch.int32)
    for b, m in enumerate(records):
        k = int(n[b])
        x[b, :k], z[b, :k], bonds[b, :k, :k] = m.coords, torch.tensor(m.atomic_numbers, dtype=torch.int32), m.bond_orders
    walk = IX.optimise_pose_flexible if flexible else IX.optimise_pose
    return {k: v.cpu() for k, v in walk(LC.receptor(), x, n, z, bonds, LC.OPTIMISE_STEPS, device=DEV).items()}


def test_every_record_of_call_a_describes_its_own_coordinates_and_graph(monkeypatch):
    from test_hydrogens_gpu import TOL as H_TOL
    from test_shape_diversity_gpu import REF_ROW_ATOL
    from ml_conformer_generator_amd.cheminformatics import shape_scores

    got, rigid = _call(monkeypatch, "all"), _call(monkeypatch, "rigid")
    relieved, refined = _call(monkeypatch, "relieved"), _call(monkeypatch, "refined")
    _, full = _setup(monkeypatch)
    lb = _DONE["last_batch"]
    items, std_ref = LC.batch(), LC.standardized()
    ctx = _Context(H_TOL)
    kept_rows = [b for b, it in enumerate(items) if std_ref[it["name"]]["status"] == 0]
    dropped = [it["name"] for it in items].index(LC.DROPPED)
    for call in (got, rigid, relieved, refined):
        assert [m.sample_id for m in call] == kept_rows == [m.batch_row for m in call] and all(m.valid for m in call)
    assert dropped not in kept_rows and _DONE["valid fraction"] == len(kept_rows) / len(items)
    x_std, x_rel = lb["standardized"]["coords"], lb["x_relaxed"]

    flex_alone, rigid_alone = _standalone(relieved, True), _standalone(relieved, False)
    placed = _placed_tanimoto(ctx.ref_xyz, got)[0, 1:]
    n_max = max(len(m.atomic_numbers) for m in got)
    xs = torch.zeros(len(got), n_max, 3)
    for k, m in enumerate(got):
        xs[k, : len(m.atomic_numbers)] = m.coords
    counts_n = torch.tensor([len(m.atomic_numbers) for m in got], dtype=torch.int32)
    own_scores = shape_scores(ctx.ref_xyz, xs, counts_n, DEV)[0].cpu()
    shape_at = {}                                     # `shape_scores` alone at the earlier coordinate sets, for the stale check
    for label, rows in (("x_relaxed", [x_rel[m.batch_row, : len(m.atomic_numbers)] for m in got]),
                        ("refined", [m.coords for m in refined]), ("relieved", [m.coords for m in relieved])):
        xe = torch.zeros_like(xs)
        for k, x in enumerate(rows):
            xe[k, : x.shape[0]] = x
        shape_at[label] = shape_scores(ctx.ref_xyz, xe, counts_n, DEV)[0].cpu()

    worst = _Worst()
    stale = {}                                        # (field, earlier set) -> the gaps of the posed rows, in tolerances
    count = dict(relief=0, still=0, walked=0, unwalked=0, rigid_walked=0, rigid_unwalked=0, turned=0, posed=0)
    for k, (m, r, p, q) in enumerate(zip(got, rigid, relieved, refined)):
        b, name = m.sample_id, items[m.sample_id]["name"]
        want, n = std_ref[name], len(m.atomic_numbers)
        mol = _graph(m)

        # ---- the standardisation and the relaxation, as in the first composed test
        assert (m.atom_map, m.atoms_removed, m.n_fragments) == (want["atom_map"], want["atoms_removed"], want["n_fragments"]), name
        assert m.atomic_numbers == want["atomic_numbers"] and m.bond_orders.tolist() == want["bond_orders"], name
        assert torch.equal(x_std[b, :n].view(torch.int32), full["xyz"][b, want["atom_map"]].view(torch.int32)), name
        topo = GR.topology(*mol[:2])
        ev = GR.evaluate(x_rel[b, :n].numpy(), x_std[b, :n].numpy(), topo)               # item 5: `strain_after` keeps describing
        worst("strain_after at x_relaxed", abs(m.strain_after - ev["E"]), GR.C_A * GR.U32 * ev["S_E"], name)     # x_relaxed
        assert GR.rule_a(m.strain_after, ev["grad"], ev)[0], name

        # (the product poses the rows of one and of two atoms too - a translation, a line on a line -, so every record of
        #  this batch carries every value; a record without a pose would fail on the next lines)
        assert m.pose is not None and r.pose is not None, name
        count["posed"] += 1

        # ---- item 1: the two walks, bit for bit a stand-alone launch on the record of the call without them
        for rec_m, alone, flexible in ((m, flex_alone, True), (r, rigid_alone, False)):
            kept = int(alone["kept"][k])
            assert rec_m.pose_trials_kept == kept >= 0, name
            moved_bits = alone["coords"][k, :n] if kept else p.coords
            assert torch.equal(rec_m.coords.contiguous().view(torch.int32), moved_bits.contiguous().view(torch.int32)), name
            assert np.float32(rec_m.interaction_score_before) == np.float32(p.interaction_score), name
            assert flexible or rec_m.interaction_score <= rec_m.interaction_score_before, name      # (flexible: W + 0.840 CLASH)
            if kept == 0:
                assert rec_m.interaction_score == rec_m.interaction_score_before and rec_m.pose_optimisation_rmsd == 0.0, name
            if flexible:
                used = int(alone["torsions"][k])
                tree = FP.tree(*mol)
                assert rec_m.pose_torsions == used == tree["used"], name
                assert alone["torsion_atoms"][k, :used].tolist() == [list(t) for t in tree["torsions"]], name
                angles = alone["torsion_angles"][k, :used].tolist() if kept else [0.0] * used
                assert [_word(v) for v in rec_m.pose_torsion_angles] == [_word(v) for v in angles], name
                for field, col in (("pose_conformer_rmsd", "conformer_rmsd"), ("intramolecular_clash_before", "clash_before"),
                                   ("intramolecular_clash", "clash_after")):
                    v = float(alone[col][k]) if kept or col == "clash_before" else (0.0 if col == "conformer_rmsd" else
                                                                                     float(alone["clash_before"][k]))
                    assert _word(getattr(rec_m, field)) == _word(v), (name, field)
            else:
                assert all(getattr(rec_m, f) is None for f in ("pose_torsions", "pose_torsion_angles", "pose_conformer_rmsd",
                                                               "intramolecular_clash_before", "intramolecular_clash")), name
        if m.pose_torsions == 0:                      # a row without a torsion: the rigid walk's bits
            skip = ("pose_torsions", "pose_torsion_angles", "pose_conformer_rmsd", "intramolecular_clash_before",
                    "intramolecular_clash")
            assert _late_bits(m, skip) == _late_bits(r, skip), name
            assert m.pose_conformer_rmsd == 0.0 and m.pose_torsion_angles == [], name
        # `pose` composes from x_relaxed: in the rigid call within the walk tests' 2e-4, in the flexible call up to the
        # conformer change, restated: the record's own summed turns applied to the relieved conformer by the restatement's
        # `twist`, within the walk's drift bound
        R, t = r.pose
        worst("pose, rigid call", float((r.coords.double() - (x_rel[b, :n].double() @ R.double() + t.double())).abs().max()), 2e-4, name)
        worst("det R", abs(float(torch.det(R.double())) - 1.0), 1e-5, name)
        R, t = m.pose
        dev = (m.coords.double() - (x_rel[b, :n].double() @ R.double() + t.double())).norm(dim=1).numpy()
        tree = FP.tree(*mol)
        q0 = p.coords.double().numpy() - p.coords.double().numpy().mean(0)
        turns = np.zeros(FP.MAX_TORSIONS)
        turns[: m.pose_torsions] = m.pose_torsion_angles
        turned = np.linalg.norm(FP.twist(q0, turns, tree) - q0, axis=1)
        bound = 2e-4 + FP.drift_bound(p.coords.numpy(), tree, m.pose_trials_kept)
        worst("pose, flexible call, up to the restated turn", float(np.abs(dev - turned).max()), bound, name)
        rms = float(np.sqrt((turned ** 2).mean()))
        worst("pose_conformer_rmsd vs the restated turn", abs(m.pose_conformer_rmsd - rms),       # `flex_pose_ref.check_trace`'s
              2 * FP.drift_bound(p.coords.numpy(), tree, m.pose_trials_kept) + 4 * FP.U * rms, name)      # rule for it
        count["walked"] += m.pose_trials_kept > 0
        count["unwalked"] += m.pose_trials_kept == 0
        count["rigid_walked"] += r.pose_trials_kept > 0
        count["rigid_unwalked"] += r.pose_trials_kept == 0
        count["turned"] += any(m.pose_torsion_angles)

        # ---- item 5: the values the table pins to earlier coordinates
        assert m.receptor_clashes_before == q.receptor_clashes == p.receptor_clashes_before, name
        rmsd = float(((p.coords.double() - q.coords.double()) ** 2).sum(1).mean().sqrt())
        worst("relief_rmsd", abs(m.relief_rmsd - rmsd), 1e-3 * rmsd + 1e-5, name)
        assert (m.relief_rmsd > 0) == (not torch.equal(p.coords, q.coords)) and m.relief_rmsd == p.relief_rmsd, name
        count["relief"] += m.relief_rmsd > 0
        count["still"] += m.relief_rmsd == 0
        walk_rmsd = float(((m.coords.double() - p.coords.double()) ** 2).sum(1).mean().sqrt())
        worst("pose_optimisation_rmsd", abs(m.pose_optimisation_rmsd - walk_rmsd), 1e-3 * walk_rmsd + 1e-5, name)

        # ---- item 2: the readers of the returned coordinates, each against its restatement at the record's own `coords`
        h = CC.hydrogen_conditions(mol, m.coords.numpy(), name)
        assert m.hydrogen_parents == h["parents"] and m.hydrogens_unplaced == h["unplaced"] == 0, name
        charges = (m.partial_charges.double().tolist(), m.hydrogen_charges.double().tolist())
        own_h = dict(coords=m.hydrogen_coords.double().numpy(), parents=m.hydrogen_parents, counts=h["counts"])
        at, _ = ctx.readers(mol, m.coords.numpy(), charges, placed=own_h)
        restated = dict(at, hydrogen_coords=(np.asarray(h["coords"], dtype=np.float64).reshape(-1, 3), H_TOL))
        terms = np.array([m.interaction_terms[t] for t in IR.TERMS])
        have = dict(hydrogen_coords=m.hydrogen_coords.double().numpy(), receptor_hydrogen_clashes=m.receptor_hydrogen_clashes,
                    pharmacophore_tanimoto=m.pharmacophore_tanimoto, pharmacophore_matches=m.pharmacophore_matches,
                    interaction_score=m.interaction_score, interaction_terms=terms,
                    interaction_atom_scores=m.interaction_atom_scores.double().numpy(), receptor_hbonds=m.receptor_hbonds,
                    electrostatic_tanimoto=m.electrostatic_tanimoto, receptor_clashes=m.receptor_clashes,
                    receptor_max_overlap=m.receptor_max_overlap, overlay_tanimoto=m.overlay_tanimoto,
                    shape_tanimoto=m.shape_tanimoto)
        assert m.interaction_terms["n_rot"] == IR.rotatable_bonds(*mol), name
        for field, (value, tol) in restated.items():
            if tol is None:
                assert have[field] == value, (name, field, have[field], value)
                worst(field, 0.0, 0.0, name)
            else:                                     # the worst error over its own tolerance, element by element
                ratio = _gap(have[field], value, tol)
                tol1 = float(np.max(tol)) if np.max(tol) > 0 else 0.0
                worst(field, ratio * tol1 if tol1 else (0.0 if ratio == 0 else math.inf), tol1, name)
        worst("overlay_tanimoto vs placed grid", abs(m.overlay_tanimoto - float(placed[k])), REF_ROW_ATOL, name)
        worst("shape_tanimoto vs shape_scores alone", abs(m.shape_tanimoto - float(own_scores[k])), 2e-4, name)
        assert tuple(m.hydrogen_coords.shape) == (h["n_hydrogens"], 3), name

        # ---- item 4: the same restatements at the row's three earlier coordinate sets
        for label, earlier in (("x_relaxed", x_rel[b, :n]), ("refined", q.coords), ("relieved", p.coords)):
            old, _ = ctx.readers(mol, earlier.numpy(), charges)
            for field, (value, tol) in at.items():
                if field == "hydrogen_coords":
                    value = restated[field][0]
                gap = float(value != old[field][0]) if tol is None else _gap(value, old[field][0], tol)
                stale.setdefault((field, label), []).append(gap)
            stale.setdefault(("shape_tanimoto", label), []).append(abs(float(own_scores[k]) - float(shape_at[label][k])) / 2e-4)
    worst.report()

    # ---- item 4, judged: per value and earlier set, two rows further than twice the tolerance (an integer: one row)
    integer = {f for f, (_, tol) in at.items() if tol is None}
    for field in list(at) + ["shape_tanimoto"]:
        gaps = {label: sorted(stale[(field, label)], reverse=True) for label in ("x_relaxed", "refined", "relieved")}
        if field in integer:
            print(f"COMPOSED e2e stale: {field}: differs on "
                  f"{ {label: int(sum(g)) for label, g in gaps.items()} } of {count['posed']} rows")
            assert all(sum(g) >= 1 for g in gaps.values()), (field, gaps)
        else:
            print(f"COMPOSED e2e stale: {field}: the second-largest gap is "
                  f"{ {label: round(g[1], 1) for label, g in gaps.items()} } tolerances (minimum {min(g[1] for g in gaps.values()):.1f})")
            assert all(g[1] > 2.0 for g in gaps.values()), (field, gaps)

    # ---- item 6: coverage.  The walk has no "left alone" half: the restatement started from the fp64 pose keeps no trial
    # on one row at this budget (the host file), but from the product's own relieved poses every row keeps one of its two
    # trials in either call, so the `kept == 0` branches above do not run on this batch (the stage tests hold them)
    print(f"COMPOSED e2e coverage: {len(got)} records, {count['posed']} posed; the relief moved {count['relief']} and left "
          f"{count['still']}; the flexible walk moved {count['walked']} and left {count['unwalked']}, the rigid walk moved "
          f"{count['rigid_walked']} and left {count['rigid_unwalked']}; {count['turned']} turned a torsion")
    assert count["relief"] >= 2 and count["still"] >= 1 and count["walked"] >= 2 and count["rigid_walked"] >= 2
    assert count["turned"] >= 2


@pytest.mark.parametrize("option", list(LEFT_OUT))
def test_an_option_left_out_changes_no_bit_of_the_other_values(monkeypatch, option):
    change, base, fields = LEFT_OUT[option]
    full = _call(monkeypatch, base)
    less = _call(monkeypatch, "without " + option, **dict(CHANGES[base], **change))
    assert len(less) == len(full)
    for a, b in zip(full, less):
        if option == "substructure_counts":           # no pattern left: the fields are gone
            assert all(getattr(b, k) is None for k in fields), (option, a.sample_id)
        elif option == "smiles":
            assert all(getattr(b._measured, k) is None for k in fields) and b.smiles is None, (option, a.sample_id)
        else:
            assert all(getattr(b, k) is None for k in fields), (option, a.sample_id)
        assert any(getattr(a, k) is not None for k in fields), (option, a.sample_id)
        left, right = _late_bits(a, fields), _late_bits(b, fields)
        if option == "smiles":
            left.pop("smiles"), right.pop("smiles")
        assert left == right, (option, a.sample_id)
        if option == "add_hydrogens":                 # ... the electrostatic score among them: placed once, either way
            assert _word(a.electrostatic_tanimoto) == _word(b.electrostatic_tanimoto), a.sample_id


@pytest.mark.parametrize("entry", ["generate_conformers_sharded", "forward"])
def test_the_three_entries_return_the_same_records(monkeypatch, entry):
    full = _call(monkeypatch, "all")
    other = _call(monkeypatch, entry, entry=entry)
    assert [_late_bits(m) for m in other] == [_late_bits(m) for m in full]


# ----------------------------------------------------------------------------------------------- the selection
UNIQUE_KINDS = ("exact", "stereo", "scaffold", "framework")


def _identity(m, kind):
    """The identity `unique=kind` groups a record by, through the restatements: the parent graph's, with the returned
    coordinates for "stereo"."""
    mol = _graph(m)
    if kind == "exact":
        return CR.identity_bytes(*mol)
    if kind == "stereo":
        return STR.identity_bytes(*mol, _xyz(m.coords))
    return SFR.identity(*mol, generic=kind == "framework")


def _restated_late_selection(mols, min_esp=None, max_e=None, n_required=0, n_excluded=0, excluded=(), unique=False,
                             rank_by="shape"):
    """`postprocess.select`'s docstring in plain Python for the later options, in its order: the electrostatic and the
    interaction threshold (None and NaN do not pass), the required and the excluded patterns (the first `n_required` and
    the next `n_excluded` of the record's patterns), `exclude_graphs` (`excluded`: exact identities), then `unique`: of the
    rows with one identity the first in ranking order.  Returns (positions into `mols` in the order the call returns
    them, the positions left behind every stage)."""
    def rank(i):
        m = mols[i]
        if rank_by == "interaction":
            s = math.nan if m.interaction_score is None else -m.interaction_score
        elif rank_by == "electrostatic":
            s = math.nan if m.electrostatic_tanimoto is None else m.shape_tanimoto + m.electrostatic_tanimoto
        else:
            s = m.shape_tanimoto
        return (-s if s == s else math.inf, m.sample_id)
    rows, stages = list(range(len(mols))), []
    if min_esp is not None:
        rows = [i for i in rows if mols[i].electrostatic_tanimoto is not None and mols[i].electrostatic_tanimoto >= min_esp]
        stages.append(list(rows))
    if max_e is not None:
        rows = [i for i in rows if mols[i].interaction_score is not None and mols[i].interaction_score <= max_e]
        stages.append(list(rows))
    if n_required or n_excluded:
        rows = [i for i in rows if all(mols[i].substructure_counts[p] >= 1 for p in range(n_required))]
        stages.append(list(rows))
        rows = [i for i in rows if not any(mols[i].substructure_counts[p] >= 1 for p in range(n_required, n_required + n_excluded))]
        stages.append(list(rows))
    if excluded:
        rows = [i for i in rows if _identity(mols[i], "exact") not in excluded]
        stages.append(list(rows))
    if unique:
        first = {}
        for i in sorted(rows, key=rank):
            first.setdefault(_identity(mols[i], unique), i)
        rows = [i for i in rows if first[_identity(mols[i], unique)] == i]
        stages.append(list(rows))
    return rows, stages


def _thresholds(mols, ctx):
    """(min_electrostatic_tanimoto, max_interaction_score) from call A's records: each midway between two of the values it
    separates and further than the value's own tolerance from both; the lower two electrostatic scores and, of what that
    leaves, the highest interaction score fall outside."""
    def tolerance(m, field):
        mol = _graph(m)
        h = HR.place(*mol, m.coords.numpy())
        own = dict(coords=m.hydrogen_coords.double().numpy(), parents=m.hydrogen_parents, counts=h["counts"])
        at, _ = ctx.readers(mol, m.coords.numpy(), (m.partial_charges.double().tolist(), m.hydrogen_charges.double().tolist()), own)
        return at[field][1]
    posed = sorted((m for m in mols if m.pose is not None), key=lambda m: m.electrostatic_tanimoto)
    assert all(m.electrostatic_tanimoto == m.electrostatic_tanimoto for m in posed)          # finite on every posed row
    a, b = posed[1], posed[2]
    min_esp = (a.electrostatic_tanimoto + b.electrostatic_tanimoto) / 2
    assert all(abs(m.electrostatic_tanimoto - min_esp) > tolerance(m, "electrostatic_tanimoto") for m in (a, b))
    left = sorted(posed[2:], key=lambda m: m.interaction_score)
    a, b = left[-2], left[-1]
    max_e = (a.interaction_score + b.interaction_score) / 2
    assert all(abs(m.interaction_score - max_e) > tolerance(m, "interaction_score") for m in (a, b))
    return min_esp, max_e


def test_the_selection_with_the_later_filters_reads_the_rows_it_returns(monkeypatch):
    from test_hydrogens_gpu import TOL as H_TOL
    from test_scaffold_gpu import _check_fields
    from ml_conformer_generator_amd import scaffold as SF
    mols = _call(monkeypatch, "all")
    by_id = {m.sample_id: m for m in mols}
    ctx = _Context(H_TOL)
    min_esp, max_e = _thresholds(mols, ctx)
    gen, _ = _setup(monkeypatch)
    options = dict(_options(), substructure_counts=LC.COUNTS)                 # the same patterns in the same order, now gates
    n_req, n_exc = len(LC.REQUIRE), len(LC.EXCLUDE)

    def check(got, want, without=()):
        assert [m.sample_id for m in got] == [mols[i].sample_id for i in want]
        for m in got:                                 # and they are the records of call A, bit for bit
            assert _late_bits(m, without) == _late_bits(by_id[m.sample_id], without), m.sample_id

    # ---- the two thresholds and each `unique` value in turn, under either of the two later rankings
    survivors = {}
    for rank_by in ("electrostatic", "interaction"):
        for kind in UNIQUE_KINDS:
            want, stages = _restated_late_selection(mols, min_esp, max_e, unique=kind, rank_by=rank_by)
            assert len(mols) > len(stages[0]) > len(stages[1]) > len(stages[2]) >= 2, (kind, [len(s) for s in stages])
            got = gen.generate_conformers(**dict(options, min_electrostatic_tanimoto=min_esp, max_interaction_score=max_e,
                                                 unique=kind, rank_by=rank_by,
                                                 substructure_counts=LC.REQUIRE + LC.EXCLUDE + LC.COUNTS))
            rings = kind in ("scaffold", "framework")
            check(got, want, SF._RECORD_FIELDS if rings else ())
            for m in got:
                if rings:
                    _check_fields(m, _graph(m), generic=kind == "framework", smiles=True)
                else:
                    assert m.n_rings is None and m.scaffold_atoms is None
            survivors[(rank_by, kind)] = tuple(want)
            # the survivor of each group is the best of its group by the call's ranking
            groups = {}
            for i in stages[1]:
                groups.setdefault(_identity(mols[i], kind), []).append(i)
            score = (lambda m: -m.interaction_score) if rank_by == "interaction" else \
                (lambda m: m.shape_tanimoto + m.electrostatic_tanimoto)
            for members in groups.values():
                best = min(members, key=lambda i: (-score(mols[i]), mols[i].sample_id))
                assert best in want and all(i == best or i not in want for i in members), (kind, rank_by, members)
        assert len({frozenset(survivors[(rank_by, kind)]) for kind in UNIQUE_KINDS}) == 4, survivors
    assert any(survivors[("electrostatic", k)] != survivors[("interaction", k)] for k in UNIQUE_KINDS), survivors

    # ---- the substructure gates and `exclude_graphs` behind the thresholds
    _, before = _restated_late_selection(mols, min_esp, max_e, n_req, n_exc)
    known = mols[before[-1][0]]                       # a row that passes every gate: its graph is excluded
    want, stages = _restated_late_selection(mols, min_esp, max_e, n_req, n_exc, excluded={_identity(known, "exact")},
                                            unique="exact", rank_by="interaction")
    sizes = [len(s) for s in stages]
    assert len(mols) > sizes[0] > sizes[1] > sizes[2] > sizes[3] > sizes[4] >= 1 and sizes[5] >= 1, sizes
    got = gen.generate_conformers(**dict(options, min_electrostatic_tanimoto=min_esp, max_interaction_score=max_e,
                                         require_substructures=LC.REQUIRE, exclude_substructures=LC.EXCLUDE,
                                         exclude_graphs=[known], unique="exact", rank_by="interaction"))
    check(got, want)
    print(f"COMPOSED LATE select: of {len(mols)} records min_electrostatic_tanimoto={min_esp:.4f} leaves {sizes[0]}, "
          f"max_interaction_score={max_e:.4f} {sizes[1]}, the required pattern {sizes[2]}, the excluded pattern {sizes[3]}, "
          f"exclude_graphs {sizes[4]}, unique='exact' {sizes[5]}: {[m.sample_id for m in got]}; survivors by unique "
          f"{ {k: [mols[i].sample_id for i in v] for k, v in survivors.items()} }")


# ----------------------------------------------------------------------------------------------- call B: into a pocket
def test_call_b_into_a_found_pocket_counts_and_scores_the_returned_coordinates(monkeypatch):
    """`reference_shape=Pocket` with the relief, the walk, the hydrogens and the interaction score: `atoms_outside` is the
    mesh restatement's count at the RETURNED coordinates - counted again behind the receptor stages, which move the rows
    after the pose counted them - and every value that reads a receptor reads the pocket's own."""
    import mesh_ref as MR
    from test_hydrogens_gpu import TOL as H_TOL
    gen, _ = _setup(monkeypatch)
    pocket = LC.pocket(DEV)
    kw = dict(reference_shape=pocket, n_atoms=LC.WIDTH - 2, n_samples=len(LC.batch()), variance=2, optimise_geometry=False,
              standardize=True, overlay=True, add_hydrogens=True, max_atoms_outside=None)
    posed = gen.generate_conformers(**kw)
    got = gen.generate_conformers(relieve_clashes=LC.RELIEF_STEPS, optimise_pose=LC.OPTIMISE_STEPS,
                                  interaction_scores=True, **kw)
    assert [m.sample_id for m in got] == [m.sample_id for m in posed] == [m.sample_id for m in _call(monkeypatch, "all")]
    ctx = _Context(H_TOL, (torch.as_tensor(pocket.receptor[0]).float(), torch.as_tensor(pocket.receptor[1])))
    tri = torch.from_numpy(pocket.vertices[pocket.faces].reshape(-1, 9).copy())
    worst = _Worst()
    n_recounted = n_moved = n_posed = 0
    for m, a in zip(got, posed):
        name, mol, n = LC.batch()[m.sample_id]["name"], _graph(m), len(m.atomic_numbers)
        assert m.pose is not None and a.pose is not None, name
        n_posed += 1
        w = MR.winding(tri, m.coords)
        assert float(((w.abs() - 0.5).abs()).min()) > MR.WINDING_TOL, name          # no atom on the decision
        assert m.atoms_outside == int((~MR.inside(w)).sum()) == MR.atoms_outside(tri, m.coords[None], [n])[0], name
        assert a.atoms_outside == MR.atoms_outside(tri, a.coords[None], [n])[0], name
        n_recounted += m.atoms_outside != a.atoms_outside
        n_moved += not torch.equal(m.coords, a.coords)
        cl, over = ctx.clashes(m.coords.numpy(), mol[0])
        assert (m.receptor_clashes, m.receptor_max_overlap) == (cl, over), name
        assert m.receptor_clashes_before == ctx.clashes(a.coords.numpy(), mol[0])[0] == a.receptor_clashes, name
        h = CC.hydrogen_conditions(mol, m.coords.numpy(), name)
        assert m.hydrogen_parents == h["parents"], name
        if h["n_hydrogens"]:
            worst("hydrogen_coords", float(np.abs(m.hydrogen_coords.double().numpy() - h["coords"]).max()), H_TOL, name)
        assert m.receptor_hydrogen_clashes == ctx.clashes(m.hydrogen_coords.numpy(), [1] * h["n_hydrogens"])[0], name
        args = ctx.interaction_args(mol, m.coords.numpy())
        have = dict(score=m.interaction_score, terms=np.array([m.interaction_terms[t] for t in IR.TERMS]),
                    atom_scores=m.interaction_atom_scores.double().numpy(), hbonds=m.receptor_hbonds)
        for key, ratio in IR.ratios(have, *args, factor=1.0).items():
            worst("interaction " + key + " (error / bound at factor 1, against FACTOR)", ratio, IR.FACTOR, name)
        assert m.receptor_hbonds == IR.score(*args)["hbonds"], name
    worst.report()
    print(f"COMPOSED e2e pocket: {n_posed} posed rows, {n_moved} moved behind the pose, atoms_outside "
          f"{[a.atoms_outside for a in posed]} -> {[m.atoms_outside for m in got]}: recounted on {n_recounted}")
    assert n_moved >= 2 and n_recounted >= 1


# ----------------------------------------------------------------------------------------------- the graph and its atom order
def _unstandardised(item, n):
    """What the per-atom graph values of a record of n atoms would read had the step been fed the graph AS GENERATED - both
    fragments, in the injected order - and its first n entries been taken: the restatements on the joined graph."""
    full = item["mol"]
    ch, rings = ER.charges(*full), SFR.perceive(*full)
    xyz = _xyz(item["xyz"])
    stereo = STR.descriptors(STR.tetrahedral(*full, xyz), STR.double_bonds(*full, xyz), full[2], list(range(full[2])))
    return dict(partial_charges=ch["q"][:n], hydrogen_charges=ch["q_h"][:n], ring_sizes=rings["ring_size"][:n],
                ring_systems=rings["ring_system"][:n], stereo_descriptors=stereo[:n],
                canonical_order=[a for a in CR.canonical(*full)["order"] if a < n],
                scaffold_atoms=lambda generic: [a for a in SFR.scaffold(*full, generic=generic)[3] if a < n],
                substructure_first=lambda pattern: SBC.reference(full, pattern, nh=HR.counts(*full))["first"])


def test_the_graph_readers_of_call_a_read_the_parent_graph_in_record_order(monkeypatch):
    """Item 3: exact against the restatement on the record's parent graph; and on the rows whose parent sat behind a
    smaller fragment every per-atom value differs from the restatement on the joined graph as generated."""
    from test_scaffold_gpu import _check_fields
    from ml_conformer_generator_amd import scaffold as SF
    got = _call(monkeypatch, "all")
    items = LC.batch()
    ref_graph = LC.reference()[1]
    ref_bits = FR.fingerprint(ref_graph[0], ref_graph[1].tolist(), len(ref_graph[0]))
    patterns = LC.REQUIRE + LC.EXCLUDE + LC.COUNTS
    annotated = SF.of_records(_copies(got), device=DEV)            # (it writes onto the records it is given)
    worst = _Worst()
    shifted = 0
    for k, m in enumerate(got):
        name, n, mol = items[m.sample_id]["name"], len(m.atomic_numbers), _graph(m)
        canon = CR.canonical(*mol)
        assert m.canonical_status == 0 and m.canonical_order == canon["order"], name
        plain = m.to_smiles(isomeric=False)
        assert CR.identity_bytes(*CR.read_smiles(plain)[:3]) == CR.identity_bytes(*mol), name
        bits, key = FR.fingerprint_and_key(*mol)
        assert m.graph_key == key, name
        assert np.float32(m.chemical_tanimoto).view(np.uint32) == FR.tanimoto(bits, ref_bits).view(np.uint32), name
        nh = HR.counts(*mol)
        assert len(m.substructure_patterns) == len(patterns) and m.substructure_status == [0] * len(patterns), name
        for i, pat in enumerate(patterns):
            ref = SBC.reference(mol, m.substructure_patterns[i], nh=nh)
            assert m.substructure_counts[i] == ref["count"], (name, pat)
            assert (m.substructure_first[i] is None) == (ref["count"] == 0), (name, pat)
            assert ref["count"] == 0 or SBC.is_embedding(mol, pat, m.substructure_first[i], nh), (name, pat)
        ch = ER.charges(*mol)
        assert ch["status"] == 0
        worst("partial_charges", float(np.abs(m.partial_charges.double().numpy() - np.array(ch["q"])).max()), ER.Q_TOL, name)
        worst("hydrogen_charges", float(np.abs(m.hydrogen_charges.double().numpy() - np.array(ch["q_h"])).max()), ER.Q_TOL, name)
        _check_fields(annotated[k], mol, smiles=True)               # `scaffold.of_records` on the record (the call's own
        #                                                             ring fields: the `unique="scaffold"` test below)
        shift = m.atom_map[0]
        if not shift:
            continue
        shifted += 1
        assert m.atom_map == list(range(shift, shift + n)) and 0 < shift < n, name
        wrong = _unstandardised(items[m.sample_id], n)
        for field in ("partial_charges", "hydrogen_charges"):       # further apart than both could be from the restatement
            assert np.abs(getattr(m, field).double().numpy() - np.array(wrong[field])).max() > 2 * ER.Q_TOL, (name, field)
        assert m.canonical_order != wrong["canonical_order"], name
        scores = m.interaction_atom_scores.tolist()                 # (no restatement without the other fragment's pose:
        assert scores[shift:] != scores[:-shift], name              #  every index `shift` too high reads another atom's)
        for i, pat in enumerate(patterns):
            if m.substructure_first[i] is not None:
                assert m.substructure_first[i] != wrong["substructure_first"](m.substructure_patterns[i]), (name, pat)
        if any(m.stereo_descriptors):
            assert m.stereo_descriptors != wrong["stereo_descriptors"], name
    worst.report()
    for i in range(len(LC.REQUIRE + LC.EXCLUDE)):                   # the patterns split the kept rows
        found = [m.substructure_counts[i] >= 1 for m in got]
        assert any(found) and not all(found), patterns[i]
    assert shifted >= 2 and {items[m.sample_id]["name"] for m in got if m.atom_map[0]} == set(LC.SHIFTED)
    assert any(any(m.stereo_descriptors) for m in got if m.atom_map[0])            # a shifted row with a descriptor
    print(f"COMPOSED e2e coverage: a shifted atom_map on {shifted} rows, each per-atom graph value differs there from the "
          "joined graph's")


def test_the_stereo_fields_of_call_a_read_the_returned_coordinates_and_no_stage_changes_them(monkeypatch):
    """The stereo fields against the restatement on the parent graph at the returned coordinates, under the stage test's own
    precondition (no |chi| or |cos| inside `STEREO_BAND`).  They are exempt from the stale-coordinate check because no stage
    changes chirality; what is asserted instead: the descriptors are equal at all four earlier coordinate sets."""
    got, rigid = _call(monkeypatch, "all"), _call(monkeypatch, "rigid")
    relieved, refined = _call(monkeypatch, "relieved"), _call(monkeypatch, "refined")
    x_rel = _DONE["last_batch"]["x_relaxed"]
    low, high = LC.STEREO_BAND
    defined = undefined = 0
    for m, r, p, q in zip(got, rigid, relieved, refined):
        name, n, mol = LC.batch()[m.sample_id]["name"], len(m.atomic_numbers), _graph(m)
        xyz = _xyz(m.coords)
        margins = STR.margins(*mol, xyz)
        assert all(not (low <= v <= high) for v in margins), (name, margins)
        st = STR.stereo(*mol, xyz)
        assert (m.stereo_status, m.stereo_order) == (0, st["order"]), name
        assert (m.n_stereo_defined, m.n_stereo_undefined) == (st["counts"][0] + st["counts"][1], st["counts"][2]), name
        own = STR.descriptors(STR.tetrahedral(*mol, xyz), STR.double_bonds(*mol, xyz), n, list(range(n)))
        assert m.stereo_descriptors == own, name
        for earlier in (x_rel[m.batch_row, :n], q.coords, p.coords, r.coords):
            e = _xyz(earlier)
            assert STR.descriptors(STR.tetrahedral(*mol, e), STR.double_bonds(*mol, e), n, list(range(n))) == own, name
        sz, sadj, _, tet, dbs = STR.read_isomeric(m.smiles)
        back = STR.stereo(sz, sadj, len(sz), None, perceived=(tet, dbs))
        assert CR.identity_bytes(sz, sadj, len(sz)) + bytes(back["stereo"]) == STR.identity_bytes(*mol, xyz), name
        defined += m.n_stereo_defined > 0
        undefined += m.n_stereo_undefined > 0
    print(f"COMPOSED e2e coverage: stereo defined on {defined} rows, undefined on {undefined}")
    assert defined >= 2 and undefined >= 1


@pytest.mark.parametrize("kind", ["scaffold", "framework"])
def test_the_ring_fields_of_a_unique_scaffold_call_read_the_parent_graph_in_record_order(monkeypatch, kind):
    """The ring and scaffold fields come with `unique="scaffold"` / `"framework"` only.  Call A with that option - and
    with the graphs excluded that share the scaffold of the row whose parent sits behind a smaller fragment, so that this row
    is the one its group keeps: its fields are the restatement's on the parent graph, in record order, and differ from
    the restatement's on the joined graph as generated."""
    from test_scaffold_gpu import _check_fields
    from ml_conformer_generator_amd import scaffold as SF
    mols = _call(monkeypatch, "all")
    items = LC.batch()
    by_id = {m.sample_id: m for m in mols}
    target = next(m for m in mols if items[m.sample_id]["name"] == LC.SHIFTED[0])
    rivals = [m for m in mols if m is not target and _identity(m, kind) == _identity(target, kind)]
    assert len(rivals) >= 2                                         # it shares its scaffold: `unique` alone might drop it
    gen, _ = _setup(monkeypatch)
    got = gen.generate_conformers(**dict(_options(), unique=kind, exclude_graphs=rivals))
    want, stages = _restated_late_selection(mols, excluded={_identity(m, "exact") for m in rivals}, unique=kind)
    assert [m.sample_id for m in got] == [mols[i].sample_id for i in want] and len(stages[1]) < len(stages[0]) < len(mols)
    live = 0
    for m in got:
        name, n, mol = items[m.sample_id]["name"], len(m.atomic_numbers), _graph(m)
        assert _late_bits(m, SF._RECORD_FIELDS) == _late_bits(by_id[m.sample_id], SF._RECORD_FIELDS), name
        _check_fields(m, mol, generic=kind == "framework", smiles=True)
        shift = m.atom_map[0]
        if shift and 0 < len(m.scaffold_atoms) < n:
            wrong = _unstandardised(items[m.sample_id], n)
            assert m.ring_sizes != wrong["ring_sizes"] and m.ring_systems != wrong["ring_systems"], name
            assert m.scaffold_atoms != wrong["scaffold_atoms"](kind == "framework"), name
            live += 1
    assert target.sample_id in [m.sample_id for m in got] and live >= 1
    print(f"COMPOSED e2e coverage: unique={kind!r} keeps {[m.sample_id for m in got]}; a shifted atom_map with a non-empty "
          f"proper-subset scaffold on {live}")
