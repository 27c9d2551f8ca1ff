"""Receptor contacts without a GPU (ml_conformer_generator_amd/contacts.py, DESIGN.md section 6 "Receptor contacts"): the
PDB residue groups, the grouped sort, the restatement's mutation check on the committed cases, the option values of
`interaction_scores`, every refusal before any device work, the record fields through stub seams, the recovery filter's
place, and the fifth public header against the `_lib` table."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import contacts_cases as CC
import contacts_ref as CR
import interactions_cases as K
import interactions_ref as IR
import stream_probe as SP
from conftest import REPO
from ml_conformer_generator_amd import _lib
from ml_conformer_generator_amd import contacts as CT
from ml_conformer_generator_amd import interactions as IX
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import receptor as RC
from ml_conformer_generator_amd.handoff import Measured, measured_from_tensors
from test_interactions_host import _graph_shard, _record_receptor, _seam_interactions
from test_shape_overlay_host import _no_device, _ref, _shell_generator, _stub_overlay

HEADER = os.path.join(REPO, "include", "mlconfgen_hip_contacts.h")

PDB = """\
HEADER    HAND-WRITTEN
MODEL        1
ATOM      1  N   SER A  10      11.000  12.000  13.000  1.00  0.00           N
ATOM      2  CA  SER A  10      12.000  12.000  13.000  1.00  0.00           C
ATOM      3  HA  SER A  10      12.500  12.500  13.000  1.00  0.00           H
ATOM      4  OG ASER A  10      13.000  12.000  13.000  0.50  0.00           O
ATOM      5  OG BSER A  10      13.100  12.100  13.000  0.50  0.00           O
ATOM      6  N   LEU A  10A     14.000  12.000  13.000  1.00  0.00           N
ATOM      7  CA  LEU A  10A     15.000  12.000  13.000  1.00  0.00           C
ATOM      8  N   ASP B  10      16.000  12.000  13.000  1.00  0.00           N
ATOM      9  CA  SER A  10      12.000  13.000  13.000  1.00  0.00           C
ATOM     10  N   GLY    7       17.000  12.000  13.000  1.00  0.00           N
HETATM   11  O   HOH B 301      18.000  12.000  13.000  1.00  0.00           O
ENDMDL
MODEL        2
ATOM     12  N   LYS C   1      19.000  12.000  13.000  1.00  0.00           N
ENDMDL
"""


# ----------------------------------------------------------------------------------------------- groups and the sort
def test_parse_pdb_groups_against_a_hand_written_text():
    ids, labels = RC.parse_pdb_groups(PDB)
    assert ids.dtype == torch.int32
    # the altloc B record, the hydrogen and the second model are gone; the late CA of A:SER10 joins its residue again
    assert ids.tolist() == [0, 0, 0, 1, 1, 2, 0, 3, 4]
    assert labels == ["A:SER10", "A:LEU10A", "B:ASP10", "_:GLY7", "B:HOH301"]
    xyz, z = RC.parse_pdb(PDB)
    names = RC.parse_pdb_names(PDB)
    assert len(ids) == len(z) == len(names) == 9
    assert [n for n in names] == [("SER", "N"), ("SER", "CA"), ("SER", "OG"), ("LEU", "N"), ("LEU", "CA"), ("ASP", "N"),
                                  ("SER", "CA"), ("GLY", "N"), ("HOH", "O")]
    assert [labels[i].split(":")[1][:3] for i in ids.tolist()] == [r for r, _ in names]           # the same records, in order
    assert xyz[:, 0].tolist() == [11.0, 12.0, 13.0, 14.0, 15.0, 16.0, 12.0, 17.0, 18.0]
    prepared = CT.prepare_receptor(PDB)
    assert prepared.group_labels == tuple(labels) and sorted(prepared.groups.tolist()) == sorted(ids.tolist())
    # the group travels with its atom through the sort
    by_x = {float(x): int(g) for x, g in zip(prepared.xyzr[:, 0], prepared.groups) if float(x) != 12.0}
    assert by_x == {11.0: 0, 13.0: 0, 14.0: 1, 15.0: 1, 16.0: 2, 17.0: 3, 18.0: 4}


def test_grouped_sort_returns_the_typed_sort_bit_for_bit_on_ties_too():
    g = np.random.default_rng(4)
    xyz = torch.from_numpy(g.uniform(-20, 20, size=(700, 3)).astype(np.float32))
    xyz[100:140] = xyz[:40]                                        # ties on x, y, z ...
    radius = torch.from_numpy(g.choice([1.7, 1.8, 1.9], size=700).astype(np.float32))
    types = torch.from_numpy(g.integers(0, 8, size=700).astype(np.uint8))
    radius[100:120], types[100:110] = radius[:20], types[:10]      # ... on the radius too, and on the type as well
    groups = torch.from_numpy(g.integers(0, 50, size=700).astype(np.int32))
    a_xyzr, a_types = RC.sort_typed_receptor(xyz, radius, types)
    b_xyzr, b_types, b_groups = RC.sort_grouped_receptor(xyz, radius, types, groups)
    assert torch.equal(a_xyzr.view(torch.int32), b_xyzr.view(torch.int32)) and torch.equal(a_types, b_types)
    assert b_groups.dtype == torch.int32
    def atoms(x, r, t, grp):                                       # the multiset of (x, y, z, radius, type, group)
        return sorted(zip((tuple(v) for v in x.view(torch.int32).tolist()), r.view(torch.int32).tolist(), t.tolist(), grp.tolist()))
    assert atoms(xyz, radius, types, groups) == atoms(b_xyzr[:, :3].contiguous(), b_xyzr[:, 3].contiguous(), b_types, b_groups)
    perm = torch.from_numpy(g.permutation(700))
    c = RC.sort_grouped_receptor(xyz[perm], radius[perm], types[perm], groups[perm])
    assert all(torch.equal(u, v) for u, v in zip(c, (b_xyzr, b_types, b_groups)))     # whatever the order the atoms came in
    # the existing prepared type and its constructor are as they were
    old = IX.PreparedReceptor(a_xyzr, a_types, RC.tile_spheres(a_xyzr))
    assert IX.prepare_receptor(old) is old and len(old) == 3
    prepared = CT.prepare_receptor((xyz, torch.full((700,), 6), types), groups=groups)
    assert isinstance(prepared.typed, IX.PreparedReceptor) and torch.equal(prepared.typed.types, prepared.types)


def test_prepare_receptor_refusals_and_hydrogens():
    xyz = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    z = torch.tensor([6, 1, 7, 8, 1])
    prepared = CT.prepare_receptor((xyz, z), groups=[4, 9, 4, 7, 9])
    assert sorted(prepared.groups.tolist()) == [4, 4, 7] and prepared.group_labels is None    # the hydrogens' ids go with them
    assert CT.prepare_receptor(prepared) is prepared
    for bad in (None, [1, 2, 3], [0, 0, 0, 0, -1], [0.0] * 5, [True] * 5, "abcde"):
        with pytest.raises(ValueError):
            CT.prepare_receptor((xyz, z), groups=bad)
    with pytest.raises(ValueError, match="residues"):
        CT.prepare_receptor(PDB, groups=[0] * 9)
    with pytest.raises(ValueError):
        CT.prepare_receptor(IX.prepare_receptor((xyz, z)))
    for bad in (([1, 0], [1, 1]), ([1, 1], [1, 1]), ([1], [16]), ([1, 2], [1]), (list(range(257)), [1] * 257), ([-1], [1]), 5):
        with pytest.raises(ValueError):
            CT.load_reference(bad)
    for bad in (True, 16, -1, 2.0, None):
        with pytest.raises(ValueError):
            CT.check_kinds(bad)
    assert CT.labels(prepared, [[4, 7, 0]], [[3, 12, 0]]) == [((4, ("contact", "hydrophobic")), (7, ("hbond_donor", "hbond_acceptor")))]
    assert CT.labels(CT.prepare_receptor(PDB), [[1, 4]], [[1, 8]], [2]) == [(("A:LEU10A", ("contact",)), ("B:HOH301", ("hbond_acceptor",)))]


# ----------------------------------------------------------------------------------------------- the restatement
def _same(a, b):
    return a["status"] == b["status"] and a["entries"] == b["entries"] and np.array_equal(a["atom_kinds"], b["atom_kinds"])


@pytest.mark.parametrize("mistake", CR.MISTAKES)
def test_restatement_catches_each_planted_mistake_on_the_committed_cases(mistake):
    pool = list(CC.cases()) + [CC.two_kinds_one_group()] + CC.threshold_rows("contact") + CC.threshold_rows("hbond")
    caught = [c.name for c in pool if not _same(c.expected(), c.expected(mistake))]
    assert caught, mistake
    assert all(_same(c.expected(), c.expected()) for c in pool[:3])


def test_restatement_is_independent_of_the_receptor_order_and_reads_the_committed_facts():
    c = CC.cases()[4]
    perm = np.random.default_rng(2).permutation(len(c.rec))
    shuffled = CC.Case("p", c.x, c.z, c.t, c.rec[perm], c.rec_z[perm], c.rec_t[perm], c.groups[perm])
    assert _same(c.expected(), shuffled.expected())
    assert CC.two_kinds_one_group().expected()["entries"] == [(5, 7)]
    for kind, n_ok in (("groups", 256), ("candidates", 200)):
        assert len(CC.capacity(kind, 0).expected()["entries"]) == n_ok and CC.capacity(kind, 0).expected()["status"] == CR.OK
        assert CC.capacity(kind, 1).expected()["status"] == CR.OVERFLOW
    assert CR.compare(dict(status=CR.OK, entries=[(1, 7), (3, 12)]), [(1, 6), (2, 2), (3, 1)]) == (4, 3, 2, 2 / 3, 2 / 5)
    assert CR.compare(dict(status=CR.OK, entries=[(1, 7)]), [(1, 6)], mask=1)[:3] == (1, 0, 0)
    n = CR.compare(dict(status=CR.OK, entries=[]), [])
    assert n[:3] == (0, 0, 0) and math.isnan(n[3]) and math.isnan(n[4])
    assert CC.pocket_pdb_text() == CC.pocket_pdb()                 # the committed fixture is its recipe's output
    rec, tan = CT.compare_counts(torch.tensor([[4, 3, 2], [0, 0, 0], [-1, -1, -1], [2, 0, 0]], dtype=torch.int32))
    assert rec.dtype == torch.float64 and rec[0].item() == 2 / 3 and tan[0].item() == 2 / 5 and tan[3].item() == 0.0
    assert torch.isnan(rec[1:]).all() and torch.isnan(tan[1:3]).all()
    assert CT.compare_entries([1, 3], [7, 12], [1, 2, 3], [6, 2, 1]) == ([(1, 6)], [(2, 2)])


# ----------------------------------------------------------------------------------------------- options
def _graph(n=17):
    z = ([6, 6, 7, 6, 8, 6, 6] * 3)[:n]
    bonds = torch.zeros(n, n, dtype=torch.int8)
    for i in range(n - 1):
        bonds[i, i + 1] = bonds[i + 1, i] = 1
    return z, bonds


def _pdb_receptor():
    """`_record_receptor`'s shell round where the stub pose puts the shard's molecules, as a PDB string."""
    return CC.pdb_from_points(_record_receptor()[0].numpy())


def test_new_option_values_parse():
    gen = _shell_generator()
    parse = postprocess.parse_request
    pdb = _pdb_receptor()
    assert CT.parse_option("contacts") == (True, True, None) and CT.parse_option(("contacts", 1)) == (True, True, 1.0)
    assert CT.parse_option(True) == (True, False, None) and CT.parse_option("yes") == ("yes", False, None)
    plain = parse(gen, _ref(), overlay=True, receptor=pdb, interaction_scores=True)
    assert plain.scores_interactions and not plain.scores_contacts and plain.contact_receptor is None
    req = parse(gen, _ref(), overlay=True, receptor=pdb, interaction_scores="contacts")
    assert req.scores_interactions and req.scores_contacts and not req.removes and req.ref_contact_graph is None
    assert isinstance(req.contact_receptor, CT.PreparedReceptor) and isinstance(req.typed_receptor, IX.PreparedReceptor)
    assert all(torch.equal(a, b) for a, b in zip(req.typed_receptor, plain.typed_receptor))      # the score reads the same receptor
    req = parse(gen, _ref(), overlay=True, receptor=pdb, interaction_scores="contacts", reference_graph=_graph())
    assert req.ref_contact_graph is not None and req.min_contact_recovery is None and len(req.ref_contact_graph[0]) == 17
    req = parse(gen, _ref(), overlay=True, receptor=pdb, interaction_scores=("contacts", 0.25), reference_graph=_graph())
    assert req.min_contact_recovery == 0.25 and req.removes and req.scores_contacts
    req = parse(gen, _ref(), overlay=True, receptor=pdb, interaction_scores=["contacts", 0], reference_graph=_graph())
    assert req.min_contact_recovery == 0.0
    assert postprocess.Request().scores_contacts is False and postprocess.Request().min_contact_recovery is None


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_contact_refusals_happen_before_any_device_work(entry, monkeypatch):
    from ml_conformer_generator_amd import host_pool as HP
    from ml_conformer_generator_amd import mesh as mcg_mesh
    gen = _shell_generator()
    monkeypatch.setattr(gen, "_generate_shard", _no_device)
    gen._interaction_scores = gen._contact_fingerprint = gen._receptor_coords = gen._score = gen._pose = _no_device
    gen._pharm_perceive = gen._match_substructures = _no_device
    call = getattr(gen, entry)
    pdb = _pdb_receptor()
    pair = _record_receptor()
    nan = float("nan")
    cases = [dict(interaction_scores="contacts"),                                             # no receptor
             dict(interaction_scores="contacts", receptor=pdb),                               # no overlay
             dict(overlay=True, interaction_scores="contacts"),
             dict(overlay=True, receptor=(pair[0], pair[1]), interaction_scores="contacts"),  # no residue identities
             dict(overlay=True, receptor=pair, interaction_scores="contacts"),
             dict(overlay=True, receptor=pair, interaction_scores=("contacts", 0.5), reference_graph=_graph()),
             dict(overlay=True, receptor=pdb, interaction_scores=("contacts", 0.5)),          # no reference graph
             dict(overlay=True, receptor=pdb, interaction_scores="contacts", reference_graph=_graph(16)),    # ... of another size
             dict(overlay=True, receptor=pdb, interaction_scores="contact"),
             dict(overlay=True, receptor=pdb, interaction_scores=("contacts",)),
             dict(overlay=True, receptor=pdb, interaction_scores=("contacts", 0.5, 1)),
             dict(overlay=True, receptor=pdb, interaction_scores=("contact", 0.5), reference_graph=_graph())]
    for bad in (nan, float("inf"), -0.1, 1.5, True, "0.5", None, [0.5]):
        cases.append(dict(overlay=True, receptor=pdb, interaction_scores=("contacts", bad), reference_graph=_graph()))
    for kw in cases:
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    with pytest.raises(ValueError, match=r"contacts\.contact_fingerprint\(groups="):
        call(reference_conformer=_ref(), n_samples=4, overlay=True, receptor=pair, interaction_scores="contacts")
    with pytest.raises(ValueError, match="reference_graph"):
        call(reference_conformer=_ref(), n_samples=4, overlay=True, receptor=pdb, interaction_scores=("contacts", 0.5))
    with pytest.raises(ValueError):                      # a reference_context has no coordinates to pose onto, and no graph
        call(reference_conformer=None, reference_context=torch.zeros(1, 3), n_samples=4, overlay=True, receptor=pdb,
             interaction_scores=("contacts", 0.5))
    for finisher in ("rdkit", HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                                         "finish_tag_chunk")):
        gen.finisher = finisher
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, overlay=True, receptor=pdb, interaction_scores="contacts")
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, overlay=True, receptor=pdb, interaction_scores=("contacts", 0.5),
                 reference_graph=_graph())


# ----------------------------------------------------------------------------------------------- the record path
def _seam_contacts(calls):
    """`_contact_fingerprint` by the restatement, on the host."""
    def run(prepared, coords, n_nodes, atomic_numbers, bond_orders, reference=None):
        assert isinstance(prepared, CT.PreparedReceptor)
        B, N = int(coords.shape[0]), int(coords.shape[1])
        calls.append(("contacts", B, reference is not None))
        out = dict(groups=torch.zeros(B, 256, dtype=torch.int32), kinds=torch.zeros(B, 256, dtype=torch.uint8),
                   n_groups=torch.zeros(B, dtype=torch.int32), atom_kinds=torch.zeros(B, N, dtype=torch.uint8),
                   status=torch.zeros(B, dtype=torch.int32))
        counts = torch.zeros(B, 3, dtype=torch.int32)
        for b in range(B):
            k = int(n_nodes[b])
            z, adj = atomic_numbers[b, :k].tolist(), bond_orders[b, :k, :k].tolist()
            t = IR.ligand_types(z, adj, k, K.pharm_types((z, adj, k)))
            fp = CR.fingerprint(coords[b, :k].numpy(), IR.radii(z), t, prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(),
                                prepared.types.numpy(), prepared.groups.numpy())
            m = len(fp["entries"])
            out["status"][b], out["n_groups"][b] = fp["status"], m
            if m:
                out["groups"][b, :m] = torch.tensor([g for g, _ in fp["entries"]], dtype=torch.int32)
                out["kinds"][b, :m] = torch.tensor([v for _, v in fp["entries"]], dtype=torch.uint8)
            out["atom_kinds"][b, :k] = torch.from_numpy(fp["atom_kinds"])
            if reference is not None:
                counts[b] = torch.tensor(CR.compare(fp, list(zip(*reference)))[:3], dtype=torch.int32)
        if reference is not None:
            rec, tan = CT.compare_counts(counts)
            out.update(n_bits=counts[:, 0], n_ref_bits=counts[:, 1], n_common=counts[:, 2], recovery=rec, tanimoto=tan)
        return out
    return run


FIELDS = ("residue_contacts", "contact_groups", "contact_kinds", "contact_atom_kinds", "contact_status")
COMPARED = ("contact_recovery", "contact_tanimoto", "contacts_recovered", "contacts_missed")


def test_record_path_carries_the_fields_and_launches_nothing_unasked():
    calls = []
    gen = _shell_generator()
    gen._interaction_scores = _seam_interactions(calls)
    gen._contact_fingerprint = _seam_contacts(calls)
    gen.min_n_nodes = 4                                                           # (the reference below has seven atoms)
    gen._generate_shard = _graph_shard
    gen._pose = _stub_overlay(lambda k: k * 0.0 + 0.5)
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    gen._receptor_coords = lambda rec, coords, n, z: torch.full(tuple(coords.shape[:2]), -1.0)
    pdb = _pdb_receptor()
    # the reference: the posed toluene's own place, so that its fingerprint has bits to recover
    ref = gen._pose(None, _graph_shard(None, None, 0, None, 1)["x"], torch.tensor([7]))["coords"][0, :7].clone()
    z_ref, adj_ref, _ = K.MOLECULES["toluene"][0]
    graph = (z_ref, torch.tensor(adj_ref, dtype=torch.int8).reshape(7, 7))
    kw = dict(reference_conformer=ref, n_samples=8, overlay=True, receptor=pdb, optimise_geometry=False)

    scored = gen.generate_conformers(interaction_scores=True, **kw)
    assert calls == [("interactions", 8)]                                         # True alone: the contact seam is not touched
    assert all(getattr(m, f) is None for m in scored for f in FIELDS + COMPARED)
    del calls[:]
    got = gen.generate_conformers(interaction_scores="contacts", **kw)
    assert calls == [("interactions", 8), ("contacts", 8, False)]                 # one call each over the rows, no reference
    keep = lambda mols: [m for m in mols if m.sample_id != 6]                     # noqa: E731 (6 holds a NaN: never equal)
    plainly = lambda v: (v.tolist() if torch.is_tensor(v) else                     # noqa: E731
                         [plainly(x) for x in v] if isinstance(v, (list, tuple)) else v)
    flat = lambda m: {k: plainly(getattr(m, k)) for k in vars(m._measured) if not k.startswith("contact")}   # noqa: E731
    assert [flat(m) for m in keep(got)] == [flat(m) for m in keep(scored)]        # everything else as `True` gives it
    prepared = CT.prepare_receptor(pdb)
    seen = 0
    for m in got:
        if m.sample_id == 6:                                                      # its pose failed: None throughout
            assert all(getattr(m, f) is None for f in FIELDS + COMPARED) and m.pose is None
            continue
        z, adj = m.atomic_numbers, m.bond_orders.tolist()
        t = IR.ligand_types(z, adj, len(z), K.pharm_types((z, adj, len(z))))
        own = CR.fingerprint(m.coords.numpy(), IR.radii(z), t, prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(),
                             prepared.types.numpy(), prepared.groups.numpy())
        assert list(zip(m.contact_groups, m.contact_kinds)) == own["entries"] and m.contact_status == own["status"] == CT.OK
        assert m.contact_atom_kinds == own["atom_kinds"].tolist() and len(m.contact_atom_kinds) == len(z)
        assert m.residue_contacts == tuple((prepared.group_labels[g], CT.kind_names(v)) for g, v in own["entries"])
        assert all(getattr(m, f) is None for f in COMPARED)                       # no reference graph: no recovery
        seen += len(own["entries"])
    assert seen > 0 and any(":" in lab for m in keep(got) for lab, _ in m.residue_contacts)

    del calls[:]
    compared = gen.generate_conformers(interaction_scores="contacts", reference_graph=graph, **kw)
    assert calls == [("interactions", 8), ("contacts", 1, False), ("contacts", 8, True)]    # the reference: once, same seam
    t_ref = IR.ligand_types(z_ref, adj_ref, 7, K.pharm_types((z_ref, adj_ref, 7)))
    ref_fp = CR.fingerprint(ref.numpy(), IR.radii(z_ref), t_ref, prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(),
                            prepared.types.numpy(), prepared.groups.numpy())
    assert sum(CR.popcount(v & CR.DEFAULT_KINDS) for _, v in ref_fp["entries"]) > 0
    recovery = {}
    for m, plain in zip(compared, got):
        if m.sample_id == 6:
            assert all(getattr(m, f) is None for f in FIELDS + COMPARED)
            continue
        assert m.residue_contacts == plain.residue_contacts
        want = CR.compare(dict(status=CR.OK, entries=list(zip(m.contact_groups, m.contact_kinds))), ref_fp["entries"])
        assert m.contact_recovery == want[3] and m.contact_tanimoto == want[4]
        names = lambda found: tuple((prepared.group_labels[g], CT.kind_names(v)) for g, v in found)         # noqa: E731
        hit, miss = CT.compare_entries(m.contact_groups, m.contact_kinds, *zip(*ref_fp["entries"]))
        assert m.contacts_recovered == names(hit) and m.contacts_missed == names(miss)
        assert m.contact_reference == (tuple(g for g, _ in ref_fp["entries"]), tuple(v for _, v in ref_fp["entries"]),
                                       CT.DEFAULT_KINDS)
        recovery[m.sample_id] = m.contact_recovery
    assert recovery[0] == 1.0 and len(set(recovery.values())) >= 2                # toluene at its own place recovers itself

    def ids(entry="generate_conformers", **more):
        return [m.sample_id for m in getattr(gen, entry)(**dict(kw, reference_graph=graph, **more))]
    values = sorted(set(recovery.values()))
    t = (values[0] + values[1]) / 2
    want = [i for i in sorted(recovery) if recovery[i] >= t]
    assert 0 < len(want) < len(recovery)
    for entry in ("generate_conformers", "generate_conformers_sharded", "forward"):
        assert ids(entry, interaction_scores=("contacts", t)) == want, entry
    assert ids(interaction_scores=("contacts", 0.0)) == sorted(recovery)          # a failed pose never passes
    assert ids(interaction_scores=("contacts", 1.0)) == [i for i in sorted(recovery) if recovery[i] >= 1.0]


def test_recovery_filter_sits_beside_the_score_filter_and_nan_does_not_pass():
    nan = float("nan")
    Req = postprocess.Request
    score = [-1.0, -5.0, -2.0, -3.0, -3.0, 2.0]
    recovery = [1.0, 0.5, nan, None, 0.25, 0.75]
    n = len(score)
    measured = [Measured(interaction_score=s, contact_recovery=r) for s, r in zip(score, recovery)]
    rows = lambda: postprocess.Rows(list(range(n)), list(range(n)), list(measured), list(range(n)), sub=[([1], [0])] * n)   # noqa: E731
    none = lambda rows: (_ for _ in ()).throw(AssertionError("no pair matrix was asked for"))        # noqa: E731
    sel = lambda req: postprocess.select(rows(), req, none, none)                                    # noqa: E731
    assert sel(Req(scores_contacts=True, min_contact_recovery=0.5)) == [0, 1, 5]
    assert sel(Req(scores_contacts=True, min_contact_recovery=0.0)) == [0, 1, 4, 5]                  # NaN and None never pass
    assert sel(Req(scores_contacts=True, min_contact_recovery=0.5, max_interaction_score=-1.0)) == [0, 1]
    assert Req(min_contact_recovery=0.0).removes and not Req(scores_contacts=True).removes
    src = inspect.getsource(postprocess.select)
    assert src.index("req.max_interaction_score is not None") < src.index("req.min_contact_recovery is not None") \
        < src.index("req.n_required or req.n_excluded")
    head = postprocess.__doc__
    assert head.index("`max_interaction_score`, the contact recovery") < head.index("`require_substructures`,\n       `exclude")


def test_measured_from_tensors_reads_the_contact_spellings():
    groups = torch.zeros(3, 256, dtype=torch.int32)
    kinds = torch.zeros(3, 256, dtype=torch.uint8)
    groups[0, :2], kinds[0, :2] = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([3, 12], dtype=torch.uint8)
    atoms = torch.tensor([[1, 0, 255], [0, 0, 0], [255, 255, 255]], dtype=torch.uint8)
    out = measured_from_tensors(dict(contact_status=torch.tensor([0, -1, 1], dtype=torch.int32), contact_groups=groups,
                                     contact_kinds=kinds, contact_atom_kinds=atoms,
                                     contact_recovery=torch.tensor([0.5, 0.25, float("nan")], dtype=torch.float64),
                                     contact_tanimoto=torch.tensor([0.2, 0.1, float("nan")], dtype=torch.float64),
                                     contact_labels=("A:SER1", "A:LEU2", "B:ASP3"), contact_reference=((0,), (2,), 14)), 3)
    assert (out[0].contact_groups, out[0].contact_kinds, out[0].contact_atom_kinds) == ([0, 2], [3, 12], [1, 0])
    assert out[0].contact_recovery == 0.5 and out[0].contact_labels[2] == "B:ASP3" and out[0].contact_reference[2] == 14
    assert all(getattr(out[1], f.name) is None for f in Measured.__dataclass_fields__.values() if f.name.startswith("contact"))
    assert out[2].contact_status == 1 and out[2].contact_groups == [] and out[2].contact_atom_kinds == []
    assert math.isnan(out[2].contact_recovery)
    assert measured_from_tensors({}, 2)[0] == Measured()


# ----------------------------------------------------------------------------------------------- the fifth header
def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mcg_[a-z0-9_]+)\s*\(", text)))


def _c_arguments(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    params = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    return [ctypes.c_void_p if "*" in p else {"int": ctypes.c_int, "float": ctypes.c_float}[" ".join(p.split()).split()[0]]
            for p in params.split(",")]


def test_contacts_header_and_binding_agree():
    assert declared_symbols() == sorted(_lib.CONTACT_SIGNATURES) == ["mcg_receptor_contacts"]
    assert not set(_lib.CONTACT_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.FLEX_SIGNATURES) | set(_lib.POCKET_SIGNATURES)
                                               | set(_lib.SEARCH_SIGNATURES))
    for name, (res, args) in _lib.CONTACT_SIGNATURES.items():
        assert res is ctypes.c_int and args == _c_arguments(name), name
    text = open(HEADER).read()
    for name, value in (("MAX_GROUPS", CT.MAX_GROUPS), ("MAX_CANDIDATES", CT.MAX_CANDIDATES), ("CONTACT", CT.CONTACT),
                        ("HYDROPHOBIC", CT.HYDROPHOBIC), ("HBOND_DONOR", CT.HBOND_DONOR), ("HBOND_ACCEPTOR", CT.HBOND_ACCEPTOR),
                        ("ALL_KINDS", CT.ALL_KINDS), ("OK", CT.OK), ("EMPTY", CT.EMPTY), ("NONFINITE", CT.NONFINITE),
                        ("OVERFLOW", CT.OVERFLOW)):
        assert re.search(rf"#define MCG_CONTACT_{name} {value}\b", text), name
    assert (CT.MAX_GROUPS, CT.MAX_CANDIDATES) == (CR.MAX_GROUPS, CR.MAX_CANDIDATES) == (256, 2048)
    assert '#include "mlconfgen_hip.h"' in text
    main = open(os.path.join(REPO, "include", "mlconfgen_hip.h")).read()
    assert "mcg_receptor_contacts" not in main and _lib.lib().mcg_abi_version() == 4
    h = _lib.lib()
    fn = h.mcg_receptor_contacts
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.CONTACT_SIGNATURES["mcg_receptor_contacts"][1]


def test_contacts_header_is_plain_c_and_cxx(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "mlconfgen_hip_contacts.h"\nint main(void) { return MCG_CONTACT_MAX_GROUPS == 0 || '
                   'MCG_CONTACT_OVERFLOW == 0 || MCG_RECEPTOR_MAX_ATOMS == 0 || mcg_abi_version() == 0; }\n')
    inc = os.path.join(REPO, "include")
    if shutil.which("gcc"):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    if shutil.which("g++"):
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_makefile_names_both_new_files():
    text = open(os.path.join(REPO, "ml_conformer_generator_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*?)\n\S", text, flags=re.S | re.M).group(1)
    hdrs = re.search(r"^HDRS = (.*?)\n\S", text, flags=re.S | re.M).group(1)
    assert "mcg_contacts.hip" in srcs.split() and "../../include/mlconfgen_hip_contacts.h" in hdrs.split()


def test_c_entry_refuses_bad_arguments_without_a_device():
    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = [p, p, p, p, 2, 8, p, p, p, 100, None, p, p, 2, 14, p, p, p, p, p, p, None]
    assert len(ok) == len(_lib.CONTACT_SIGNATURES["mcg_receptor_contacts"][1])
    for at, value in [(k, None) for k in (0, 1, 2, 3, 6, 7, 8, 11, 12, 15, 16, 17, 18, 19)] + \
            [(4, 0), (4, 16385), (5, 0), (5, 65), (9, 0), (9, 131073), (13, -1), (13, 257), (14, -1), (14, 16)]:
        args = list(ok)
        args[at] = value
        assert h.mcg_receptor_contacts(*args) == 1, (at, value)
        assert b"mcg_receptor_contacts" in h.mcg_last_error()


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_contacts`: the entry's argument checks in a stand-alone program under host-side ASan + UBSan, on the CPU."""
    exe = str(tmp_path / "contacts_arg_check")
    csrc = os.path.join(REPO, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_contacts", f"CONTACTS_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 not refused" in ran.stdout, ran.stdout + ran.stderr


def test_the_stream_taking_entry_is_run_on_a_side_stream():
    import test_contacts_stream_gpu as G
    header = SP.HEADER.replace("mlconfgen_hip.h", "mlconfgen_hip_contacts.h")
    assert SP.stream_entries(header) == ["mcg_receptor_contacts"] == sorted(G.COVERAGE)
    for entry, (test, arrangements) in G.COVERAGE.items():
        assert callable(getattr(G, test)) and arrangements == "AB"
