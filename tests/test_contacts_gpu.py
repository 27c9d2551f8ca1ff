"""`mcg_receptor_contacts` on the MI355X against the restatement of tests/contacts_ref.py, bit for bit: entries, per-atom
kinds, statuses and the integer counts are exact, so every comparison here is an equality.  Then the module's wrappers, the
cross-kernel invariants with `mcg_receptor_interactions`, the stream contract, and the generation entries with
`interaction_scores="contacts"`."""
import math

import numpy as np
import pytest
import torch

import contacts_cases as CC
import contacts_ref as CR
import interactions_ref as IR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0x5B


def _mods():
    from ml_conformer_generator_amd import contacts as CT, interactions as IX
    return CT, IX


def _pad(case_list, width):
    """x [B,W,3], radii [B,W], types [B,W], n [B] with junk beyond every row's atoms."""
    B = len(case_list)
    x = np.full((B, width, 3), 7.5, dtype=np.float32)
    r = np.full((B, width), 1.9, dtype=np.float32)
    t = np.full((B, width), 7, dtype=np.uint8)
    n = np.zeros(B, dtype=np.int32)
    for b, c in enumerate(case_list):
        x[b, : c.n], r[b, : c.n], t[b, : c.n], n[b] = c.x, IR.radii(c.z), c.t, c.n
    return tuple(torch.from_numpy(a) for a in (x, r, t, n))


def _launch(case_list, width, prepared, **kw):
    CT, _ = _mods()
    x, r, t, n = _pad(case_list, width)
    return {k: v.cpu() for k, v in CT.fingerprint_typed(prepared, x, n, r, t, device=DEV, **kw).items()}


def _prepared(case):
    CT, _ = _mods()
    return CT.prepare_receptor(case.receptor, groups=torch.from_numpy(case.groups))


def _row(out, b, n):
    k = int(out["n_groups"][b])
    assert not out["groups"][b, k:].any() and not out["kinds"][b, k:].any(), "zero behind the count"
    return dict(entries=list(zip(out["groups"][b, :k].tolist(), out["kinds"][b, :k].tolist())),
                atom_kinds=out["atom_kinds"][b].numpy(), status=int(out["status"][b]))


def _check(got, want, n, what):
    assert got["status"] == want["status"], (what, got["status"], want["status"])
    assert got["entries"] == want["entries"], (what, got["entries"], want["entries"])
    assert got["atom_kinds"][:n].tolist() == want["atom_kinds"].tolist() and not got["atom_kinds"][n:].any(), what


@pytest.mark.parametrize("case", CC.cases(), ids=lambda c: c.name)
def test_cases_match_the_restatement(case):
    """R = 1, 255, 256, 257, 513 and molecules of 1, 27, 63 and 64 atoms at N = 64."""
    out = _launch([case], 64, _prepared(case))
    want = case.expected()
    _check(_row(out, 0, case.n), want, case.n, case.name)
    print(f"\nCONTACTS {case.name}: {len(want['entries'])} groups, kinds {sorted({k for _, k in want['entries']})}")


def test_a_group_in_two_tiles_and_two_kinds_in_one():
    case = CC.cases()[4]                                           # R = 513: three tiles, group j % 40
    prepared = _prepared(case)
    want = case.expected()
    y, rj, tj, g = (prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(), prepared.types.numpy(), prepared.groups.numpy())
    touched = np.bitwise_or.reduce(CR.pair_kinds(case.x, IR.radii(case.z), case.t, y, rj, tj), axis=0) != 0
    spread = [grp for grp, _ in want["entries"] if len({j // 256 for j in np.flatnonzero(touched & (g == grp))}) >= 2]
    assert spread, "no group is touched in two different tiles: the case does not show what it is for"
    _check(_row(_launch([case], 64, prepared), 0, case.n), want, case.n, "R513")
    two = CC.two_kinds_one_group()
    got = _row(_launch([two], 8, _prepared(two)), 0, two.n)
    _check(got, two.expected(), two.n, "two kinds")
    assert got["entries"] == [(5, CR.CONTACT | CR.HYDROPHOBIC | CR.HBOND_DONOR)] and got["atom_kinds"][:2].tolist() == [5, 3]


def test_bits_do_not_depend_on_batch_row_width_skipping_or_receptor_order():
    case = CC.cases()[3]
    prepared = _prepared(case)
    want = case.expected()
    others = [CC.cases()[1], CC.cases()[2]]
    small = CC.pocket("n7", 41, 7, 300)
    p_small = _prepared(small)
    for width, row, skip in ((27, 0, True), (64, 0, False), (64, 7, True), (33, 3, False)):
        batch = [others[i % 2] for i in range(8)]
        batch[row] = case
        _check(_row(_launch(batch, width, prepared, skip_tiles=skip), row, case.n), want, case.n, (width, row, skip))
    for width, row in ((8, 0), (64, 0), (64, 7)):
        batch = [CC.Case("n7'", small.x[::-1] + np.float32(0.6), small.z, small.t, small.rec, small.rec_z, small.rec_t,
                         small.groups)] * 8
        batch[row] = small
        _check(_row(_launch(batch, width, p_small), row, small.n), small.expected(), small.n, ("n7", width, row))
    CT, _ = _mods()
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(case.rec)))
    shuffled = CT.prepare_receptor(tuple(t[perm] for t in case.receptor), groups=torch.from_numpy(case.groups)[perm])
    assert all(torch.equal(a, b) for a, b in zip(shuffled[:4], prepared[:4]))
    _check(_row(_launch([case], 64, shuffled), 0, case.n), want, case.n, "permuted")


def test_empty_and_non_finite_rows_beside_good_rows():
    a, b = CC.cases()[1], CC.pocket("n9", 42, 9, 255)
    prepared = _prepared(a)
    x, r, t, n = _pad([a, a, a, a], 32)
    n[1] = 0
    x[2, 5, 1] = float("nan")
    CT, _ = _mods()
    ref = a.expected()["entries"][:5]
    out = {k: v.cpu() for k, v in CT.fingerprint_typed(prepared, x, n, r, t, device=DEV,
                                                       reference=([g for g, _ in ref], [k for _, k in ref])).items()}
    assert out["status"].tolist() == [CR.OK, CR.EMPTY, CR.NONFINITE, CR.OK]
    for row in (0, 3):
        _check(_row(out, row, a.n), a.expected(), a.n, row)
    for row in (1, 2):
        assert int(out["n_groups"][row]) == 0 and not out["groups"][row].any() and not out["kinds"][row].any()
        assert not out["atom_kinds"][row].any()
    n_ref = sum(CR.popcount(k & CR.DEFAULT_KINDS) for _, k in ref)
    assert [out[k][1].item() for k in ("n_bits", "n_ref_bits", "n_common")] == [0, n_ref, 0]
    assert [out[k][2].item() for k in ("n_bits", "n_ref_bits", "n_common")] == [-1, -1, -1]
    assert math.isnan(out["recovery"][2]) and math.isnan(out["tanimoto"][2])


@pytest.mark.parametrize("which", ["contact", "hbond"])
def test_fp32_neighbours_of_the_thresholds(which):
    rows = CC.threshold_rows(which)
    out = _launch(rows, 4, _prepared(rows[0]))
    wants = [c.expected() for c in rows]
    bit = CR.CONTACT if which == "contact" else CR.HBOND_DONOR
    sides = {bool(w["entries"] and w["entries"][0][1] & bit) for w in wants}
    assert sides == {True, False}, "the rows lie on one side of the threshold only"
    for b, (c, w) in enumerate(zip(rows, wants)):
        _check(_row(out, b, 1), w, 1, c.name)


@pytest.mark.parametrize("kind,extra,status", [("groups", 0, CR.OK), ("groups", 1, CR.OVERFLOW), ("candidates", 0, CR.OK),
                                               ("candidates", 1, CR.OVERFLOW)])
def test_capacities_exactly_and_one_over(kind, extra, status):
    """256 groups / 2 048 receptor atoms in contact fit; one more is OVERFLOW - a status, not a fault - and the row beside
    it is untouched."""
    case = CC.capacity(kind, extra)
    want = case.expected()
    assert want["status"] == status and len(want["entries"]) == ((256 if kind == "groups" else 200) if status == CR.OK else 0)
    lone = CC.Case("lone", [[0.0, 0.0, 30.0]], [6], [4], case.rec, case.rec_z, case.rec_t, case.groups)
    ref = ([0, 1, 2], [2, 2, 2])
    out = _launch([case, lone, case], 2, _prepared(case), reference=ref)
    for b in (0, 2):
        _check(_row(out, b, 1), want, 1, case.name)
        if status == CR.OVERFLOW:
            assert [out[k][b].item() for k in ("n_bits", "n_ref_bits", "n_common")] == [-1, -1, -1]
    _check(_row(out, 1, 1), lone.expected(), 1, "the row beside it")


@pytest.mark.parametrize("k_ref", [0, 1, 256])
def test_reference_join(k_ref):
    CT, _ = _mods()
    full = CC.capacity("groups", 0)
    base = full.expected()["entries"]                              # 256 entries, all HYDROPHOBIC | CONTACT
    g = np.random.default_rng(k_ref)
    ref = [(grp, int(g.integers(0, 16))) for grp, _ in base][:k_ref]
    near = CC.Case("near", [[2.5, 0.2, -0.4]], [6], [4], full.rec, full.rec_z, full.rec_t, full.groups)
    rows = [full, near]
    for mask in (CT.DEFAULT_KINDS, CT.ALL_KINDS, CT.CONTACT):
        out = _launch(rows, 2, _prepared(full), reference=([a for a, _ in ref], [b for _, b in ref]), kinds=mask)
        for b, c in enumerate(rows):
            n_bits, n_ref, n_common, rec, tan = CR.compare(c.expected(), ref, mask)
            assert [out[k][b].item() for k in ("n_bits", "n_ref_bits", "n_common")] == [n_bits, n_ref, n_common], (mask, b)
            for got, want in ((out["recovery"][b].item(), rec), (out["tanimoto"][b].item(), tan)):
                assert (math.isnan(got) and math.isnan(want)) or got == want, (mask, b, got, want)
            assert out["recovery"].dtype == torch.float64
        if k_ref == 0:
            assert torch.isnan(out["recovery"]).all()


def test_cross_kernel_invariants_with_the_interaction_score():
    CT, IX = _mods()
    batch = list(CC.cases()[1:5]) + [CC.cases()[6], CC.two_kinds_one_group()]
    for case in batch:
        prepared = _prepared(case)
        x, r, t, n = _pad([case], 64)
        fp = {k: v.cpu() for k, v in CT.fingerprint_typed(prepared, x, n, r, t, device=DEV).items()}
        sc = IX.score_typed(prepared.typed, x, n, r, t, torch.zeros(1, dtype=torch.int32), device=DEV)
        k = int(fp["n_groups"][0])
        kinds = fp["kinds"][0, :k].tolist()
        hb = CR.HBOND_DONOR | CR.HBOND_ACCEPTOR
        assert (int(sc["hbonds"][0]) > 0) == any(v & hb for v in kinds), case.name
        hyd = sc["atom_terms"][0, : case.n, 3].cpu()
        # some pair's hyd term is 1 - decided per pair by the score's own restatement - iff there is a HYDROPHOBIC entry ...
        terms = IR.pair_terms(case.x, IR.radii(case.z), case.t, prepared.xyzr[:, :3].numpy(), prepared.xyzr[:, 3].numpy(),
                              prepared.types.numpy())[0]
        assert bool((terms[3] == 1.0).any()) == any(v & CR.HYDROPHOBIC for v in kinds), case.name
        # ... and on the kernels' own outputs: an atom with the HYDROPHOBIC bit has a HYD sum of at least 1, one with a hydrogen
        # bond bit a HB sum of at least 1, and a molecule whose atoms' HYD sums all stay below 1 has no HYDROPHOBIC entry
        atoms = fp["atom_kinds"][0, : case.n]
        assert bool((hyd[(atoms & CR.HYDROPHOBIC) != 0] >= 1).all()), case.name
        assert bool((sc["atom_terms"][0, : case.n, 4].cpu()[(atoms & hb) != 0] >= 1).all()), case.name
        if not bool((hyd >= 1).any()):
            assert not any(v & CR.HYDROPHOBIC for v in kinds), case.name
        assert bool(((atoms & hb) != 0).any()) == (int(sc["hbonds"][0]) > 0)


def test_one_row_against_a_receptor_above_65536_atoms():
    """The tile list's second compaction round: the inputs of tests/large_receptor_cases.py, read-only; tile skipping on."""
    import large_receptor_cases as LR
    CT, _ = _mods()
    R, kind = 131072, "BOTH"
    rec = LR.receptor(R)
    groups = torch.arange(R, dtype=torch.int32) // 8                    # runs of eight atoms of the kernel's order
    prepared = CT.PreparedReceptor(rec.ix, rec.ix_types, rec.ix_spheres, groups)
    launch = LR.launch(R, kind, "interactions")
    row, xb, _ = launch["rows"][0]
    idx = LR.subset(R, kind, "interactions", 0)
    y, rj, tj = LR.receptor_args(R, "interactions", idx)
    want = CR.fingerprint(xb, LR.ligand_radii("interactions", row), row.t, y, rj, tj, groups.numpy()[idx])
    out = {k: v.cpu() for k, v in CT.fingerprint_typed(
        prepared, torch.from_numpy(launch["x"][:1]), torch.from_numpy(launch["n"][:1]), torch.from_numpy(launch["r"][:1]),
        torch.from_numpy(launch["t"][:1]), device=DEV, skip_tiles=True).items()}
    _check(_row(out, 0, row.n), want, row.n, "large")
    tiles = {int(grp) * 8 // 256 for grp, _ in want["entries"]}
    print(f"\nCONTACTS large: {len(want['entries'])} groups in tiles {sorted(tiles)}")
    assert want["entries"] and min(tiles) < LR.ROUND <= max(tiles), "groups of both rounds are in contact"


def test_sentinels_around_every_output_buffer():
    """The raw entry on caller-owned buffers with 256 guard bytes on either side: nothing outside its outputs is written."""
    from ml_conformer_generator_amd import _lib
    CT, _ = _mods()
    cases = [CC.cases()[1], CC.cases()[5], CC.cases()[1]]
    prepared = _prepared(cases[0])
    x, r, t, n = (a.to(DEV) for a in _pad(cases, 31))
    B, N, G = 3, 31, 256
    nbytes = dict(groups=B * 256 * 4, kinds=B * 256, n_groups=B * 4, atom_kinds=B * N, status=B * 4, counts=B * 3 * 4)
    raw = {k: torch.full((m + 2 * G,), SENTINEL, dtype=torch.uint8, device=DEV) for k, m in nbytes.items()}
    rec, rec_t, rec_g, sph = (a.to(DEV) for a in (prepared.xyzr, prepared.types, prepared.groups, prepared.spheres))
    ref_g = torch.tensor([3, 4, 9], dtype=torch.int32, device=DEV)
    ref_k = torch.tensor([2, 6, 15], dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().mcg_receptor_contacts(
        _lib.dptr(x), _lib.dptr(r), _lib.dptr(t), _lib.dptr(n), B, N, _lib.dptr(rec), _lib.dptr(rec_t), _lib.dptr(rec_g),
        int(rec.shape[0]), _lib.dptr(sph), _lib.dptr(ref_g), _lib.dptr(ref_k), 3, CT.DEFAULT_KINDS,
        *(raw[k].data_ptr() + G for k in ("groups", "kinds", "n_groups", "atom_kinds", "status", "counts")),
        _lib.current_stream_ptr(DEV)), "mcg_receptor_contacts")
    torch.cuda.synchronize()
    host = {k: v.cpu() for k, v in raw.items()}
    for k, flat in host.items():
        assert (flat[:G] == SENTINEL).all() and (flat[-G:] == SENTINEL).all(), k
    inner = {k: host[k][G:-G].contiguous() for k in host}
    want = _launch(cases, N, prepared, reference=([3, 4, 9], [2, 6, 15]))
    assert torch.equal(inner["groups"].view(torch.int32).view(B, 256), want["groups"])
    assert torch.equal(inner["kinds"].view(B, 256), want["kinds"]) and torch.equal(inner["atom_kinds"].view(B, N), want["atom_kinds"])
    assert torch.equal(inner["status"].view(torch.int32), want["status"])
    assert torch.equal(inner["n_groups"].view(torch.int32), want["n_groups"])
    assert torch.equal(inner["counts"].view(torch.int32).view(B, 3)[:, 2], want["n_common"])


def test_contact_fingerprint_on_graphs_equals_the_typed_launch():
    import interactions_cases as K
    CT, IX = _mods()
    from test_interactions_gpu import _padded
    mols = [K.MOLECULES[name][0] for name in ("toluene", "acetamide", "biphenyl", "pyridine", "ethanol", "butane")]
    z, bonds, n = _padded(mols, 41)
    g = np.random.default_rng(8)
    x = torch.zeros(len(mols), 41, 3)
    case = CC.cases()[2]
    for b, (_, _, k) in enumerate(mols):
        x[b, :k] = torch.from_numpy((IR.walk(k, g) * 0.8 + case.x.mean(0)).astype(np.float32))
    prepared = _prepared(case)
    out = {k: v.cpu() for k, v in CT.contact_fingerprint(prepared, x, n, z, bonds, device=DEV).items()}
    seen = 0
    for b, (zz, adj, k) in enumerate(mols):
        t = IR.ligand_types(zz, adj, k, K.pharm_types((zz, adj, k)))
        want = CR.fingerprint(x[b, :k].numpy(), IR.radii(zz), t, case.rec, IR.radii(case.rec_z), case.rec_t, case.groups)
        _check(_row(out, b, k), want, k, b)
        seen += len(want["entries"])
    assert seen > 0
    named = CT.labels(prepared, out["groups"], out["kinds"], out["n_groups"])
    assert [len(r) for r in named] == out["n_groups"].tolist() and all(isinstance(lab, int) for r in named for lab, _ in r)


# ----------------------------------------------------------------------------------------------- generation entries
NEW = ("contact_groups", "contact_kinds", "contact_atom_kinds", "contact_status", "contact_recovery", "contact_tanimoto",
       "contact_labels", "contact_reference")


def _plainly(v):
    return v.tolist() if torch.is_tensor(v) else [_plainly(x) for x in v] if isinstance(v, (list, tuple)) else v


def _flat(m):
    """Every measured value of a record but the new ones, as its properties give it."""
    return {k: _plainly(getattr(m, k)) for k in vars(m._measured) if k not in NEW}


def _own(CT, prepared, m, reference):
    k = len(m.atomic_numbers)
    out = CT.contact_fingerprint(prepared, m.coords[None], torch.tensor([k], dtype=torch.int32),
                                 torch.tensor([m.atomic_numbers], dtype=torch.int32), m.bond_orders[None], reference=reference,
                                 device=DEV)
    c = int(out["n_groups"][0])
    return dict(groups=out["groups"][0, :c].tolist(), kinds=out["kinds"][0, :c].tolist(), atoms=out["atom_kinds"][0].tolist(),
                status=int(out["status"][0]), recovery=float(out["recovery"][0]), tanimoto=float(out["tanimoto"][0]))


def _describes(CT, prepared, m, reference):
    """The record's contact fields are `contact_fingerprint` of its own returned coordinates and graph."""
    own = _own(CT, prepared, m, reference)
    assert (m.contact_groups, m.contact_kinds, m.contact_atom_kinds, m.contact_status) == (
        own["groups"], own["kinds"], own["atoms"], own["status"]), m.sample_id
    for got, want in ((m.contact_recovery, own["recovery"]), (m.contact_tanimoto, own["tanimoto"])):
        assert got == want or (math.isnan(got) and math.isnan(want)), m.sample_id
    assert m.residue_contacts == tuple((prepared.group_labels[g], CT.kind_names(k)) for g, k in zip(own["groups"], own["kinds"]))
    hit, miss = CT.compare_entries(own["groups"], own["kinds"], *reference)
    names = lambda found: tuple((prepared.group_labels[g], CT.kind_names(k)) for g, k in found)          # noqa: E731
    assert m.contacts_recovered == names(hit) and m.contacts_missed == names(miss)
    return own


def test_generation_with_contacts(monkeypatch):
    from test_receptor_relief_gpu import _posed_setup
    CT, _ = _mods()
    gen, ref, kw, base = _posed_setup(monkeypatch)
    pdb = CC.pocket_pdb()
    n_ref = int(ref.shape[0])
    z_ref = ([6, 6, 7, 6, 8, 6, 6, 8, 6, 7] * 7)[:n_ref]
    bonds_ref = torch.zeros(n_ref, n_ref, dtype=torch.int8)
    for i in range(n_ref - 1):
        bonds_ref[i, i + 1] = bonds_ref[i + 1, i] = 1
    graph = (z_ref, bonds_ref)
    launched = []
    real = gen._contact_fingerprint
    monkeypatch.setattr(gen, "_contact_fingerprint", lambda *a, **k: launched.append(int(a[1].shape[0])) or real(*a, **k))

    scored = gen.generate_conformers(receptor=pdb, interaction_scores=True, **kw)
    assert launched == [] and all(getattr(m, f) is None for m in scored for f in NEW + ("residue_contacts", "contacts_missed"))
    got = gen.generate_conformers(receptor=pdb, interaction_scores="contacts", reference_graph=graph, **kw)
    assert launched == [1, len(got)]                                             # the reference once, then the rows
    assert got == scored and [_flat(m) for m in got] == [_flat(m) for m in scored]           # every other bit as `True` gives it
    prepared = CT.prepare_receptor(pdb)
    ref_out = CT.contact_fingerprint(prepared, ref[None].float(), torch.tensor([n_ref], dtype=torch.int32),
                                     torch.tensor([z_ref], dtype=torch.int32), bonds_ref[None], device=DEV)
    c = int(ref_out["n_groups"][0])
    reference = (ref_out["groups"][0, :c].tolist(), ref_out["kinds"][0, :c].tolist())
    assert sum(CR.popcount(k & CR.DEFAULT_KINDS) for k in reference[1]) > 0, "the reference touches nothing that counts"
    recovery = {}
    for m in got:
        if m.pose is None:
            assert all(getattr(m, f) is None for f in NEW)
            continue
        own = _describes(CT, prepared, m, reference)
        assert m.contact_reference == (tuple(reference[0]), tuple(reference[1]), CT.DEFAULT_KINDS)
        recovery[m.sample_id] = own["recovery"]
    assert len(recovery) >= 8 and len(set(recovery.values())) >= 2 and any(m.contact_groups for m in got if m.pose is not None)
    values = sorted(set(recovery.values()))
    t = (values[0] + values[1]) / 2 if len(values) > 1 else values[0]
    want = [i for i in sorted(recovery) if recovery[i] >= t]
    for entry in ("generate_conformers", "generate_conformers_sharded", "forward"):
        kept = getattr(gen, entry)(receptor=pdb, interaction_scores=("contacts", t), reference_graph=graph, **kw)
        assert [m.sample_id for m in kept] == want and 0 < len(kept) < len(recovery), entry
    again = gen.generate_conformers_sharded(receptor=pdb, interaction_scores="contacts", reference_graph=graph, **kw)
    assert [(_flat(m), m.residue_contacts, m.contact_recovery) for m in again if m.pose is not None] == \
        [(_flat(m), m.residue_contacts, m.contact_recovery) for m in got if m.pose is not None]
    # with optimise_pose the fields describe the optimised coordinates
    moved = gen.generate_conformers(receptor=pdb, interaction_scores="contacts", reference_graph=graph, optimise_pose=True, **kw)
    n_moved = 0
    for m, before in zip(moved, got):
        if m.pose is None:
            continue
        _describes(CT, prepared, m, reference)
        n_moved += int(not torch.equal(m.coords, before.coords))
    assert n_moved > 0
    # without the reference's graph: the fingerprint alone
    bare = gen.generate_conformers(receptor=pdb, interaction_scores="contacts", **kw)
    assert [(m.contact_groups, m.contact_kinds) for m in bare] == [(m.contact_groups, m.contact_kinds) for m in got]
    assert all(m.contact_recovery is None and m.contacts_missed is None and m.contact_reference is None for m in bare)
    print(f"\nCONTACTS e2e: reference {len(reference[0])} groups; recovery {sorted(recovery.values())}; >= {t:.3f} keeps {want}; "
          f"{n_moved} rows moved by optimise_pose; {got[0].residue_contacts[:3]}")
