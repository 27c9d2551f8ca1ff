"""Rings and scaffolds, host side (no GPU): the restatement (`scaffold_ref`) against the hand-written values of the named
cases, its two forms against each other on a seeded fuzz, renumbering, the mutation checks, the options of the generation
entries against a stand-in for `gen._ring_scaffolds` backed by the restatement, and the C entries' argument checks."""
import ctypes
import os
import random
import subprocess

import pytest
import torch

import canonical_cases as C
import canonical_ref as R
import scaffold_cases as SC
import scaffold_ref as SR
from ml_conformer_generator_amd import canonical as CN
from ml_conformer_generator_amd import postprocess
from ml_conformer_generator_amd import scaffold as SF
from ml_conformer_generator_amd.handoff import GeneratedMolecule, measured_from_tensors
from test_canonical_host import _graph_shard, _seam_canonical
from test_fingerprint_host import _MolStage, _seam_fingerprints
from test_shape_overlay_host import _no_device, _ref, _shell_generator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", list(SC.NAMED))
def test_reference_reproduces_the_hand_written_values(name):
    mol = SC.NAMED[name][0]
    want = SC.expected(name)
    assert SR.perceive(*mol) == want
    assert SR.perceive(*mol, form="pruning") == want


def test_hand_written_values_say_what_the_issue_says():
    counts = {name: dict(zip(SR.COUNT_NAMES, SC.expected(name)["counts"])) for name in SC.NAMED}
    assert counts["cubane"]["n_rings"] == 5 and counts["naphthalene"]["n_rings"] == 2 and counts["norbornane"]["n_rings"] == 2
    assert counts["14-ring"]["max_ring_size"] == 14 and counts["bicyclo[2.2.2]octane"]["max_ring_size"] == 6
    assert (counts["spiro[4.5]decane"]["n_ring_systems"], counts["spiro[4.5]decane"]["min_ring_size"],
            counts["spiro[4.5]decane"]["max_ring_size"]) == (1, 5, 6)
    assert counts["biphenyl"]["n_ring_systems"] == 2 and counts["biphenyl"]["linker_atoms"] == 0
    assert counts["diphenylmethane"]["linker_atoms"] == 1 == counts["2,2-diphenylpropane"]["linker_atoms"]
    assert counts["benzophenone"]["exo_atoms"] == 1 == counts["cyclohexanone"]["exo_atoms"]
    assert SC.expected("64-ring")["masks"][0] == 2 ** 64 - 1 and SC.expected("64-ring")["ring_nb"][63] == 1 | 1 << 62
    assert SC.expected("64-chain")["masks"] == [0, 0, 0, 0] == SC.expected("butane")["masks"]
    assert counts["phenyl-C10-cyclopropane"]["linker_atoms"] == 10


def test_two_forms_agree_on_the_fuzz():
    mols = SC.fuzz_set()
    assert len(mols) == 320 and {m[2] for m in mols} == set(range(1, 65))
    assert all(max(sum(1 for c in row if c) for row in m[1]) <= 4 for m in mols)
    with_linker = with_exo = 0
    for k, m in enumerate(mols):
        closed = SR.perceive(*m)
        assert closed == SR.perceive(*m, form="pruning"), k
        with_linker += closed["counts"][5] > 0
        with_exo += closed["counts"][6] > 0
    assert with_linker >= 16 and with_exo >= 16


def test_renumbering_permutes_the_atoms_and_keeps_counts_and_identities():
    rng = random.Random(7)
    for name, (mol, _) in SC.NAMED.items():
        base = SR.perceive(*mol)
        p = list(range(mol[2]))
        rng.shuffle(p)
        moved = R.permute(*mol, p)
        got = SR.perceive(*moved)
        assert got == SR.permuted(base, p), name
        assert got["counts"] == base["counts"], name
        if mol[2] <= 19:                               # (the wide rings take the canonical restatement seconds)
            for generic in (False, True):
                assert SR.identity(*moved, generic=generic) == SR.identity(*mol, generic=generic), name


def test_scaffold_identities_of_the_restatement():
    toluene, benzene = SC.NAMED["toluene"][0], SC.NAMED["benzene"][0]
    assert SR.identity(*toluene) == SR.identity(*SC.ETHYLBENZENE) == SR.identity(*benzene) == R.identity_bytes(*benzene)
    assert SR.identity(*SC.PYRIDINE) != SR.identity(*benzene)
    assert SR.identity(*SC.PYRIDINE, generic=True) == SR.identity(*benzene, generic=True)
    ketone = SC.NAMED["cyclohexanone"][0]
    assert SR.identity(*ketone) != SR.identity(*SC.CYCLOHEXANE)
    assert SR.identity(*ketone, generic=True) == SR.identity(*SC.CYCLOHEXANE, generic=True)
    assert SR.identity(*SC.NAMED["butane"][0]) == b"" == SR.identity(*SC.NAMED["one atom"][0])
    assert SR.scaffold(*SC.NAMED["benzophenone"][0])[3] == list(range(14))
    assert SR.scaffold(*SC.NAMED["benzophenone"][0], generic=True)[3] == list(range(13))
    assert SR.scaffold(*SC.NAMED["2,2-diphenylpropane"][0])[3] == list(range(13))


# ----------------------------------------------------------------------------------------------- the mutation check
@pytest.mark.parametrize("mutation", SR.MUTATIONS)
def test_every_planted_mistake_is_caught_by_a_named_case(mutation):
    caught = [name for name, (mol, _) in SC.NAMED.items() if SR.perceive(*mol, mutate=mutation) != SC.expected(name)]
    assert SC.CATCHES[mutation] in caught, caught
    assert set(SC.CATCHES) == set(SR.MUTATIONS)


# ----------------------------------------------------------------------------------------------- the module, host side
def test_group_by_scaffold_and_record_fields():
    a, b = (5, b"x"), (5, b"y")
    assert SF.group_by_scaffold([a, b, a, None, SF.EMPTY_IDENTITY, None, b, (0, b"")]) == [[0, 2], [1, 6], [3], [4, 7], [5]]
    assert SF.group_by_scaffold([]) == []
    mols = [SC.NAMED["benzophenone"][0], SC.NAMED["butane"][0]]
    found = _seam_scaffolds([])(*C.pad_batch(mols, 16), False)
    recs = measured_from_tensors(SF.record_fields(found, with_smiles=True), 2)
    assert (recs[0].n_rings, recs[0].n_ring_systems, recs[0].min_ring_size, recs[0].max_ring_size) == (2, 2, 6, 6)
    assert recs[0].scaffold_atoms == list(range(14)) and recs[0].scaffold_status == 0 and recs[0].scaffold_key > 0
    assert isinstance(recs[0].ring_sizes, tuple)                                  # (batch, row): sliced on first read
    assert recs[1].scaffold_atoms == [] and recs[1].scaffold_status == CN.STATUS_EMPTY and recs[1].scaffold_key == 0
    assert recs[1].scaffold_smiles == "" and R.identity_bytes(*R.read_smiles(recs[0].scaffold_smiles)[:3]) == \
        R.identity_bytes(*mols[0])
    ordered = _seam_canonical([])(found["atomic_numbers"], found["bond_orders"], found["n"])      # the bytes are canonical's
    assert [e and e[1] for e in SF.identities_of(found, ordered)][:1] == \
        CN.identity_bytes(found["atomic_numbers"], found["bond_orders"], found["n"], ordered=ordered)[:1] == \
        [R.identity_bytes(*mols[0])]
    with pytest.raises(ValueError):
        SF.ring_perception(torch.zeros(1, 65, dtype=torch.int32), torch.zeros(1, 65, 65, dtype=torch.int8), torch.tensor([3]))
    with pytest.raises(ValueError):
        SF.induced_subgraph(torch.zeros(1, 5, dtype=torch.int32), torch.zeros(1, 5, 5, dtype=torch.int8), torch.tensor([3]),
                            torch.zeros(1, dtype=torch.int64), mode=2)
    with pytest.raises(ValueError):
        SF.murcko_scaffolds(torch.zeros(1, 5, dtype=torch.int32), torch.zeros(1, 5, 5, dtype=torch.int8), torch.tensor([3]),
                            generic="yes")


# ----------------------------------------------------------------------------------------------- options
# `test_canonical_host._graph_shard`'s stub shape scores, by sample id: 0.3 0.9 0.5 0.8 0.2 0.6 0.4 0.7
# atom 0 joins nine cyclopropanes: a linker atom with nine neighbours - the scaffold has no canonical order (DEGREE)
_HUB = R.mol([6] * 28, [b for k in range(9) for b in [(0, 1 + 3 * k, 1), (1 + 3 * k, 2 + 3 * k, 1), (2 + 3 * k, 3 + 3 * k, 1),
                                                      (3 + 3 * k, 1 + 3 * k, 1)]])


def _shard_molecules():
    """sample id -> molecule.  0, 1 and 3 share benzene's scaffold, 6 (pyridine) only its framework; 2 and 7 are acyclic;
    4 and 5 are one graph whose scaffold has no canonical order."""
    return [SC.NAMED["toluene"][0], SC.NAMED["benzene"][0], SC.NAMED["butane"][0], SC.ETHYLBENZENE, _HUB,
            C.renumbered(random.Random(8), _HUB), SC.PYRIDINE, SC.NAMED["one atom"][0]]


def _seam_scaffolds(calls):
    """`_ring_scaffolds` by the restatement, on the host: `scaffold.murcko_scaffolds`' result."""
    def run(z, bonds, n, generic):
        z, bonds, n = torch.as_tensor(z), torch.as_tensor(bonds), torch.as_tensor(n).reshape(-1).tolist()
        calls.append((len(n), bool(generic)))
        B, W = len(n), int(bonds.shape[1])
        sub = dict(atomic_numbers=torch.zeros(B, W, dtype=torch.int32), bond_orders=torch.zeros(B, W, W, dtype=torch.int8),
                   n=torch.zeros(B, dtype=torch.int32), atom_map=torch.full((B, W), -1, dtype=torch.int32))
        per = dict(ring_size=torch.zeros(B, W, dtype=torch.int32), ring_system=torch.full((B, W), -1, dtype=torch.int32),
                   counts=torch.zeros(B, 8, dtype=torch.int32))
        for b, k in enumerate(n):
            mol = (z[b, :k].tolist(), bonds[b, :k, :k].tolist(), k)
            p = SR.perceive(*mol)
            per["ring_size"][b, :k] = torch.tensor(p["ring_size"], dtype=torch.int32)
            per["ring_system"][b, :k] = torch.tensor(p["ring_system"], dtype=torch.int32)
            per["counts"][b] = torch.tensor(p["counts"], dtype=torch.int32)
            sz, sadj, sn, keep = SR.scaffold(*mol, generic=bool(generic), perceived=p)
            sub["n"][b] = sn
            if sn:
                sub["atomic_numbers"][b, :sn] = torch.tensor(sz, dtype=torch.int32)
                sub["bond_orders"][b, :sn, :sn] = torch.tensor(sadj, dtype=torch.int8)
                sub["atom_map"][b, :sn] = torch.tensor(keep, dtype=torch.int32)
        ordered = _seam_canonical([])(sub["atomic_numbers"], sub["bond_orders"], sub["n"])
        return dict(sub, order=ordered["order"], status=ordered["status"], key=ordered["key"],
                    identity=SF.identities_of(sub, ordered), perceived=per)
    return run


def _generator(calls, finisher=None):
    gen = _shell_generator(finisher=finisher)
    gen._ring_scaffolds = _seam_scaffolds(calls)
    gen._canonical_order = _seam_canonical([])
    gen._graph_fingerprints = _seam_fingerprints([])
    gen._score = lambda ref, coords, n: coords[:, 0, 1].clone()
    return gen


def test_parse_request_accepts_the_two_new_values_and_refuses_the_bad_ones():
    gen = _shell_generator()
    for value in ("scaffold", "framework"):
        req = postprocess.parse_request(gen, None, unique=value)
        assert req.unique == value and req.needs_scaffold and req.measures and req.removes
        assert not (req.needs_identity or req.needs_canonical or req.needs_fingerprints or req.needs_stereo)
    for value in (False, True, "exact", "stereo"):
        assert not postprocess.parse_request(gen, None, unique=value).needs_scaffold
    assert not postprocess.Request().needs_scaffold and "scaffold" in [f.name for f in
                                                                        __import__("dataclasses").fields(postprocess.Rows)]
    for bad in ("Scaffold", "scaffolds", "murcko", b"scaffold", 1, None, "frameworks"):
        with pytest.raises(ValueError, match="unique must be True or False"):
            postprocess.parse_request(gen, None, unique=bad)
    assert len(postprocess.REQUEST_KEYWORDS) == 37


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_scaffold_refusals_happen_before_any_device_work(entry):
    from ml_conformer_generator_amd import host_pool as HP
    gen = _shell_generator()
    gen._generate_shard = gen._ring_scaffolds = gen._canonical_order = gen._score = _no_device
    call = getattr(gen, entry)
    for bad in ("scaffolds", "Framework", 2):
        with pytest.raises(ValueError, match="unique must be True or False"):
            call(reference_conformer=_ref(), n_samples=4, unique=bad)
    gen.finisher = HP.TaskRef(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_host_tasks.py"),
                              "finish_tag_chunk")
    for value in ("scaffold", "framework"):
        with pytest.raises(ValueError, match="finisher"):
            call(reference_conformer=_ref(), n_samples=4, unique=value)


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_proxy_path_keeps_the_best_ranked_row_of_each_scaffold(entry):
    mols = _shard_molecules()
    calls = []
    gen = _generator(calls)
    gen._generate_shard = _graph_shard(mols)
    kw = dict(reference_conformer=_ref(), n_samples=8)
    call = getattr(gen, entry)

    plain = call(**kw)
    assert calls == [] and [m.sample_id for m in plain] == list(range(8))         # no option: the seam is not touched
    assert all(m.n_rings is None and m.scaffold_atoms is None and m.scaffold_status is None for m in plain)

    def ids(**more):
        return [m.sample_id for m in call(**dict(kw, **more))]
    # no score: the lowest sample id of each scaffold; the acyclic rows 2 and 7 collapse into one; the rows without an
    # identity, 4 and 5, both stay although they are one graph
    assert ids(unique="scaffold") == [0, 2, 4, 5, 6] and calls == [(8, False)]
    assert ids(unique="framework") == [0, 2, 4, 5] and calls[-1] == (8, True)      # pyridine is benzene's framework
    # ranked by the shape score: 1 (0.9) of the benzenes, 7 (0.7) of the acyclic rows
    assert ids(unique="scaffold", shape_scores=True) == [1, 4, 5, 6, 7]
    assert ids(unique="framework", shape_scores=True) == [1, 4, 5, 7]
    # `unique` stands in front of the walk: the three best of the five that remain
    assert sorted(ids(unique="scaffold", top_k=3)) == [1, 5, 7]
    assert sorted(ids(unique="scaffold", top_k=3)) != sorted(ids(top_k=3)) == [1, 3, 7]
    # `exclude_graphs` stands in front of `unique`: benzene itself goes first, then its scaffold keeps the best of the rest
    benzene = SC.NAMED["benzene"][0][:2]
    assert ids(unique="scaffold", exclude_graphs=[benzene]) == [0, 2, 4, 5, 6]
    assert ids(unique="scaffold", exclude_graphs=[benzene], shape_scores=True) == [3, 4, 5, 6, 7]

    got = call(unique="scaffold", smiles=True, **kw)
    assert [m.sample_id for m in got] == [0, 2, 4, 5, 6]
    for m in got:
        mol = mols[m.sample_id]
        assert m == plain[m.sample_id]
        ref = SR.perceive(*mol)
        assert (m.n_rings, m.n_ring_systems, m.min_ring_size, m.max_ring_size) == tuple(ref["counts"][:4])
        assert m.ring_sizes == ref["ring_size"] and m.ring_systems == ref["ring_system"]
        assert m.scaffold_atoms == SR.scaffold(*mol, perceived=ref)[3]
    by_id = {m.sample_id: m for m in got}
    assert by_id[0].scaffold_smiles == "c1ccccc1" and by_id[0].smiles == "Cc1ccccc1"
    assert by_id[2].scaffold_smiles == "" and by_id[2].scaffold_status == CN.STATUS_EMPTY and by_id[2].scaffold_key == 0
    assert by_id[4].scaffold_smiles is None and by_id[4].scaffold_status == CN.STATUS_DEGREE == by_id[5].scaffold_status
    assert by_id[6].scaffold_smiles == "c1ccncc1" and by_id[6].scaffold_key != by_id[0].scaffold_key != 0
    assert all(m.scaffold_smiles is None for m in call(unique="scaffold", **kw))   # the string rides on `smiles`


def test_object_path_reads_the_mols_own_graphs():
    mols = _shard_molecules()
    calls = []
    gen = _generator(calls, finisher="rdkit")
    gen._generate_shard = _MolStage(gen, mols)                                   # sample 2 is dropped by the finish
    kw = dict(reference_conformer=_ref(), n_samples=8, sample_seed=5)

    def ids(**more):
        return [m.props["sample_id"] for m in gen.generate_conformers(**dict(kw, **more))]
    assert ids() == [0, 1, 3, 4, 5, 6, 7] and calls == []
    assert ids(unique="scaffold") == [0, 4, 5, 6, 7] and calls == [(7, False)]     # the live Mols in ONE batched call
    assert ids(unique="framework") == [0, 4, 5, 7]
    assert ids(unique="scaffold", exclude_graphs=[SC.NAMED["toluene"][0][:2]]) == [1, 4, 5, 6, 7]


def test_of_records_annotates_after_the_fact(monkeypatch):
    mols = [SC.NAMED["benzophenone"][0], SC.NAMED["butane"][0]]
    recs = [GeneratedMolecule(z, torch.zeros(n, 3), torch.tensor(adj, dtype=torch.int8)) for z, adj, n in mols]
    seam = _seam_scaffolds([])
    monkeypatch.setattr(SF, "murcko_scaffolds", lambda z, b, n, device=None, generic=False, check=True: seam(z, b, n, generic))
    out = SF.of_records(recs)
    assert out[0] is recs[0] and recs[0].n_rings == 2 and recs[0].scaffold_atoms == list(range(14))
    assert recs[0].ring_sizes == [6] * 12 + [0, 0] and recs[1].ring_systems == [-1] * 4 and recs[1].scaffold_smiles == ""
    assert recs[0]._measured is not recs[1]._measured and GeneratedMolecule([6], torch.zeros(1, 3),
                                                                            torch.zeros(1, 1, dtype=torch.int8)).n_rings is None
    assert SF.of_records([]) == []


# ----------------------------------------------------------------------------------------------- C ABI
def test_scaffold_entries_refuse_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check

    def rings(z=p, bonds=p, n=p, B=3, W=42, nb=p, size=p, system=p, masks=p, counts=p):
        return h.mcg_ring_scaffold(z, bonds, n, B, W, nb, size, system, masks, counts, None)

    def sub(z=p, bonds=p, n=p, mask=p, mode=0, B=3, W=42, zo=p, bo=p, no=p, mo=p):
        return h.mcg_induced_subgraph(z, bonds, n, mask, mode, B, W, zo, bo, no, mo, None)

    for bad in (dict(z=None), dict(bonds=None), dict(n=None), dict(nb=None), dict(size=None), dict(system=None),
                dict(masks=None), dict(counts=None), dict(B=-1), dict(B=16385), dict(W=0), dict(W=65), dict(W=-3)):
        assert rings(**bad) == 1, bad
        assert b"mcg_ring_scaffold" in h.mcg_last_error(), bad
    for bad in (dict(z=None), dict(bonds=None), dict(n=None), dict(mask=None), dict(zo=None), dict(bo=None), dict(no=None),
                dict(mo=None), dict(mode=-1), dict(mode=2), dict(B=-1), dict(B=16385), dict(W=0), dict(W=65)):
        assert sub(**bad) == 1, bad
        assert b"mcg_induced_subgraph" in h.mcg_last_error(), bad
    assert rings(B=0) == 0 and sub(B=0) == 0 and sub(B=0, mode=1) == 0           # nothing to do, nothing launched
    assert h.mcg_abi_version() == 4 and {"mcg_ring_scaffold", "mcg_induced_subgraph"} <= set(_lib.SIGNATURES)


def test_argument_check_program_builds_and_passes_under_host_sanitizers(tmp_path):
    """`make asan_scaffold`: both entries' argument checks in a stand-alone program under host-side ASan + UBSan, on the
    CPU."""
    exe = str(tmp_path / "scaffold_arg_check")
    csrc = os.path.join(ROOT, "ml_conformer_generator_amd", "csrc")
    built = subprocess.run(["make", "-C", csrc, "asan_scaffold", f"SCAFFOLD_CHECK={exe}"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and "0 wrong" in ran.stdout, ran.stdout + ran.stderr
