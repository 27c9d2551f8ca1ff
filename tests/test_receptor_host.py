"""Receptor contacts, host side (no GPU): PDB parsing, the radius table, the receptor forms and their refusals, every
refusal of the generation entries before any device work, the C entry's argument checks, records / Mol properties and
the clash filter through a stub contact seam on the proxy and the object path, and the same list on both ranks of a
world-size-2 gloo run."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ml_conformer_generator_amd import receptor as RC
from ml_conformer_generator_amd.cheminformatics import select_scored
from test_shape_overlay_host import (PosedMol, _free_port, _no_device, _ref, _shell_generator, _Stage, _stub_overlay,
                                     _stub_shard)


def _atom(serial, name, res, x, y, z, element="", alt=" ", rec="ATOM  "):
    """One fixed-column PDB ATOM / HETATM line."""
    return (f"{rec}{serial:5d} {name:<4}{alt}{res:>3} A{serial:4d}    {x:8.3f}{y:8.3f}{z:8.3f}  1.00 20.00"
            f"          {element:>2}")


def _name(n):
    """A PDB atom name in columns 13-16: one-letter elements start in column 14, four-character names in column 13."""
    return n if len(n) == 4 else " " + n


# ----------------------------------------------------------------------------------------------- PDB parsing
def test_pdb_element_column_and_atom_name_fallback():
    lines = [_atom(1, _name("CA"), "ALA", 1.0, 2.0, 3.0, "C"),
             _atom(2, _name("N"), "ALA", 4.0, 5.0, 6.0, "N"),
             _atom(3, "CL1 ", "LIG", 7.0, 8.0, 9.0, "CL", rec="HETATM"),      # two-letter element column
             _atom(4, "ZN  ", "ZN", 0.5, 0.5, 0.5, "ZN", rec="HETATM"),
             _atom(5, _name("OG"), "SER", 1.5, 1.5, 1.5)[:76],                # no element column: from the name
             _atom(6, "FE  ", "HEM", 2.5, 2.5, 2.5, rec="HETATM")[:76],       # two-letter element starting in col 13
             _atom(7, "BR1 ", "LIG", 3.5, 3.5, 3.5, rec="HETATM")[:76],
             _atom(8, _name("SD"), "MET", 4.5, 4.5, 4.5)[:78]]                # blank element column
    coords, z = RC.parse_pdb("\n".join(lines) + "\nEND\n")
    assert z.tolist() == [6, 7, 17, 30, 8, 26, 35, 16]
    assert coords.dtype == torch.float32 and coords[0].tolist() == [1.0, 2.0, 3.0]
    assert coords[7].tolist() == [4.5, 4.5, 4.5]


def test_pdb_skips_hydrogens_alt_locations_and_later_models():
    lines = ["HEADER    TEST", "MODEL        1",
             _atom(1, _name("CA"), "ALA", 1.0, 0.0, 0.0, "C"),
             _atom(2, _name("H"), "ALA", 2.0, 0.0, 0.0, "H"),
             _atom(3, _name("D"), "ALA", 3.0, 0.0, 0.0, "D"),
             _atom(4, "HG21", "THR", 4.0, 0.0, 0.0)[:76],                     # a hydrogen by its four-character name
             _atom(5, "HB2 ", "ALA", 4.0, 0.0, 0.0)[:76],                     # a hydrogen name in column 13
             _atom(6, _name("OG1"), "THR", 5.0, 0.0, 0.0, "O", alt="A"),
             _atom(7, _name("OG1"), "THR", 6.0, 0.0, 0.0, "O", alt="B"),    # second alternate location: skipped
             _atom(8, _name("CB"), "THR", 7.0, 0.0, 0.0, "C", alt="C"),
             "TER", "ENDMDL", "MODEL        2",
             _atom(9, _name("CA"), "ALA", 9.0, 0.0, 0.0, "C"), "ENDMDL"]
    coords, z = RC.parse_pdb("\n".join(lines))
    assert coords[:, 0].tolist() == [1.0, 5.0] and z.tolist() == [6, 8]
    assert RC.parse_pdb("REMARK nothing\n")[0].shape == (0, 3)


def test_pdb_refusals():
    good = _atom(1, _name("CA"), "ALA", 1.0, 2.0, 3.0, "C")
    bad_xyz = good[:30] + "   x.xxx" + good[38:]
    bad_el = _atom(1, _name("Q"), "UNK", 1.0, 2.0, 3.0, "Q")
    for text in (bad_xyz, bad_el, "HEADER only\nEND\n", _atom(1, _name("H"), "ALA", 1.0, 2.0, 3.0, "H"),
                 good[:30] + "     nan     0.0     0.0" + good[54:]):
        with pytest.raises(ValueError):
            RC.load_receptor(text)
    coords, z = RC.load_receptor(good)
    assert coords.shape == (1, 3) and z.tolist() == [6]


def test_radius_table():
    assert RC.vdw_radius(6) == 1.70 and RC.vdw_radius(7) == 1.55 and RC.vdw_radius(8) == 1.52
    assert RC.vdw_radius(16) == 1.80 and RC.vdw_radius(17) == 1.75 and RC.vdw_radius(35) == 1.85
    assert RC.vdw_radius(5) == 1.92                                      # boron: Mantina et al. 2009
    assert RC.vdw_radius(26) == RC.DEFAULT_RADIUS == 2.00                # iron: not in Bondi's table
    assert RC.vdw_radius(20) == 2.00
    from ml_conformer_generator_amd.config import ELEMENTS
    assert all(z in RC.VDW_RADII for z in ELEMENTS)                      # every generated element has a listed radius
    r = RC.vdw_radii(torch.tensor([[6, 7, 0], [5, 26, 200]]))
    assert r.dtype == torch.float32
    assert r.tolist() == [[pytest.approx(1.70), pytest.approx(1.55), 2.0], [pytest.approx(1.92), 2.0, 2.0]]
    # an N...O pair at an H-bond distance of 2.6 A does not clash
    ov = (np.float32(1.55) + np.float32(1.52)) - np.float32(2.6)
    assert 0.46 < ov < RC.CLASH_OVERLAP


def test_receptor_forms_and_refusals():
    xyz = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    coords, z = RC.load_receptor((xyz, [6, 1, 8]))                       # hydrogens dropped
    assert coords.tolist() == [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]] and z.tolist() == [6, 8]
    mol = PosedMol(xyz.numpy(), z=[7, 1, 16])
    coords, z = RC.load_receptor(mol)
    assert coords.tolist() == [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]] and z.tolist() == [7, 16]
    nan = xyz.clone()
    nan[2, 1] = float("nan")
    big = torch.arange(3 * (RC.MAX_RECEPTOR_ATOMS + 1), dtype=torch.float32).reshape(-1, 3)
    for bad in ((xyz, [1, 1, 1]), (nan, [6, 6, 6]), (xyz, [6, 6]), (xyz, [6.0, 6.0, 6.0]), (xyz, [6, 0, 6]),
                (big, torch.full((RC.MAX_RECEPTOR_ATOMS + 1,), 6)), 42, None, (xyz,)):
        with pytest.raises(ValueError):
            RC.load_receptor(bad)
    assert RC.load_receptor((big[:-1], torch.full((RC.MAX_RECEPTOR_ATOMS,), 6)))[0].shape[0] == RC.MAX_RECEPTOR_ATOMS


def test_receptor_overlap_refusals_happen_before_any_device_work():
    rec = (torch.tensor([[0.0, 0.0, 0.0]]), [6])
    x = torch.zeros(3, 20, 3)
    n = torch.tensor([20, 5, 0], dtype=torch.int32)
    z = torch.full((3, 42), 6)
    for r, coords, nn, zz in (((torch.zeros(1, 3), [1]), x, n, z),                 # no heavy atoms
                              (rec, x, torch.tensor([21, 5, 0]), z),                  # check_n_nodes
                              (rec, x, torch.tensor([4, 5]), z),
                              (rec, torch.zeros(2, 65, 3), torch.tensor([3, 3]), torch.full((2, 65), 6)),
                              (rec, x, n, torch.full((3, 19), 6)),                    # atomic numbers too narrow
                              (rec, x, n, torch.full((2, 42), 6))):
        with pytest.raises(ValueError):
            RC.receptor_overlap(r, coords, nn, zz, device="cpu")
    assert RC.receptor_overlap(rec, torch.zeros(0, 20, 3), torch.zeros(0, dtype=torch.int32), torch.zeros(0, 42),
                               device="cpu").shape == (0, 20)


def test_clash_summary_and_split_rule():
    inf, nan = math.inf, float("nan")
    ov = torch.tensor([[0.6, 0.59, -inf], [-0.2, -1.0, -inf], [nan, 2.0, -inf], [-inf, -inf, -inf]])
    clashes, worst = RC.clash_summary(ov)
    assert clashes.tolist() == [1, 0, 1, 0] and clashes.dtype == torch.int32
    assert worst[0] == pytest.approx(0.6) and worst[1] == pytest.approx(-0.2)
    assert math.isnan(float(worst[2])) and worst[3] == -inf
    assert RC.default_splits(1, 1, 1) == 1 and RC.default_splits(64, 40, 100000) == 103
    assert RC.default_splits(16384, 64, 100000) == 1 and RC.default_splits(4, 20, 10 ** 5) == 256


def test_receptor_entry_refuses_bad_arguments_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check
    ok = dict(x=p, r=p, nn=p, B=3, N=27, y=p, yr=p, R=100, S=2, ws=p, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return h.mcg_receptor_overlap(a["x"], a["r"], a["nn"], a["B"], a["N"], a["y"], a["yr"], a["R"], a["S"],
                                      a["ws"], a["out"], None)

    for bad in (dict(x=None), dict(r=None), dict(nn=None), dict(y=None), dict(yr=None), dict(out=None), dict(ws=None),
                dict(B=0), dict(B=-1), dict(B=RC.MAX_BATCH + 1), dict(N=0), dict(N=65), dict(R=0), dict(R=-5),
                dict(R=RC.MAX_RECEPTOR_ATOMS + 1), dict(S=0), dict(S=257)):
        assert call(**bad) == 1, bad                                     # MCG_ERR_ARG = hipErrorInvalidValue
        assert b"mcg_receptor_overlap" in h.mcg_last_error(), bad
    assert "mcg_receptor_overlap" in _lib.SIGNATURES


# ----------------------------------------------------------------------------------------------- generation refusals
def _pocket(n=40):
    """Receptor heavy atoms on a ring 6 A around the reference's centroid, clear of every reference atom."""
    ref = _ref()
    c = ref.mean(0)
    t = torch.arange(n, dtype=torch.float32) * (2 * math.pi / n)
    xyz = torch.stack([c[0] + 30.0 * torch.cos(t), c[1] + 30.0 * torch.sin(t), c[2].expand(n)], dim=1)
    return xyz, torch.full((n,), 6)


@pytest.mark.parametrize("entry", ["generate_conformers", "generate_conformers_sharded", "forward"])
def test_receptor_refusals_happen_before_any_device_work(entry):
    gen = _shell_generator()
    gen._generate_shard = gen._score = gen._pose = _no_device
    gen._pair = gen._receptor_coords = _no_device
    call = getattr(gen, entry)
    pocket = _pocket()
    holding = (torch.cat([pocket[0], _ref()[3:4] + 0.2]), torch.cat([pocket[1], torch.tensor([8])]))   # the ligand's atom
    nan = (pocket[0].clone(), pocket[1])
    nan[0][0, 0] = float("inf")
    ctx = torch.tensor([50.0, 100.0, 130.0])
    for kw in (dict(receptor=pocket),                                            # not posed: not in the pocket's frame
               dict(receptor=pocket, shape_scores=True),
               dict(overlay=True, max_receptor_clashes=0),                       # a filter without a receptor
               dict(max_receptor_clashes=0),
               dict(overlay=True, receptor=pocket, max_receptor_clashes=-1),
               dict(overlay=True, receptor=pocket, max_receptor_clashes=True),
               dict(overlay=True, receptor=pocket, max_receptor_clashes=1.0),
               dict(overlay=True, receptor=pocket, max_receptor_clashes="1"),
               dict(overlay=True, receptor=holding),                             # the complex, ligand included
               dict(overlay=True, receptor=holding, max_receptor_clashes=3),
               dict(overlay=True, receptor=nan),
               dict(overlay=True, receptor=(pocket[0][:2], [1, 1])),             # no heavy atoms
               dict(overlay=True, receptor="HEADER\nEND\n"),
               dict(overlay=True, receptor=3.5)):
        with pytest.raises(ValueError):
            call(reference_conformer=_ref(), n_samples=4, **kw)
    with pytest.raises(ValueError):
        call(reference_context=ctx, n_atoms=17, n_samples=4, overlay=True, receptor=pocket)


# ----------------------------------------------------------------------------------------------- stub contact seam
def _stub_contacts(calls):
    """A device-free stand-in for `receptor_overlap`: overlap[b, i] = 10 k_b - i + 0.05 on the real atoms (-inf beyond),
    with k_b = the posed row's coords[b, 0, 1] (the generated x00 under the stub pose), so a molecule has 10 k_b
    clashes (at most its atom count) and a maximum overlap of 10 k_b + 0.05.  Records (B, atomic numbers) per call."""
    def run(rec, coords, n, z):
        calls.append((int(coords.shape[0]), torch.as_tensor(z)[:, : coords.shape[1]].clone()))
        B, N = coords.shape[0], coords.shape[1]
        k = coords[:, 0, 1].double().view(B, 1)
        ov = 10.0 * k - torch.arange(N, dtype=torch.float64).view(1, N) + 0.05
        real = torch.arange(N).view(1, N) < torch.as_tensor(n).view(B, 1)
        return torch.where(real, ov, torch.full_like(ov, -math.inf)).float()
    return run


def _proxy_gen(calls):
    gen = _shell_generator()
    gen._generate_shard = _stub_shard()
    gen._pose = _stub_overlay(lambda k: k + 1.0)        # (x, 0, 0) @ rot_z(90) -> (0, x, 0): coords[0, 1] = x00
    gen._score = lambda ref, coords, n: coords[:, 1, 0].clone()
    gen._receptor_coords = _stub_contacts(calls)
    return gen


def test_proxy_path_records_carry_the_contacts():
    calls = []
    gen = _proxy_gen(calls)
    posed = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True)
    assert calls == [] and all(m.receptor_clashes is None and m.receptor_max_overlap is None for m in posed)
    got = gen.generate_conformers(reference_conformer=_ref(), n_samples=8, overlay=True, receptor=_pocket())
    assert len(calls) == 1 and calls[0][0] == 8                  # one seam call over the shard, after posing
    assert bool((calls[0][1] == 6).all())                        # the rows' elements
    assert [m.sample_id for m in got] == [m.sample_id for m in posed] == [0, 1, 2, 4, 5, 6, 7]
    for a, b in zip(posed, got):
        torch.testing.assert_close(a.coords, b.coords, rtol=0, atol=0, equal_nan=True)
        if b.sample_id == 5:                                     # pose failed: not in the receptor's frame
            assert b.receptor_clashes is None and b.receptor_max_overlap is None
            continue
        k = (7 * b.sample_id) % 10
        assert b.receptor_clashes == k
        assert b.receptor_max_overlap == pytest.approx(k + 0.05, abs=1e-5)


def test_proxy_path_filters_before_the_selection():
    calls = []
    gen = _proxy_gen(calls)
    kw = dict(reference_conformer=_ref(), n_samples=8, overlay=True, receptor=_pocket())
    base = gen.generate_conformers(shape_scores=True, **kw)
    clashes = {m.sample_id: m.receptor_clashes for m in base}      # 0: 0, 1: 7, 2: 4, 4: 8, 5: None, 6: 2, 7: 9
    scores = {m.sample_id: m.shape_tanimoto for m in base}
    for k in (0, 4, 7, 100):
        want = [s for s in sorted(clashes) if clashes[s] is not None and clashes[s] <= k]
        got = gen.generate_conformers(max_receptor_clashes=k, **kw)
        assert [m.sample_id for m in got] == want, k
        ids = want
        for top_k in (1, 2):                                     # top_k ranks the survivors only
            ranked = gen.generate_conformers(max_receptor_clashes=k, top_k=top_k, shape_scores=True, **kw)
            assert [m.sample_id for m in ranked] == [ids[i] for i in select_scored([scores[s] for s in ids], ids, top_k)]
    assert gen.last_valid_fraction == pytest.approx(7 / 8)       # taken before the selection
    pair_calls = []

    def pair(ref, coords, n):
        pair_calls.append(int(coords.shape[0]))
        return torch.zeros(coords.shape[0], coords.shape[0])
    gen._pair = pair
    got = gen.generate_conformers(max_receptor_clashes=4, max_pairwise_tanimoto=0.5, **kw)
    assert pair_calls == [3] and sorted(m.sample_id for m in got) == [0, 2, 6]   # the pair matrix of the survivors
    sharded = gen.generate_conformers_sharded(max_receptor_clashes=4, **kw)      # no process group: one rank
    assert [m.sample_id for m in sharded] == [0, 2, 6]
    assert [m.sample_id for m in gen.forward(max_receptor_clashes=0, **kw)] == [0]


class _StageGen:
    """`_generate_shard` for the object path: finished stand-in Mols with four heavy atoms at (sid / 10, 0, 0) and one
    hydrogen; sample 2 is dropped by the finish, sample 6's pose fails."""
    def __init__(self, gen):
        self.gen = gen

    def __call__(self, ref_context, ref_n_atoms, variance, sizes, n_samples, *rest):
        ids = torch.as_tensor(rest[7]).tolist() if len(rest) > 7 and rest[7] is not None else list(range(n_samples))
        mols = []
        for i in ids:
            x0 = float("nan") if i == 6 else i / 10.0
            mols.append(None if i == 2 else PosedMol([[x0, 0, 0]] * 4 + [[0, 0, 1.0]], z=[7, 6, 6, 8, 1]))
        self.gen._finish_stage = _Stage(mols)
        return dict(x=torch.zeros(n_samples, 5, 3))


def _object_gen(calls):
    gen = _shell_generator(finisher="rdkit")
    gen._generate_shard = _StageGen(gen)
    gen._pose = _stub_overlay(lambda k: k * 0 + 0.5)
    gen._score = lambda ref, coords, n: 1.0 - coords[:, 0, 1].clone()      # lower sample id: higher score
    gen._receptor_coords = _stub_contacts(calls)
    return gen


def test_object_path_mols_carry_the_contacts():
    calls = []
    gen = _object_gen(calls)
    got = gen.generate_conformers(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True,
                                  receptor=_pocket())
    assert len(calls) == 1 and calls[0][0] == 5                  # the live Mols whose pose succeeded
    assert calls[0][1].tolist() == [[7, 6, 6, 8]] * 5            # heavy atoms' GetAtomicNum(), hydrogens ignored
    assert [m.props["sample_id"] for m in got] == [0, 1, 3, 4, 5, 6]
    for m in got:
        sid = m.props["sample_id"]
        if sid == 6:
            assert "receptor_clashes" not in m.props and "receptor_max_overlap" not in m.props
            continue
        assert m.props["receptor_clashes"] == min(sid, 4)
        assert m.props["receptor_max_overlap"] == pytest.approx(sid + 0.05, abs=1e-5)
    calls.clear()
    got = gen.generate_conformers(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True,
                                  receptor=_pocket(), max_receptor_clashes=3, top_k=2)
    assert [m.props["sample_id"] for m in got] == [0, 1]
    got = gen.generate_conformers(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True,
                                  receptor=_pocket(), max_receptor_clashes=3)
    assert [m.props["sample_id"] for m in got] == [0, 1, 3]     # 6: pose failed; 4, 5: four clashes
    plain = gen.generate_conformers(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True)
    assert all("receptor_clashes" not in m.props for m in plain)


def _receptor_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    gen = _object_gen(calls)
    mols = gen.generate_conformers_sharded(reference_conformer=_ref(), n_samples=7, sample_seed=5, overlay=True,
                                           receptor=_pocket(), max_receptor_clashes=3, gather="all")
    q.put((rank, [(m.props["sample_id"], m.props["receptor_clashes"]) for m in mols], sum(c[0] for c in calls)))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_gather_all_filters_the_same_on_both_ranks_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_receptor_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    # each rank measured its own shard (5 measurable Mols between them), and both return the same filtered list
    assert [r[1] for r in res] == [[(0, 0), (1, 1), (3, 3)]] * 2
    assert sum(r[2] for r in res) == 5 and all(r[2] > 0 for r in res)
