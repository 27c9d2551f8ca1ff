"""Explicit hydrogens without a GPU ("Explicit hydrogens"): `hydrogens.implicit_counts` against the
fp64 restatement and against counts known by hand, the geometry the restatement itself produces (lengths, angles,
planes, the rotor scan) with a mutation check of those assertions, the writers, and every refusal that must come back
before any device work."""
import ctypes
import math

import numpy as np
import pytest
import torch

import hydrogens_cases as C
import hydrogens_ref as HR
import pharmacophore_cases as PC
import pharmacophore_ref as PR
from ml_conformer_generator_amd import hydrogens as HY


def _counts(mols):
    W = max([m[2] for m in mols] + [1])
    z, bonds = torch.zeros(len(mols), W, dtype=torch.int32), torch.zeros(len(mols), W, W, dtype=torch.int8)
    for b, (zs, adj, n) in enumerate(mols):
        if n:
            z[b, :n] = torch.tensor(zs, dtype=torch.int32)
            bonds[b, :n, :n] = torch.tensor(adj, dtype=torch.int8)
    out = HY.implicit_counts(z, bonds, torch.tensor([m[2] for m in mols], dtype=torch.int32))
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(mols), W)
    for b, m in enumerate(mols):
        assert not out[b, m[2]:].any()
    return [out[b, : m[2]].tolist() for b, m in enumerate(mols)]


def test_known_counts():
    f, ref = C.fixtures(), C.references()
    for name, total in C.KNOWN_COUNTS.items():
        assert f[name]["hydrogens"] == total
    names = [k for k in f if f[k]["hydrogens"] is not None]
    got = _counts([f[k]["mol"] for k in names])
    for name, row in zip(names, got):
        assert sum(row) == f[name]["hydrogens"], name
        assert row == ref[name]["nh"], name
    # imidazole: exactly one N-H, on the lower-index N; pyrrole's comes from the ring rule
    assert got[names.index("imidazole")] == [1, 1, 0, 1, 1]
    assert got[names.index("pyrrole")] == [1, 1, 1, 1, 1]
    assert PR.atom_quantities(*f["pyrrole"]["mol"])[0][3] == 0


def test_counts_equal_the_restatement_on_every_fixture_and_on_molecule_like_graphs():
    mols = [fx["mol"] for fx in C.fixtures().values()]
    mols += [m for _, (m, *_rest) in sorted(PC.PINNED.items())] + PC.molecule_like_set()[:168] + PC.big_molecules()
    got = _counts(mols)
    ring_rule = 0
    for m, row in zip(mols, got):
        want = HR.counts(*m)
        assert row == want
        ring_rule += sum(1 for a, b in zip(want, PR.atom_quantities(*m)) if a != b[3])
    assert ring_rule >= 5                         # the 5-ring rule is exercised beyond the hand-written molecules
    # junk at and beyond the atom count and on the diagonal is ignored
    z, adj, n = C.fixtures()["imidazole"]["mol"]
    zz = torch.full((1, 9), 7, dtype=torch.int32)
    zz[0, :n] = torch.tensor(z)
    bb = torch.full((1, 9, 9), 4, dtype=torch.int8)
    bb[0, :n, :n] = torch.tensor(adj, dtype=torch.int8) + 3 * torch.eye(n, dtype=torch.int8)
    assert HY.implicit_counts(zz, bb, torch.tensor([n]))[0].tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0]


def _assertions(place):
    """Every geometric statement of the host test, as a function of the placement function: the mutation check runs it
    again on mutated restatements."""
    f = C.fixtures()
    res = {k: place(*f[k]["mol"], f[k]["xyz"]) for k in f}
    for name, r in res.items():                   # X-H lengths, and the angle to every neighbour of a k = 1 or linear parent
        z, adj, n = f[name]["mol"]
        x = f[name]["xyz"].astype(np.float64)
        nb = PR.neighbours(z, adj, n)
        for p, h in zip(r["parents"], r["coords"]):
            assert abs(np.linalg.norm(h - x[p]) - (HR.RCOV[z[p]] + 0.31)) < 1e-9, name
            if len(nb[p]) == 1:
                want = {HR.TETRAHEDRAL: 109.4712, HR.PLANAR: 120.0, HR.LINEAR: 180.0}[r["hybridisation"][p]]
                assert abs(HR.angle(h, x[p], x[nb[p][0]]) - want) < 1e-6, (name, p)
    # methane-like and formaldehyde-like: the angles BETWEEN the hydrogens
    for name, want in (("ethane", 109.4712), ("methane", 109.4712), ("formaldehyde", 120.0)):
        r, x = res[name], f[name]["xyz"].astype(np.float64)
        hs = [h for p, h in zip(r["parents"], r["coords"]) if p == 0]
        for i in range(len(hs)):
            for j in range(i):
                assert abs(HR.angle(hs[i], x[0], hs[j]) - want) < 2e-4, name
    # a tetrahedral centre with two neighbours: H-C-H 109.47, both H-C-C equal, and the first hydrogen on the +n side
    r, x = res["propane"], f["propane"]["xyz"].astype(np.float64)
    h0, h1 = [h for p, h in zip(r["parents"], r["coords"]) if p == 1]
    assert abs(HR.angle(h0, x[1], h1) - 2 * 54.7356) < 1e-6
    assert abs(HR.angle(h0, x[1], x[0]) - HR.angle(h0, x[1], x[2])) < 1e-6
    assert float((h0 - x[1]).dot(np.cross(x[0] - x[1], x[2] - x[1]))) > 0.5
    # benzene: every C-H along the bisector, in the ring plane
    r, x = res["benzene"], f["benzene"]["xyz"].astype(np.float64)
    for p, h in zip(r["parents"], r["coords"]):
        assert abs(HR.angle(h, x[p], x[(p + 1) % 6]) - 120.0) < 1e-4 and HR.out_of_plane(h, x[0], x[2], x[4]) < 1e-6
    # the amide N-H lie in the amide plane, the phenol O-H in the ring plane
    r, x = res["acetamide"], f["acetamide"]["xyz"].astype(np.float64)
    assert r["hybridisation"][3] == HR.PLANAR
    amide = [h for p, h in zip(r["parents"], r["coords"]) if p == 3]
    assert len(amide) == 2 and all(HR.out_of_plane(h, x[1], x[2], x[3]) < 1e-6 for h in amide)
    r, x = res["phenol"], f["phenol"]["xyz"].astype(np.float64)
    assert r["hybridisation"][6] == HR.PLANAR
    (hydroxyl,) = [h for p, h in zip(r["parents"], r["coords"]) if p == 6]
    assert HR.out_of_plane(hydroxyl, x[0], x[2], x[4]) < 1e-6
    # the unhindered methyl and hydroxyl are staggered / anti (delta = 0): the first hydrogen's torsion to w is 180
    r, x = res["ethanol"], f["ethanol"]["xyz"].astype(np.float64)
    assert r["rotor_delta"] == [0, -1, 0]
    first = r["coords"][0]
    b1, b2 = _unit_perp(first - x[0], x[1] - x[0]), _unit_perp(x[2] - x[1], x[1] - x[0])
    assert abs(float(b1.dot(b2)) + 1.0) < 1e-9
    # the hindered hydroxyl leaves delta = 0, and ends clear of the atom in its way
    r, x = res["hindered ethanol"], f["hindered ethanol"]["xyz"].astype(np.float64)
    assert r["rotor_delta"][2] not in (0, -1) and r["rotor_delta"][0] == 0
    (hydroxyl,) = [h for p, h in zip(r["parents"], r["coords"]) if p == 2]
    assert np.linalg.norm(hydroxyl - x[3]) > 2.4
    assert r["unplaced"] == 1 and r["counts"][3] == 0        # the unbonded F: its hydrogen has no direction


def _unit_perp(v, axis):
    axis = axis / np.linalg.norm(axis)
    v = v - v.dot(axis) * axis
    return v / np.linalg.norm(v)


def test_geometry_of_the_restatement():
    _assertions(HR.place)
    ref = C.references()
    assert ref["water"]["n_hydrogens"] == 2 and ref["no atoms"]["n_hydrogens"] == 0
    assert ref["hydrogen cyanide"]["hybridisation"] == [HR.LINEAR, HR.LINEAR]
    for name, r in ref.items():                   # ascending parent, then m; counts add up
        assert r["parents"] == sorted(r["parents"]) and sum(r["counts"]) == r["n_hydrogens"] == len(r["coords"]), name
        assert sum(r["nh"]) == r["n_hydrogens"] + r["unplaced"], name
    bad = C.fixtures()["ethanol"]["xyz"].copy()
    bad[1, 2] = np.inf
    assert HR.place(*C.fixtures()["ethanol"]["mol"], bad)["n_hydrogens"] == -1


@pytest.mark.parametrize("mutation", ["flip_n", "conjugation", "scan"])
def test_mutations_of_the_restatement_are_caught(mutation):
    kw = {"flip_n": dict(flip_n=True), "conjugation": dict(conjugation=False), "scan": dict(scan=False)}[mutation]
    with pytest.raises(AssertionError):
        _assertions(lambda *a: HR.place(*a, **kw))


def _records_with_hydrogens():
    from ml_conformer_generator_amd.handoff import molecules_from_tensors
    f, ref = C.fixtures(), C.references()
    names = ["ethanol", "acetamide", "methane"]
    x, z, bonds, n = C.pad_batch([f[k] for k in names], 6, 6)
    H = max(ref[k]["n_hydrogens"] for k in names)
    hx, hp = torch.zeros(3, H, 3), torch.full((3, H), -1, dtype=torch.int32)
    for b, k in enumerate(names):
        hx[b, : ref[k]["n_hydrogens"]] = torch.tensor(ref[k]["coords"], dtype=torch.float32)
        hp[b, : ref[k]["n_hydrogens"]] = torch.tensor(ref[k]["parents"], dtype=torch.int32)
    common = (torch.from_numpy(x), torch.from_numpy(z).to(torch.int8), torch.from_numpy(bonds), torch.from_numpy(n),
              torch.ones(3, dtype=torch.uint8))
    with_h = molecules_from_tensors(*common, hydrogen_coords=hx, hydrogen_parents=hp,
                                    hydrogens_unplaced=torch.tensor([0, 0, -1], dtype=torch.int32))
    return names, ref, molecules_from_tensors(*common), with_h


def test_writers_and_record_fields():
    names, ref, plain, with_h = _records_with_hydrogens()
    for a, b in zip(plain, with_h):               # the defaults write today's text
        assert a.to_molblock() == b.to_molblock() == b.to_molblock(hydrogens=False)
        assert a.to_xyz_block() == b.to_xyz_block() == b.to_xyz_block(hydrogens=False)
        assert a.hydrogen_coords is None and a.hydrogen_parents is None and a.hydrogens_unplaced is None
        assert a.receptor_hydrogen_clashes is None and b.receptor_hydrogen_clashes is None
        with pytest.raises(ValueError, match="carries no hydrogens"):
            a.to_molblock(hydrogens=True)
        with pytest.raises(ValueError, match="carries no hydrogens"):
            a.to_xyz_block(hydrogens=True)
    eth = with_h[0]
    assert eth.to_molblock() == ("generated\n  mlconfgen-mi355x\n\n  3  2  0  0  0  0  0  0  0  0999 V2000\n"
                                 + "".join("%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0\n" % (*c, s)
                                           for s, c in zip("CCO", eth.coords.tolist()))
                                 + "  2  1  1  0\n  3  2  1  0\nM  END\n")
    for name, m in zip(names[:2], with_h[:2]):
        r = ref[name]
        n, h = len(m.atomic_numbers), r["n_hydrogens"]
        assert m.hydrogens_unplaced == 0 and m.hydrogen_parents == r["parents"]
        assert m.hydrogen_coords.dtype == torch.float32 and tuple(m.hydrogen_coords.shape) == (h, 3)
        lines = m.to_molblock(hydrogens=True).split("\n")
        n_bonds = int((m.bond_orders != 0).sum()) // 2
        assert lines[3] == "%3d%3d  0  0  0  0  0  0  0  0999 V2000" % (n + h, n_bonds + h)
        atoms, bonds = lines[4: 4 + n + h], lines[4 + n + h: 4 + n + h + n_bonds + h]
        assert [a[31:34].strip() for a in atoms[n:]] == ["H"] * h and lines[4 + n + h + n_bonds + h] == "M  END"
        assert atoms[:n] == m.to_molblock().split("\n")[4: 4 + n]
        assert bonds[:n_bonds] == m.to_molblock().split("\n")[4 + n: 4 + n + n_bonds]
        assert [(int(b[0:3]), int(b[3:6]), int(b[6:9])) for b in bonds[n_bonds:]] == \
            [(n + 1 + k, p + 1, 1) for k, p in enumerate(r["parents"])]
        xyz = m.to_xyz_block(hydrogens=True).split("\n")
        assert xyz[0] == str(n + h) and [ln.split()[0] for ln in xyz[2 + n: 2 + n + h]] == ["H"] * h
        assert np.allclose([[float(v) for v in ln.split()[1:]] for ln in xyz[2 + n: 2 + n + h]], r["coords"], atol=1e-6)
    lost = with_h[2]                               # a row the kernel reported as non-finite: no hydrogens on the record
    assert lost.hydrogen_coords is None and lost.hydrogen_parents is None and lost.hydrogens_unplaced is None
    with pytest.raises(ValueError, match="carries no hydrogens"):
        lost.to_xyz_block(hydrogens=True)


def test_refusals_of_the_option_come_before_any_device_work():
    from ml_conformer_generator_amd import host_pool, postprocess
    from test_distributed_gloo import _shell_generator
    gen = _shell_generator()

    def no_device(*a, **k):
        raise AssertionError("device work started before the option was checked")
    gen._generate_shard = no_device
    ctx = dict(reference_context=torch.tensor([50.0, 100.0, 130.0]), n_atoms=27, n_samples=2)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="add_hydrogens must be True or False"):
            gen.generate_conformers(add_hydrogens=bad, **ctx)
        with pytest.raises(ValueError, match="add_hydrogens must be True or False"):
            gen.generate_conformers_sharded(add_hydrogens=bad, **ctx)
    for finisher in ("rdkit", host_pool.TaskRef("somewhere.py", "finish")):
        gen.finisher = finisher
        with pytest.raises(ValueError, match=r"Chem\.AddHs\(mol, addCoords=True\)"):
            gen.generate_conformers(add_hydrogens=True, **ctx)
        with pytest.raises(ValueError, match=r"Chem\.AddHs\(mol, addCoords=True\)"):
            gen.generate_conformers_sharded(add_hydrogens=True, **ctx)
        assert postprocess.parse_request(gen, None, add_hydrogens=False).add_hydrogens is False
    gen.finisher = None
    assert postprocess.parse_request(gen, None, add_hydrogens=True).add_hydrogens is True
    assert postprocess.Request().add_hydrogens is False


def test_argument_errors_of_the_python_layer_need_no_device():
    x, z, b, n = torch.zeros(2, 5, 3), torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 5, 5, dtype=torch.int8), \
        torch.tensor([5, 5])
    for args in ((torch.zeros(2, 5, 2), z, b, n), (x.to(torch.int32), z, b, n), (x, z, torch.zeros(2, 5, 4, dtype=torch.int8), n),
                 (x, z[:, :4], b, n), (x, z.float(), b, n), (x, z, b.float(), n), (x, z, b, torch.tensor([5])),
                 (x, z, b, torch.tensor([5, 6])), (x, z, b, torch.tensor([-1, 5])), (x[:1], z, b, n),
                 (torch.zeros(2, 65, 3), torch.ones(2, 65, dtype=torch.int32), torch.zeros(2, 65, 65, dtype=torch.int8), n)):
        with pytest.raises(ValueError):
            HY.add_hydrogens(*args)
    with pytest.raises(ValueError):
        HY.implicit_counts(torch.ones(2, 65, dtype=torch.int32), torch.zeros(2, 65, 65, dtype=torch.int8), n)


def test_argument_errors_of_the_entry_point_need_no_device():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))    # never read: every call is refused first
    ok = [p] * 7 + [4, 8, 8, 24] + [p] * 5 + [None, None]

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return h.mcg_hydrogens_place(*a)
    cases = [dict(a9=65, a10=195), dict(a9=0), dict(a10=23), dict(a9=1, a10=3), dict(a7=-1), dict(a7=16385), dict(a8=0)]
    cases += [{f"a{k}": None} for k in (0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15)]
    for change in cases:
        assert call(**change) != 0, change
        assert b"mcg_hydrogens_place" in h.mcg_last_error()
    assert HY.slots(1) == 4 and HY.slots(2) == 6 and HY.slots(64) == 192
    assert call(a7=0) == 0                        # an empty batch launches nothing
