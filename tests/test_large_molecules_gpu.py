"""Molecules above 42 atoms on the MI355X: the denoiser in all three operand modes, one GCL layer and the sampler kernels
against the oracle evaluated in fp64, at sizes where an atom's edge rows run through five to eight tiles, where the unit
tables disappear, where the per-molecule sampler kernels take a second trip of their 64-lane loop.  Run with `-m gpu`.

Every case asserts, through `mcg_debug_route`, the kernels it is there to cover (tests/large_molecule_cases.py); the host
half (tests/test_large_molecules_host.py) shows that the pass rule used here leaves a correct fp32 evaluation ten times
the room it needs and sees one missing edge of a 114-atom molecule at 210 x the tolerance.

Ground truth: oracle.egnn_oracle in fp64 (weights and inputs are exactly representable: the real-number value of the
network to ~1e-16), evaluated molecule by molecule (large_molecule_cases.oracle_per_molecule), once per case and module.

Each dynamics case prints one line
    LARGE-N <case> <mode>/<variant> route=... viol64=<x tolerance> rms/fp32=<ratio> t=+<s since the module's first test>
and the module's wall time follows at the end (`LARGE-N module wall time`).

rms ratio: the rms distance of the kernel's output from fp64 over that of the fp32 CPU oracle on the same inputs, bounded
by 1.5 as in test_split_operand_modes_are_as_accurate_as_fp32_against_fp64 (established there at n <= 39).  Measured on an
MI355X at these sizes: see DESIGN.md, "Molecules above 42 atoms", and profiles/large_molecules_gpu.txt.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

from conftest import TapeNoise, load_golden, sd_for
from large_molecule_cases import CASES, WEIGHT_RECIPE, WEIGHT_SEED, build_inputs, oracle_per_molecule
from parity_tolerance import close as _close
from parity_tolerance import traj_violation, violation

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T_START = [time.time()]          # reset when the module's first test starts (collection of a whole suite is not its time)
RMS_BOUND = 1.5
_W = {"weight_seed": WEIGHT_SEED, "weight_recipe": WEIGHT_RECIPE}


def close(a, b):
    return _close(a, b, split=3 if b.shape[-1] == 11 else None)


def edge_mask_of(node_mask):
    B, N, _ = node_mask.shape
    nm = node_mask.squeeze(2)
    return (nm.unsqueeze(1) * nm.unsqueeze(2) * (1 - torch.eye(N)).unsqueeze(0)).reshape(B * N * N, 1)


_DYN = {}


def dyn_for(g, mode):
    """One EGNNDynamics per (weights, operand mode) for the whole module."""
    from ml_conformer_generator_amd.egnn import EGNNDynamics
    key = (int(g["weight_seed"]), str(g["weight_recipe"]) if "weight_recipe" in g else "v2", mode)
    if key not in _DYN:
        d = EGNNDynamics(device=DEV)
        d.load_reference_state_dict(sd_for(g))
        d.set_precision(mode)
        _DYN[key] = d
    return _DYN[key]


def sampler_for(T, g, mode):
    from ml_conformer_generator_amd.equivariant_diffusion import EquivariantDiffusion, PredefinedNoiseSchedule
    gm = EquivariantDiffusion(dynamics=dyn_for(g, mode), in_node_nf=8, timesteps=1000, noise_precision=1e-5)
    gm.gamma = PredefinedNoiseSchedule(timesteps=T, precision=1e-5)
    gm.T = T
    return gm


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs, the fp64 value and the fp32 CPU oracle's own rms distance from it - computed once per case."""
    c = CASES[name]
    sd = sd_for(_W)
    t, z, nm, em, ctx = build_inputs(c["sizes"], c["N"], c["seed"])
    ref64 = oracle_per_molecule({k: v.double() for k, v in sd.items()}, t, z, nm, ctx)
    ref32 = oracle_per_molecule(sd, t, z, nm, ctx)
    sc = float(ref64.abs().max())
    base = float((ref32.double() - ref64).pow(2).mean().sqrt()) / sc
    assert violation(ref32, ref64, split=3) < 0.1          # the inputs leave a correct fp32 evaluation 10 x the room
    return dict(t=t, z=z, nm=nm, ctx=ctx, ref64=ref64, sc=sc, base=base)


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    T_START[0] = time.time()
    yield
    print(f"\nLARGE-N module wall time {time.time() - T_START[0]:.1f} s")


def assert_route(d, plan, expected, keep_agg=False):
    from ml_conformer_generator_amd import _lib
    got = _lib.debug_route(d.handle, plan.handle, keep_agg)
    wrong = {k: (got[k], v) for k, v in expected.items() if got[k] != v}
    assert not wrong, f"route (got, expected) differs in {wrong}; full route {got}"
    return got


def route_text(r):
    return (f"{r['edge']}/{r['agg']}/{r['coord']}/pab={r['pab']}/node={r['node']}/fused={int(r['fused'])}"
            f"/pspan={r['pspan']}/uspan={r['unit_span']}")


DYNAMICS_RUNS = [(name, mode, variant) for name in sorted(CASES) for (mode, variant) in CASES[name]["routes"]]


@pytest.mark.parametrize("name,mode,variant", DYNAMICS_RUNS, ids=[f"{n}-{m}-{v}" for n, m, v in DYNAMICS_RUNS])
def test_dynamics_vs_fp64_oracle(name, mode, variant):
    """One denoiser call per case, operand mode and edge-kernel variant.
    * the route is the one the case claims;
    * f32 / f32x6: within the stated per-call tolerance of the fp64 value (rtol 1e-4, atol 1e-5 of each channel group's
      magnitude), and at most 1.5 x as far from it (rms) as the fp32 CPU oracle is;  bf16: the stated 3e-2 * max(1, max|ref|);
    * padded slots exactly zero, a second run bit-identical, inputs untouched."""
    c, k = CASES[name], case_data(name)
    d = dyn_for(_W, mode)
    sizes = torch.tensor(c["sizes"], dtype=torch.int32)
    plan = d.plan(sizes, c["N"])
    assert plan.edge_mt == (1 if mode == "f32" else c["edge_mt_wide"])
    lat = {"auto": -1, "lat0": 0, "lat1": 1}[variant]
    plan.set_latency_mode(lat)
    try:
        r = assert_route(d, plan, c["routes"][(mode, variant)])
        td, zd, cd = k["t"].reshape(-1).to(DEV).contiguous(), k["z"].to(DEV), k["ctx"].to(DEV)
        out = d.run(plan, td, zd, cd)
        out2 = d.run(plan, td, zd, cd)
        torch.cuda.synchronize()
    finally:
        plan.set_latency_mode(-1)
    assert torch.equal(out, out2), "second run differs"
    assert torch.equal(zd.cpu(), k["z"]) and torch.equal(cd.cpu(), k["ctx"]) and torch.equal(td.cpu(), k["t"].reshape(-1))
    out = out.cpu()
    assert bool(torch.isfinite(out).all())
    assert float((out * (1 - k["nm"])).abs().max()) == 0.0, "padded slots are not exactly zero"
    v = violation(out, k["ref64"], split=3)
    ratio = float((out.double() - k["ref64"]).pow(2).mean().sqrt()) / k["sc"] / k["base"]
    print(f"\nLARGE-N {name} {mode}/{variant} sizes={c['sizes'] if len(c['sizes']) < 8 else str(c['sizes'][:4]) + '...'} "
          f"route={route_text(r)} viol64={v:.4f} rms/fp32={ratio:.3f} t=+{time.time() - T_START[0]:.1f}s")
    if mode == "bf16":
        err = float((out.double() - k["ref64"]).abs().max())
        assert err <= 3e-2 * max(1.0, k["sc"]), (err, k["sc"])
        assert ratio > 20.0                                  # (and it IS the bf16 path: two orders of magnitude further away)
    else:
        assert v <= 1.0, f"{v} x the stated tolerance of the fp64 value"
        assert ratio <= RMS_BOUND, f"rms distance from fp64 is {ratio} x the fp32 CPU oracle's"


def test_exact_fp32_refuses_a_200_atom_molecule_at_plan_creation():
    """Case F in exact fp32: 199 edge rows per atom run through 14 tiles, an atom keeps eight partial sums - refused on the
    host with a message that names the molecule and the limit; nothing is launched."""
    from ml_conformer_generator_amd import _lib
    c = CASES["F"]
    assert ("f32", "auto") not in c["routes"] and c["sets"] is None
    d = dyn_for(_W, "f32")
    with pytest.raises(_lib.McgError, match=r"200 atoms.*up to 115 atoms"):
        d.plan(torch.tensor(c["sizes"], dtype=torch.int32), c["N"])
    with pytest.raises(_lib.McgError, match=r"up to 115 atoms"):
        d.plan(torch.tensor([116, 116], dtype=torch.int32), 116)


def test_fused_and_unfused_node_launch_agree_bit_for_bit_on_case_a():
    """bf16, case A (atoms span two 64-row units): the node phase of a GCL layer as ONE launch (MCG_OPT_NODE_FUSED = 2) and
    as three (1).  Both meet the bf16 tolerance against fp64, and - as route()'s comment claims - give bit-identical h,
    hence a bit-identical output."""
    from ml_conformer_generator_amd import _lib
    from ml_conformer_generator_amd.egnn import EGNNDynamics
    c, k = CASES["A"], case_data("A")
    d = EGNNDynamics(device=DEV)
    d.load_reference_state_dict(sd_for(_W))
    d.set_precision("bf16")
    sizes = torch.tensor(c["sizes"], dtype=torch.int32)
    td, zd, cd = k["t"].reshape(-1).to(DEV).contiguous(), k["z"].to(DEV), k["ctx"].to(DEV)
    L = _lib.lib()
    outs = {}
    for value, fused in ((2, True), (1, False)):
        d.set_option(_lib.OPT_NODE_FUSED, value)
        plan = d.plan(sizes, c["N"])
        assert_route(d, plan, dict(c["routes"][("bf16", "auto")], fused=fused))
        cnt = np.zeros(32, dtype=np.int64)
        _lib.check(L.mcg_debug_gemm_launches(cnt.ctypes.data, 1), "mcg_debug_gemm_launches")
        outs[fused] = d.run(plan, td, zd, cd).cpu()
        _lib.check(L.mcg_debug_gemm_launches(cnt.ctypes.data, 0), "mcg_debug_gemm_launches")
        assert (int(cnt.reshape(4, 8)[1][6]) > 0) == fused, cnt.reshape(4, 8)      # the fused launch ran / did not run
        err = float((outs[fused].double() - k["ref64"]).abs().max())
        print(f"\nLARGE-N A bf16/node_fused={value} max|err| {err:.3e} of max|ref| {k['sc']:.3e}")
        assert err <= 3e-2 * max(1.0, k["sc"]), (fused, err)
    assert torch.equal(outs[True][:, :, 3:], outs[False][:, :, 3:]), "h differs between the fused and the unfused node phase"
    assert torch.equal(outs[True], outs[False])


def test_reference_dynamics_fixture_at_114_atoms():
    """`dynamics_b3n114.npz`: one call of the REFERENCE's own `dynamics` on molecules of 114, 68 and 9 atoms."""
    g = load_golden("dynamics_b3n114.npz")
    nm = g["node_mask"]
    assert nm.sum(1).reshape(-1).tolist() == [114.0, 68.0, 9.0]
    for mode in ("f32", "f32x6"):
        d = dyn_for(g, mode)
        out = d(g["t"].to(DEV), g["xh"].to(DEV), nm.to(DEV), edge_mask_of(nm).to(DEV), g["context"].to(DEV))
        plan = next(reversed(d._plans.values()))
        assert_route(d, plan, dict(edge="Ns", agg="Combine", coord="Kernel", pspan=8) if mode == "f32"
                     else dict(edge="W64X6", agg="Combine", coord="Kernel", pspan=3))
        ok, err, sc = close(out, g["out"])
        assert ok, f"{mode}: err {err} scale {sc}"
        assert float((out.cpu() * (1 - nm)).abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["f32", "f32x6"])
def test_one_gcl_layer_at_case_d_vs_fp64(mode):
    """ONE GCL layer (block 3, gcl_0) on case D through mcg_egnn_gcl_debug + mcg_plan_peek against the fp64 layer: the
    first-layer projections, the aggregate - here the sum of up to EIGHT per-tile partial rows per atom (three per-unit rows
    in f32x6), pinned directly instead of through nine blocks - the node MLP's hidden layer and the new h."""
    import torch.nn.functional as F
    from oracle import egnn_oracle as EO
    c, k = CASES["D"], case_data("D")
    sd64 = {kk: v.double() for kk, v in sd_for(_W).items()}
    nm = k["nm"]
    B, N, _ = nm.shape
    g = torch.Generator().manual_seed(404)
    nmf = nm.reshape(B * N, 1)
    h_in = torch.randn(B * N, 420, generator=g) * nmf
    x_in = torch.randn(B * N, 3, generator=g) * nmf
    x0 = torch.randn(B * N, 3, generator=g) * nmf
    real = nmf.reshape(-1) > 0
    row, col = EO.dense_edge_index(N, B)
    d0, _ = EO.pair_geometry(x0.double(), row, col)
    d1, _ = EO.pair_geometry(x_in.double(), row, col)
    p = "dynamics.egnn.e_block_3.gcl_0."
    h_ref, _, msg_ref, agg_ref = EO.gcl(sd64, p, h_in.double(), row, col, torch.cat([d1, d0], 1), nmf.double(),
                                        edge_mask_of(nm).double())
    w1, b1 = sd64[p + "edge_mlp.0.weight"], sd64[p + "edge_mlp.0.bias"]
    pab_ref = torch.cat([F.linear(h_in.double(), w1[:, :420], b1), F.linear(h_in.double(), w1[:, 420:840])], 1)
    hid_ref = F.silu(F.linear(torch.cat([h_in.double(), agg_ref], 1), sd64[p + "node_mlp.0.weight"], sd64[p + "node_mlp.0.bias"]))
    assert float(agg_ref.abs().max()) > 0.05 and float(msg_ref.abs().max()) > 0.1      # the pins carry signal
    d = dyn_for(_W, mode)
    plan = d.plan(torch.tensor(c["sizes"], dtype=torch.int32), N, edge_mt=1 if mode == "f32" else 4, n_ranges=1)
    exp = dict(c["routes"][(mode, "auto")], agg="Combine")
    exp.pop("unit_span", None)
    assert_route(d, plan, exp, keep_agg=True)
    got = d.gcl_debug(plan, 6, h_in[real], x_in[real], x0[real])
    pab = got["pab"].cpu()
    pab = torch.cat([pab[:, :420], pab[:, 432:852]], 1)
    for what, a, b in (("pab", pab, pab_ref[real]), ("agg", got["agg"], agg_ref[real]), ("hidden", got["hidden"], hid_ref[real]),
                       ("h", got["h_out"], h_ref[real])):
        v = violation(a, b)
        print(f"\nLARGE-N D gcl {mode} {what}: {v:.4f} x tolerance of fp64")
        assert v <= 1.0, f"{mode} {what}: {v} x tolerance"


# ------------------------------------------------------------------------------------------------ sampler kernels

SENTINEL = 7.25e30
PAD = 256


def guarded(shape, fill):
    """A device buffer of `shape` with PAD sentinel floats in front and behind: (whole allocation, view of the middle)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), SENTINEL, device=DEV, dtype=torch.float32)
    mid = whole[PAD:PAD + n]
    mid.copy_(fill.reshape(-1).to(DEV) if torch.is_tensor(fill) else torch.full((n,), float(fill)))
    return whole, mid.view(shape)


def sentinels_intact(whole):
    return bool((whole[:PAD] == SENTINEL).all()) and bool((whole[-PAD:] == SENTINEL).all())


def sampler_sizes(N):
    return [n for n in (1, 63, 64, 65) if n <= N] + [N]


def centred_noise64(rx, rh, nm):
    """sample_combined_position_feature_noise in fp64: mask, remove the real atoms' mean from x, mask h."""
    rx, rh, nm = rx.double(), rh.double(), nm.double()
    ex = rx * nm
    ex = ex - (ex.sum(1, keepdim=True) / nm.sum(1, keepdim=True)) * nm
    return torch.cat([ex, rh * nm], 2)


@pytest.mark.parametrize("N", [64, 65, 114, 130])
def test_noise_and_blend_kernels_beyond_one_loop_trip(N):
    """`mcg_sampler_noise` and `mcg_sampler_blend` (modes 0 and 1) on their own: one 64-lane workgroup per molecule that
    loops i += 64 - molecules of 1, 63, 64, 65 and N atoms in one batch - against an fp64 restatement of the same formulas
    under the stated per-call tolerance.  Padded noise rows are exactly zero, mode 0 writes all N slots, and the sentinels
    in front of and behind every output stay intact."""
    from ml_conformer_generator_amd import _lib
    from ml_conformer_generator_amd.egnn import BatchPlan
    from oracle import host_oracle as HO
    L = _lib.lib()
    sizes = sampler_sizes(N)
    B = len(sizes)
    plan = BatchPlan(torch.tensor(sizes, dtype=torch.int32), N, DEV, edge_mt=1 if N <= 115 else 4)
    nm, _ = HO.masks_from_sizes(torch.tensor(sizes), N)
    g = torch.Generator().manual_seed(1000 + N)
    rx, rh = torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g)          # raw draws: padded rows are NOT zero
    st = _lib.current_stream_ptr(DEV)
    rxd, rhd = rx.to(DEV), rh.to(DEV)
    eps64 = centred_noise64(rx, rh, nm)

    whole, eps = guarded((B, N, 11), 3.0)
    _lib.check(L.mcg_sampler_noise(plan.handle, _lib.dptr(rxd), _lib.dptr(rhd), eps.data_ptr(), st), "mcg_sampler_noise")
    torch.cuda.synchronize()
    assert sentinels_intact(whole)
    e = eps.cpu()
    assert float((e * (1 - nm)).abs().max()) == 0.0
    assert violation(e, eps64, split=3) <= 1.0, violation(e, eps64, split=3)
    assert torch.equal(e[:, :, 3:], rh * nm)                                               # h noise is a masked copy

    zk = torch.randn(B, N, 11, generator=g)                                                # (padded rows of z_known not zero either)
    zkd = zk.to(DEV)                                                                       # (named: alive until the launch has run)
    alpha_s, sigma_s = 0.8125, 0.59375
    whole, z = guarded((B, N, 11), -5.0)
    _lib.check(L.mcg_sampler_blend(plan.handle, z.data_ptr(), _lib.dptr(zkd), None, _lib.dptr(rxd), _lib.dptr(rhd),
                                   alpha_s, sigma_s, 0.0, 0, st), "mcg_sampler_blend")
    torch.cuda.synchronize()
    assert sentinels_intact(whole)
    ref0 = alpha_s * zk.double() + sigma_s * eps64                                         # every one of the N slots
    assert violation(z.cpu(), ref0, split=3) <= 1.0, violation(z.cpu(), ref0, split=3)
    assert torch.equal(z.cpu() * (1 - nm), (alpha_s * zk) * (1 - nm))                      # padded slots: alpha_s * z_known exactly

    fm = torch.zeros(B, N, 1)
    for b, n in enumerate(sizes):
        for i in (0, 5, 62, 66, n - 1):
            if i < n:
                fm[b, i] = 1.0
    assert float(fm.sum(1).min()) >= 1.0                     # every fragment holds an atom ...
    assert N <= 66 or float(fm[:, 64:].sum()) >= 2.0         # ... and some lie in the loop's second trip
    z_in = torch.randn(B, N, 11, generator=g)
    fmd = fm.to(DEV)
    blend = 0.421875
    whole, z = guarded((B, N, 11), z_in)
    _lib.check(L.mcg_sampler_blend(plan.handle, z.data_ptr(), _lib.dptr(zkd), _lib.dptr(fmd), _lib.dptr(rxd),
                                   _lib.dptr(rhd), alpha_s, sigma_s, blend, 1, st), "mcg_sampler_blend")
    torch.cuda.synchronize()
    assert sentinels_intact(whole)
    f, zi = fm.double(), z_in.double()
    noised = alpha_s * zk.double() + sigma_s * eps64
    cnt = f.sum(1, keepdim=True)
    shift = (zi[:, :, :3] * f).sum(1, keepdim=True) / cnt - (noised[:, :, :3] * f).sum(1, keepdim=True) / cnt
    noised[:, :, :3] = noised[:, :, :3] + shift * f
    ref1 = blend * noised * f + (1 - blend) * zi * f + zi * (1 - f)
    assert violation(z.cpu(), ref1, split=3) <= 1.0, violation(z.cpu(), ref1, split=3)
    assert torch.equal(z.cpu() * (1 - fm), z_in * (1 - fm))                                # outside the fragment: untouched


@pytest.mark.parametrize("mode", ["f32", "f32x6"])
def test_teacher_forced_steps_and_decode_beyond_64_atoms_vs_fp64_sampler_oracle(mode):
    """`mcg_sampler_step` at three levels and `mcg_sampler_decode` on molecules of 114, 70, 65 and 9 atoms, each fed the
    same latent and the same raw draws as oracle.diffusion_oracle.SamplerOracle with fp64 weights and inputs (its schedule
    scalars stay the reference's fp32 expressions, as the HIP path's do): no error compounding.  z_s and x within the
    stated per-call tolerance, atom types exact."""
    from oracle import diffusion_oracle as DO
    from oracle import host_oracle as HO
    sizes, N, T = [114, 70, 65, 9], 114, 20
    B = len(sizes)
    nm, em = HO.masks_from_sizes(torch.tensor(sizes), N)
    g = torch.Generator().manual_seed(77)
    ctx = torch.randn(B, 1, 3, generator=g).repeat(1, N, 1) * nm
    sd64 = {k: v.double() for k, v in sd_for(_W).items()}
    gm = sampler_for(T, _W, mode)
    run = gm._Run(gm, nm.to(DEV), ctx)
    from ml_conformer_generator_amd import _lib
    assert _lib.debug_route(gm.dynamics.handle, run.plan.handle)["edge"] == ("Ns" if mode == "f32" else "W64X6")
    per = B * N * 11
    try:
        for s_int in (18, 9, 0):
            z_in = centred_noise64(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nm).float()
            tape = torch.randn(per, generator=g)
            orc = DO.SamplerOracle(sd64, T, noise_fn=TapeNoise(tape))
            s, t = orc._times(s_int, B)
            ref = orc.step(s, t, z_in.double(), nm.double(), em.double(), ctx.double())
            assert ref.dtype == torch.float64
            gm.noise_fn = TapeNoise(tape, DEV)
            z_out = gm._step(run, z_in.to(DEV).contiguous().clone(), s_int).cpu()
            assert gm.noise_fn.pos == orc.noise_fn.pos == per
            v = violation(z_out, ref, split=3)
            print(f"\nLARGE-N step {mode} s={s_int}: {v:.4f} x tolerance of the fp64 sampler oracle")
            assert v <= 1.0, (s_int, v)
            assert float((z_out * (1 - nm)).abs().max()) == 0.0
        z0 = centred_noise64(torch.randn(B, N, 3, generator=g), torch.randn(B, N, 8, generator=g), nm).float()
        tape = torch.randn(per, generator=g)
        orc = DO.SamplerOracle(sd64, T, noise_fn=TapeNoise(tape))
        x_ref, h_ref = orc.decode(z0.double(), nm.double(), em.double(), ctx.double())
        gm.noise_fn = TapeNoise(tape, DEV)
        x, h = gm._decode(run, z0.to(DEV).contiguous())
        assert gm.noise_fn.pos == orc.noise_fn.pos == per
        ok, err, sc = close(x.cpu(), x_ref)
        assert ok, (err, sc)
        assert torch.equal(h.cpu().to(torch.int64), h_ref.to(torch.int64))
        assert float((x.cpu() * (1 - nm)).abs().max()) == 0.0
    finally:
        gm.noise_fn = None


@pytest.mark.parametrize("mode", ["f32", "f32x6"])
def test_reference_trajectory_at_101_atoms(mode):
    """`sampler_T8_b3n101.npz`: the reference's own forward sampler on molecules of 70, 101 and 9 atoms under a recorded
    noise tape, every z_s kept.  Same number and order of draws, every step within 1e-3 of its own magnitude, final x within
    tolerance, atom types exact."""
    g = load_golden("sampler_T8_b3n101.npz")
    nm = g["node_mask"]
    assert nm.sum(1).reshape(-1).tolist() == [70.0, 101.0, 9.0]
    gm = sampler_for(int(g["T"]), g, mode)
    gm.noise_fn = TapeNoise(g["noise"], DEV)
    gm.trace = []
    try:
        x, h = gm(nm.to(DEV), edge_mask_of(nm).to(DEV), g["context"].to(DEV), int(g["resample_steps"]))
        assert gm.noise_fn.pos == g["noise"].numel()
        v = traj_violation(torch.stack(gm.trace).cpu(), g["z_trace"])
    finally:
        gm.noise_fn, gm.trace = None, None
    print(f"\nLARGE-N trajectory sampler_T8_b3n101 {mode}: {v:.4f} x tolerance")
    assert v <= 1.0, f"trajectory at {v} x tolerance"
    assert traj_violation(x.cpu().unsqueeze(0), g["x"].unsqueeze(0), split=None) <= 1.0
    assert torch.equal(h.cpu().to(torch.int64), g["h"].to(torch.int64))


@pytest.mark.parametrize("mode", ["f32", "f32x6"])
def test_reference_inpainting_at_80_atoms(mode):
    """`inpaint_T5_rs1_b2n80.npz`: the reference's `inpaint` with a fixed fragment of 7 atoms, resampling 1, molecules of
    80 and fewer atoms (layout of inpaint_T5.npz)."""
    g = load_golden("inpaint_T5_rs1_b2n80.npz")
    nm = g["node_mask"]
    assert int(nm.sum(1).max()) == 80 and int(g["fixed_mask"].sum(1).max()) == 7
    gm = sampler_for(int(g["T"]), g, mode)
    gm.noise_fn = TapeNoise(g["noise"], DEV)
    gm.trace = []
    try:
        x, h = gm.inpaint(nm.to(DEV), edge_mask_of(nm).to(DEV), g["context"].to(DEV), g["z_known"], g["fixed_mask"],
                          int(g["resample_steps"]), int(g["blend_power"]))
        assert gm.noise_fn.pos == g["noise"].numel()
        v = traj_violation(torch.stack(gm.trace).cpu(), g["z_trace"])
    finally:
        gm.noise_fn, gm.trace = None, None
    print(f"\nLARGE-N trajectory inpaint_T5_rs1_b2n80 {mode}: {v:.4f} x tolerance")
    assert v <= 1.0, f"trajectory at {v} x tolerance"
    assert traj_violation(x.cpu().unsqueeze(0), g["x"].unsqueeze(0), split=None) <= 1.0
    assert torch.equal(h.cpu().to(torch.int64), g["h"].to(torch.int64))
