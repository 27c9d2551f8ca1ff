"""The shape-moment and frame stage pinned against fp64, host side (no GPU): closed forms and self-checks of the restatement
(`tests/shape_ref.py`), the measurement behind the GPU tolerances (the project's fp32 tensor path over every case of
`tests/shape_cases.py`), the proof that those tolerances would catch the mistakes a kernel could make, the builders'
conditions, and the refusal of rows wider than 64 atoms by the grid Tanimoto in C and in Python."""
import ctypes
import math

import numpy as np
import pytest
import torch

import shape_cases as C
import shape_ref as R

GOLDEN_NAMES = ["ceyyag", "yibfeu", "paba", "crown_6", "walk12", "walk27"]
QUANTITIES = ("volume", "centre", "tensor", "moments", "offdiag", "diag", "frame_centre")


# ----------------------------------------------------------------------------------------------- closed forms
def test_single_atom_closed_form():
    for params in C.PARAMS:
        radius, amp, _ = C.PARAMS[params]
        alpha = R.get_alpha(radius, amp)
        p = np.array([[0.3, -0.2, 0.5]], dtype=np.float32)
        for terms in C.ORDERS:
            r = R.restate(p, n_terms=terms, amplitude=amp, atom_radius=radius, threshold=3.0)
            assert abs(r["volume"] - amp * (math.pi / alpha) ** 1.5) <= 1e-14 * r["volume"]
            assert float(np.abs(r["tensor"] - np.eye(3) / (2 * alpha)).max()) <= 1e-14 / alpha
            assert float(np.abs(r["centre"] - p[0].astype(np.float64)).max()) <= 1e-15
            assert r["counts"].tolist() == [0] * (terms - 1)


def test_pair_closed_form():
    c = C.case("pair")
    alpha, A = R.get_alpha(), R.AMPLITUDE
    p = c.points.astype(np.float64)
    d2 = float(((p[0] - p[1]) ** 2).sum())
    k1, k2 = (math.pi / alpha) ** 1.5, (math.pi / (2 * alpha)) ** 1.5
    w1, w2 = A * k1, A * A * math.exp(-alpha * d2 / 2) * k2         # gamma of the pair = d^2 / 2
    vol = 2 * w1 - w2
    along = (2 * w1 * (d2 / 4 + 1 / (2 * alpha)) - w2 / (4 * alpha)) / vol          # both atoms d/2 from the midpoint
    across = (2 * w1 / (2 * alpha) - w2 / (4 * alpha)) / vol
    r = C.reference("pair")
    assert r["counts"].tolist() == [1, 0, 0, 0, 0]
    assert abs(r["volume"] - vol) <= 1e-13 * vol
    assert float(np.abs(r["centre"] - p.mean(axis=0)).max()) <= 1e-13
    assert float(np.abs(r["moments"] - np.array([along, across, across])).max()) <= 1e-13 * along
    assert abs(r["per_order"][1]["volume"] - 2 * w1) <= 1e-13 * vol and abs(r["per_order"][2]["volume"] + w2) <= 1e-13 * vol


# ----------------------------------------------------------------------------------------------- restatement self-checks
def test_restatement_is_invariant_under_rotation_and_translation():
    g = np.random.default_rng(7)
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    t = np.array([3.1, -2.7, 1.9])
    for c in C.cases():
        ref = C.reference(c.name, 8)
        p = c.points.astype(np.float64)
        alpha, amp = ref["alpha"], ref["amplitude"]
        a = R.from_points(p, ref["cliques"], 8, alpha, amp)
        b = R.from_points(p @ q + t, ref["cliques"], 8, alpha, amp)
        assert abs(a["volume"] - b["volume"]) <= 1e-10 * abs(a["volume"]), c.name
        assert float(np.abs(a["moments"] - b["moments"]).max()) <= 1e-10 * float(a["moments"].max()), c.name
        assert float(np.abs(b["centre"] - (a["centre"] @ q + t)).max()) <= 1e-10 * (1 + float(np.abs(b["centre"]).max()))


def test_restatement_matches_the_fixture_moments():
    """All six goldens, crown_6 included, at the fixture tests' own 2e-5 (eigenvalues stay well conditioned where
    eigenvectors are not)."""
    g = np.load(C.GOLDEN, allow_pickle=False)
    for k in GOLDEN_NAMES:
        r = R.restate(g[f"xyz_{k}"].astype(np.float32))
        err = float(np.abs(r["moments"] - g[f"moments_{k}"].astype(np.float64)).max())
        print(f"SHAPE-REF fixture {k}: max |moment - fixture| = {err:.2e}")
        assert err < 2e-5, k


# ----------------------------------------------------------------------------------------------- the tolerance, measured
def _tensor_path(x: np.ndarray, n: np.ndarray, n_terms: int, radius: float, amp: float, thr: float):
    """The project's fp32 tensor path on the CPU: (counts, volume, centre, tensor, moments, frames) of every row."""
    from ml_conformer_generator_amd import cheminformatics as CH
    xt, nn = torch.from_numpy(x), torch.from_numpy(n).long()
    B, N, _ = xt.shape
    real = torch.arange(N).unsqueeze(0) < nn.reshape(B, 1)
    alpha = CH.get_alpha(radius, amp)
    d = torch.sqrt(((xt.unsqueeze(2) - xt.unsqueeze(1)) ** 2).sum(-1))
    adj = (d < thr) & (d > 0) & real.unsqueeze(1) & real.unsqueeze(2)
    cl = CH._grow_cliques(adj, n_terms)
    counts = torch.stack([torch.bincount(cl[k][:, 0], minlength=B) for k in range(2, n_terms + 1)], dim=1)
    vol, first, _, _ = CH._shape_moments(xt, real, cl, alpha, amp)
    centre = (first / vol.unsqueeze(1)).to(torch.float32)
    centred = (xt - centre.unsqueeze(1)) * real.unsqueeze(2)
    _, _, ii, ij = CH._shape_moments(centred, real, cl, alpha, amp)
    tensor = CH._moment_tensor(ii, ij, vol)
    moments, frames = CH.shape_quadrupole_batch(xt, nn, "cpu", amp, radius, n_terms, thr)
    return counts.numpy(), vol.numpy(), centre.numpy(), tensor.numpy(), moments.numpy(), frames.numpy()


def test_tensor_path_error_in_units_sets_the_gpu_tolerance(capsys):
    """The measurement behind `shape_ref.TOL_UNITS`: the worst distance of the fp32 tensor path from the restatement over
    every case, order, centring mode and parameter set, in the error units of `shape_ref`.  It must stay within HALF of
    TOL_UNITS (the GPU tests hold the kernels within TOL_UNITS); its clique counts must be the restatement's exactly."""
    cases = C.cases()
    ones = {k: 1.0 for k in QUANTITIES}
    worst = {k: (0.0, "") for k in QUANTITIES}
    far, worst_plain = {}, (0.0, "")
    for params, (radius, amp, thr) in C.PARAMS.items():
        for centre in (False, True):
            x = np.zeros((len(cases), C.WIDTH, 3), dtype=np.float32)
            n = np.array([c.points.shape[0] for c in cases], dtype=np.int32)
            for b, c in enumerate(cases):
                x[b, : n[b]] = R.centre_atoms_fp32(c.points)[0] if centre else c.points
            for terms in C.ORDERS:
                counts, vol, cen, ten, mom, frames = _tensor_path(x, n, terms, radius, amp, thr)
                for b, c in enumerate(cases):
                    ref = C.reference(c.name, terms, centre, params)
                    tag = f"{c.name} n_terms={terms} centre={int(centre)} {params}"
                    assert counts[b].tolist() == ref["counts"].tolist(), tag
                    got = {"volume": R.ratio(abs(vol[b] - ref["volume"]), ref["u_volume"]),
                           "centre": R.ratio(float(np.abs(cen[b] - ref["centre"]).max()), ref["u_centre"]),
                           "tensor": R.ratio(float(np.abs(ten[b] - ref["tensor"]).max()), ref["u_tensor"]),
                           "moments": R.ratio(float(np.abs(mom[b] - ref["moments"]).max()), ref["u_moments"])}
                    if c.centre_only and not centre:
                        if terms == 6 and params == "default":
                            far = {"volume_rel": abs(vol[b] - ref["volume"]) / ref["volume"],
                                   "tensor_abs": float(np.abs(ten[b] - ref["tensor"]).max()), **got}
                        continue
                    chk = R.check_frame(x[b, : n[b]], frames[b], None, mom[b], ref, tol_units=ones)
                    assert chk["padding"] == 0.0 and chk["descending"] == 0.0, tag
                    got.update({k: chk[k] for k in ("offdiag", "diag", "frame_centre")})
                    plain = R.ratio(float(np.abs(ten[b] - ref["tensor"]).max()), ref["u_tensor_plain"])
                    if plain > worst_plain[0]:
                        worst_plain = (plain, tag)
                    for k, v in got.items():
                        assert math.isfinite(v), (tag, k)
                        if v > worst[k][0]:
                            worst[k] = (v, tag)
    with capsys.disabled():
        print()
        for k in QUANTITIES:
            print(f"SHAPE-REF tensor path, worst {k:13s} {worst[k][0]:7.2f} units at {worst[k][1]}   "
                  f"(TOL_UNITS {R.TOL_UNITS[k]:.1f})")
        print(f"SHAPE-REF tensor path, worst tensor in units WITHOUT the condition of gamma: {worst_plain[0]:.1f} at "
              f"{worst_plain[1]}")
        print("SHAPE-REF tensor path on the far hexagon WITHOUT centring (n_terms 6, defaults): "
              + ", ".join(f"{k} {v:.3g}" for k, v in far.items()))
    for k in QUANTITIES:
        assert worst[k][0] <= 0.5 * R.TOL_UNITS[k], (k, worst[k])
        assert R.TOL_UNITS[k] == 4.0 * R.MEASURED_UNITS[k] and R.TOL_UNITS[k] <= 50.0, k


# ----------------------------------------------------------------------------------------------- the tolerance has teeth
def _doubled_hexagon() -> np.ndarray:
    """The hexagon with its first atom repeated: the compact case made to carry a coincident pair, and to lose the symmetry
    that makes the atoms' mean equal the shape centre in all three compact cases."""
    p = C.case("hexagon").points
    return np.concatenate([p, p[:1]])


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_each_planted_mistake_exceeds_ten_tolerances(mutation):
    """Every mutated restatement is further than 10 x the GPU tolerance from the true one, in `tensor` or `volume`, on at least
    one compact case.  Two mistakes need a geometry the plain compact cases cannot give: `<=` at the threshold shows only
    where a pair lies exactly AT it (the threshold is set to the cube's largest fp32 distance, its body diagonal), and
    coincident atoms / the atoms' mean as centre show only with a coincident pair / without the symmetry (the hexagon with
    one atom doubled)."""
    trials = [(C.case(k).points, C.THRESHOLD) for k in C.COMPACT]
    trials.append((_doubled_hexagon(), C.THRESHOLD))
    cube = C.case("cube").points
    trials.append((cube, float(R.fp32_distances(cube).max())))
    best = 0.0
    for p, thr in trials:
        true = R.restate(p, threshold=thr)
        bad = R.restate(p, threshold=thr, mutation=mutation)
        v = abs(bad["volume"] - true["volume"]) / (R.TOL_UNITS["volume"] * true["u_volume"])
        t = float(np.abs(bad["tensor"] - true["tensor"]).max()) / (R.TOL_UNITS["tensor"] * true["u_tensor"])
        best = max(best, v, t)
    print(f"SHAPE-REF mutation {mutation}: {best:.3g} tolerances")
    assert best > 10.0, mutation


# ----------------------------------------------------------------------------------------------- the cases
def test_builders_conditions_hold_and_the_batch_holds_every_case():
    cases = C.cases()                                      # every builder asserts its own condition
    assert len(cases) == len(C.BUILDERS) == 17 and len({c.name for c in cases}) == 17
    x, n, where = C.ragged_batch()
    assert x.shape == (18, 64, 3) and x.dtype == np.float32 and int(n[C.EMPTY_ROW]) == 0
    for c in cases:
        b = where[c.name]
        assert int(n[b]) == c.points.shape[0] and np.array_equal(x[b, : n[b]], c.points)
        assert float(np.abs(x[b, n[b]:]).sum()) == 0.0
    assert sorted(int(v) for v in n)[:3] == [0, 1, 2] and int(n.max()) == 64
    assert [c.name for c in cases if c.centre_only] == ["far_hexagon"]
    kinds = {c.degenerate for c in cases}
    assert kinds == {"none", "top2", "low2", "all3", "near"}


# ----------------------------------------------------------------------------------------------- the width gap
def test_grid_tanimoto_entries_refuse_rows_wider_than_64_without_a_gpu():
    from ml_conformer_generator_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its host-side check
    for N in (65, 128, 0):
        assert h.mcg_shape_tanimoto(p, 17, p, p, 3, N, p, 4, p, 40, 0.8, 2.7, p, p, None) == 1, N
        assert b"mcg_shape_tanimoto:" in h.mcg_last_error() and b"N <= 64" in h.mcg_last_error(), N
        assert h.mcg_shape_tanimoto_field(p, p, p, 3, N, p, 4, p, 40, 0.8, 2.7, p, None) == 1, N
        assert b"mcg_shape_tanimoto_field" in h.mcg_last_error() and b"N <= 64" in h.mcg_last_error(), N


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"_lib.{name} touched before the width was checked")


def test_python_scoring_refuses_rows_wider_than_64_before_any_device_work(monkeypatch):
    from ml_conformer_generator_amd import cheminformatics as CH
    monkeypatch.setattr(CH, "_lib", _Untouchable())
    ref = torch.from_numpy(C.case("paba").points)
    wide, n = torch.zeros(2, 65, 3), torch.tensor([65, 10])
    with pytest.raises(ValueError, match="at most 64 atoms"):
        CH.shape_tanimoto_batch(ref, wide, n)
    with pytest.raises(ValueError, match="at most 64 atoms"):
        CH.evaluate_shape(ref, wide, n)
    with pytest.raises(ValueError, match="at most 64 atoms"):
        CH.tanimoto_score(ref, torch.zeros(65, 3))
    with pytest.raises(AssertionError, match="touched"):               # 64 wide is not refused: it goes on to the library
        CH.shape_tanimoto_batch(ref, torch.zeros(2, 64, 3), torch.tensor([64, 10]), device="cpu")
