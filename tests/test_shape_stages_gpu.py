"""The shape-moment and frame kernels and the grid Tanimoto on the MI355X, stage by stage against the fp64 restatement of
`tests/shape_ref.py`, over the cases of `tests/shape_cases.py` (single atoms, pairs at the threshold, coincident atoms,
rings, tetrahedra, cubes, chains, disconnected molecules, atom 63 in cliques): nothing degenerate is left out.  The
tolerances are the counts of error units measured in `tests/test_shape_stages_host.py` (`shape_ref.TOL_UNITS`)."""
import math

import numpy as np
import pytest
import torch

import shape_cases as C
import shape_ref as R
from shape_pair_cases import lattice64 as _lattice64
from test_shape_diversity_gpu import PAIR_ATOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _batch():
    x, n, where = C.ragged_batch()
    return torch.from_numpy(x).to(DEV), torch.from_numpy(n).to(DEV), where


def _moments_kernel(x, n, terms, centre, params):
    """`mcg_shape_moments` called directly: (volume [B] fp64, centre [B,3], tensor [B,3,3], counts [B, terms-1]) on the host."""
    from ml_conformer_generator_amd import _lib
    radius, amp, thr = C.PARAMS[params]
    B, N, _ = x.shape
    x = x.contiguous()
    n = n.to(torch.int32).contiguous()
    centre_o = torch.empty(B, 3, device=DEV)
    tensor_o = torch.empty(B, 9, device=DEV)
    volume_o = torch.empty(B, dtype=torch.float64, device=DEV)
    counts_o = torch.empty(B, terms - 1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().mcg_shape_moments(_lib.dptr(x), _lib.dptr(n), B, N, R.get_alpha(radius, amp), float(amp), float(thr),
                                            terms, int(centre), _lib.dptr(centre_o), _lib.dptr(tensor_o), _lib.dptr(volume_o),
                                            _lib.dptr(counts_o), _lib.current_stream_ptr(DEV)), "mcg_shape_moments")
    return (volume_o.cpu().numpy(), centre_o.cpu().numpy().astype(np.float64),
            tensor_o.cpu().numpy().astype(np.float64).reshape(B, 3, 3), counts_o.cpu().numpy())


def _frames(x, n, terms, centre, params):
    """`shape_frames_hip(..., xform_out=...)`: (moments [B,3], frames [B,N,3], xform [B,12]) on the host."""
    from ml_conformer_generator_amd.cheminformatics import shape_frames_hip
    radius, amp, thr = C.PARAMS[params]
    xform = torch.full((x.shape[0], 12), float("nan"), device=DEV)
    mom, fr = shape_frames_hip(x, n, DEV, amplitude=amp, atom_radius=radius, n_terms=terms, neighbour_threshold=thr,
                               centre_atoms=centre, xform_out=xform)
    return mom.cpu().numpy(), fr.cpu().numpy(), xform.cpu().numpy()


@pytest.mark.parametrize("params", list(C.PARAMS))
@pytest.mark.parametrize("terms", C.ORDERS)
def test_moments_kernel_against_fp64(terms, params):
    """`mcg_shape_moments` alone: clique counts exact, volume, shape centre and second-moment tensor within TOL_UNITS of
    the restatement for every case, with and without `centre_atoms`.  The far hexagon without centring is checked for
    finite output only (see `test_frames_against_fp64`)."""
    x, n, where = _batch()
    worst = {"volume": 0.0, "centre": 0.0, "tensor": 0.0}
    for centre in (False, True):
        vol, cen, ten, counts = _moments_kernel(x, n, terms, centre, params)
        for c in C.cases():
            b = where[c.name]
            ref = C.reference(c.name, terms, centre, params)
            tag = f"{c.name} n_terms={terms} centre={int(centre)} {params}"
            assert counts[b].tolist() == ref["counts"].tolist(), tag
            if c.centre_only and not centre:
                assert math.isfinite(vol[b]) and np.isfinite(cen[b]).all() and np.isfinite(ten[b]).all(), tag
                continue
            got = {"volume": R.ratio(abs(vol[b] - ref["volume"]), R.TOL_UNITS["volume"] * ref["u_volume"]),
                   "centre": R.ratio(float(np.abs(cen[b] - ref["centre"]).max()), R.TOL_UNITS["centre"] * ref["u_centre"]),
                   "tensor": R.ratio(float(np.abs(ten[b] - ref["tensor"]).max()), R.TOL_UNITS["tensor"] * ref["u_tensor"])}
            for k, v in got.items():
                worst[k] = max(worst[k], v)
                assert v <= 1.0, (tag, k, v)
        e = C.EMPTY_ROW
        assert vol[e] == 0.0 and counts[e].tolist() == [0] * (terms - 1) and not np.isfinite(ten[e]).any()
    print(f"SHAPE-STAGES moments n_terms={terms} {params}: worst error / tolerance "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("params", list(C.PARAMS))
@pytest.mark.parametrize("terms", C.ORDERS)
def test_frames_against_fp64(terms, params):
    """`shape_frames_hip(..., xform_out=...)`: sorted moments against fp64 `eigvalsh` and the basis-independent invariants of
    `shape_ref.check_frame` on every row, the fully degenerate cases included.  The empty row has NaN moments and frames
    of exact 0.  The far hexagon WITHOUT centring is checked for finite output only: at (200, -150, 90) the fp32
    gamma = q - |s|^2 / k cancels for any evaluation order (q is about 7e4 k, rounded to 4e-3 k, against a gamma of a few
    A^2); the project's fp32 tensor path is 4.3e-3 relative off in volume and 7.4e-3 absolute in the tensor there."""
    x, n, where = _batch()
    worst = {}
    for centre in (False, True):
        mom, fr, xf = _frames(x, n, terms, centre, params)
        for c in C.cases():
            b = where[c.name]
            ref = C.reference(c.name, terms, centre, params)
            tag = f"{c.name} n_terms={terms} centre={int(centre)} {params}"
            if c.centre_only and not centre:
                assert np.isfinite(mom[b]).all() and np.isfinite(fr[b]).all() and np.isfinite(xf[b]).all(), tag
                continue
            got = R.check_frame(c.points, fr[b], xf[b], mom[b], ref)
            got["moments"] = R.ratio(float(np.abs(mom[b].astype(np.float64) - ref["moments"]).max()),
                                     R.TOL_UNITS["moments"] * ref["u_moments"])
            for k, v in got.items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= 1.0, (tag, k, v)
        e = C.EMPTY_ROW
        assert np.isnan(mom[e]).all() and float(np.abs(fr[e]).max()) == 0.0
    print(f"SHAPE-STAGES frames n_terms={terms} {params}: worst measured / allowed "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("centre", [False, True])
def test_a_case_alone_and_in_the_ragged_batch_gives_the_same_bits(centre):
    """Every case alone at N = n and in its row of the ragged batch at N = 64 (next to the empty row and the 64-atom helix):
    `mcg_shape_moments`' four outputs, the sorted moments, the frame and its transform, bit for bit."""
    x, n, where = _batch()
    vol, cen, ten, counts = _moments_kernel(x, n, 6, centre, "default")
    mom, fr, xf = _frames(x, n, 6, centre, "default")
    for c in C.cases():
        b, k = where[c.name], c.points.shape[0]
        xa = torch.from_numpy(c.points).to(DEV).unsqueeze(0)
        na = torch.tensor([k], dtype=torch.int32, device=DEV)
        a_vol, a_cen, a_ten, a_counts = _moments_kernel(xa, na, 6, centre, "default")
        a_mom, a_fr, a_xf = _frames(xa, na, 6, centre, "default")
        for one, many in ((a_vol[0], vol[b]), (a_cen[0], cen[b]), (a_ten[0], ten[b]), (a_counts[0], counts[b]),
                          (a_mom[0], mom[b]), (a_fr[0], fr[b, :k]), (a_xf[0], xf[b])):
            assert np.array_equal(np.asarray(one), np.asarray(many), equal_nan=True), c.name


# ----------------------------------------------------------------------------------------------- grid half
def _proper_rotations(count):
    g = np.random.default_rng(11)
    out = []
    for _ in range(count):
        q, _ = np.linalg.qr(g.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    rots = np.stack(out).astype(np.float32)
    assert all(np.linalg.det(r.astype(np.float64)) > 0.999 for r in rots)
    return rots


def _tanimoto_kernel(ref, cand, n_nodes, rots, axes):
    """`mcg_shape_tanimoto` through the C entry: score [B, R] on the host."""
    from ml_conformer_generator_amd import _lib
    from ml_conformer_generator_amd.cheminformatics import ALPHA, AMPLITUDE
    B, N, _ = cand.shape
    Rn, n = rots.shape[0], axes.shape[1]
    ref_d = torch.from_numpy(ref).to(DEV).contiguous()
    cand_d = torch.from_numpy(cand).to(DEV).contiguous()
    nn = torch.from_numpy(n_nodes).to(DEV, torch.int32).contiguous()
    rots_d = torch.from_numpy(rots.reshape(Rn, 9)).to(DEV).contiguous()
    axes_d = torch.from_numpy(axes).to(DEV).contiguous()
    f = torch.empty(n ** 3, device=DEV)
    score = torch.full((B * Rn,), float("nan"), device=DEV)
    _lib.check(_lib.lib().mcg_shape_tanimoto(_lib.dptr(ref_d), ref.shape[0], _lib.dptr(cand_d), _lib.dptr(nn), B, N,
                                             _lib.dptr(rots_d), Rn, _lib.dptr(axes_d), n, float(ALPHA), float(AMPLITUDE),
                                             _lib.dptr(f), _lib.dptr(score), _lib.current_stream_ptr(DEV)),
               "mcg_shape_tanimoto")
    return score.cpu().numpy().reshape(B, Rn)


def _grid_candidates():
    """Candidates of 0, 1, 23 and 64 atoms at N = 64; the empty row's coordinates are not zero."""
    p = _lattice64()
    cand = np.zeros((4, 64, 3), dtype=np.float32)
    n_nodes = np.array([0, 1, 23, 64], dtype=np.int32)
    cand[0, :10] = p[:10]
    cand[1, 0] = p[21]
    cand[2, :23] = p[20:43] + np.float32(0.3)
    cand[3] = p[::-1] + np.float32(0.2)
    return cand, n_nodes


@pytest.mark.parametrize("n", [5, 7, 40])
@pytest.mark.parametrize("n_ref", [3, 64])
def test_grid_tanimoto_against_fp64(n_ref, n):
    """`mcg_shape_tanimoto` against `shape_ref.grid_tanimoto`: references of 3 and 64 atoms, candidates of 0, 1, 23 and 64 atoms,
    grids of 125 points (fewer than a workgroup's lanes), 343 (partial strides) and 64 000, one and five arbitrary proper
    rotations.  PAIR_ATOL, the project's bound of fp32 densities and sums against fp64 on this grid
    (`tests/test_shape_diversity_gpu.py`)."""
    from ml_conformer_generator_amd.cheminformatics import ALPHA, AMPLITUDE, _grid_axes
    ref = np.ascontiguousarray(_lattice64()[:n_ref])
    axes = _grid_axes(torch.from_numpy(ref), n).numpy()
    cand, n_nodes = _grid_candidates()
    rots = _proper_rotations(5)
    f = R.grid_density(ref, axes, ALPHA, AMPLITUDE)
    worst = 0.0
    for use in (rots, rots[3:4]):
        got = _tanimoto_kernel(ref, cand, n_nodes, use, axes)
        assert got.shape == (4, use.shape[0]) and (got[0] == 0.0).all()             # the empty row: exactly 0
        for b in range(4):
            for r in range(use.shape[0]):
                want = R.grid_tanimoto(ref, cand[b, : n_nodes[b]], use[r], axes, ALPHA, AMPLITUDE, f=f)
                err = abs(float(got[b, r]) - want)
                worst = max(worst, err)
                assert err < PAIR_ATOL, (n_ref, n, b, r, got[b, r], want)
    print(f"SHAPE-STAGES grid n_ref={n_ref} n={n}: max |score - fp64| = {worst:.2e} (allowed {PAIR_ATOL:.0e})")


def test_all_64_atoms_of_a_row_count():
    """At N = 64 with n_nodes = 64 the last atom is scored: moving atom 63 alone changes the score, and both scores match
    the restatement.  (A row wider than 64 is refused: `tests/test_shape_stages_host.py`.)"""
    from ml_conformer_generator_amd.cheminformatics import ALPHA, AMPLITUDE, _grid_axes, _orientations, shape_tanimoto_batch
    ref = _lattice64()
    cand = np.stack([ref, ref])
    cand[1, 63] += np.array([2.0, 2.0, 1.0], dtype=np.float32)
    n_nodes = torch.tensor([64, 64])
    scores, _, _ = shape_tanimoto_batch(torch.from_numpy(ref), torch.from_numpy(cand), n_nodes, DEV)
    scores = scores.cpu().numpy()
    axes = _grid_axes(torch.from_numpy(ref), 40).numpy()
    rot = _orientations().numpy()
    want = [R.grid_tanimoto(ref, cand[b], rot[0], axes, ALPHA, AMPLITUDE) for b in range(2)]
    print(f"SHAPE-STAGES atom 63: fp64 {want[0]:.6f} -> {want[1]:.6f}, kernel {scores[0, 0]:.6f} -> {scores[1, 0]:.6f}")
    assert abs(want[0] - want[1]) > 10 * PAIR_ATOL                       # the move is worth seeing
    for b in range(2):
        assert abs(float(scores[b, 0]) - want[b]) < PAIR_ATOL, b
    assert float(scores[0, 0]) != float(scores[1, 0])
