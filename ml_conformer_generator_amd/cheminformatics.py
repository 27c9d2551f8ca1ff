"""Shape similarity of generated samples to the reference.

Mirrors the shape half of `evaluate_samples` (`cheminformatics/pipeline.py:30-85`): principal shape frames
(`get_shape_quadrupole_for_molecule`, `cheminformatics/shape_similarity.py:18-202`), the four-orientation search
and `tanimoto_score` (:448-492), batched over all candidates on the device.  The grid overlap is a HIP kernel
(`mcg_shape_tanimoto`); the frame construction is batched tensor algebra around it (neighbour cliques grown
level by level as index tensors, Gaussian inclusion-exclusion moments accumulated per molecule), with the 3x3
eigen-decomposition on the host in the reference's own LAPACK path so that eigenvector signs - which decide
between a frame and its mirror image - are the reference's.  The RDKit fingerprint similarity and mol-block
output of `evaluate_samples` are outside this build.  `shape_frames_hip` / `shape_scores` are the device scoring path of the
generation entries: the same frames by two HIP launches (`mcg_shape_moments`, `mcg_shape_frames`: cliques enumerated in
LDS, never stored) around the same host `eigh`, bit-identical for a molecule whatever its batch.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Tuple

import torch

from . import _args, _lib
from ._args import check_n_nodes        # its first home: callers and tests still find it here

ATOM_RADIUS = 1.60      # shape_similarity.py:14
AMPLITUDE = 2.70        # shape_similarity.py:15


def get_alpha(atom_radius: float = ATOM_RADIUS, gaussian_amplitude: float = AMPLITUDE) -> float:
    lam = 4 * math.pi / 3 / gaussian_amplitude
    return (math.pi / lam ** (2 / 3)) / atom_radius ** 2


ALPHA = get_alpha()


def rotation_matrix(angles: torch.Tensor) -> torch.Tensor:
    """M such that rotate_coord(coord, angles) == coord @ M  (shape_similarity.py:448-463)."""
    c, s = torch.cos(angles), torch.sin(angles)
    rx = torch.tensor([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    ry = torch.tensor([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    rz = torch.tensor([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    return rx @ ry @ rz


def _orientations() -> torch.Tensor:
    """The four orientations of `evaluate_samples`' search: identity, pi about x, y, z (all proper), [4,3,3] fp32."""
    pi = torch.pi
    return torch.stack([rotation_matrix(a) for a in (torch.zeros(3), torch.tensor([pi, 0, 0]), torch.tensor([0, pi, 0]),
                                                     torch.tensor([0, 0, pi]))]).to(torch.float32)


def _grid_axes(ref_coord: torch.Tensor, n: int, bounds_scale: float = 6.0, max_sigma: float = ATOM_RADIUS):
    """The reference's `Grid` axes.  Its min/max run over the xyz axis of cat(ref, cand), so the bounds are
    the per-atom extrema of the first three atoms - which belong to the reference (shape_similarity.py:476-480,
    405-419); candidates never influence the grid."""
    if ref_coord.shape[0] < 3:
        raise ValueError("the reference needs at least 3 atoms")
    lo = ref_coord[:3].min(dim=1).values - bounds_scale * max_sigma
    hi = ref_coord[:3].max(dim=1).values + bounds_scale * max_sigma
    return torch.stack([torch.linspace(lo[k], hi[k], n) for k in range(3)])


@torch.no_grad()
def shape_tanimoto_batch(ref_coord: torch.Tensor, cand_coords: torch.Tensor, n_nodes: torch.Tensor,
                         device=None, n: int = 40, alpha: float = ALPHA, amplitude: float = AMPLITUDE
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """scores[B,4] for the orientations (identity, pi about x, y, z), the best score per candidate and its
    orientation index - the search `evaluate_samples` runs one candidate at a time.  A padded width above
    MAX_SCORED_ATOMS is refused with ValueError before any device work (the kernel holds 64 atoms per row)."""
    B, N, _ = cand_coords.shape
    if N > MAX_SCORED_ATOMS:
        raise ValueError(f"the shape kernels take at most {MAX_SCORED_ATOMS} atoms per molecule, got a padded width of {N}")
    dev = _args.resolve_device(device, cand_coords)
    ref = ref_coord.to(torch.float32).cpu().contiguous()
    axes = _grid_axes(ref, n)
    ref_d, cand_d = ref.to(dev), cand_coords.to(dev, torch.float32).contiguous()
    nn = n_nodes.to(dev, torch.int32).contiguous()
    rots_d, axes_d = _orientations().to(dev).contiguous(), axes.to(dev).contiguous()
    f = torch.empty(n ** 3, device=dev)
    score = torch.empty(B * 4, device=dev)
    _lib.check(_lib.lib().mcg_shape_tanimoto(_lib.dptr(ref_d), ref.shape[0], _lib.dptr(cand_d), _lib.dptr(nn), B, N,
                                             _lib.dptr(rots_d), 4, _lib.dptr(axes_d), n, float(alpha), float(amplitude),
                                             _lib.dptr(f), _lib.dptr(score), _lib.current_stream_ptr(dev)),
               "mcg_shape_tanimoto")
    scores = score.reshape(B, 4)
    best, which = scores.max(dim=1)
    return scores, best, which


def tanimoto_score(ref_coord: torch.Tensor, cand_coord: torch.Tensor, alpha: float = ALPHA,
                   amplitude: float = AMPLITUDE, n: int = 40) -> float:
    """Single-pair form with the reference's signature (shape_similarity.py:468-492)."""
    cand = cand_coord.to(torch.float32).unsqueeze(0)
    scores, _, _ = shape_tanimoto_batch(ref_coord, cand, torch.tensor([cand.shape[1]]), n=n, alpha=alpha,
                                        amplitude=amplitude)
    return float(scores[0, 0])


# ----------------------------------------------------------------------------- principal shape frames
def _grow_cliques(adj: torch.Tensor, n_terms: int) -> Dict[int, torch.Tensor]:
    """All mutually-neighbouring index subsets i1 < ... < ik (k = 2..n_terms) of every molecule of the batch,
    as tensors [C_k, 1 + k] of (molecule, i1..ik) rows in lexicographic order (the reference enumerates them
    one molecule at a time with a Python backtracking search, shape_similarity.py:269-311)."""
    B, N, _ = adj.shape
    ar = torch.arange(N, device=adj.device)
    upper = adj & (ar.view(1, 1, N) > ar.view(1, N, 1))
    cur = torch.nonzero(upper)                                   # [C2, 3] = (b, i, j), i < j
    out = {2: cur}
    for k in range(3, n_terms + 1):
        if cur.shape[0] == 0:
            out[k] = cur.new_zeros((0, k + 1))
            continue
        nxt = []
        for lo in range(0, cur.shape[0], 1 << 18):              # bounded [chunk, N] candidate masks
            c = cur[lo: lo + (1 << 18)]
            cand = ar.view(1, N) > c[:, -1:].expand(-1, 1)
            for m in range(1, c.shape[1]):
                cand = cand & adj[c[:, 0], c[:, m]]
            rows, v = torch.nonzero(cand, as_tuple=True)
            nxt.append(torch.cat([c[rows], v.unsqueeze(1)], dim=1))
        cur = torch.cat(nxt, dim=0)
        out[k] = cur
    return out


def _shape_moments(points: torch.Tensor, real: torch.Tensor, cliques: Dict[int, torch.Tensor], alpha: float,
                   amplitude: float):
    """Gaussian-volume moments of every molecule with inclusion-exclusion signs (shape_similarity.py:36-129,
    integrals :337-402): volume [B], first moments [B,3], diagonal [B,3] and off-diagonal (xy, xz, yz) [B,3]
    second moments.  Terms are evaluated in fp32 like the reference; the per-molecule sums run in fp64."""
    B = points.shape[0]
    dev = points.device
    vol = torch.zeros(B, dtype=torch.float64, device=dev)
    first = torch.zeros(B, 3, dtype=torch.float64, device=dev)
    ii = torch.zeros(B, 3, dtype=torch.float64, device=dev)
    ij = torch.zeros(B, 3, dtype=torch.float64, device=dev)

    def add(mol, c, a, amp, sign):
        k = (math.pi / a) ** 1.5
        w = (amp * k).to(torch.float32)
        off = torch.stack([c[:, 0] * c[:, 1], c[:, 0] * c[:, 2], c[:, 1] * c[:, 2]], dim=1)
        vol.index_add_(0, mol, sign * w.double())
        first.index_add_(0, mol, sign * (w.unsqueeze(1) * c).double())
        ii.index_add_(0, mol, sign * (w.unsqueeze(1) * (c ** 2 + 1 / (2 * a))).double())
        ij.index_add_(0, mol, sign * (w.unsqueeze(1) * off).double())

    mol1, at1 = torch.nonzero(real, as_tuple=True)
    add(mol1, points[mol1, at1], alpha, torch.full((mol1.shape[0],), amplitude, device=dev), 1.0)
    for order, idx in cliques.items():
        if idx.shape[0] == 0:
            continue
        centers = points[idx[:, :1], idx[:, 1:]]                                  # [C, order, 3]
        gamma = (centers ** 2).sum(-1).sum(-1) - (centers.sum(1) ** 2).sum(-1) / order     # :223-225
        amp = amplitude ** order * torch.exp(-alpha * gamma)
        add(idx[:, 0], centers.mean(1), order * alpha, amp, float((-1) ** (order - 1)))
    return vol, first, ii, ij


def _moment_tensor(ii: torch.Tensor, ij: torch.Tensor, vol: torch.Tensor) -> torch.Tensor:
    t = torch.stack([torch.stack([ii[:, 0], ij[:, 0], ij[:, 1]], 1), torch.stack([ij[:, 0], ii[:, 1], ij[:, 2]], 1),
                     torch.stack([ij[:, 1], ij[:, 2], ii[:, 2]], 1)], 1)
    return t.to(torch.float32) / vol.to(torch.float32).view(-1, 1, 1)


@torch.no_grad()
def shape_quadrupole_batch(coords: torch.Tensor, n_nodes: torch.Tensor, device=None, amplitude: float = AMPLITUDE,
                           atom_radius: float = ATOM_RADIUS, n_terms: int = 6,
                           neighbour_threshold: float = 2 * AMPLITUDE) -> Tuple[torch.Tensor, torch.Tensor]:
    """`get_shape_quadrupole_for_molecule` (shape_similarity.py:18-202) for a padded batch: principal moments
    [B,3] (descending) and coordinates in the principal shape frame [B,N,3] (zero on padded slots)."""
    dev = _args.resolve_device(device, coords)
    x = coords.to(dev, torch.float32)
    B, N, _ = x.shape
    real = torch.arange(N, device=dev).unsqueeze(0) < n_nodes.to(dev).reshape(B, 1)
    alpha = get_alpha(atom_radius, amplitude)
    d = torch.sqrt(((x.unsqueeze(2) - x.unsqueeze(1)) ** 2).sum(-1))
    adj = (d < neighbour_threshold) & (d > 0) & real.unsqueeze(1) & real.unsqueeze(2)       # :244-260
    cliques = _grow_cliques(adj, n_terms)
    vol, first, _, _ = _shape_moments(x, real, cliques, alpha, amplitude)
    centred = (x - (first / vol.unsqueeze(1)).to(torch.float32).unsqueeze(1)) * real.unsqueeze(2)     # :86-89
    _, _, ii, ij = _shape_moments(centred, real, cliques, alpha, amplitude)
    _, vecs = torch.linalg.eigh(_moment_tensor(ii, ij, vol).cpu())                         # :143-144 (host LAPACK)
    rotated = (centred @ vecs.to(dev)) * real.unsqueeze(2)
    _, _, ii, ij = _shape_moments(rotated, real, cliques, alpha, amplitude)
    main = torch.diagonal(_moment_tensor(ii, ij, vol), dim1=1, dim2=2)                     # :184-199
    moments, order = torch.sort(main, dim=1, descending=True)
    frames = torch.gather(rotated, 2, order.unsqueeze(1).expand(B, N, 3))
    return moments, frames


@torch.no_grad()
def evaluate_shape(reference_coord: torch.Tensor, sample_coords: torch.Tensor, n_nodes: torch.Tensor, device=None
                   ) -> Tuple[torch.Tensor, List[dict]]:
    """Shape half of `evaluate_samples` (cheminformatics/pipeline.py:30-85) for heavy-atom coordinates:
    the reference in its principal frame, and per sample the best of the four orientations with its aligned
    coordinates.  `sample_coords` [B,N,3] padded, `n_nodes` [B].  N above MAX_SCORED_ATOMS is refused with ValueError
    before any device work, as `shape_tanimoto_batch` refuses it: the grid kernel would score a wider sample on its first
    64 atoms."""
    if int(sample_coords.shape[1]) > MAX_SCORED_ATOMS:
        raise ValueError(f"the shape kernels take at most {MAX_SCORED_ATOMS} atoms per molecule, got a padded width of "
                         f"{int(sample_coords.shape[1])}")
    dev = _args.resolve_device(device, sample_coords)
    ref = reference_coord.to(torch.float32)
    ref = ref - ref.mean(0)                                                             # :38-39
    _, ref_pf = shape_quadrupole_batch(ref.unsqueeze(0), torch.tensor([ref.shape[0]]), dev)
    ref_pf = ref_pf[0].cpu()
    x = sample_coords.to(dev, torch.float32)
    B, N, _ = x.shape
    nn = n_nodes.to(dev).reshape(B)
    real = (torch.arange(N, device=dev).unsqueeze(0) < nn.unsqueeze(1)).unsqueeze(2)
    com = (x * real).sum(1, keepdim=True) / nn.view(B, 1, 1).clamp(min=1)             # :66-67
    _, frames = shape_quadrupole_batch((x - com) * real, nn, dev)
    scores, best, which = shape_tanimoto_batch(ref_pf, frames, nn, dev)
    aligned = torch.einsum("bnk,bkj->bnj", frames, _orientations().to(dev)[which])
    aligned_c, best_c, which_c, nn_c = aligned.cpu(), best.cpu(), which.cpu(), nn.cpu()
    results = [{"coords": aligned_c[b, : int(nn_c[b])].clone(), "shape_tanimoto": float(best_c[b]),
                "orientation": int(which_c[b])} for b in range(B)]
    return ref_pf, results


# ----------------------------------------------------------------------------- device scoring path (HIP frames)
MAX_SCORED_ATOMS = 64          # csrc/mcg_shape_frames.hip: one 64-bit neighbour mask per atom


@torch.no_grad()
def shape_frames_hip(coords: torch.Tensor, n_nodes: torch.Tensor, device=None, amplitude: float = AMPLITUDE,
                     atom_radius: float = ATOM_RADIUS, n_terms: int = 6, neighbour_threshold: float = 2 * AMPLITUDE,
                     centre_atoms: bool = False, with_counts: bool = False, xform_out: Optional[torch.Tensor] = None):
    """`shape_quadrupole_batch` through the HIP kernels (`mcg_shape_moments` -> host `eigh` -> `mcg_shape_frames`):
    principal moments [B,3] and frames [B,N,3] on the device, bit-identical for a molecule whatever its batch, row or
    padded width.  `centre_atoms`: subtract the real atoms' mean first (what `evaluate_shape` does to its inputs).
    `with_counts`: also the exact number of cliques of order 2..n_terms per molecule, int64 [B, n_terms-1].
    A molecule whose moment tensor is not finite (non-finite coordinates, no atoms) gets NaN moments and frames; the
    other molecules of the batch are unaffected.  `n_nodes` outside [0, N] is refused with ValueError.
    `xform_out` (float32 [B,12] on the device): also the frame transform (`mcg_shape_frames_tf`): M [3,3] row-major, then
    t [3], with frames = (coords - t) @ M on the real rows."""
    dev = _args.resolve_device(device, coords)
    x = coords.to(dev, torch.float32).contiguous()
    B, N, _ = x.shape
    if N > MAX_SCORED_ATOMS:
        raise ValueError(f"the shape kernels take at most {MAX_SCORED_ATOMS} atoms per molecule, got a padded width of {N}")
    check_n_nodes(n_nodes, B, N)
    moments = torch.empty(B, 3, device=dev)
    frames = torch.empty(B, N, 3, device=dev)
    counts = torch.empty(B, n_terms - 1, dtype=torch.int64, device=dev) if with_counts else None
    if B == 0 or N == 0:
        frames.zero_()
        return (moments, frames, counts) if with_counts else (moments, frames)
    nn = n_nodes.to(dev, torch.int32).reshape(B).contiguous()
    alpha = get_alpha(atom_radius, amplitude)
    centre = torch.empty(B, 3, device=dev)
    tensor = torch.empty(B, 9, device=dev)
    volume = torch.empty(B, dtype=torch.float64, device=dev)
    L, stream = _lib.lib(), _lib.current_stream_ptr(dev)
    _lib.check(L.mcg_shape_moments(_lib.dptr(x), _lib.dptr(nn), B, N, alpha, float(amplitude), float(neighbour_threshold),
                                   int(n_terms), int(bool(centre_atoms)), _lib.dptr(centre), _lib.dptr(tensor),
                                   _lib.dptr(volume), _lib.dptr(counts), stream), "mcg_shape_moments")
    t = tensor.reshape(B, 3, 3).cpu()
    bad = ~torch.isfinite(t).all(dim=2).all(dim=1)           # LAPACK refuses the whole batch for one NaN matrix
    if bool(bad.any()):
        t[bad] = torch.eye(3)          # placeholder: such a molecule's centre and volume are NaN, so are its frames
    _, vecs = torch.linalg.eigh(t)                                       # the reference's host LAPACK path (:143-144)
    vecs = vecs.contiguous().to(dev)
    args = (_lib.dptr(x), _lib.dptr(nn), B, N, _lib.dptr(centre), _lib.dptr(vecs), _lib.dptr(volume), alpha,
            float(amplitude), float(neighbour_threshold), int(n_terms), int(bool(centre_atoms)), _lib.dptr(moments),
            _lib.dptr(frames))
    if xform_out is None:
        _lib.check(L.mcg_shape_frames(*args, stream), "mcg_shape_frames")
    else:
        _lib.check(L.mcg_shape_frames_tf(*args, _lib.dptr(xform_out), stream), "mcg_shape_frames_tf")
    return (moments, frames, counts) if with_counts else (moments, frames)


def check_reference_atoms(n_ref: int) -> None:
    if n_ref < 3 or n_ref > MAX_SCORED_ATOMS:
        raise ValueError(f"shape scoring needs a reference of 3 to {MAX_SCORED_ATOMS} heavy atoms, got {n_ref}")


class ConformerReference:
    """A reference conformer of the shape kernels: `coords` [n_ref,3] fp32, its heavy atoms, on the host.  It rides as row 0
    of the samples' `shape_frames_hip` launch, which gives its frame, transform and grid axes anew on every call."""
    refinable = True
    pose_keys = ()                # what its pose adds to `shape_overlay`'s keys: (key, per-row shape, dtype)

    def __init__(self, coords):
        self.coords = torch.as_tensor(coords, dtype=torch.float32).cpu()
        check_reference_atoms(int(self.coords.shape[0]))

    def rows(self, x: torch.Tensor, nn: torch.Tensor, dev):
        """The rows of the frames launch: the reference as row 0 of [B+1, max(W, n_ref), 3], then the samples."""
        B, W = x.shape[:2]
        n_ref = int(self.coords.shape[0])
        out = torch.zeros(B + 1, max(W, n_ref), 3, device=dev)
        out[0, :n_ref] = self.coords.to(dev)
        out[1:, :W] = x
        return out, torch.cat([torch.tensor([n_ref], dtype=torch.int32, device=dev), nn])

    def score_frames(self, frames: torch.Tensor, nn: torch.Tensor, dev):
        """(best [B], orientation [B]) of the samples' frames against the reference's (`mcg_shape_tanimoto`)."""
        return shape_tanimoto_batch(frames[0, : self.coords.shape[0]], frames[1:], nn[1:], dev)[1:]

    def launch_overlay(self, frames: torch.Tensor, xform: torch.Tensor, nn: torch.Tensor, rots: torch.Tensor, outputs: list,
                       refine: list, dev) -> None:
        """The pose launch over the rows of `rows`: `mcg_shape_overlay`, or `mcg_shape_overlay_refined` with its further
        arguments `refine`; `outputs`: the pointers score, best, which, flipped, pose, posed of `_overlay`."""
        n_ref = int(self.coords.shape[0])
        B, N = int(frames.shape[0]) - 1, int(frames.shape[1])
        ref_frame = frames[0, :n_ref].contiguous()
        axes = _grid_axes(ref_frame.cpu(), 40).to(dev).contiguous()
        f = torch.empty(40 ** 3, device=dev)
        entry = "mcg_shape_overlay_refined" if refine else "mcg_shape_overlay"
        _lib.check(getattr(_lib.lib(), entry)(
            _lib.dptr(ref_frame), n_ref, _lib.dptr(xform), _lib.dptr(frames[1:]), _lib.dptr(xform[1:]), _lib.dptr(nn[1:]),
            B, N, _lib.dptr(rots), _lib.dptr(axes), 40, float(ALPHA), float(AMPLITUDE), _lib.dptr(f), *outputs, *refine,
            _lib.current_stream_ptr(dev)), entry)

    def pose_extras(self, out: Dict[str, torch.Tensor], nn: torch.Tensor, dev) -> Dict[str, torch.Tensor]:
        return {}

    def grid(self, dev):
        """(frame transform [12], grid axes [3,n]) of the pair matrix: one frames launch over the reference alone."""
        xform = torch.empty(1, 12, device=dev)
        _, frames = shape_frames_hip(self.coords.to(dev).unsqueeze(0),
                                     torch.tensor([self.coords.shape[0]], dtype=torch.int32, device=dev), dev,
                                     centre_atoms=True, xform_out=xform)
        return xform, _grid_axes(frames[0].cpu(), 40).to(dev).contiguous()


def _reference(reference):
    """`reference` as a reference object: a `ConformerReference`, a `SolidReference`, or a conformer's raw coordinates."""
    if isinstance(reference, (ConformerReference, SolidReference)):
        return reference
    return ConformerReference(reference)


def _shape_inputs(reference, coords: torch.Tensor, n_nodes: torch.Tensor, device, max_batch: Optional[int] = None):
    """The common preamble of `shape_scores`, `shape_overlay` and `pairwise_shape_tanimoto`: (reference object, device,
    samples x [B,W,3] fp32 and counts nn [B] int32 on the device), with x = nn = None for an empty batch.  `reference`: a
    `ConformerReference`, a `SolidReference` or a conformer's raw coordinates.  Refuses, before any device work: a
    conformer outside 3..MAX_SCORED_ATOMS heavy atoms, more than `max_batch` molecules and, for a batch that is not empty,
    atom counts outside [0, W] and a padded width W above MAX_SCORED_ATOMS."""
    reference = _reference(reference)
    dev = _args.resolve_device(device, coords)
    B = int(coords.shape[0])
    if max_batch is not None and B > max_batch:
        raise ValueError(f"pairwise shape Tanimoto takes at most {max_batch} molecules, got {B}")
    if B == 0:
        return reference, dev, None, None
    W = int(coords.shape[1])
    check_n_nodes(n_nodes, B, W)         # before a conformer widens the batch
    if W > MAX_SCORED_ATOMS:
        raise ValueError(f"shape scoring takes at most {MAX_SCORED_ATOMS} atoms per molecule, got a padded width of {W}")
    return reference, dev, coords.to(dev, torch.float32).contiguous(), n_nodes.to(dev, torch.int32).reshape(B).contiguous()


@torch.no_grad()
def shape_scores(reference_coord, coords: torch.Tensor, n_nodes: torch.Tensor, device=None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(best [B], orientation [B]) on the device: the shape Tanimoto `evaluate_shape` reports for every sample
    (`evaluate_samples`, cheminformatics/pipeline.py:30-85), with the principal frames of the reference and of the samples
    from the HIP kernels (`shape_frames_hip`, reference = row 0 of the same launch) and the four-orientation search of
    `mcg_shape_tanimoto`.  A sample's score depends on its own coordinates and the reference only.
    `reference_coord`: the conformer's coordinates or a `ConformerReference`; a `SolidReference`: `shape_scores_solid`."""
    ref, dev, x, nn = _shape_inputs(reference_coord, coords, n_nodes, device)
    if x is None:
        return torch.empty(0, device=dev), torch.empty(0, dtype=torch.long, device=dev)
    x, nn = ref.rows(x, nn, dev)
    _, frames = shape_frames_hip(x, nn, dev, centre_atoms=True)
    return ref.score_frames(frames, nn, dev)


@torch.no_grad()
def shape_tanimoto_placed(reference_coord, coords: torch.Tensor, n_nodes: torch.Tensor, device=None) -> torch.Tensor:
    """[B] on the device: the shape Tanimoto of every molecule AS PLACED - no frame of its own, no orientation search -
    against the reference conformer, for molecules in the reference's own coordinates (what `shape_overlay` returns, or a
    pose moved on from there).  Scored on the grid `shape_overlay` scores on: reference and molecules are taken into the
    reference's principal frame by `ConformerReference.grid`'s transform, y = (x - t_r) @ M_r, and `mcg_shape_tanimoto`
    scores them in the identity orientation.  Against a `SolidReference` (a pose into a `pocket.Pocket`'s mesh, moved on by
    the receptor stages): the same, into the solid's frame and against its occupancy (`mcg_shape_tanimoto_field`).  Refuses
    what `shape_scores` refuses."""
    ref, dev, x, nn = _shape_inputs(reference_coord, coords, n_nodes, device)
    if x is None:
        return torch.empty(0, device=dev)
    B, W = int(x.shape[0]), int(x.shape[1])
    xform, axes = ref.grid(dev)
    xform = xform.reshape(-1, 12)
    M, t = xform[0, :9].reshape(3, 3), xform[0, 9:]

    def into_frame(p):                        # written out: a product and a fixed sum per element, no library GEMM
        d = p - t
        return (d[..., 0:1] * M[0] + d[..., 1:2] * M[1]) + d[..., 2:3] * M[2]
    real = (torch.arange(W, device=dev).view(1, W) < nn.view(B, 1)).unsqueeze(-1)
    y = torch.where(real, into_frame(x), torch.zeros((), device=dev)).contiguous()
    n = int(axes.shape[1])
    eye = torch.eye(3, device=dev).reshape(1, 9).contiguous()
    score = torch.empty(B, device=dev)
    if isinstance(ref, SolidReference):
        _lib.check(_lib.lib().mcg_shape_tanimoto_field(_lib.dptr(ref.on(dev)["f"]), _lib.dptr(y), _lib.dptr(nn), B, W,
                                                       _lib.dptr(eye), 1, _lib.dptr(axes), n, float(ALPHA), float(AMPLITUDE),
                                                       _lib.dptr(score), _lib.current_stream_ptr(dev)),
                   "mcg_shape_tanimoto_field")
        return score
    ref_frame = into_frame(ref.coords.to(dev)).contiguous()
    f = torch.empty(n ** 3, device=dev)
    _lib.check(_lib.lib().mcg_shape_tanimoto(_lib.dptr(ref_frame), int(ref_frame.shape[0]), _lib.dptr(y), _lib.dptr(nn), B,
                                             W, _lib.dptr(eye), 1, _lib.dptr(axes), n, float(ALPHA), float(AMPLITUDE),
                                             _lib.dptr(f), _lib.dptr(score), _lib.current_stream_ptr(dev)),
               "mcg_shape_tanimoto")
    return score


MAX_REFINE_STEPS = 1024       # csrc/mcg_shape_refine.hip RF_MAX_STEPS


def check_refine_steps(value, name: str = "refine_steps", lowest: int = 0, if_true: Optional[int] = None) -> int:
    """An ascent step budget as an int in `lowest`..MAX_REFINE_STEPS (an integer type, not a bool), else a ValueError that
    names `name`.  `if_true`: the budget True stands for, where the option accepts True (`refine_overlay`: 64, with
    `lowest` 1); the default is the rule of `shape_overlay(refine_steps=...)`."""
    return _args.check_steps(name, value, lowest, MAX_REFINE_STEPS, if_true)


@torch.no_grad()
def shape_overlay(reference_coord: torch.Tensor, coords: torch.Tensor, n_nodes: torch.Tensor, device=None,
                  with_scores: bool = False, refine_steps: int = 0) -> Dict[str, torch.Tensor]:
    """Every sample posed onto the reference, in the reference's own coordinates.  `reference_coord`:
    a conformer's coordinates or a `ConformerReference`, described here; a `SolidReference`: `shape_overlay_solid`.
    The principal frames of the reference (row 0) and of the samples come from one `mcg_shape_frames_tf` launch; the
    sample frame's handedness is made to match the reference's (so the pose is a rotation, never a mirror), the four
    orientations of `evaluate_samples` are scored on the reference's grid and the best becomes a rigid pose, all in one
    `mcg_shape_overlay` launch.  Returns device tensors:
      coords [B,N,3]       posed: coords @ rotation + translation on the real rows (zero on padded rows);
      rotation [B,3,3]     proper (det +1), applied to row vectors;  translation [B,3];
      tanimoto [B]         the shape Tanimoto of the pose as placed;
      orientation [B]      which of the four orientations won (-1: failed row);
      flipped [B] bool     whether the frame's smallest-moment axis was flipped to match the reference's handedness;
      (with_scores) scores [B,4]  the four orientations' scores.
    A sample whose frame is not finite (non-finite coordinates, no atoms) keeps its input coordinates and gets a NaN
    rotation, translation and tanimoto and orientation -1; the other samples are unaffected and bit-identical whatever
    their batch.  Refuses what `shape_scores` refuses.
    `refine_steps` >= 1 (`mcg_shape_overlay_refined`, DESIGN.md section 6 "Refined pose"): each of the four starts is
    then moved as a rigid body to maximise its Gaussian overlap with the reference for that many ascent steps, and the
    best refined candidate replaces the start pose where its grid Tanimoto is strictly better; the keys above describe
    the returned pose, and
      start_tanimoto [B]   the unrefined pose's tanimoto (what refine_steps=0 returns, bit for bit);
      refined [B] bool     whether the refined pose replaced it;
      (with_scores) refined_scores [B,4]  the refined candidates' scores; objective [B,4,2]  the Gaussian overlap of
                           each start before and after its ascent.
    0 (the default) is the unrefined path, unchanged.  A value outside 0..1024, a bool or a non-integer is refused with
    ValueError before any device work, and so is refining the pose into a solid."""
    steps = check_refine_steps(refine_steps)
    return _overlay(reference_coord, coords, n_nodes, device, with_scores, steps, steps > 0)


def _overlay(reference, coords, n_nodes, device, with_scores: bool, steps: int, refined_entry: bool):
    """`shape_overlay` through the reference's C entry: `mcg_shape_overlay`, (`refined_entry`) `mcg_shape_overlay_refined`
    with `steps`, or a solid's `mcg_shape_overlay_field`."""
    ref = _reference(reference)
    if refined_entry and not ref.refinable:
        raise ValueError("a pose into a solid cannot be refined: the ascent's objective is the overlap with the "
                         "reference's atoms, and a mesh has none")
    ref, dev, x, nn = _shape_inputs(ref, coords, n_nodes, device)
    B, W = int(coords.shape[0]), int(coords.shape[1])
    f32 = torch.float32
    keys = (("coords", (W, 3), f32, True), ("rotation", (3, 3), f32, True), ("translation", (3,), f32, True),
            ("tanimoto", (), f32, True), ("orientation", (), torch.long, True), ("flipped", (), torch.bool, True),
            ("scores", (4,), f32, with_scores), ("start_tanimoto", (), f32, refined_entry),
            ("refined", (), torch.bool, refined_entry), ("refined_scores", (4,), f32, refined_entry and with_scores),
            ("objective", (4, 2), f32, refined_entry and with_scores)
            ) + tuple(k + (True,) for k in ref.pose_keys)                       # (key, per-row shape, dtype, returned)
    if x is None:
        return {k: torch.zeros(0, *shape, dtype=dtype, device=dev) for k, shape, dtype, on in keys if on}
    x, nn = ref.rows(x, nn, dev)
    first, N = int(x.shape[0]) - B, int(x.shape[1])                             # the samples' first row of the launch
    xform = torch.empty(B + first, 12, device=dev)
    _, frames = shape_frames_hip(x, nn, dev, centre_atoms=True, xform_out=xform)
    rots = _orientations().reshape(4, 9).to(dev).contiguous()
    scores = torch.empty(B, 4, device=dev) if with_scores else None
    best = torch.empty(B, device=dev)
    which = torch.empty(B, dtype=torch.int32, device=dev)
    flipped = torch.empty(B, dtype=torch.int32, device=dev)
    pose = torch.empty(B, 12, device=dev)
    posed = torch.empty(B, N, 3, device=dev)
    out = dict(scores=scores)
    refine = []
    if refined_entry:
        ws = torch.empty(B, 4, 12, device=dev)
        out.update(objective=torch.empty(B, 4, 2, device=dev) if with_scores else None,
                   refined_scores=torch.empty(B, 4, device=dev) if with_scores else None,
                   start_tanimoto=torch.empty(B, device=dev), refined=torch.empty(B, dtype=torch.int32, device=dev))
        refine = [int(steps), _lib.dptr(ws), _lib.dptr(out["objective"]), _lib.dptr(out["start_tanimoto"]),
                  _lib.dptr(out["refined"]), _lib.dptr(out["refined_scores"])]
    outputs = [_lib.dptr(t) for t in (scores, best, which, flipped, pose, posed)]
    ref.launch_overlay(frames, xform, nn, rots, outputs, refine, dev)
    if refined_entry:
        out["refined"] = out["refined"].bool()
    failed = (which < 0).view(B, 1, 1)
    out.update(coords=torch.where(failed, x[first:, :W], posed[:, :W]), rotation=pose[:, :9].reshape(B, 3, 3),
               translation=pose[:, 9:], tanimoto=best, orientation=which.long(), flipped=flipped.bool())
    out.update(ref.pose_extras(out, nn, dev))
    return {k: out[k] for k, _, _, on in keys if on}


def pose_mols(reference_coord: torch.Tensor, mols: List, device=None, overlay_fn=None) -> List:
    """Pose finished Mols onto the reference in ONE batched `shape_overlay` call: the pose comes from each Mol's heavy-atom
    conformer positions (`mol_heavy_coords`) and is applied to EVERY conformer position, hydrogens included; each Mol
    gets the double property `overlay_tanimoto`.  Works on anything with `GetConformer()` whose conformer has
    `GetPositions()` and `SetAtomPosition(i, point)`.  Returns per Mol (overlay_tanimoto, rotation [3,3],
    translation [3]) on the host, or None for a dropped Mol (None in `mols`); a Mol whose pose failed is left where it
    was, with a NaN score and a None pose: (nan, None, None).  `overlay_fn(reference, coords, n_nodes)`: what poses the
    padded coordinates (default: `shape_overlay` on `device`)."""
    live = [k for k, m in enumerate(mols) if m is not None]
    out: List = [None] * len(mols)
    if not live:
        return out
    coords, n = padded_coords([mol_heavy_coords(mols[k]) for k in live])
    res = overlay_fn(reference_coord, coords, n) if overlay_fn is not None else \
        shape_overlay(reference_coord, coords, n, device)
    rot, trans, tan, which = (res["rotation"].cpu().double(), res["translation"].cpu().double(), res["tanimoto"].cpu(),
                              res["orientation"].cpu())
    for j, k in enumerate(live):
        score = float(tan[j])
        if int(which[j]) < 0:
            out[k] = (score, None, None)
        else:
            apply_pose(mols[k], rot[j], trans[j])
            out[k] = (score, rot[j].float(), trans[j].float())
        if hasattr(mols[k], "SetDoubleProp"):
            mols[k].SetDoubleProp("overlay_tanimoto", score)
    return out


def apply_pose(mol, rotation: torch.Tensor, translation: torch.Tensor) -> None:
    """Move every conformer position p of `mol` to p @ rotation + translation (in fp64)."""
    import numpy as np
    conf = mol.GetConformer()
    pos = np.asarray(conf.GetPositions(), dtype=np.float64).reshape(-1, 3)
    new = pos @ rotation.double().numpy() + translation.double().numpy()
    try:
        from rdkit.Geometry import Point3D
    except ImportError:          # a stand-in Mol: any 3-sequence
        Point3D = None
    for i, p in enumerate(new.tolist()):
        conf.SetAtomPosition(i, Point3D(*p) if Point3D is not None else tuple(p))


MAX_PAIR_BATCH = 16384        # include/mlconfgen_hip.h MCG_SHAPE_PAIR_MAX_B: F [B, 64 000] and T [B, B] stay addressable
_PAIR_KALIGN = 128            # MCG_SHAPE_PAIR_KALIGN: the density rows are padded to this many grid points


@torch.no_grad()
def pairwise_shape_tanimoto(reference_coord: torch.Tensor, coords: torch.Tensor, n_nodes: torch.Tensor,
                            device=None) -> torch.Tensor:
    """[B,B] fp32 on the device: the Gaussian-volume shape Tanimoto of every pair of molecules AS PLACED (no orientation
    search), for molecules that share the reference conformer's own coordinates (what `shape_overlay` returns).  Both
    molecules are evaluated on the grid `shape_overlay` scores on: the reference's principal frame (`shape_frames_hip`,
    `xform_out=`), `_grid_axes(ref_frame, 40)`, each molecule mapped into that frame by y = (x - t_r) @ M_r; atoms off
    the grid are cut off ("shape diversity").  One `mcg_shape_pair_tanimoto` call: the densities,
    their Gram matrix on the exact-fp32 matrix cores, and T_ij = G_ij / (G_ii + G_jj - G_ij).
    The matrix is exactly symmetric, its diagonal exactly 1 where a molecule's density is finite and not zero, and entry
    (i, j) has the same bits whatever the batch, row order or padded width.  A molecule with no atoms or a non-finite
    coordinate gets a NaN row and column; the other entries are unaffected.  Refuses, before any device work, what
    `shape_scores` refuses and more than `MAX_PAIR_BATCH` molecules.
    `reference_coord`: a conformer's coordinates or a `ConformerReference`; a `SolidReference`:
    `pairwise_shape_tanimoto_solid`."""
    ref, dev, x, nn = _shape_inputs(reference_coord, coords, n_nodes, device, max_batch=MAX_PAIR_BATCH)
    if x is None:
        return torch.zeros(0, 0, device=dev)
    B, W = x.shape[0], x.shape[1]
    xform, axes = ref.grid(dev)
    n = int(axes.shape[1])
    gp = -(-n ** 3 // _PAIR_KALIGN) * _PAIR_KALIGN
    density = torch.empty(B, gp, device=dev)
    gram = torch.empty(B, B, device=dev)
    out = torch.empty(B, B, device=dev)
    _lib.check(_lib.lib().mcg_shape_pair_tanimoto(_lib.dptr(x), _lib.dptr(nn), B, W, _lib.dptr(xform), _lib.dptr(axes), n,
                                                  float(ALPHA), float(AMPLITUDE), _lib.dptr(density), _lib.dptr(gram),
                                                  _lib.dptr(out), _lib.current_stream_ptr(dev)),
               "mcg_shape_pair_tanimoto")
    return out


# ----------------------------------------------------------------------------- solid references (watertight meshes)
MAX_MESH_POINTS = 1 << 24     # include/mlconfgen_hip.h MCG_MESH_MAX_POINTS


def _winding_ws(F: int, P: int, dev) -> Optional[torch.Tensor]:
    """The partial-sum work space of a winding launch over F triangles and P points (None: one part, none needed)."""
    S = int(_lib.lib().mcg_mesh_splits(int(F)))
    if S < 1:
        raise ValueError(f"a mesh of {F} faces is outside what the winding kernel takes")
    return torch.empty(S * P, device=dev) if S > 1 else None


def _triangles(triangles, dev) -> torch.Tensor:
    tri = torch.as_tensor(triangles, dtype=torch.float32).reshape(-1, 9).to(dev).contiguous()
    if tri.shape[0] < 1:
        raise ValueError("no triangles")
    return tri


@torch.no_grad()
def mesh_winding(triangles, points: Optional[torch.Tensor] = None, axes: Optional[torch.Tensor] = None, device=None
                 ) -> torch.Tensor:
    """Generalized winding number (`mcg_mesh_winding`, fp32, on the device) of `triangles` [F,3,3] (or [F,9]: corners a, b,
    c per face, outward) at `points` [P,3], or - `axes` [3,n] - at the n^3 grid points in meshgrid(indexing="ij") flatten
    order: +-1 inside a closed mesh, 0 outside; an open mesh is legal.  A point's value has the same bits whatever P, its
    position and the mode; a non-finite point gets NaN; exactly on the surface the value is unspecified."""
    if (points is None) == (axes is None):
        raise ValueError("pass either points or axes")
    src = points if points is not None else axes
    dev = _args.resolve_device(device, src)
    tri = _triangles(triangles, dev)
    F = int(tri.shape[0])
    if points is not None:
        pts = points.to(dev, torch.float32).reshape(-1, 3).contiguous()
        P = int(pts.shape[0])
        out = torch.empty(P, device=dev)
        if P == 0:
            return out
        args = (_lib.dptr(pts), P, None, 0)
    else:
        ax = axes.to(dev, torch.float32).contiguous()
        n = int(ax.shape[1])
        P = n ** 3
        out = torch.empty(P, device=dev)
        args = (None, 0, _lib.dptr(ax), n)
    ws = _winding_ws(F, P, dev)
    _lib.check(_lib.lib().mcg_mesh_winding(_lib.dptr(tri), F, *args, _lib.dptr(out), _lib.dptr(ws),
                                           _lib.current_stream_ptr(dev)), "mcg_mesh_winding")
    return out


@torch.no_grad()
def mesh_occupancy(triangles, axes: torch.Tensor, device=None) -> torch.Tensor:
    """f [n^3] fp32 on the device: 1 where |winding number| > 0.5 at the grid points of `axes` [3,n], else 0
    (`mcg_mesh_occupancy`): the density of the solid the mesh bounds, on the grid the shape kernels score on."""
    dev = _args.resolve_device(device, axes)
    tri = _triangles(triangles, dev)
    ax = axes.to(dev, torch.float32).contiguous()
    n = int(ax.shape[1])
    f = torch.empty(n ** 3, device=dev)
    ws = _winding_ws(int(tri.shape[0]), n ** 3, dev)
    _lib.check(_lib.lib().mcg_mesh_occupancy(_lib.dptr(tri), int(tri.shape[0]), _lib.dptr(ax), n, _lib.dptr(f),
                                             _lib.dptr(ws), _lib.current_stream_ptr(dev)), "mcg_mesh_occupancy")
    return f


@torch.no_grad()
def mesh_atoms_outside(triangles, coords: torch.Tensor, n_nodes: torch.Tensor, device=None, with_winding: bool = False):
    """outside [B] int32 on the device: how many real atoms of each row of `coords` [B,N,3] have |winding number| <= 0.5
    with respect to `triangles` (`mcg_mesh_atoms_outside`); -1 for a row with a non-finite real coordinate.
    `with_winding`: also the atoms' winding numbers [B,N] (0 on padded atoms)."""
    dev = _args.resolve_device(device, coords)
    B, N = int(coords.shape[0]), int(coords.shape[1])
    outside = torch.zeros(B, dtype=torch.int32, device=dev)
    w = torch.zeros(B, N, device=dev) if with_winding else None
    if B and N:
        if N > MAX_SCORED_ATOMS:
            raise ValueError(f"the shape kernels take at most {MAX_SCORED_ATOMS} atoms per molecule, got a padded width of {N}")
        check_n_nodes(n_nodes, B, N)
        tri = _triangles(triangles, dev)
        x = coords.to(dev, torch.float32).contiguous()
        nn = n_nodes.to(dev, torch.int32).reshape(B).contiguous()
        _lib.check(_lib.lib().mcg_mesh_atoms_outside(_lib.dptr(tri), int(tri.shape[0]), _lib.dptr(x), _lib.dptr(nn), B, N,
                                                     _lib.dptr(outside), _lib.dptr(w), _lib.current_stream_ptr(dev)),
                   "mcg_mesh_atoms_outside")
    return (outside, w) if with_winding else outside


class SolidReference:
    """A watertight mesh prepared as the reference of the shape kernels (`solid_reference`).  Host side, built at once:
      mesh            the loaded `mesh.Mesh` (own coordinates);
      M_r, t_r        `mesh.solid_frame`: frame = (x - t_r) @ M_r, M_r proper;  xform [12] fp32 = M_r row-major, then t_r
                      (the layout of `mcg_shape_frames_tf`);
      triangles       [F,9] fp32, in the solid's frame;  triangles_own [F,9] fp32, in the mesh's own coordinates;
      axes            [3,n] fp32: linspace(bbox_min - 6 ATOM_RADIUS, bbox_max + 6 ATOM_RADIUS, n) per axis of the framed solid.
    Device side, built on first use and kept per device (`on(device)`): the tensors above and the occupancy f [n^3]."""

    def __init__(self, mesh, n: int = 40):
        import numpy as np
        from . import mesh as mcg_mesh
        self.mesh = mcg_mesh.load_mesh(mesh)
        self.n = int(n)
        if not 2 <= self.n <= 256:
            raise ValueError(f"the grid takes 2 to 256 points per axis, got {n}")
        self.M_r, self.t_r = mcg_mesh.solid_frame(self.mesh)
        v = self.mesh.vertices.astype(np.float64)
        framed = (v - self.t_r) @ self.M_r
        self.triangles = torch.from_numpy(framed[self.mesh.faces].reshape(-1, 9)).to(torch.float32)
        self.triangles_own = torch.from_numpy(self.mesh.vertices[self.mesh.faces].reshape(-1, 9).copy())
        self.xform = torch.from_numpy(np.concatenate([self.M_r.reshape(-1), self.t_r])).to(torch.float32)
        fv = torch.from_numpy(framed).to(torch.float32)
        lo, hi = fv.min(dim=0).values - 6.0 * ATOM_RADIUS, fv.max(dim=0).values + 6.0 * ATOM_RADIUS
        self.axes = torch.stack([torch.linspace(lo[k], hi[k], self.n) for k in range(3)])
        self._on = {}

    def on(self, device) -> Dict[str, torch.Tensor]:
        """{triangles, triangles_own, xform, axes, f} on `device`; the occupancy launch runs the first time."""
        dev = torch.device(device)
        if dev not in self._on:
            d = dict(triangles=self.triangles.to(dev), triangles_own=self.triangles_own.to(dev),
                     xform=self.xform.to(dev).contiguous(), axes=self.axes.to(dev).contiguous())
            d["f"] = mesh_occupancy(d["triangles"], d["axes"], dev)
            self._on[dev] = d
        return self._on[dev]

    # what the shape bodies ask of a reference (`ConformerReference` has the same five)
    refinable = False
    pose_keys = (("atoms_outside", (), torch.int32),)

    def rows(self, x: torch.Tensor, nn: torch.Tensor, dev):
        """The rows of the frames launch: the samples as they are (the solid's device side is built in front of it)."""
        self.on(dev)
        return x, nn

    def score_frames(self, frames: torch.Tensor, nn: torch.Tensor, dev):
        """(best [B], orientation [B]) of the samples' frames against the occupancy (`mcg_shape_tanimoto_field`)."""
        d = self.on(dev)
        B, N = frames.shape[:2]
        rots = _orientations().reshape(4, 9).to(dev).contiguous()
        score = torch.empty(B * 4, device=dev)
        _lib.check(_lib.lib().mcg_shape_tanimoto_field(_lib.dptr(d["f"]), _lib.dptr(frames), _lib.dptr(nn), B, N,
                                                       _lib.dptr(rots), 4, _lib.dptr(d["axes"]), self.n, float(ALPHA),
                                                       float(AMPLITUDE), _lib.dptr(score), _lib.current_stream_ptr(dev)),
                   "mcg_shape_tanimoto_field")
        return tuple(score.reshape(B, 4).max(dim=1))

    def launch_overlay(self, frames: torch.Tensor, xform: torch.Tensor, nn: torch.Tensor, rots: torch.Tensor, outputs: list,
                       refine: list, dev) -> None:
        """The pose launch over the rows of `rows`: `mcg_shape_overlay_field` (`refine` is empty: `refinable`); `outputs`:
        the pointers score, best, which, flipped, pose, posed of `_overlay`."""
        d = self.on(dev)
        B, N = int(frames.shape[0]), int(frames.shape[1])
        _lib.check(_lib.lib().mcg_shape_overlay_field(
            _lib.dptr(d["f"]), _lib.dptr(d["xform"]), _lib.dptr(frames), _lib.dptr(xform), _lib.dptr(nn), B, N,
            _lib.dptr(rots), _lib.dptr(d["axes"]), self.n, float(ALPHA), float(AMPLITUDE), *outputs,
            _lib.current_stream_ptr(dev)), "mcg_shape_overlay_field")

    def pose_extras(self, out: Dict[str, torch.Tensor], nn: torch.Tensor, dev) -> Dict[str, torch.Tensor]:
        counts = mesh_atoms_outside(self.on(dev)["triangles_own"], out["coords"], nn, dev)
        return dict(atoms_outside=torch.where(out["orientation"] < 0, torch.full_like(counts, -1), counts))

    def grid(self, dev):
        """(frame transform [12], grid axes [3,n]) of the pair matrix: the solid's own."""
        d = self.on(dev)
        return d["xform"], d["axes"]


def solid_reference(mesh, n: int = 40) -> SolidReference:
    """`mesh` (anything `mesh.load_mesh` takes, or a `pocket.Pocket`: its `.mesh`) as a `SolidReference` on an n^3 grid,
    prepared once per call."""
    from . import pocket as mcg_pocket
    if isinstance(mesh, mcg_pocket.Pocket):
        mesh = mesh.mesh
    return mesh if isinstance(mesh, SolidReference) else SolidReference(mesh, n)


def shape_scores_solid(solid, coords: torch.Tensor, n_nodes: torch.Tensor, device=None
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`shape_scores` against a solid: (best [B], orientation [B]) on the device.  Every sample's principal frame
    (`shape_frames_hip`, as `shape_scores` takes it) is scored in the four orientations against the solid's occupancy on
    the solid's grid (`mcg_shape_tanimoto_field`): <f,g> / (<f,f> + <g,g> - <f,g>) with f the indicator function of the
    solid and g the sample's Gaussian density.  The indicator function as the density of a solid is this package's own
    choice, not the reference's (which scores molecules against molecules)."""
    return shape_scores(solid_reference(solid), coords, n_nodes, device)


def shape_overlay_solid(solid, coords: torch.Tensor, n_nodes: torch.Tensor, device=None, with_scores: bool = False
                        ) -> Dict[str, torch.Tensor]:
    """`shape_overlay` onto a solid: every sample posed into the mesh's own coordinates by a proper rigid transform - its
    principal frame, made to match the handedness of the solid's frame (`mesh.solid_frame`, proper), in the best of the
    four orientations scored against the solid's occupancy (`mcg_shape_overlay_field`).  `shape_overlay`'s keys with the
    same meaning and failure rows, plus
      atoms_outside [B] int32   the real atoms of the pose with |winding number| <= 0.5 (`mcg_mesh_atoms_outside`, against
                                the mesh in its own coordinates); -1 where the pose failed."""
    return shape_overlay(solid_reference(solid), coords, n_nodes, device, with_scores)


def pairwise_shape_tanimoto_solid(solid, coords: torch.Tensor, n_nodes: torch.Tensor, device=None) -> torch.Tensor:
    """`pairwise_shape_tanimoto` of molecules posed into a solid's coordinates (`shape_overlay_solid`): one
    `mcg_shape_pair_tanimoto` call with the solid's frame transform and grid in place of a reference conformer's."""
    return pairwise_shape_tanimoto(solid_reference(solid), coords, n_nodes, device)


# the options' own names for the shared rules of `_args`: each takes the value and returns it as an int / a float
check_max_atoms_outside = functools.partial(_args.check_at_least, "max_atoms_outside", lowest=0)
check_max_pairwise_tanimoto = functools.partial(_args.check_real, "max_pairwise_tanimoto", low=0.0, high=1.0, open_low=True)
check_top_k = functools.partial(_args.check_at_least, "top_k", lowest=1)


def check_min_shape_tanimoto(value) -> float:
    """`min_shape_tanimoto` as a float in [0, 1] (not NaN), else ValueError."""
    if not (0.0 <= float(value) <= 1.0):
        raise ValueError(f"min_shape_tanimoto must lie in [0, 1], got {value!r}")
    return float(value)


def ranking_key(score: Optional[float], sample_id: int):
    """The sort key of the ranking order: descending score, ties to the lower sample id, a NaN score last; a score of
    None (a call that does not score shape) ranks like every other None, which leaves the sample-id order."""
    return (0.0 if score is None else -score if score == score else math.inf, sample_id)


def select_diverse(scores: List[float], sample_ids: List[int], pair, max_pairwise_tanimoto: Optional[float],
                   top_k: Optional[int] = None, min_shape_tanimoto: Optional[float] = None, chemical_pair=None,
                   max_pairwise_chemical_tanimoto: Optional[float] = None) -> List[int]:
    """Positions of the molecules to keep, by sphere exclusion in ranking order: the molecules scoring >=
    `min_shape_tanimoto`, walked in descending score order (ties: the lower sample id; a NaN score ranks last and passes
    no threshold); a molecule is kept unless its `pair` Tanimoto with an already kept molecule is >=
    `max_pairwise_tanimoto` (a NaN pair entry excludes nothing); then the first `top_k`.  `pair[i][j]`: the [B,B] pair
    matrix over the same positions as `scores` (`pairwise_shape_tanimoto`; any array-like), not read when
    `max_pairwise_tanimoto` is None, which gives the plain ranking selection (`select_scored`).
    `chemical_pair` / `max_pairwise_chemical_tanimoto`: a second pair matrix (`fingerprint.pairwise_fingerprint_tanimoto`)
    and threshold in the same walk; with both given a molecule is excluded if EITHER matrix reaches its threshold
    against an already kept molecule.  A score of None (a call that does not score shape) ranks like every other None:
    the walk is then in sample-id order."""
    keep = [i for i, s in enumerate(scores) if min_shape_tanimoto is None or s >= min_shape_tanimoto]
    keep.sort(key=lambda i: ranking_key(scores[i], sample_ids[i]))
    walks = [(m, t) for m, t in ((pair, max_pairwise_tanimoto), (chemical_pair, max_pairwise_chemical_tanimoto))
             if t is not None]
    if walks:
        import numpy as np
        walks = [(np.asarray(m.cpu() if torch.is_tensor(m) else m, dtype=np.float64), t) for m, t in walks]  # fp32 entries, exactly
        kept: List[int] = []
        for i in keep:
            if top_k is not None and len(kept) >= top_k:
                break                        # later molecules cannot change what is already kept
            if not kept or not any(bool((p[i, kept] >= t).any()) for p, t in walks):
                kept.append(i)
        keep = kept
    return keep if top_k is None else keep[:top_k]


def select_scored(scores: List[float], sample_ids: List[int], top_k: Optional[int] = None,
                  min_shape_tanimoto: Optional[float] = None) -> List[int]:
    """Positions of the molecules to keep: score >= `min_shape_tanimoto`, then the `top_k` best, in descending score
    order with ties going to the lower sample id.  A NaN score (a molecule with no overlap with the reference grid at all)
    ranks last and passes no threshold.  (`select_diverse` without the exclusion.)"""
    return select_diverse(scores, sample_ids, None, None, top_k, min_shape_tanimoto)


def mol_heavy_coords(mol) -> torch.Tensor:
    """Heavy-atom coordinates [n,3] fp32 of an RDKit Mol (or anything with `GetConformer().GetPositions()`), as
    `evaluate_samples` reads them after `RemoveHs`."""
    import numpy as np
    pos = torch.as_tensor(np.asarray(mol.GetConformer().GetPositions(), dtype=np.float64)).to(torch.float32)
    if hasattr(mol, "GetAtoms"):
        heavy = [a.GetAtomicNum() != 1 for a in mol.GetAtoms()]
        if not all(heavy):
            pos = pos[torch.tensor(heavy)]
    return pos.reshape(-1, 3)


def padded_coords(coord_list: List[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-molecule [n_i,3] coordinates -> (padded [B, max n, 3], n_nodes [B])."""
    n = torch.tensor([int(c.shape[0]) for c in coord_list], dtype=torch.int32)
    out = torch.zeros(len(coord_list), int(n.max()) if len(coord_list) else 0, 3)
    for b, c in enumerate(coord_list):
        out[b, : c.shape[0]] = c
    return out, n


def evaluate_samples(reference, samples, generator=None, device=None):
    """`evaluate_samples` of the reference (cheminformatics/pipeline.py:17-96) with its signature and return value:
    (mol block of the reference in its principal shape frame, per sample {"mol_block", "shape_tanimoto",
    "chemical_tanimoto"}).  The shape half - principal frames and the four-orientation Gaussian-volume Tanimoto search - runs on
    the HIP path for all samples at once (`evaluate_shape`); the chemical half (Morgan fingerprints radius 2, 2 048 bits, bond
    types on, chirality off, `TanimotoSimilarity`) and the mol-block output are RDKit's own and run ONLY where RDKit imports -
    this wrapper is untested offline (RDKit is absent from the build container and the GPU boxes;
    `tests/test_rdkit_optional.py` runs it where RDKit and a GPU exist)."""
    from rdkit import Chem
    from rdkit.Chem import rdFingerprintGenerator
    from rdkit.DataStructs.cDataStructs import TanimotoSimilarity
    from rdkit.Geometry import Point3D

    if generator is None:                                                       # pipeline.py:11-14
        generator = rdFingerprintGenerator.GetMorganGenerator(radius=2, fpSize=2048, includeChirality=False, useBondTypes=True)

    def set_positions(mol, coord):                                              # pipeline.py:99-105
        conf = mol.GetConformer()
        for i, point in enumerate(coord.tolist()):
            conf.SetAtomPosition(i, Point3D(point[0], point[1], point[2]))
        return mol

    reference = Chem.RemoveHs(reference)                                        # :32
    fp_ref = generator.GetFingerprint(reference)
    ref_coord = torch.tensor(reference.GetConformer().GetPositions(), dtype=torch.float32)
    stripped = [Chem.RemoveHs(s) for s in samples]                              # :61
    if not stripped:
        _, ref_pf = shape_quadrupole_batch((ref_coord - ref_coord.mean(0)).unsqueeze(0), torch.tensor([ref_coord.shape[0]]),
                                           torch.device(device if device is not None else "cuda:0"))
        return Chem.MolToMolBlock(set_positions(reference, ref_pf[0].cpu())), []
    n_nodes = torch.tensor([m.GetNumAtoms() for m in stripped])
    coords = torch.zeros(len(stripped), int(n_nodes.max()), 3)
    for b, m in enumerate(stripped):
        coords[b, : m.GetNumAtoms()] = torch.tensor(m.GetConformer().GetPositions(), dtype=torch.float32)
    ref_pf, shape = evaluate_shape(ref_coord, coords, n_nodes, device)
    ref_mol_block = Chem.MolToMolBlock(set_positions(reference, ref_pf))        # :44-45
    results = []
    for m, r in zip(stripped, shape):
        results.append({"mol_block": Chem.MolToMolBlock(set_positions(m, r["coords"])),
                        "shape_tanimoto": r["shape_tanimoto"],
                        "chemical_tanimoto": TanimotoSimilarity(fp_ref, generator.GetFingerprint(m))})
    return ref_mol_block, results
