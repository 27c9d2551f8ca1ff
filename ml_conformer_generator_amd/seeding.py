"""Per-molecule keyed randomness (`sample_seed`): host half.

With `sample_seed=S`, everything random about molecule `i` of a generation call is a function of `(S, i)` alone, drawn
from the counter-based Philox4x32-10 generator (Salmon et al., SC'11) - no state, so any molecule's draws can be produced
on their own, in any batch layout and on any rank.  The stream (include/mlconfgen_hip.h):

  key      (S & 0xffffffff, S >> 32),  S in [0, 2^64)
  noise    counter (sample_id, draw, atom, (run << 8) | block), Box-Muller per word pair - on the device
           (`mcg_sampler_noise_keyed`, csrc/mcg_noise.hip)
  size     counter (sample_id, 0, 0, 0xffffffff);  n = lo + ((w0 * (hi - lo + 1)) >> 32)  - here, on the host

This module holds the host half: a vectorised numpy Philox and the keyed molecule sizes.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
SIZE_COUNTER_WORD = 0xFFFFFFFF       # c3 of the size draw; a noise counter's c3 = (run << 8) | block never reaches it
MAX_RUNS = 1 << 24                   # run ordinals fit the 24 high bits of c3
MAX_SAMPLE_ID = 1 << 32              # sample ids are counter word c0

_U32 = np.uint64(0xFFFFFFFF)


def philox_key(sample_seed: int) -> Tuple[int, int]:
    """(k0, k1) of a sample seed; refuses anything outside [0, 2^64)."""
    s = check_seed(sample_seed)
    return s & 0xFFFFFFFF, s >> 32


def check_seed(sample_seed) -> int:
    if isinstance(sample_seed, bool) or not isinstance(sample_seed, (int, np.integer)):
        raise TypeError(f"sample_seed must be an int, not {type(sample_seed).__name__}")
    s = int(sample_seed)
    if not 0 <= s < 1 << 64:
        raise ValueError("sample_seed must lie in [0, 2^64)")
    return s


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 of counters [..., 4] under key (k0, k1): words [..., 4] uint32 (vectorised over the counters)."""
    c = np.array(counter, dtype=np.uint64) & _U32
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _U32, (k1 + np.uint64(PHILOX_W1)) & _U32
        p0, p1 = m0 * c0, m1 * c2                       # < 2^64: exact in uint64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32)
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def check_sample_ids(sample_ids, n_samples: Optional[int] = None) -> torch.Tensor:
    """[B] int64 CPU tensor of sample ids in [0, 2^32); with `n_samples`, exactly that many."""
    ids = torch.as_tensor(sample_ids).reshape(-1)
    if ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise TypeError("sample_ids must be integers")
    ids = ids.to("cpu", torch.int64)
    if n_samples is not None and ids.numel() != n_samples:
        raise ValueError(f"sample_ids holds {ids.numel()} ids for n_samples={n_samples}")
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= MAX_SAMPLE_ID):
        raise ValueError("sample_ids must lie in [0, 2^32)")
    return ids


def keyed_sizes(sample_seed: int, sample_ids: Sequence[int], min_n_nodes: int, max_n_nodes: int) -> torch.Tensor:
    """Molecule sizes [B] int64 (CPU): n_i = lo + ((w0 * (hi - lo + 1)) >> 32), w0 the first word of Philox at counter
    (sample_id, 0, 0, 0xffffffff).  A function of (seed, id) alone: the same on every rank and in every batch layout."""
    lo, hi = int(min_n_nodes), int(max_n_nodes)
    if hi < lo:
        raise ValueError("max_n_nodes must be >= min_n_nodes")
    ids = check_sample_ids(sample_ids).numpy().astype(np.uint64)
    ctr = np.zeros((ids.size, 4), dtype=np.uint64)
    ctr[:, 0] = ids
    ctr[:, 3] = SIZE_COUNTER_WORD
    w0 = philox4x32_10(ctr, philox_key(sample_seed))[:, 0].astype(np.uint64)
    n = np.uint64(lo) + ((w0 * np.uint64(hi - lo + 1)) >> np.uint64(32))     # (2^32-1) * span < 2^64 for any span < 2^32
    return torch.from_numpy(n.astype(np.int64))
