"""A numpy restatement of the receptor contact fingerprint (ml_conformer_generator_amd/contacts.py, DESIGN.md section 6,
"Receptor contacts"): every threshold is decided on the same fp32 d the kernel decides it on - float32 operations in the
kernel's order, `interactions_ref.surface_distances` - so the comparison with the kernel is bit for bit.  No GPU.

`fingerprint` takes the receptor's atoms in ANY order with their group ids; the result does not depend on that order.
`mistake=`: one of MISTAKES, a planted error for the mutation check of tests/test_contacts_host.py - a restatement that could
not tell these from the definition would pin nothing."""
import numpy as np

import interactions_ref as IR

CONTACT, HYDROPHOBIC, HBOND_DONOR, HBOND_ACCEPTOR = 1, 2, 4, 8
DEFAULT_KINDS = HYDROPHOBIC | HBOND_DONOR | HBOND_ACCEPTOR
T_DONOR, T_ACCEPTOR, T_HYDROPHOBIC = 1, 2, 4
MAX_GROUPS, MAX_CANDIDATES = 256, 2048
OK, EMPTY, NONFINITE, OVERFLOW = 0, 1, 2, 3
CONTACT_D, HBOND_D = np.float32(0.5), np.float32(-0.7)
MISTAKES = ("lt_at_contact", "hbond_direction_swapped", "last_writer_wins", "group_of_unsorted_index")


def pair_kinds(x, ri, ti, y, rj, tj, mistake=None):
    """[n,R] uint8: the kind bits of every pair, 0 where the pair is not looked at (r2 >= 64.0f)."""
    looked, d64 = IR.surface_distances(x, ri, y, rj)
    d = d64.astype(np.float32)                                     # (holds the fp32 values: the cast back is exact)
    ti, tj = np.asarray(ti, dtype=np.int64)[:, None], np.asarray(tj, dtype=np.int64)[None, :]
    close = looked & ((d < CONTACT_D) if mistake == "lt_at_contact" else (d <= CONTACT_D))
    bond = looked & (d <= HBOND_D)
    lig_don, lig_acc = (ti & T_DONOR) != 0, (ti & T_ACCEPTOR) != 0
    rec_don, rec_acc = (tj & T_DONOR) != 0, (tj & T_ACCEPTOR) != 0
    donates, accepts = lig_don & rec_acc, lig_acc & rec_don
    if mistake == "hbond_direction_swapped":
        donates, accepts = accepts, donates
    return (close * CONTACT + (close & ((ti & tj & T_HYDROPHOBIC) != 0)) * HYDROPHOBIC + (bond & donates) * HBOND_DONOR
            + (bond & accepts) * HBOND_ACCEPTOR).astype(np.uint8)


def fingerprint(x, ri, ti, y, rj, tj, groups, mistake=None, order=None):
    """dict of one molecule against a receptor: entries [(group, kinds)] ascending, atom_kinds [n] uint8, status.
    `order`: with the mistake "group_of_unsorted_index", the permutation the receptor is sorted by while the group ids stay
    behind (default: reversed)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    n = len(x)
    if n == 0:
        return dict(entries=[], atom_kinds=np.zeros(0, dtype=np.uint8), status=EMPTY)
    if not np.isfinite(x).all():
        return dict(entries=[], atom_kinds=np.zeros(n, dtype=np.uint8), status=NONFINITE)
    y, rj, tj, groups = np.asarray(y, dtype=np.float32).reshape(-1, 3), np.asarray(rj), np.asarray(tj), np.asarray(groups)
    if mistake == "group_of_unsorted_index":
        order = np.arange(len(y))[::-1] if order is None else np.asarray(order)
        y, rj, tj = y[order], rj[order], tj[order]
    k = pair_kinds(x, ri, ti, y, rj, tj, mistake)
    per_atom = np.bitwise_or.reduce(k, axis=0)                     # [R]: over the ligand's atoms
    touched = np.flatnonzero(per_atom)
    found = {}
    for j in touched:
        g = int(groups[j])
        if mistake == "last_writer_wins":
            found[g] = int(k[:, j][k[:, j] != 0][-1])
        else:
            found[g] = found.get(g, 0) | int(per_atom[j])
    if len(touched) > MAX_CANDIDATES or len(found) > MAX_GROUPS:
        return dict(entries=[], atom_kinds=np.zeros(n, dtype=np.uint8), status=OVERFLOW)
    return dict(entries=sorted(found.items()), atom_kinds=np.bitwise_or.reduce(k, axis=1).astype(np.uint8), status=OK)


def popcount(v):
    return bin(int(v)).count("1")


def compare(result, reference, mask=DEFAULT_KINDS):
    """(n_bits, n_ref_bits, n_common, recovery, tanimoto) of a `fingerprint` result against a reference list [(group,
    kinds)]: exact integers and their fp64 quotients, NaN on an empty denominator; -1, -1, -1, NaN, NaN where the row failed."""
    if result["status"] in (NONFINITE, OVERFLOW):
        return -1, -1, -1, float("nan"), float("nan")
    ref = dict(reference)
    n_bits = sum(popcount(k & mask) for _, k in result["entries"])
    n_ref = sum(popcount(k & mask) for k in ref.values())
    n_common = sum(popcount(k & ref.get(g, 0) & mask) for g, k in result["entries"])
    union = n_bits + n_ref - n_common
    return (n_bits, n_ref, n_common, n_common / n_ref if n_ref else float("nan"),
            n_common / union if union else float("nan"))
