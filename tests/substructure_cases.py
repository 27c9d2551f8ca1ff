"""The cases of the substructure tests ("Substructure patterns"): the named table with the numbers
the definition pins, the budget pair, seeded random patterns, the converters between the product's `Pattern`, its packed
tensors and the restatement's form, and the molecules and padded-batch builder of `canonical_cases`."""
import random

import canonical_cases as C
import canonical_ref as CR
import substructure_ref as R
from ml_conformer_generator_amd import substructure as S

pad_batch = C.pad_batch


def ring_smarts(k, atom="*", bond="~"):
    return f"{atom}{bond}1" + f"{bond}{atom}" * (k - 1) + f"{bond}1"


def path_smarts(k, atom="*", bond="~"):
    return bond.join([atom] * k)


AROM6 = "c:1:c:c:c:c:c:1"                    # `c1ccccc1` with the ring bonds code 4 only
ANY6, ANY5, ANY4 = ring_smarts(6), ring_smarts(5), ring_smarts(4)
PATH32 = path_smarts(32)
CHAIN64 = C.EDGES["64-atom chain"]


def molecule(name):
    return C.NAMED[name][0] if name in C.NAMED else C.EDGES[name]


# (pattern, molecule, count, popcount(covered)): the table of the definition
TABLE = [
    (AROM6, "benzene", 12, 6), (AROM6, "toluene", 12, 6), (AROM6, "hexamethylbenzene", 12, 6),
    (AROM6, "biphenyl", 24, 12), (AROM6, "naphthalene", 24, 10), (AROM6, "decalin", 0, 0), (AROM6, "cube", 0, 0),
    (ANY6, "decalin", 24, 10), (ANY6, "cube", 192, 8), (ANY6, "Wagner graph", 48, 8),
    (ANY4, "cube", 48, 8), (ANY4, "Wagner graph", 32, 8),
    (ANY5, "cube", 0, 0), (ANY5, "Wagner graph", 80, 8),
    ("C-C", "64-atom chain", 126, 64), (PATH32, "64-atom chain", 66, 64),
    ("[#6]~!@[#6]", "toluene", 2, 2), ("[#6]~@[#6]", "toluene", 12, 6),
]
TABLE_PATTERNS = list(dict.fromkeys(t[0] for t in TABLE))
TABLE_MOLECULES = list(dict.fromkeys(t[1] for t in TABLE))

K12 = CR.mol([6] * 12, [(a, b, 1) for a in range(12) for b in range(a)])
PATH6, PATH7 = path_smarts(6), path_smarts(7)
K12_PATH6_NODES, K12_PATH6_COUNT = 64472, 665280
K12_PATH7_COUNT = 658728                       # the lower bound the 7-path reaches: every root stops at the budget

PYRIDINE = CR.mol([7, 6, 6, 6, 6, 6], [(i, (i + 1) % 6, 4) for i in range(6)])
ETHANE = CR.mol([6, 6], [(0, 1, 1)])


# ----------------------------------------------------------------------------------------------- converters
def signed64(v):
    """An unsigned 64-bit pattern as the int64 that holds it."""
    return v - (1 << 64) if v >= 1 << 63 else v


def ref_atom(q):
    return R.qatom(None if q.elements is None else set(q.elements), q.dmin, q.dmax, q.hmin, q.hmax, q.ring, q.aromatic)


def to_ref(pattern):
    """A product `Pattern` (or a string of its subset) -> the restatement's (atoms, bonds, order) in matching order, by
    the restatement's own ordering rule."""
    pattern = S.as_pattern(pattern)
    return R.ordered([ref_atom(q) for q in pattern.atoms], {(q.a, q.b): (set(q.codes), q.ring) for q in pattern.bonds})


def unpack(compiled, p):
    """Pattern p of a `Compiled` read back from the packed tensors: (atoms, bonds) in the restatement's form."""
    tri = {0: None, 1: True, 2: False}
    m = int(compiled.pat_n[p])
    atoms, bonds = [], {}
    for k in range(m):
        mask = int(compiled.pat_atoms[p, k, 0]) & (2 ** 64 - 1)
        w = int(compiled.pat_atoms[p, k, 1])
        z = None if mask == 2 ** 64 - 1 else {b for b in range(64) if mask >> b & 1}
        atoms.append(R.qatom(z, w & 255, w >> 8 & 255, w >> 16 & 255, w >> 24 & 255, tri[w >> 32 & 255], tri[w >> 40 & 255]))
        for q in range(32):
            byte = int(compiled.pat_bonds[p, k, q])
            assert byte == int(compiled.pat_bonds[p, q, k])
            if byte and q < k:
                bonds[(k, q)] = ({c for c in (1, 2, 3, 4) if byte >> (c - 1) & 1}, tri[byte >> 4 & 3])
    assert int(compiled.pat_atoms[p, m:].abs().sum()) == 0 and int(compiled.pat_bonds[p, m:].sum()) == 0
    return atoms, bonds


def reference(mol, pattern, nh=None, **mutant):
    """The restatement's answer for a product pattern, `first` mapped back to the caller's pattern atom order."""
    atoms, bonds, order = to_ref(pattern)
    out = R.match(mol, atoms, bonds, nh=nh, **mutant)
    if out["first"] is not None:
        by_atom = dict(zip(order, out["first"]))
        out["first"] = [by_atom[i] for i in range(len(order))]
    return out


def is_embedding(mol, pattern, image, nh=None):
    """Whether `image` (the caller's pattern atom order) is an embedding, checked directly from the definition."""
    z, adj, n = mol
    pattern = S.as_pattern(pattern)
    deg, arom, ring, ring_bond, nh = R.derive(z, adj, n, nh)
    if len(set(image)) != len(image) or len(image) != len(pattern.atoms) or not all(0 <= a < n for a in image):
        return False
    for q, a in zip(pattern.atoms, image):
        if not ((q.elements is None or z[a] in q.elements) and q.dmin <= deg[a] <= q.dmax and q.hmin <= nh[a] <= q.hmax
                and q.ring in (None, ring[a]) and q.aromatic in (None, arom[a])):
            return False
    return all(adj[image[q.a]][image[q.b]] in q.codes and q.ring in (None, ring_bond[image[q.a]][image[q.b]])
               for q in pattern.bonds)


# ----------------------------------------------------------------------------------------------- seeded fuzz
FUZZ_SEED = 20261020


def random_pattern(rng, m, hydrogens=True):
    """A random pattern of m atoms over C N O: a random forest plus a few extra bonds, so some are disconnected and some
    have rings; element sets, degree and hydrogen bounds, ring and aromaticity flags, code masks and ring requirements
    are each set on a share of the atoms and bonds."""
    atoms = []
    for _ in range(m):
        kw = {}
        if rng.random() < 0.5:
            kw["elements"] = [6] if rng.random() < 0.5 else rng.sample([6, 7, 8], rng.randint(1, 2))
        if rng.random() < 0.2:
            lo = rng.randint(1, 2)
            kw["degree"] = (lo, lo + rng.randint(0, 2))
        if hydrogens and rng.random() < 0.15:
            lo = rng.randint(0, 2)
            kw["hydrogens"] = (lo, lo + rng.randint(0, 2))
        if rng.random() < 0.2:
            kw["ring"] = rng.random() < 0.6
        if rng.random() < 0.12:
            kw["aromatic"] = rng.random() < 0.5
        atoms.append(S.atom(**kw))
    pairs = set()
    for a in range(1, m):
        if rng.random() < 0.85:
            pairs.add((rng.randrange(a), a))
    for _ in range(rng.randint(0, 2)):
        a, b = rng.randrange(m), rng.randrange(m)
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    bonds = []
    for a, b in sorted(pairs):
        codes = S.ANY_CODES if rng.random() < 0.6 else rng.sample([1, 2, 4], rng.randint(1, 2))
        ring = None if rng.random() < 0.7 else rng.random() < 0.5
        bonds.append(S.bond(a, b, codes, ring))
    return S.Pattern(tuple(atoms), tuple(bonds))


def fuzz_patterns(count=16, seed=FUZZ_SEED, max_atoms=6):
    rng = random.Random(seed)
    return [random_pattern(rng, 1 + k % max_atoms) for k in range(count)]


def seam_by_restatement(calls):
    """`_match_substructures` by the restatement, on the host (hydrogens by the count rule without the aromatic N-H)."""
    import torch

    def run(z, bonds, n, compiled):
        z, bonds, n = torch.as_tensor(z), torch.as_tensor(bonds), torch.as_tensor(n).reshape(-1).tolist()
        P = len(compiled.patterns)
        calls.append((len(n), P))
        count = torch.zeros(len(n), P, dtype=torch.int32)
        status = torch.zeros(len(n), P, dtype=torch.int32)
        first = torch.full((len(n), P, compiled.max_atoms), -1, dtype=torch.int32)
        covered = torch.zeros(len(n), P, dtype=torch.int64)
        for b, k in enumerate(n):
            mol = (z[b, :k].tolist(), bonds[b, :k, :k].tolist(), k)
            for p, pattern in enumerate(compiled.patterns):
                out = reference(mol, pattern)
                count[b, p], status[b, p], covered[b, p] = out["count"], out["status"], signed64(R.covered_mask(out["covered"]))
                if out["first"] is not None:
                    first[b, p, : len(out["first"])] = torch.tensor(out["first"], dtype=torch.int32)
        return dict(count=count, status=status, first=first, covered=covered)
    return run
