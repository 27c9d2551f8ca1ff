"""Plain-Python restatement of the canonical labelling of DESIGN.md section 6 ("Canonical graphs and SMILES"), written
from the words of the definition and not from the kernel, and a SMILES reader for exactly the subset
`smiles.write_smiles` emits (the product has no reader).  A molecule is (z, adj, n): atomic numbers, an n x n list of
symmetric bond codes 0 none / 1 / 2 / 3 / 4 aromatic, and the atom count, as in `fingerprint_ref`."""
import itertools

MAX_DEGREE = 8
LEAF_BUDGET = 4096
EMPTY, DEGREE, BUDGET = 1, 2, 4
SEED = 0x6d636731
SEED_HI = SEED ^ 0x9e3779b9
_V2 = (0, 2, 4, 6, 3)            # twice the bond order, aromatic 1.5
_M = 0xFFFFFFFF


def mol(z, bonds):
    n = len(z)
    adj = [[0] * n for _ in range(n)]
    for a, b, c in bonds:
        adj[a][b] = adj[b][a] = c
    return list(z), adj, n


def permute(z, adj, n, p):
    """The molecule with new atom k = old atom p[k]."""
    return [z[a] for a in p], [[adj[a][b] for b in p] for a in p], n


def ranks(keys):
    """rank(a) = the number of atoms with a smaller key; tied atoms share a rank."""
    first = {}
    for pos, k in enumerate(sorted(keys)):
        first.setdefault(k, pos)
    return [first[k] for k in keys]


def refine(rank, nbrs, codes=True):
    """Refinement to the point where the number of distinct ranks stops growing.  `nbrs[a]`: the (j, code) pairs of a."""
    while True:
        keys = [(rank[a], tuple(sorted((rank[j], c if codes else 0) for j, c in nbrs[a]))) for a in range(len(rank))]
        new = ranks(keys)
        if len(set(new)) == len(set(rank)):
            return new
        rank = new


def certificate(z, adj, order):
    n = len(order)
    return tuple(z[a] for a in order) + tuple(adj[order[i]][order[j]] for i in range(1, n) for j in range(i))


def is_twin(z, adj, n, u, v):
    return z[u] == z[v] and all(adj[u][w] == adj[v][w] for w in range(n) if w != u and w != v)


class _OverBudget(Exception):
    pass


def canonical(z, adj, n, twins=True, codes=True, budget=LEAF_BUDGET):
    """dict(order, status, leaves, certificate) of one molecule.  `twins=False` / `codes=False`: the definition with the
    twin rule removed / with the bond code left out of the refinement key (the mutation checks)."""
    if n == 0:
        return dict(order=[], status=EMPTY, leaves=0, certificate=None)
    nbrs = [[(j, adj[a][j]) for j in range(n) if j != a and adj[a][j] != 0] for a in range(n)]
    if any(len(x) > MAX_DEGREE for x in nbrs):
        return dict(order=[], status=DEGREE, leaves=0, certificate=None)
    state = dict(leaves=0, best=None, order=None)

    def visit(rank):
        if len(set(rank)) == n:
            if state["leaves"] == budget:          # a branch is still unexplored behind the last leaf allowed
                raise _OverBudget
            state["leaves"] += 1
            order = sorted(range(n), key=lambda a: rank[a])
            cert = certificate(z, adj, order)
            if state["best"] is None or cert < state["best"]:
                state["best"], state["order"] = cert, order
            return
        count = {}
        for r in rank:
            count[r] = count.get(r, 0) + 1
        r = min(k for k, c in count.items() if c > 1)
        tried = []
        for v in [a for a in range(n) if rank[a] == r]:
            if twins and any(is_twin(z, adj, n, u, v) for u in tried):
                continue
            tried.append(v)
            visit(refine([x + 1 if (x == r and a != v) else x for a, x in enumerate(rank)], nbrs, codes))

    key0 = [(z[a], len(nbrs[a]), sum(_V2[c] for _, c in nbrs[a])) for a in range(n)]
    try:
        visit(refine(ranks(key0), nbrs, codes))
    except _OverBudget:
        return dict(order=[], status=BUDGET, leaves=budget, certificate=None)
    return dict(order=state["order"], status=0, leaves=state["leaves"], certificate=state["best"])


def identity_bytes(z, adj, n):
    """n, Z in canonical order (two bytes each, low first), then the lower-triangle codes; None where not canonicalisable."""
    out = canonical(z, adj, n)
    if out["status"] != 0:
        return None
    order = out["order"]
    body = b"".join(bytes([z[a] & 255, z[a] >> 8]) for a in order)
    return bytes([n]) + body + bytes(adj[order[i]][order[j]] for i in range(1, n) for j in range(i))


# ------------------------------------------------------------------------------------------------- the 64-bit key
def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M


def _mix(h, k):
    k = (k * 0xcc9e2d51) & _M
    k = _rotl(k, 15)
    k = (k * 0x1b873593) & _M
    h ^= k
    h = _rotl(h, 13)
    return (h * 5 + 0xe6546b64) & _M


def _final(h, n_words):
    h ^= 4 * n_words
    h ^= h >> 16
    h = (h * 0x85ebca6b) & _M
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & _M
    return h ^ (h >> 16)


def key(z, adj, n, order):
    """64 bits of the certificate: per seed, row k of the relabelled graph hashed as [Z, code(k,0) .. code(k,k-1)], then
    [n, the row hashes]; the low half under SEED, the high half under SEED_HI."""
    halves = []
    for seed in (SEED, SEED_HI):
        h = _mix(seed, n)
        for k in range(n):
            r = _mix(seed, z[order[k]] & _M)
            for j in range(k):
                r = _mix(r, adj[order[k]][order[j]])
            h = _mix(h, _final(r, k + 1))
        halves.append(_final(h, n + 1))
    return (halves[1] << 32) | halves[0]


# ------------------------------------------------------------------------------------------------- brute force
def isomorphic(a, b):
    (za, adja, n), (zb, adjb, m) = a, b
    if n != m or sorted(za) != sorted(zb):
        return False
    for p in itertools.permutations(range(n)):
        if all(za[p[i]] == zb[i] for i in range(n)) and \
                all(adja[p[i]][p[j]] == adjb[i][j] for i in range(n) for j in range(i)):
            return True
    return False


# ------------------------------------------------------------------------------------------------- the reader
_SYMBOL_Z = {"H": 1, "B": 5, "C": 6, "N": 7, "O": 8, "F": 9, "Si": 14, "P": 15, "S": 16, "Cl": 17, "As": 33, "Se": 34,
             "Br": 35, "I": 53}
_BOND = {"-": 1, "=": 2, "#": 3, ":": 4}


def read_smiles(text):
    """(z, adj, n, hydrogens) of a string of the writer's subset: bare B C N O P S F Cl Br I, lowercase b c n o p s,
    bracket atoms [Sym], [SymH], [SymHh] (lowercase inside the bracket too), bonds - = # :, ring closures 1..9 and
    %10..%99 with the bond symbol at the closing end, branches and dots.  No symbol between two lowercase atoms reads as
    code 4, otherwise as code 1.  `hydrogens[a]`: the bracket's count, None for a bare atom."""
    z, lower, hyd, bonds = [], [], [], []
    prev, pending, stack, open_rings = None, None, [], {}
    i = 0

    def implied(a, b):
        return 4 if lower[a] and lower[b] else 1

    def atom(sym, low, h):
        nonlocal prev, pending
        z.append(_SYMBOL_Z[sym])
        lower.append(low)
        hyd.append(h)
        a = len(z) - 1
        if prev is not None:
            bonds.append((prev, a, pending if pending is not None else implied(prev, a)))
        prev, pending = a, None

    while i < len(text):
        ch = text[i]
        if ch == "[":
            j = text.index("]", i)
            body = text[i + 1: j]
            k = 1
            while k < len(body) and body[k].islower() and body[:k + 1].capitalize() in _SYMBOL_Z:
                k += 1
            sym, rest = body[:k], body[k:]
            h = 0
            if rest:
                assert rest[0] == "H", text
                h = int(rest[1:]) if len(rest) > 1 else 1
            atom(sym.capitalize(), sym[0].islower(), h)
            i = j + 1
        elif ch in _BOND:
            pending = _BOND[ch]
            i += 1
        elif ch == "(":
            stack.append(prev)
            i += 1
        elif ch == ")":
            prev = stack.pop()
            i += 1
        elif ch == ".":
            prev, pending = None, None
            i += 1
        elif ch.isdigit() or ch == "%":
            if ch == "%":
                num, i = int(text[i + 1: i + 3]), i + 3
            else:
                num, i = int(ch), i + 1
            if num in open_rings:
                a = open_rings.pop(num)
                bonds.append((a, prev, pending if pending is not None else implied(a, prev)))
                pending = None
            else:
                assert pending is None, text       # the writer puts the symbol at the closing end
                open_rings[num] = prev
        elif text[i: i + 2] in ("Cl", "Br"):
            atom(text[i: i + 2], False, None)
            i += 2
        elif ch in "BCNOPSFI":
            atom(ch, False, None)
            i += 1
        elif ch in "bcnops":
            atom(ch.upper(), True, None)
            i += 1
        else:
            raise AssertionError(f"unreadable at {i}: {text}")
    assert not open_rings and not stack, text
    n = len(z)
    adj = [[0] * n for _ in range(n)]
    for a, b, c in bonds:
        assert a != b and adj[a][b] == 0, text
        adj[a][b] = adj[b][a] = c
    return z, adj, n, hyd
