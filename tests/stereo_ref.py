"""Plain-Python fp64 restatement of the stereo identity of DESIGN.md section 6 ("Stereo identity"), written from the words
of the definition and not from the kernel: the candidates, the geometric signs, the descriptors at a labelling, the
pruned search (`canonical_ref`'s, with the leaf tie-break and the terminal-twin rule) and the judge of both - the brute
force over all n! numberings, which takes every descriptor straight from the geometry in the order of the labelling.
Also a reader of the isomeric subset `smiles.write_smiles(..., stereo=)` emits.  A molecule is (z, adj, n, xyz):
`canonical_ref`'s graph and n coordinate triples."""
import itertools
import math

import canonical_ref as R

THRESHOLD = 0.1
_M = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------- vectors
def _sub(p, q):
    return (p[0] - q[0], p[1] - q[1], p[2] - q[2])


def _dot(p, q):
    return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]


def _det(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))


def _neighbours(adj, n, a):
    return [j for j in range(n) if j != a and adj[a][j] != 0]


def terminal_twins(z, adj, n, a):
    """Whether a carries two terminal twins: two degree-1 neighbours of equal Z bonded to it with the same code."""
    ends = [(z[j], adj[a][j]) for j in _neighbours(adj, n, a) if len(_neighbours(adj, n, j)) == 1]
    return len(set(ends)) < len(ends)


# ------------------------------------------------------------------------------------------------- candidates
def chi(xyz, a, nb):
    """The normalised signed volume of a centre with its neighbours `nb` in the order given; None where a vector has no
    length."""
    if len(nb) == 4:
        v = [_sub(xyz[j], xyz[nb[3]]) for j in nb[:3]]
    else:
        v = [_sub(xyz[j], xyz[a]) for j in nb]
    length = math.sqrt(_dot(v[0], v[0])) * math.sqrt(_dot(v[1], v[1])) * math.sqrt(_dot(v[2], v[2]))
    return _det(*v) / length if length > 0 else None


def tetrahedral(z, adj, n, xyz):
    """Per atom None (no candidate), or (neighbours ascending, s) with s in {-1, 0, 1}; 0 = undefined."""
    out = []
    for a in range(n):
        nb = _neighbours(adj, n, a)
        if z[a] not in (6, 14) or any(adj[a][j] != 1 for j in nb) or len(nb) not in (3, 4) or terminal_twins(z, adj, n, a):
            out.append(None)
            continue
        x = chi(xyz, a, nb)
        out.append((nb, 0 if x is None or not abs(x) >= THRESHOLD else (1 if x > 0 else -1)))
    return out


def _end_ok(z, adj, n, a):
    nb = _neighbours(adj, n, a)
    return z[a] in (6, 7) and [adj[a][j] for j in nb].count(2) == 1 and all(adj[a][j] in (1, 2) for j in nb) and \
        len(nb) in (2, 3) and not terminal_twins(z, adj, n, a)


def dihedral_cos(xyz, a, b, x, y):
    """The cosine of the dihedral x-a=b-y from the components perpendicular to the axis; None where one vanishes."""
    e = _sub(xyz[b], xyz[a])
    ee = _dot(e, e)
    if not ee > 0:
        return None
    dx, dy = _sub(xyz[x], xyz[a]), _sub(xyz[y], xyz[b])
    tx, ty = _dot(dx, e) / ee, _dot(dy, e) / ee
    px = (dx[0] - tx * e[0], dx[1] - tx * e[1], dx[2] - tx * e[2])
    py = (dy[0] - ty * e[0], dy[1] - ty * e[1], dy[2] - ty * e[2])
    length = math.sqrt(_dot(px, px)) * math.sqrt(_dot(py, py))
    return _dot(px, py) / length if length > 0 else None


def double_bonds(z, adj, n, xyz):
    """{(a, b), a < b: None (undefined) or {(x, y): +1 cis / -1 trans} over the substituents x of a and y of b}."""
    out = {}
    for a in range(n):
        for b in range(a + 1, n):
            if adj[a][b] != 2 or not (_end_ok(z, adj, n, a) and _end_ok(z, adj, n, b)):
                continue
            xs = [j for j in _neighbours(adj, n, a) if j != b]
            ys = [j for j in _neighbours(adj, n, b) if j != a]
            cos = {(x, y): dihedral_cos(xyz, a, b, x, y) for x in xs for y in ys}
            ok = all(c is not None and abs(c) >= THRESHOLD for c in cos.values())
            sign = {k: (1 if c > 0 else -1) for k, c in cos.items()} if ok else None
            if ok and len(xs) == 2:
                ok = all(sign[(xs[0], y)] != sign[(xs[1], y)] for y in ys)
            if ok and len(ys) == 2:
                ok = all(sign[(x, ys[0])] != sign[(x, ys[1])] for x in xs)
            out[(a, b)] = sign if ok else None
    return out


def margins(z, adj, n, xyz):
    """Every |chi| and |cos| the definition compares with the threshold (a vector without length counts as 0)."""
    out = []
    for a in range(n):
        nb = _neighbours(adj, n, a)
        if z[a] in (6, 14) and all(adj[a][j] == 1 for j in nb) and len(nb) in (3, 4) and not terminal_twins(z, adj, n, a):
            out.append(abs(chi(xyz, a, nb) or 0.0))
    for a in range(n):
        for b in range(a + 1, n):
            if adj[a][b] == 2 and _end_ok(z, adj, n, a) and _end_ok(z, adj, n, b):
                out += [abs(dihedral_cos(xyz, a, b, x, y) or 0.0) for x in _neighbours(adj, n, a) if x != b
                        for y in _neighbours(adj, n, b) if y != a]
    return out


def counts(z, adj, n, xyz):
    """(defined tetrahedral descriptors, defined double bonds, undefined candidates)."""
    tet = [t for t in tetrahedral(z, adj, n, xyz) if t is not None]
    dbs = list(double_bonds(z, adj, n, xyz).values())
    return (sum(1 for t in tet if t[1] != 0), sum(1 for d in dbs if d is not None),
            sum(1 for t in tet if t[1] == 0) + sum(1 for d in dbs if d is None))


# ------------------------------------------------------------------------------------------------- descriptors
def _parity(values):
    """+1 / -1: the parity of the permutation that sorts `values`."""
    inversions = sum(1 for i in range(len(values)) for j in range(i) if values[j] > values[i])
    return -1 if inversions & 1 else 1


def descriptors(tet, dbs, n, L):
    """Per ATOM 4 tet + db at the labelling L (rank of every atom), by the integer rule: the stored sign times the parity
    that sorts the neighbours by L."""
    val = [0] * n
    for a, t in enumerate(tet):
        if t is not None and t[1] != 0:
            val[a] = 4 * (1 if t[1] * _parity([L[j] for j in t[0]]) > 0 else 2)
    for (a, b), sign in dbs.items():
        if sign is not None:
            x = min({k[0] for k in sign}, key=lambda j: L[j])
            y = min({k[1] for k in sign}, key=lambda j: L[j])
            val[a if L[a] > L[b] else b] += 1 if sign[(x, y)] > 0 else 2
    return val


def stereo_vector(tet, dbs, n, order):
    L = [0] * n
    for k, a in enumerate(order):
        L[a] = k
    val = descriptors(tet, dbs, n, L)
    return tuple(val[a] for a in order)


def geometric_vector(z, adj, n, xyz, tet, dbs, order):
    """The stereo vector at a labelling straight from the geometry: the sign of chi with the neighbours in the order of
    the labelling, the dihedral of the two lowest substituents.  Which candidate is defined is the definition's."""
    L = [0] * n
    for k, a in enumerate(order):
        L[a] = k
    val = [0] * n
    for a, t in enumerate(tet):
        if t is not None and t[1] != 0:
            val[a] = 4 * (1 if chi(xyz, a, sorted(t[0], key=lambda j: L[j])) > 0 else 2)
    for (a, b), sign in dbs.items():
        if sign is not None:
            x = min((j for j in _neighbours(adj, n, a) if j != b), key=lambda j: L[j])
            y = min((j for j in _neighbours(adj, n, b) if j != a), key=lambda j: L[j])
            val[a if L[a] > L[b] else b] += 1 if dihedral_cos(xyz, a, b, x, y) > 0 else 2
    return tuple(val[a] for a in order)


# ------------------------------------------------------------------------------------------------- the search
def is_terminal_twin(z, adj, n, u, v):
    """Twins (`canonical_ref.is_twin`) of degree at most 1: swapping them moves no descriptor."""
    return R.is_twin(z, adj, n, u, v) and len(_neighbours(adj, n, u)) <= 1


def stereo(z, adj, n, xyz, first_leaf_wins=False, full_twin_rule=False, budget=R.LEAF_BUDGET, perceived=None):
    """dict(order, status, leaves, certificate, stereo, counts) of one embedded molecule: `canonical_ref.canonical`'s
    search, where a leaf with the best certificate wins if its stereo vector is smaller and only terminal twins are
    skipped.  `first_leaf_wins` / `full_twin_rule`: the two mutations.  `perceived`: (`tetrahedral`'s, `double_bonds`'
    result) from elsewhere than coordinates - the isomeric reader's; `counts` is then None."""
    cnt = None if perceived else counts(z, adj, n, xyz) if n else (0, 0, 0)
    if n == 0:
        return dict(order=[], status=R.EMPTY, leaves=0, certificate=None, stereo=None, counts=cnt)
    nbrs = [[(j, adj[a][j]) for j in range(n) if j != a and adj[a][j] != 0] for a in range(n)]
    if any(len(x) > R.MAX_DEGREE for x in nbrs):
        return dict(order=[], status=R.DEGREE, leaves=0, certificate=None, stereo=None, counts=cnt)
    tet, dbs = perceived or (tetrahedral(z, adj, n, xyz), double_bonds(z, adj, n, xyz))
    twin = R.is_twin if full_twin_rule else is_terminal_twin
    state = dict(leaves=0, best=None, order=None)

    def visit(rank):
        if len(set(rank)) == n:
            if state["leaves"] == budget:
                raise R._OverBudget
            state["leaves"] += 1
            order = sorted(range(n), key=lambda a: rank[a])
            found = (R.certificate(z, adj, order), stereo_vector(tet, dbs, n, order))
            if state["best"] is None or (found[0] < state["best"][0] if first_leaf_wins else found < state["best"]):
                state["best"], state["order"] = found, order
            return
        count = {}
        for r in rank:
            count[r] = count.get(r, 0) + 1
        r = min(k for k, c in count.items() if c > 1)
        tried = []
        for v in [a for a in range(n) if rank[a] == r]:
            if any(twin(z, adj, n, u, v) for u in tried):
                continue
            tried.append(v)
            visit(R.refine([x + 1 if (x == r and a != v) else x for a, x in enumerate(rank)], nbrs))

    key0 = [(z[a], len(nbrs[a]), sum(R._V2[c] for _, c in nbrs[a])) for a in range(n)]
    try:
        visit(R.refine(R.ranks(key0), nbrs))
    except R._OverBudget:
        return dict(order=[], status=R.BUDGET, leaves=budget, certificate=None, stereo=None, counts=cnt)
    return dict(order=state["order"], status=0, leaves=state["leaves"], certificate=state["best"][0],
                stereo=state["best"][1], counts=cnt)


def brute_force(z, adj, n, xyz, certificate):
    """The smallest stereo vector over ALL n! numberings whose certificate is `certificate` - the search's minimal one,
    which `canonical_ref` defines over its leaves and `test_canonical_host` checks against brute-force isomorphism; those
    numberings are one labelling's images under every automorphism.  Every descriptor comes from the geometry."""
    tet, dbs = tetrahedral(z, adj, n, xyz), double_bonds(z, adj, n, xyz)
    best = None
    for order in itertools.permutations(range(n)):
        if R.certificate(z, adj, order) == certificate:
            v = geometric_vector(z, adj, n, xyz, tet, dbs, order)
            best = v if best is None or v < best else best
    return best


def same_stereoisomer(a, b):
    """Brute force over all n! maps: whether some graph isomorphism carries every defined descriptor of molecule `a`
    onto `b`'s - handedness and cis / trans read from the geometry through the map - and undefined onto undefined."""
    (za, adja, n, xa), (zb, adjb, m, xb) = a, b
    if n != m or sorted(za) != sorted(zb):
        return False
    ta, da = tetrahedral(za, adja, n, xa), double_bonds(za, adja, n, xa)
    tb, db = tetrahedral(zb, adjb, n, xb), double_bonds(zb, adjb, n, xb)
    for p in itertools.permutations(range(n)):                       # atom i of a -> atom p[i] of b
        if any(za[i] != zb[p[i]] for i in range(n)) or \
                any(adja[i][j] != adjb[p[i]][p[j]] for i in range(n) for j in range(i)):
            continue
        ok = True
        for i, t in enumerate(ta):
            if t is None:
                continue
            u = tb[p[i]]
            if (t[1] == 0) != (u[1] == 0):
                ok = False
            elif t[1] != 0 and (chi(xa, i, t[0]) > 0) != (chi(xb, p[i], [p[j] for j in t[0]]) > 0):
                ok = False
        for (i, j), sign in da.items():
            other = db[(min(p[i], p[j]), max(p[i], p[j]))]
            if (sign is None) != (other is None):
                ok = False
            elif sign is not None:
                for (x, y), c in sign.items():
                    if (dihedral_cos(xb, p[i], p[j], p[x], p[y]) > 0) != (c > 0):
                        ok = False
        if ok:
            return True
    return False


def identity_bytes(z, adj, n, xyz):
    out = stereo(z, adj, n, xyz)
    if out["status"] != 0:
        return None
    return R.identity_bytes(z, adj, n) + bytes(out["stereo"])


def stereo_key(z, adj, n, order, v):
    """`canonical_ref.key`'s mixing over [n, the row hashes, v[0..n-1]]."""
    halves = []
    for seed in (R.SEED, R.SEED_HI):
        h = R._mix(seed, n)
        for k in range(n):
            r = R._mix(seed, z[order[k]] & _M)
            for j in range(k):
                r = R._mix(r, adj[order[k]][order[j]])
            h = R._mix(h, R._final(r, k + 1))
        for k in range(n):
            h = R._mix(h, v[k])
        halves.append(R._final(h, 2 * n + 1))
    return (halves[1] << 32) | halves[0]


def per_atom(order, v):
    """The descriptors in the molecule's own atom order, L-relative as stored: (tet, db) per atom."""
    out = [(0, 0)] * len(order)
    for k, a in enumerate(order):
        out[a] = (v[k] >> 2, v[k] & 3)
    return out


# ------------------------------------------------------------------------------------------------- the isomeric reader
def read_isomeric(text):
    """(z, adj, n, tet, dbs) of a string of `smiles.write_smiles(..., stereo=)`'s subset: `canonical_ref.read_smiles`'s,
    plus bracket atoms with "@" / "@@" and "/" "\\" on single bonds - in front of an atom or a ring-OPENING digit.
    Atoms are numbered as written.  `tet` / `dbs` are `tetrahedral`'s / `double_bonds`' results relative to that
    numbering, by the OpenSMILES rules: looking from the first neighbour, the rest anticlockwise is "@"; the neighbour
    order is the preceding atom, the implicit H, the ring-closure digits as written, the branches."""
    plain, chir, slashes = [], {}, []          # the string without marks; atom -> "@"...; (atom before, atom after, symbol)
    z, lower, written, bonds = [], [], [], []
    prev, pending, slash, stack, open_rings = None, None, None, [], {}
    i = 0

    def atom(sym, low, mark, h):
        nonlocal prev, pending, slash
        z.append(R._SYMBOL_Z[sym])
        lower.append(low)
        a = len(z) - 1
        written.append(([prev] if prev is not None else []) + (["H"] if h else []))
        if mark:
            chir[a] = mark
        if prev is not None:
            bonds.append((prev, a, pending if pending is not None else (4 if lower[prev] and low else 1)))
            written[prev].append(a)
            if slash:
                slashes.append((prev, a, slash))
        prev, pending, slash = a, None, None

    while i < len(text):
        ch = text[i]
        if ch == "[":
            j = text.index("]", i)
            body = text[i + 1: j]
            mark = "@@" if "@@" in body else "@" if "@" in body else None
            body = body.replace("@", "")
            k = 1
            while k < len(body) and body[k].islower() and body[:k + 1].capitalize() in R._SYMBOL_Z:
                k += 1
            sym, rest = body[:k], body[k:]
            assert rest in ("", "H") or not mark, text
            atom(sym.capitalize(), sym[0].islower(), mark, rest == "H" and mark)
            i = j + 1
        elif ch in R._BOND:
            pending, i = R._BOND[ch], i + 1
        elif ch in "/\\":
            slash, i = ch, i + 1
        elif ch == "(":
            stack.append(prev)
            i += 1
        elif ch == ")":
            prev, i = stack.pop(), i + 1
        elif ch == ".":
            prev, pending, i = None, None, i + 1
        elif ch.isdigit() or ch == "%":
            num, i = (int(text[i + 1: i + 3]), i + 3) if ch == "%" else (int(ch), i + 1)
            if num in open_rings:
                a, sym, slot = open_rings.pop(num)
                bonds.append((a, prev, pending if pending is not None else (4 if lower[a] and lower[prev] else 1)))
                written[a][slot] = prev
                written[prev].append(a)
                if sym:
                    slashes.append((a, prev, sym))
                pending = None
            else:
                written[prev].append(None)
                open_rings[num] = (prev, slash, len(written[prev]) - 1)
                slash = None
        elif text[i: i + 2] in ("Cl", "Br"):
            atom(text[i: i + 2], False, None, False)
            i += 2
        elif ch in "BCNOPSFI":
            atom(ch, False, None, False)
            i += 1
        elif ch in "bcnops":
            atom(ch.upper(), True, None, False)
            i += 1
        else:
            raise AssertionError(f"unreadable at {i}: {text}")
    assert not open_rings and not stack, text
    n = len(z)
    adj = [[0] * n for _ in range(n)]
    for a, b, c in bonds:
        assert a != b and adj[a][b] == 0, text
        adj[a][b] = adj[b][a] = c
    tet = [None] * n
    for a, mark in chir.items():
        order = [n if j == "H" else j for j in written[a]]
        assert len(order) == 4, text
        s = (1 if mark == "@" else -1) * _parity(order)              # chi > 0 in written order is "@"
        tet[a] = (_neighbours(adj, n, a), s)
    dbs = {}
    up = {}                                                           # (double-bond atom, substituent) -> +1 up / -1 down
    for a, b, sym in slashes:                                         # a written before b: "/" = b is up from a
        up[(a, b)] = 1 if sym == "/" else -1
        up[(b, a)] = -up[(a, b)]
    for a in range(n):
        for b in range(a + 1, n):
            if adj[a][b] != 2:
                continue
            xs = [j for j in _neighbours(adj, n, a) if j != b]
            ys = [j for j in _neighbours(adj, n, b) if j != a]
            sa = {(1 if k == 0 else -1) * up[(a, j)] for k, j in enumerate(xs) if (a, j) in up}
            sb = {(1 if k == 0 else -1) * up[(b, j)] for k, j in enumerate(ys) if (b, j) in up}
            if sa and sb:
                assert len(sa) == 1 and len(sb) == 1, text
                c = next(iter(sa)) * next(iter(sb))
                dbs[(a, b)] = {(x, y): c * (1 if i == 0 else -1) * (1 if j == 0 else -1)
                               for i, x in enumerate(xs) for j, y in enumerate(ys)}
    return z, adj, n, tet, dbs
