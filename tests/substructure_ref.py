"""Plain-Python restatement of the substructure matching of DESIGN.md section 6 ("Substructure patterns"), written from
the words of the definition and not from the kernel: lists and loops, no bit masks.  A molecule is (z, adj, n) as in
`canonical_ref`.  A pattern here is (atoms, bonds) ALREADY IN MATCHING ORDER: `atoms[k]` a dict with z (a set of atomic
numbers, or None: any), dmin, dmax, hmin, hmax, ring and arom (None any / True / False); `bonds[(k, q)]`, q < k, a pair
(codes: a set of 1..4, ring: None any / True a ring bond / False a chain bond).  `ordered` brings a pattern in the caller's
own order into that form by the matching-order rule."""
NODE_BUDGET = 65536
BUDGET = 1
V0 = {5: 3, 6: 4, 7: 3, 8: 2, 9: 1, 14: 4, 15: 3, 16: 2, 17: 1, 33: 3, 34: 2, 35: 1, 53: 1}
V2 = (0, 2, 4, 6, 3)            # twice the bond order, aromatic 1.5


def qatom(z=None, dmin=0, dmax=255, hmin=0, hmax=255, ring=None, arom=None):
    if isinstance(z, int):
        z = {z}
    return dict(z=None if z is None else set(z), dmin=dmin, dmax=dmax, hmin=hmin, hmax=hmax, ring=ring, arom=arom)


def qbond(codes=(1, 2, 3, 4), ring=None):
    return (set([codes] if isinstance(codes, int) else codes), ring)


def matching_order(m, pairs):
    """Position -> atom: per component breadth-first from its lowest-index atom, neighbours in ascending index,
    components in ascending order of their lowest atom."""
    order = []
    for start in range(m):
        if start in order:
            continue
        queue = [start]
        order.append(start)
        while queue:
            a = queue.pop(0)
            for j in range(m):
                if j not in order and ((a, j) in pairs or (j, a) in pairs):
                    order.append(j)
                    queue.append(j)
    return order


def ordered(atoms, bonds):
    """(atoms, bonds) in the caller's order, `bonds` a dict {(i, j): qbond} in either direction -> (atoms in matching
    order, {(k, q): qbond} with q < k, order: position -> the caller's index)."""
    order = matching_order(len(atoms), set(bonds))
    pos = {a: k for k, a in enumerate(order)}
    return ([atoms[a] for a in order],
            {(max(pos[i], pos[j]), min(pos[i], pos[j])): spec for (i, j), spec in bonds.items()}, order)


def connected_without(adj, n, i, j):
    """Whether i and j stay connected when their bond is removed."""
    seen, todo = {i}, [i]
    while todo:
        a = todo.pop()
        for c in range(n):
            if adj[a][c] and c not in seen and {a, c} != {i, j}:
                seen.add(c)
                todo.append(c)
    return j in seen


def derive(z, adj, n, nh=None):
    """deg, arom, ring per atom, ring_bond per pair, nh per atom (given, or max(0, (2 v0 - v2) / 2))."""
    deg = [sum(1 for c in adj[a] if c) for a in range(n)]
    arom = [4 in adj[a] for a in range(n)]
    ring_bond = [[bool(adj[a][c]) and connected_without(adj, n, a, c) for c in range(n)] for a in range(n)]
    ring = [any(ring_bond[a]) for a in range(n)]
    if nh is None:
        nh = [max(0, (2 * V0.get(z[a], 0) - sum(V2[c] for c in adj[a])) // 2) for a in range(n)]
    return deg, arom, ring, ring_bond, list(nh)


class _OverBudget(Exception):
    pass


def match(mol, atoms, bonds, nh=None, budget=NODE_BUDGET, ring_test=True, injective=True, code_mask=True):
    """count, status, first (m atoms, or None), covered (a set) and nodes (per root) of one pattern in matching order in one
    molecule.  `ring_test` / `injective` / `code_mask` = False are the mutants of the mutation checks."""
    z, adj, n = mol
    m = len(atoms)
    deg, arom, ring, ring_bond, nh = derive(z, adj, n, nh)

    def tri(want, have):
        return want is None or want == have

    def atom_ok(k, a):
        q = atoms[k]
        return (q["z"] is None or z[a] in q["z"]) and q["dmin"] <= deg[a] <= q["dmax"] and \
            q["hmin"] <= nh[a] <= q["hmax"] and tri(q["ring"], ring[a]) and tri(q["arom"], arom[a])

    def bond_ok(spec, a, c):
        codes, want = spec
        if not adj[a][c]:
            return False
        if code_mask and adj[a][c] not in codes:
            return False
        return not ring_test or tri(want, ring_bond[a][c])

    out = dict(count=0, status=0, first=None, covered=set(), nodes=[])
    for r in range(n if m else 0):                  # a pattern without atoms matches nothing
        state = dict(nodes=0)
        image = []

        def descend(k):
            for v in range(n) if k else [r]:
                if injective and v in image:
                    continue
                if not atom_ok(k, v):
                    continue
                if not all(bond_ok(bonds[(k, q)], v, image[q]) for q in range(k) if (k, q) in bonds):
                    continue
                if state["nodes"] == budget:
                    raise _OverBudget()
                state["nodes"] += 1
                image.append(v)
                if k == m - 1:
                    out["count"] += 1
                    out["covered"].update(image)
                    if out["first"] is None:
                        out["first"] = list(image)
                else:
                    descend(k + 1)
                image.pop()
        try:
            descend(0)
        except _OverBudget:
            out["status"] = BUDGET
        out["nodes"].append(state["nodes"])
    return out


def covered_mask(atoms_set):
    return sum(1 << a for a in atoms_set)
