"""The restatement of DESIGN.md section 6, "Rings and scaffolds", in plain Python over adjacency sets - by DIFFERENT
algorithms than `csrc/mcg_scaffold.hip`, so that agreement means something:
  ring bonds    bridge finding (depth-first search, low-link): a bond is a ring bond iff it is no bridge - the kernel
                floods once per bond with the bond left out.  `flood_ring_bonds` restates the kernel's rule as a second form.
  linker atoms  the closed form: a non-ring atom is a linker iff removing it leaves ring atoms in at least two components
                of its fragment - the kernel prunes.  `pruned_core` is the pruning form.
  ring sizes    breadth-first search per ring bond with the bond left out.
A molecule is (z, adj, n) as in `canonical_ref`.  `perceive(mol, form=..., mutate=...)`: `form` "closed" (bridges + closed
form) or "pruning" (flood + pruning); `mutate` plants one mistake (`MUTATIONS`) for the tests that show the named cases can
see what they pin."""
import canonical_ref as R

MUTATIONS = ("flood_keeps_bond", "prune_one_round", "exo_code_1", "split_spiro")
COUNT_NAMES = ("n_rings", "n_ring_systems", "min_ring_size", "max_ring_size", "ring_atoms", "linker_atoms", "exo_atoms",
               "ring_bonds")


def neighbours(adj, n):
    return [{j for j in range(n) if j != a and 1 <= adj[a][j] <= 4} for a in range(n)]


def bridge_ring_bonds(nb, n):
    """{(a, j), a < j}: the bonds that are no bridges.  Iterative DFS with low-link values."""
    disc, low, up = [-1] * n, [0] * n, [-1] * n
    clock = 0
    for root in range(n):
        if disc[root] >= 0:
            continue
        disc[root] = low[root] = clock
        clock += 1
        stack = [(root, -1, iter(sorted(nb[root])))]
        while stack:
            a, parent, it = stack[-1]
            for j in it:
                if j == parent:
                    continue
                if disc[j] >= 0:
                    low[a] = min(low[a], disc[j])
                else:
                    disc[j] = low[j] = clock
                    up[j] = a
                    clock += 1
                    stack.append((j, a, iter(sorted(nb[j]))))
                    break
            else:
                stack.pop()
                if parent >= 0:
                    low[parent] = min(low[parent], low[a])
    # the tree bond (parent[j], j) is a bridge iff nothing below j reaches parent[j] or above; a non-tree bond closes a cycle
    bridges = {(min(up[j], j), max(up[j], j)) for j in range(n) if up[j] >= 0 and low[j] > disc[up[j]]}
    return {(a, j) for a in range(n) for j in nb[a] if a < j} - bridges


def _reachable(nb, start, banned_bond=None, banned_atom=None):
    seen, todo = {start}, [start]
    while todo:
        a = todo.pop()
        for j in nb[a]:
            if j in seen or j == banned_atom or banned_bond in ((a, j), (j, a)):
                continue
            seen.add(j)
            todo.append(j)
    return seen


def flood_ring_bonds(nb, n, keep_bond=False):
    """The kernel's rule: (a, j) is a ring bond iff j is reachable from a with that bond left out.  `keep_bond`: the planted
    mistake - the bond is not left out."""
    return {(a, j) for a in range(n) for j in nb[a] if a < j
            and j in _reachable(nb, a, None if keep_bond else (a, j))}


def bond_size(nb, a, j):
    """The smallest cycle through ring bond (a, j): BFS from a to j with the bond left out, plus 1."""
    dist, level = {a: 0}, [a]
    while level:
        nxt = []
        for u in level:
            for v in nb[u]:
                if v in dist or (u == a and v == j):
                    continue
                dist[v] = dist[u] + 1
                if v == j:
                    return dist[v] + 1
                nxt.append(v)
        level = nxt
    raise AssertionError("not a ring bond")


def components(atoms, bonds):
    """{atom: lowest atom of its component} over the given atoms and bonds."""
    label = {a: a for a in atoms}
    changed = True
    while changed:
        changed = False
        for a, j in bonds:
            low = min(label[a], label[j])
            if label[a] != low or label[j] != low:
                label[a] = label[j] = low
                changed = True
    return label


def pruned_core(nb, n, one_round=False):
    """The atoms that remain when every atom with fewer than two remaining neighbours is removed, as long as one exists.
    `one_round`: the planted mistake - it stops after one round."""
    alive = set(range(n))
    while True:
        gone = {a for a in alive if len(nb[a] & alive) < 2}
        if not gone:
            return alive
        alive -= gone
        if one_round:
            return alive


def closed_form_linkers(nb, n, ring_atoms):
    """A non-ring atom is a linker iff removing it leaves ring atoms in at least two components of its fragment."""
    out = set()
    for a in range(n):
        if a in ring_atoms or not nb[a]:
            continue
        sides = 0
        seen = set()
        for j in sorted(nb[a]):
            if j in seen:
                continue
            part = _reachable(nb, j, banned_atom=a)
            seen |= part
            sides += 1 if part & ring_atoms else 0
        if sides >= 2:
            out.add(a)
    return out


def _mask(atoms):
    return sum(1 << a for a in atoms)


def perceive(z, adj, n, form="closed", mutate=None):
    """dict(ring_nb [n] masks, ring_size [n], ring_system [n], masks [ring, linker, exo, scaffold], counts [8]) of one
    molecule, as the kernel writes them for its real atoms."""
    assert form in ("closed", "pruning") and mutate in (None,) + MUTATIONS
    nb = neighbours(adj, n)
    if form == "pruning" or mutate == "flood_keeps_bond":
        ring_bonds = flood_ring_bonds(nb, n, keep_bond=mutate == "flood_keeps_bond")
    else:
        ring_bonds = bridge_ring_bonds(nb, n)
    ring_nb = [0] * n
    for a, j in ring_bonds:
        ring_nb[a] |= 1 << j
        ring_nb[j] |= 1 << a
    ring_atoms = {a for a in range(n) if ring_nb[a]}
    sizes = {}
    for a, j in ring_bonds:
        sizes[(a, j)] = 2 if mutate == "flood_keeps_bond" else bond_size(nb, a, j)
    ring_size = [min([s for (u, v), s in sizes.items() if a in (u, v)], default=0) for a in range(n)]
    if mutate == "split_spiro":                  # the planted mistake: a system ends at an atom with four ring bonds
        hubs = {a for a in ring_atoms if bin(ring_nb[a]).count("1") >= 4}
        label = components(ring_atoms - hubs, [(a, j) for a, j in ring_bonds if a not in hubs and j not in hubs])
        for h in hubs:
            label[h] = h
    else:
        label = components(ring_atoms, ring_bonds)
    ring_system = [label.get(a, -1) for a in range(n)]
    n_systems = len(set(label.values()))
    if form == "pruning" or mutate == "prune_one_round":
        linkers = pruned_core(nb, n, one_round=mutate == "prune_one_round") - ring_atoms
    else:
        linkers = closed_form_linkers(nb, n, ring_atoms)
    core = ring_atoms | linkers
    exo_codes = (1, 2) if mutate == "exo_code_1" else (2,)
    exo = {a for a in range(n) if a not in core and any(adj[a][j] in exo_codes for j in nb[a] & core)}
    counts = [len(ring_bonds) - len(ring_atoms) + n_systems, n_systems, min(sizes.values(), default=0),
              max(sizes.values(), default=0), len(ring_atoms), len(linkers), len(exo), len(ring_bonds)]
    return dict(ring_nb=ring_nb, ring_size=ring_size, ring_system=ring_system,
                masks=[_mask(ring_atoms), _mask(linkers), _mask(exo), _mask(core | exo)], counts=counts)


def induced(z, adj, n, mask, mode=0):
    """(z', adj', n', atom_map): the sub-graph of the atoms in `mask` (bits at and beyond n ignored), ascending, compacted;
    mode 1 writes Z = 6 and code 1; a value that is no code is written as 0."""
    keep = [a for a in range(n) if mask >> a & 1]
    def code(a, j):
        c = adj[a][j] if a != j and 1 <= adj[a][j] <= 4 else 0
        return (1 if c else 0) if mode == 1 else c
    return ([6 if mode == 1 else z[a] for a in keep], [[code(a, j) for j in keep] for a in keep], len(keep), keep)


def scaffold(z, adj, n, generic=False, perceived=None):
    """(z', adj', n', atom_map) of the scaffold (`generic`: the framework) of one molecule."""
    p = perceived or perceive(z, adj, n)
    mask = (p["masks"][0] | p["masks"][1]) if generic else p["masks"][3]
    return induced(z, adj, n, mask, 1 if generic else 0)


def identity(z, adj, n, generic=False):
    """The scaffold's identity bytes (`canonical_ref.identity_bytes`); b"" for the empty scaffold."""
    sz, sadj, sn, _ = scaffold(z, adj, n, generic)
    return b"" if sn == 0 else R.identity_bytes(sz, sadj, sn)


def permuted(out, p):
    """`perceive`'s result as it must read for the molecule with new atom k = old atom p[k]."""
    inv = {old: new for new, old in enumerate(p)}
    def mask(m):
        return sum(1 << inv[a] for a in range(len(p)) if m >> a & 1)
    groups = {}
    for new, old in enumerate(p):
        if out["ring_system"][old] >= 0:
            groups.setdefault(out["ring_system"][old], []).append(new)
    low = {label: min(members) for label, members in groups.items()}
    return dict(ring_nb=[mask(out["ring_nb"][old]) for old in p], ring_size=[out["ring_size"][old] for old in p],
                ring_system=[low.get(out["ring_system"][old], -1) for old in p],
                masks=[mask(m) for m in out["masks"]], counts=list(out["counts"]))
