"""Plain-Python restatement of the standardised-graph definition ("Standardised graphs"), written from
its words and not from the kernel: recursion where the kernel keeps a stack, sets and lists where it keeps masks.  Plus
an independent checker, `matching_exists`, that answers "is there a Kekule form at all" by enumerating every matching
of a small eligible graph - it knows nothing of the search order.

A molecule is (z, codes, n): atomic numbers, an n x n list of bond codes, the atom count.  `standardize` returns a dict
of plain lists and ints; `MUTATIONS` names the deliberate mis-readings the host tests switch on one at a time."""
import itertools
import sys

EMPTY, OVER_VALENCE, AROMATIC_BRIDGE, NOT_KEKULIZABLE, SEARCH_BUDGET = 1, 2, 4, 8, 16
KEKULE_BUDGET = 16384
V0 = {5: 3, 6: 4, 7: 3, 8: 2, 9: 1, 14: 4, 15: 3, 16: 2, 17: 1, 33: 3, 34: 2, 35: 1, 53: 1}
OPTIONAL_Z = (7, 15, 33)
# the validity proxy's maximum valence (csrc/mcg_elements.h), written out again
MAX_VALENCE = {5: 3, 6: 4, 7: 4, 8: 2, 9: 1, 14: 4, 15: 5, 16: 6, 17: 1, 33: 5, 34: 6, 35: 1}
HALF_BONDS = {1: 2, 2: 4, 3: 6, 4: 2}          # an aromatic bond counts its sigma bond here: the Kekule search places the rest
MUTATIONS = ("lowest_first", "no_optional", "no_tie_break")


class _Budget(Exception):
    pass


def clean(codes, n):
    """The n x n codes with the diagonal and every value outside 1..4 read as no bond."""
    return [[codes[i][j] if i != j and codes[i][j] in (1, 2, 3, 4) else 0 for j in range(n)] for i in range(n)]


def components(nbrs, atoms):
    """The connected components of `atoms` under `nbrs` (atom -> set), each a sorted list, in order of lowest member."""
    seen, out = set(), []
    for s in sorted(atoms):
        if s in seen:
            continue
        comp, todo = {s}, [s]
        while todo:
            for j in nbrs[todo.pop()]:
                if j in atoms and j not in comp:
                    comp.add(j)
                    todo.append(j)
        seen |= comp
        out.append(sorted(comp))
    return out


def _search(comp, nbrs, optional, mutate):
    """The Kekule search of one component of the eligible graph: ({atom: partner}, steps) or (None, steps); _Budget."""
    matched, skipped, steps = {}, set(), [0]
    pick = min if mutate == "lowest_first" else max

    def go():
        steps[0] += 1
        if steps[0] > KEKULE_BUDGET:
            raise _Budget()
        left = [a for a in comp if a not in matched and a not in skipped]
        if not left:
            return True
        a = pick(left)
        for p in sorted((j for j in nbrs[a] if j not in matched and j not in skipped),
                        reverse=mutate != "lowest_first"):
            matched[a], matched[p] = p, a
            if go():
                return True
            del matched[a], matched[p]
        if a in optional and mutate != "no_optional":
            skipped.add(a)
            if go():
                return True
            skipped.discard(a)
        return False

    return (dict(matched), steps[0]) if go() else (None, steps[0])


def eligible_graph(z, c, atoms):
    """(eligible atoms, optional ones, {atom: eligible code-4 neighbours}) of the atoms `atoms` with cleaned codes c."""
    elig = set()
    for a in atoms:
        sigma = sum(v if v in (1, 2, 3) else 1 if v == 4 else 0 for v in c[a])
        if 4 in c[a] and V0.get(z[a], 0) - sigma >= 1:
            elig.add(a)
    nbrs = {a: {j for j in elig if c[a][j] == 4} for a in elig}
    return elig, {a for a in elig if z[a] in OPTIONAL_Z}, nbrs


def standardize(z, codes, n, coords=None, mutate=None):
    """The definition applied to one molecule.  `coords`: n rows of anything, copied through untouched."""
    assert mutate is None or mutate in MUTATIONS
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    c = clean(codes, n)
    nbrs = {a: {j for j in range(n) if c[a][j]} for a in range(n)}
    frags = components(nbrs, set(range(n)))
    if mutate == "no_tie_break":
        key = lambda f: (-len(f), f[0])                                     # noqa: E731
    else:
        key = lambda f: (-len(f), -sum(z[a] for a in f), f[0])              # noqa: E731
    keep = sorted(frags, key=key)[0] if frags else []
    m = len(keep)
    new = {a: r for r, a in enumerate(keep)}
    out = dict(n_out=m, atom_map=list(keep), n_fragments=len(frags), atoms_removed=n - m,
               atomic_numbers=[z[a] for a in keep], bond_orders=[[c[a][b] for b in keep] for a in keep],
               coords=None if coords is None else [coords[a] for a in keep], steps=[])
    status = EMPTY if n == 0 else 0
    for a in keep:
        if sum(HALF_BONDS.get(v, 0) for v in c[a]) > 2 * MAX_VALENCE.get(z[a], 0):
            status |= OVER_VALENCE
    for a in keep:
        for b in keep:
            if a < b and c[a][b] == 4:
                cut = {k: nbrs[k] - ({b} if k == a else {a} if k == b else set()) for k in keep}
                side = next(f for f in components(cut, set(keep)) if a in f)
                if b not in side:                         # without the bond its ends fall apart: it lies in no ring
                    status |= AROMATIC_BRIDGE
    partner = {}
    if status == 0:
        elig, optional, enbrs = eligible_graph(z, c, keep)
        for comp in components(enbrs, elig):
            try:
                found, steps = _search(comp, enbrs, optional, mutate)
                out["steps"].append(steps)
                if found is None:
                    status |= NOT_KEKULIZABLE
                else:
                    partner.update(found)
            except _Budget:
                out["steps"].append(KEKULE_BUDGET + 1)
                status |= SEARCH_BUDGET
    out["status"] = status
    if status == 0:
        out["kekule_orders"] = [[(2 if partner.get(a) == b else 1) if c[a][b] == 4 else c[a][b] for b in keep] for a in keep]
    else:
        out["kekule_orders"] = [[0] * m for _ in range(m)]
    out["doubles"] = sorted({(min(new[a], new[p]), max(new[a], new[p])) for a, p in partner.items()}) if status == 0 else None
    return out


def matching_exists(z, codes, n, keep=None):
    """Brute force, no search order: does every component of the eligible graph of the atoms `keep` (default: all) have a
    matching that covers all its required atoms?  Every subset of the edges is looked at."""
    c = clean(codes, n)
    atoms = list(range(n)) if keep is None else list(keep)
    elig, optional, nbrs = eligible_graph(z, c, atoms)
    required = elig - optional
    edges = sorted({(min(a, b), max(a, b)) for a in elig for b in nbrs[a]})
    by_atom = {a: [e for e in edges if a in e] for a in elig}

    def cover(todo, used):
        """Can the required atoms in `todo` all be matched, given the atoms already `used`?"""
        todo = [a for a in todo if a not in used]
        if not todo:
            return True
        a = todo[0]
        return any(cover(todo[1:], used | set(e)) for e in by_atom[a] if not used & set(e))

    if len(edges) <= 16:                                  # small enough: literally every subset of the edges
        for k in range(len(edges) + 1):
            for pick in itertools.combinations(edges, k):
                ends = [a for e in pick for a in e]
                if len(ends) == len(set(ends)) and required <= set(ends):
                    return True
        return False
    return cover(sorted(required), frozenset())
