"""SMILES of a heavy-atom molecular graph, written on the host ("Canonical graphs and SMILES").

THE PACKAGE'S OWN, LABELLED DEFINITION: the output is valid OpenSMILES, and with the graph in the order of
`canonical.canonical_graphs` it is this package's canonical string - it is NOT RDKit's canonical SMILES, and no string
equality with any toolkit is claimed.  No charges, no isotopes; no reader.  Stereochemistry only where the caller hands
in the descriptors of `stereo.py` (`stereo=`, below); without them the string is the constitution's.

Traversal   components in ascending order of their lowest atom, joined with "."; depth-first from that atom, neighbours
            in ascending index; all children but the last in parentheses; a back edge is a ring closure, opened at the
            ancestor.
At an atom  first the closures ending here, in ascending order of the opening atom, the bond symbol at this closing end,
            each number becoming free; then the closures opening here, in ascending order of the closing atom, each
            taking the lowest free number: 1..9, then %10..%99.  More than 99 open at once: ValueError.
Lowercase   an atom is written lowercase if and only if its element is B, C, N, O, P or S and it has a code-4 bond.
Bonds       code 1: nothing, or "-" between two lowercase atoms; 2: "="; 3: "#"; 4: nothing between two lowercase atoms,
            else ":".
Brackets    in exactly two cases, both with the count h of `hydrogens.implicit_counts` on the graph AS GIVEN (on a
            canonical graph its lowest-index rule is therefore the lowest canonical position): an aromatic N with h = 1
            is "[nH]"; an element outside B C N O P S F Cl Br I is "[Sym]", "[SymH]" or "[SymHh]", Se and As with a
            code-4 bond lowercase inside the bracket (and lowercase for the bond symbols).  Everything else is bare: its
            hydrogens are whatever the reader's valence model implies.
Isomeric    `stereo[k]` = 4 tet + db of atom k (`stereo.py`), RELATIVE TO THE NUMBERING THE GRAPH IS GIVEN IN: tet 1 / 2 =
            the handedness of k's neighbours in ascending index (the implicit H last), db 1 cis / 2 trans of the lowest
            substituents of the two ends, stored at the end of larger index.  A defined tetrahedral atom becomes a
            bracket atom, "[C@]", "[C@@H]", "[Si@H]" ...: looking from the first neighbour, the remaining three
            anticlockwise is "@" (OpenSMILES); the neighbour order is the writer's own - the preceding atom, the implicit
            H, the ring-closure digits in the order written (the closures ending here, then the ones opening here), then
            the branches - and the mark follows from the parity of that order against the ascending one.  A defined
            double bond gets "/" or "\\" on ONE single bond per end: a tree edge where the end has one (the lowest
            substituent first), a ring-closure bond only otherwise - the symbol then stands at the OPENING digit.  The
            double bonds are taken in ascending order of their storing atom, those that share a single bond with one
            already written directly behind it: the shared bond's direction is reused and the other end fitted to it.
            Where both ends are already fixed and contradict the descriptor, the double bond gets no mark of its own
            and is counted (`write_smiles_counted`): the string is then not faithful at that bond.  Marks may sit on
            centres that are not stereogenic by a reader's own rules (3-pentanol's C3): a reader ignores them there.
The "[nH]" of an imidazole-type ring may sit on the other N than the hydrogen `hydrogens.add_hydrogens` placed on the same
record: that kernel applies its lowest-index rule to the record's own atom order, the writer to the canonical one - a
tautomer-level difference between two of the package's own rules.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .elements import Z_TO_SYMBOL

_ORGANIC = {5: "B", 6: "C", 7: "N", 8: "O", 15: "P", 16: "S", 9: "F", 17: "Cl", 35: "Br", 53: "I"}
_AROMATIC = (5, 6, 7, 8, 15, 16)
_BRACKET_AROMATIC = (33, 34)     # As, Se: lowercase inside their bracket
MAX_OPEN_CLOSURES = 99


def _graph(atomic_numbers, bond_orders):
    z = [int(v) for v in torch.as_tensor(atomic_numbers).reshape(-1).tolist()]
    c = torch.as_tensor(bond_orders)
    n = len(z)
    if c.dim() != 2 or tuple(c.shape) != (n, n) or c.dtype.is_floating_point or c.dtype == torch.bool:
        raise ValueError(f"bond_orders must be integer codes [{n},{n}], got {list(c.shape)} of type {c.dtype}")
    codes = c.cpu().to(torch.int64)
    if n and (int(codes.min()) < 0 or int(codes.max()) > 4 or not torch.equal(codes, codes.t())):
        raise ValueError("bond_orders must be symmetric with codes 0 none / 1 / 2 / 3 / 4 aromatic")
    if any(v < 1 for v in z):
        raise ValueError(f"atomic numbers must be >= 1, got {min(z)}")
    adj = codes.tolist()
    for a in range(n):
        adj[a][a] = 0
    return z, adj, n


def _closure_number(k: int) -> str:
    return str(k) if k < 10 else "%" + str(k)


def write_smiles(atomic_numbers, bond_orders, stereo: Optional[Sequence[int]] = None) -> str:
    """The SMILES string of one heavy-atom graph by this module's definition: `atomic_numbers` [n], `bond_orders` [n,n]
    symmetric codes 0 none / 1 / 2 / 3 / 4 aromatic (the diagonal is ignored), atoms in whatever order they are given -
    the canonical string when that is the canonical order.  `stereo` [n]: 4 tet + db per atom relative to the given
    numbering (the module text, "Isomeric"; `stereo.stereo_order`'s `stereo` row for a graph in canonical order,
    `stereo.own_order_descriptors` for a record's own order) - the isomeric string; None: unchanged.  Pure Python, no
    device.  ValueError: codes that are not integers 0..4 or not symmetric, an atomic number < 1 or without a symbol,
    more than 99 ring closures open at once, `stereo` of another length, and - `hydrogens.implicit_counts`' limit - more
    than 64 atoms in a graph that needs a bracket atom."""
    return write_smiles_counted(atomic_numbers, bond_orders, stereo)[0]


def _sides(n, adj, stereo, pos, tree_edge) -> Tuple[dict, int]:
    """({(earlier-written atom, later-written atom): "/" or "\\"}, the double bonds left without a mark of their own)."""
    bonds = []
    for a in range(n):
        if stereo[a] & 3:
            (b,) = [j for j in range(a) if adj[a][j] == 2][:1] or [None]
            if b is not None:
                bonds.append((b, a, stereo[a] & 3))
    marks, unmarked = {}, 0

    def subs(c, other):
        return [j for j in range(n) if adj[c][j] == 1 and j != other]

    def side_of(c, sub):                                   # +1: sub is "up" from c, by the symbol already on the bond
        key = (sub, c) if pos[sub] < pos[c] else (c, sub)
        sym = marks.get(key)
        if sym is None:
            return None
        return (1 if sym == "/" else -1) * (1 if key[0] == c else -1)

    def put(c, sub, side):
        key = (sub, c) if pos[sub] < pos[c] else (c, sub)
        marks[key] = "/" if side * (1 if key[0] == c else -1) > 0 else "\\"

    def end_state(c, other):
        """(side of the LOWEST substituent fixed by marks already there or None, the substituent to mark if free,
        consistent)."""
        ss = subs(c, other)
        fixed = [(1 if k == 0 else -1) * side_of(c, j) for k, j in enumerate(ss) if side_of(c, j) is not None]
        if fixed:
            return fixed[0], None, len(set(fixed)) == 1
        tree = [j for j in ss if tree_edge(c, j)]
        return None, (tree or ss)[0], True

    todo = sorted(bonds, key=lambda t: t[1])
    while todo:
        nxt = next((t for t in todo if any(side_of(c, j) is not None for c, o in ((t[0], t[1]), (t[1], t[0]))
                                            for j in subs(c, o))), todo[0])
        todo.remove(nxt)
        a, b, d = nxt
        want = 1 if d == 1 else -1                         # the product of the sides of the two lowest substituents
        fa, pa, oka = end_state(a, b)
        fb, pb, okb = end_state(b, a)
        if not (oka and okb) or (fa is not None and fb is not None and fa * fb != want):
            unmarked += 1
            continue
        if fa is None and fb is None:
            fa = -1 if pos[pa] < pos[a] else 1             # the first mark of a system is written "/"
            fa *= 1 if pa == subs(a, b)[0] else -1
        if fa is None:
            fa = want * fb
        if fb is None:
            fb = want * fa
        if pa is not None:
            put(a, pa, fa * (1 if pa == subs(a, b)[0] else -1))
        if pb is not None:
            put(b, pb, fb * (1 if pb == subs(b, a)[0] else -1))
    return marks, unmarked


def write_smiles_counted(atomic_numbers, bond_orders, stereo: Optional[Sequence[int]] = None) -> Tuple[str, int]:
    """(`write_smiles`' string, the defined double bonds that got no mark of their own - 0 without `stereo`)."""
    z, adj, n = _graph(atomic_numbers, bond_orders)
    if stereo is not None:
        stereo = [int(v) for v in stereo]
        if len(stereo) != n:
            raise ValueError(f"stereo must hold one descriptor per atom ({n}), got {len(stereo)}")
    if n == 0:
        return "", 0
    nbrs = [[j for j in range(n) if adj[a][j] != 0] for a in range(n)]
    has4 = [any(adj[a][j] == 4 for j in nbrs[a]) for a in range(n)]
    lower = [has4[a] and (z[a] in _AROMATIC or z[a] in _BRACKET_AROMATIC) for a in range(n)]
    for v in z:
        if v not in _ORGANIC and v not in Z_TO_SYMBOL:
            raise ValueError(f"atomic number {v} has no symbol in this package")
    hyd = None
    if any((z[a] == 7 and lower[a]) or z[a] not in _ORGANIC for a in range(n)):
        from .hydrogens import implicit_counts
        hyd = implicit_counts(torch.tensor([z], dtype=torch.int32), torch.tensor([adj], dtype=torch.int8),
                              torch.tensor([n], dtype=torch.int32))[0].tolist()

    def atom_text(a: int) -> str:
        if a in chiral:
            return "[" + (_ORGANIC.get(z[a]) or Z_TO_SYMBOL[z[a]]) + chiral[a] + ("H" if len(nbrs[a]) == 3 else "") + "]"
        if z[a] in _ORGANIC:
            sym = _ORGANIC[z[a]]
            if lower[a]:
                return "[nH]" if z[a] == 7 and hyd[a] == 1 else sym.lower()
            return sym
        sym = Z_TO_SYMBOL[z[a]]
        h = hyd[a]
        return "[" + (sym.lower() if lower[a] else sym) + ("" if h == 0 else "H" if h == 1 else f"H{h}") + "]"

    def bond_text(a: int, b: int, closing: bool = False) -> str:
        code, both = adj[a][b], lower[a] and lower[b]
        if code == 1:
            if (a, b) in marks and not closing:        # a closure's direction stands at its opening digit
                return marks[(a, b)]
            return "-" if both else ""
        if code == 4:
            return "" if both else ":"
        return "=" if code == 2 else "#"

    # pass 1: the depth-first tree and its back edges
    visited = [False] * n
    children: List[List[int]] = [[] for _ in range(n)]
    opens: List[List[int]] = [[] for _ in range(n)]            # opens[ancestor]: the atoms that close a ring to it
    closes: List[List[int]] = [[] for _ in range(n)]           # closes[descendant]: the ancestors it closes a ring to
    roots = []
    for root in range(n):
        if visited[root]:
            continue
        roots.append(root)
        visited[root] = True
        stack = [(root, -1, 0)]                                # (atom, parent, position in its neighbour list)
        while stack:
            a, parent, k = stack.pop()
            if k == len(nbrs[a]):
                continue
            stack.append((a, parent, k + 1))
            j = nbrs[a][k]
            if not visited[j]:
                visited[j] = True
                children[a].append(j)
                stack.append((j, a, 0))
            elif j != parent and j not in children[a] and a not in opens[j] and j not in opens[a]:
                opens[j].append(a)                             # j was reached first: the ancestor
                closes[a].append(j)

    # the stereo marks: from the tree, before anything is written
    chiral, marks, unmarked = {}, {}, 0
    if stereo is not None and any(stereo):
        pos, parent_of, count = [0] * n, [-1] * n, 0
        walk = list(reversed(roots))
        while walk:
            a = walk.pop()
            pos[a], count = count, count + 1
            for j in reversed(children[a]):
                parent_of[j] = a
                walk.append(j)
        marks, unmarked = _sides(n, adj, stereo, pos, lambda c, j: parent_of[c] == j or parent_of[j] == c)
        for a in range(n):
            tet = stereo[a] >> 2
            if tet in (1, 2) and len(nbrs[a]) in (3, 4):
                written = ([parent_of[a]] if parent_of[a] >= 0 else []) + ([n] if len(nbrs[a]) == 3 else []) + \
                    sorted(closes[a]) + sorted(opens[a]) + children[a]          # n: the implicit H, last in ascending order
                odd = sum(1 for i in range(4) for j in range(i) if written[j] > written[i]) & 1
                chiral[a] = "@" if (tet == 1) != bool(odd) else "@@"

    # pass 2: the string
    free = list(range(MAX_OPEN_CLOSURES, 0, -1))               # popped from the end: the lowest free number
    number = {}
    out: List[str] = []
    for r, root in enumerate(roots):
        if r:
            out.append(".")
        todo = [("atom", root, -1)]
        while todo:
            kind, a, parent = todo.pop()
            if kind != "atom":
                out.append(kind)
                continue
            if parent >= 0:
                out.append(bond_text(parent, a))
            out.append(atom_text(a))
            for j in sorted(closes[a]):
                k = number.pop((j, a))
                out.append(bond_text(j, a, closing=True) + _closure_number(k))
                free.append(k)
                free.sort(reverse=True)
            for j in sorted(opens[a]):
                if not free:
                    raise ValueError(f"more than {MAX_OPEN_CLOSURES} ring closures are open at once: SMILES has no "
                                     "number for the next one")
                number[(a, j)] = free.pop()
                out.append(marks.get((a, j), "") + _closure_number(number[(a, j)]))
            kids = children[a]
            for pos in range(len(kids) - 1, -1, -1):           # pushed in reverse: the first child is written first
                if pos < len(kids) - 1:
                    todo.append((")", -1, -1))
                todo.append(("atom", kids[pos], a))
                if pos < len(kids) - 1:
                    todo.append(("(", -1, -1))
    return "".join(out), unmarked
