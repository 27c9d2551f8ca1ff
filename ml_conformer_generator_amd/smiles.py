"""SMILES of a heavy-atom molecular graph, written on the host ("Canonical graphs and SMILES").

THE PACKAGE'S OWN, LABELLED DEFINITION: the output is valid OpenSMILES, and with the graph in the order of
`canonical.canonical_graphs` it is this package's canonical string - it is NOT RDKit's canonical SMILES, and no string
equality with any toolkit is claimed.  No stereochemistry, no charges, no isotopes; no reader.

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
The "[nH]" of an imidazole-type ring may sit on the other N than the hydrogen `hydrogens.add_hydrogens` placed on the same
record: that kernel applies its lowest-index rule to the record's own atom order, the writer to the canonical one - a
tautomer-level difference between two of the package's own rules.
"""
from __future__ import annotations

from typing import List

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


def write_smiles(atomic_numbers, bond_orders) -> str:
    """The SMILES string of one heavy-atom graph by this module's definition: `atomic_numbers` [n], `bond_orders` [n,n]
    symmetric codes 0 none / 1 / 2 / 3 / 4 aromatic (the diagonal is ignored), atoms in whatever order they are given -
    the canonical string when that is the canonical order.  Pure Python, no device.  ValueError: codes that are not
    integers 0..4 or not symmetric, an atomic number < 1 or without a symbol, more than 99 ring closures open at once, and
    - `hydrogens.implicit_counts`' limit - more than 64 atoms in a graph that needs a bracket atom."""
    z, adj, n = _graph(atomic_numbers, bond_orders)
    if n == 0:
        return ""
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
        if z[a] in _ORGANIC:
            sym = _ORGANIC[z[a]]
            if lower[a]:
                return "[nH]" if z[a] == 7 and hyd[a] == 1 else sym.lower()
            return sym
        sym = Z_TO_SYMBOL[z[a]]
        h = hyd[a]
        return "[" + (sym.lower() if lower[a] else sym) + ("" if h == 0 else "H" if h == 1 else f"H{h}") + "]"

    def bond_text(a: int, b: int) -> str:
        code, both = adj[a][b], lower[a] and lower[b]
        if code == 1:
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
                out.append(bond_text(j, a) + _closure_number(k))
                free.append(k)
                free.sort(reverse=True)
            for j in sorted(opens[a]):
                if not free:
                    raise ValueError(f"more than {MAX_OPEN_CLOSURES} ring closures are open at once: SMILES has no "
                                     "number for the next one")
                number[(a, j)] = free.pop()
                out.append(_closure_number(number[(a, j)]))
            kids = children[a]
            for pos in range(len(kids) - 1, -1, -1):           # pushed in reverse: the first child is written first
                if pos < len(kids) - 1:
                    todo.append((")", -1, -1))
                todo.append(("atom", kids[pos], a))
                if pos < len(kids) - 1:
                    todo.append(("(", -1, -1))
    return "".join(out)
