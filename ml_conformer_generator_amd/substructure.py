"""Substructure patterns matched against molecular graphs, on the GPU ("Substructure patterns"):
whether, how often and where a molecule contains a given piece - behind `require_substructures=`,
`exclude_substructures=` and `substructure_counts=`.

THE PACKAGE'S OWN, LABELLED DEFINITION: a small query-graph language and a subgraph-monomorphism search, exact in integers.
Not RDKit's `HasSubstructMatch`, not full SMARTS, and no agreement with any toolkit is claimed.
  molecule   atomic numbers Z, symmetric bond codes 0 none / 1 / 2 / 3 / 4 aromatic, n <= 64 atoms, no degree cap.  Per
             atom: deg (bonded atoms), arom (it has a code-4 bond), ring (it has a ring bond), nh (its hydrogens: an
             optional input; absent, max(0, (2 v0 - v2) / 2) - the count rule without the aromatic N-H).  A bond is a
             ring bond iff its two ends stay connected when it is removed.
  pattern    1 <= m <= 32 query atoms - an element set (Z <= 53, or any), dmin <= deg <= dmax, hmin <= nh <= hmax, ring
             any / yes / no, aromatic any / yes / no - and query bonds between them - a set of allowed codes and ring
             any / ring bond / chain bond.  Atom pairs without a query bond are unconstrained (monomorphism, as SMARTS has
             it, not an induced subgraph); disconnected patterns are allowed.
  order      the matching order (`matching_order`): per component breadth-first from its lowest-index atom, neighbours in
             ascending index, components in ascending order of their lowest atom.  The kernel gets the pattern in that
             order; `first` is mapped back to the caller's atom indices here.
  embedding  an injective map of the positions to atoms that satisfies every query atom and lands every query bond on a
             bond whose code and ring state are allowed.
  search     per root atom r ascending: position 0 takes r; position k then every atom, ascending, that is unused, in
             k's domain and rightly bonded to the image of every earlier position k has a query bond with.  Each accepted
             assignment is a node; ALL embeddings are enumerated.
  budget     at most NODE_BUDGET = 65 536 nodes per (molecule, pattern, root): a root that would take one more stops and
             the pair gets status BUDGET.  The tree of a root is walked completely, so whether it fits depends on the
             graph and the pattern, not on the numbering.
  outputs    count (embeddings found; a lower bound under BUDGET), status (0 or BUDGET), first (the embedding found
             first: the smallest in matching order; -1 beyond m and where count is 0), covered (the atoms in any embedding,
             a 64-bit mask).  count, status and popcount(covered) do not depend on the molecule's numbering where status is 0.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _args, _lib

MAX_ATOMS = 64                  # include/mlconfgen_hip.h MCG_SUBSTRUCTURE_MAX_ATOMS
MAX_PATTERN_ATOMS = 32          # MCG_SUBSTRUCTURE_MAX_PATTERN_ATOMS
MAX_PATTERNS = 64               # MCG_SUBSTRUCTURE_MAX_PATTERNS: per launch; more are chunked
MAX_B = 16384                   # MCG_SUBSTRUCTURE_MAX_B
NODE_BUDGET = 65536             # MCG_SUBSTRUCTURE_NODE_BUDGET
MAX_Z = 53                      # the largest atomic number an element set may name
STATUS_BUDGET = 1
STATUS_NAMES = {STATUS_BUDGET: "BUDGET"}
ANY_ELEMENT = (1 << 64) - 1
ANY_CODES = (1, 2, 3, 4)
REFUSAL_WITH_FINISHER = ("substructure options cannot be combined with a custom finisher: its results carry no graph this "
                         "package can read")

_SYMBOLS = {"B": 5, "C": 6, "N": 7, "O": 8, "F": 9, "Si": 14, "P": 15, "S": 16, "Cl": 17, "As": 33, "Se": 34, "Br": 35,
            "I": 53}
_BARE = ("Cl", "Br", "B", "C", "N", "O", "F", "P", "S", "I")
_BARE_AROMATIC = {"b": 5, "c": 6, "n": 7, "o": 8, "p": 15, "s": 16}
_BRACKET_AROMATIC = dict(_BARE_AROMATIC, **{"se": 34, "as": 33})


def describe_status(status: int) -> str:
    """"ok" for 0, else the names of the set bits of a `status` word, joined with "|"."""
    status = int(status)
    if status == 0:
        return "ok"
    names = [name for bit, name in STATUS_NAMES.items() if status & bit]
    rest = status & ~sum(STATUS_NAMES)
    return "|".join(names + ([f"0x{rest:x}"] if rest else []))


# ----------------------------------------------------------------------------------------------- the query language
@dataclasses.dataclass(frozen=True)
class QueryAtom:
    """One query atom: `elements` the allowed atomic numbers (None: any), `dmin <= deg <= dmax`, `hmin <= nh <= hmax`,
    `ring` / `aromatic` None any, True yes, False no."""
    elements: Optional[Tuple[int, ...]] = None
    dmin: int = 0
    dmax: int = 255
    hmin: int = 0
    hmax: int = 255
    ring: Optional[bool] = None
    aromatic: Optional[bool] = None

    @property
    def constrains_hydrogens(self) -> bool:
        return (self.hmin, self.hmax) != (0, 255)

    def __repr__(self) -> str:
        parts = ["*" if self.elements is None else ",".join(f"#{z}" for z in self.elements)]
        if (self.dmin, self.dmax) != (0, 255):
            parts.append(f"D{self.dmin}" if self.dmin == self.dmax else f"D{self.dmin}..{self.dmax}")
        if self.constrains_hydrogens:
            parts.append(f"H{self.hmin}" if self.hmin == self.hmax else f"H{self.hmin}..{self.hmax}")
        if self.ring is not None:
            parts.append("R" if self.ring else "R0")
        if self.aromatic is not None:
            parts.append("a" if self.aromatic else "A")
        return "[" + ";".join(parts) + "]"


@dataclasses.dataclass(frozen=True)
class QueryBond:
    """One query bond between the pattern atoms `a` < `b`: `codes` the allowed bond codes (of 1, 2, 3, 4 aromatic), `ring`
    None any, True a ring bond, False a chain bond."""
    a: int
    b: int
    codes: Tuple[int, ...] = ANY_CODES
    ring: Optional[bool] = None

    def __repr__(self) -> str:
        sym = {(1,): "-", (2,): "=", (3,): "#", (4,): ":", ANY_CODES: "~", (1, 4): "-,:"}.get(self.codes, str(self.codes))
        return f"{self.a}{sym}{'' if self.ring is None else '@' if self.ring else '!@'}{self.b}"


def _bounds(name: str, lo, hi) -> Tuple[int, int]:
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255:
            raise ValueError(f"{name} bounds must be integers in 0..255, got {v!r}")
    if lo > hi:
        raise ValueError(f"{name}: the lower bound {lo} is above the upper bound {hi}")
    return lo, hi


def _tristate(name: str, v) -> Optional[bool]:
    if v is not None and not isinstance(v, bool):
        raise ValueError(f"{name} must be None (any), True or False, got {v!r}")
    return v


def atom(elements=None, degree=None, hydrogens=None, ring=None, aromatic=None) -> QueryAtom:
    """A query atom.  `elements`: None (any), one atomic number or an iterable of them (1..53); `degree` / `hydrogens`:
    None (any), an exact count or a (min, max) pair; `ring` / `aromatic`: None (any), True, False."""
    if elements is not None:
        zs = list(elements) if hasattr(elements, "__iter__") and not isinstance(elements, (str, bytes)) else [elements]
        for z in zs:
            if isinstance(z, bool) or not isinstance(z, int) or not 1 <= z <= MAX_Z:
                raise ValueError(f"a query atom's elements must be atomic numbers in 1..{MAX_Z}, got {z!r}")
        if not zs:
            raise ValueError("a query atom's element set is empty")
        elements = tuple(sorted(set(zs)))

    def pair(name, v):
        if v is None:
            return 0, 255
        return _bounds(name, *(v if isinstance(v, (tuple, list)) and len(v) == 2 else (v, v)))
    dmin, dmax = pair("degree", degree)
    hmin, hmax = pair("hydrogens", hydrogens)
    return QueryAtom(elements, dmin, dmax, hmin, hmax, _tristate("ring", ring), _tristate("aromatic", aromatic))


def bond(a: int, b: int, codes=ANY_CODES, ring=None) -> QueryBond:
    """A query bond between the pattern atoms `a` and `b`: `codes` one code or an iterable of the allowed codes (of 1, 2, 3,
    4 aromatic; default any), `ring`: None (any), True (a ring bond), False (a chain bond)."""
    cs = list(codes) if hasattr(codes, "__iter__") and not isinstance(codes, (str, bytes)) else [codes]
    for c in cs:
        if isinstance(c, bool) or not isinstance(c, int) or not 1 <= c <= 4:
            raise ValueError(f"a query bond's codes must be of 1, 2, 3, 4 (aromatic), got {c!r}")
    if not cs:
        raise ValueError("a query bond's code set is empty")
    for v in (a, b):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"a query bond joins two pattern atom indices, got {v!r}")
    if a == b:
        raise ValueError(f"a query bond from atom {a} to itself")
    return QueryBond(min(a, b), max(a, b), tuple(sorted(set(cs))), _tristate("ring", ring))


@dataclasses.dataclass(frozen=True)
class Pattern:
    """A query graph: `atoms` (1..32 `QueryAtom`) and `bonds` (`QueryBond`, at most one per atom pair), in the caller's own
    atom order.  Frozen and hashable; `name` is a label and takes no part in the matching."""
    atoms: Tuple[QueryAtom, ...]
    bonds: Tuple[QueryBond, ...] = ()
    name: str = ""

    def __post_init__(self):
        object.__setattr__(self, "atoms", tuple(self.atoms))
        object.__setattr__(self, "bonds", tuple(sorted(self.bonds, key=lambda q: (q.a, q.b))))
        if not 1 <= len(self.atoms) <= MAX_PATTERN_ATOMS:
            raise ValueError(f"a pattern has 1 to {MAX_PATTERN_ATOMS} query atoms, got {len(self.atoms)}")
        if not all(isinstance(q, QueryAtom) for q in self.atoms) or not all(isinstance(q, QueryBond) for q in self.bonds):
            raise ValueError("a pattern is built from atom(...) and bond(...)")
        seen = set()
        for q in self.bonds:
            if q.b >= len(self.atoms):
                raise ValueError(f"query bond {q!r} names an atom the pattern does not have ({len(self.atoms)} atoms)")
            if (q.a, q.b) in seen:
                raise ValueError(f"two query bonds between the pattern atoms {q.a} and {q.b}")
            seen.add((q.a, q.b))

    @property
    def needs_hydrogens(self) -> bool:
        return any(q.constrains_hydrogens for q in self.atoms)

    def __repr__(self) -> str:
        label = f"{self.name!r}: " if self.name else ""
        return f"Pattern({label}{' '.join(map(repr, self.atoms))} | {' '.join(map(repr, self.bonds))})"


def from_graph(src, bonds: str = "codes", elements: bool = True, name: str = "") -> Pattern:
    """The heavy-atom graph of `src` - a `GeneratedMolecule`, a Mol or an (atomic_numbers, bond_orders) pair, read with
    `fingerprint.mol_graph` - as a pattern: the elements exact (`elements=False`: any), the bond codes exact
    (`bonds="codes"`) or any (`bonds="any"`), no degree, hydrogen, ring or aromaticity constraint: the molecule may carry
    anything else around the piece.  The `fixed_fragment` use."""
    from .fingerprint import mol_graph
    if bonds not in ("codes", "any"):
        raise ValueError(f'bonds must be "codes" or "any", got {bonds!r}')
    z, codes = mol_graph(src)
    n = len(z)
    if not 1 <= n <= MAX_PATTERN_ATOMS:
        raise ValueError(f"a pattern has 1 to {MAX_PATTERN_ATOMS} query atoms, the graph has {n} heavy atoms")
    if elements and any(not 1 <= v <= MAX_Z for v in z):
        raise ValueError(f"a query atom's elements must be atomic numbers in 1..{MAX_Z}, the graph has {sorted(set(z))}")
    rows = torch.as_tensor(codes).tolist()
    qb = [bond(i, j, rows[i][j] if bonds == "codes" else ANY_CODES) for i in range(n) for j in range(i + 1, n) if rows[i][j]]
    return Pattern(tuple(atom(v if elements else None) for v in z), tuple(qb), name)


class _Reader:
    """The position-tracking reader behind `parse`."""

    def __init__(self, text: str):
        self.s, self.i = text, 0

    def fail(self, why: str, at: Optional[int] = None):
        at = self.i if at is None else at
        shown = repr(self.s[at]) if at < len(self.s) else "the end"
        raise ValueError(f"pattern {self.s!r}: position {at} ({shown}): {why}")

    def peek(self, k: int = 1) -> str:
        return self.s[self.i: self.i + k]

    def number(self) -> Optional[int]:
        j = self.i
        while j < len(self.s) and self.s[j].isdigit():
            j += 1
        if j == self.i:
            return None
        v, self.i = int(self.s[self.i: j]), j
        return v


_UNSUPPORTED = {"$": "recursive SMARTS $() is not supported", "X": "the connectivity primitive X is not supported",
                "v": "the valence primitive v is not supported", "@": "chirality is not supported",
                ":": "atom maps are not supported", "!": "a general negation is not supported (only !R and !@)",
                "+": "no charges in this package", "-": "no charges in this package", "r": "ring sizes are not supported",
                "x": "ring-bond counts are not supported", "h": "the implicit-hydrogen primitive h is not supported"}


def _bracket_atom(r: _Reader) -> QueryAtom:
    r.i += 1                                                  # the "["
    if r.peek().isdigit():
        r.fail("isotopes are not supported")
    zs, wants = [], []
    while True:
        at, n_read = r.i, len(zs)
        if r.peek() == "#":
            r.i += 1
            z = r.number()
            if z is None or not 1 <= z <= MAX_Z:
                r.fail(f"an atomic number in 1..{MAX_Z} is needed behind '#'", at)
            zs.append(z)
            wants.append(None)
        else:
            for width in (2, 1):
                sym = r.peek(width)
                if len(sym) == width and (sym in _SYMBOLS or sym in _BRACKET_AROMATIC):
                    zs.append(_SYMBOLS.get(sym, _BRACKET_AROMATIC.get(sym)))
                    wants.append(sym in _BRACKET_AROMATIC)
                    r.i += width
                    break
            else:
                if r.peek() in ("*", "a", "A"):
                    zs.append(None)
                    wants.append({"*": None, "a": True, "A": False}[r.peek()])
                    r.i += 1
            if len(zs) == n_read:
                r.fail(_UNSUPPORTED.get(r.peek(), "an element symbol, '#<Z>', '*', 'a' or 'A' is needed here")
                       if r.peek() else "the bracket atom is not closed")
        if r.peek() != ",":
            break
        r.i += 1
    if len(set(wants)) != 1:
        r.fail("the alternatives of a bracket atom must share one aromaticity requirement", r.i - 1)
    if None in zs and len(zs) > 1:
        r.fail("a wildcard cannot be one of several alternatives", r.i - 1)
    q = dict(elements=None if None in zs else zs, aromatic=wants[0], degree=None, hydrogens=None, ring=None)

    def once(key, value, at):
        if q[key] is not None:
            r.fail(f"the {key} of a bracket atom is given twice", at)
        q[key] = value
    while True:
        at, c = r.i, r.peek()
        if c == "]":
            r.i += 1
            break
        if c in (";", "&"):
            r.i += 1
        elif c == "D":
            r.i += 1
            d = r.number()
            once("degree", 1 if d is None else d, at)
        elif c == "H":
            r.i += 1
            h = r.number()
            once("hydrogens", 1 if h is None else h, at)
        elif c == "R" or r.peek(2) == "!R":
            r.i += 1 if c == "R" else 2
            k = r.number()
            if k not in (None, 0) or (c == "!" and k is not None):
                r.fail("only R, R0 and !R are supported (no ring counts)", at)
            once("ring", c == "R" and k is None, at)
        elif c == "":
            r.fail("the bracket atom is not closed")
        else:
            r.fail(_UNSUPPORTED.get(c, "this is not part of the subset (D<n>, H<n>, R, R0, !R)"))
    for key in ("degree", "hydrogens"):
        if q[key] is not None and q[key] > 255:
            r.fail(f"a {key} above 255", r.i - 1)
    return atom(**q)


def _bond_symbol(r: _Reader) -> Optional[Tuple[Tuple[int, ...], Optional[bool]]]:
    """(codes, ring) of the bond symbols at the reader, None where there is none."""
    codes, ring, any_read = None, None, False
    while True:
        at, c = r.i, r.peek()
        if c in ("-", "=", "#", ":", "~"):
            if codes is not None:
                r.fail("two bond orders on one bond")
            codes = {"-": (1,), "=": (2,), "#": (3,), ":": (4,), "~": ANY_CODES}[c]
            r.i += 1
        elif c == "@" or r.peek(2) == "!@":
            if ring is not None:
                r.fail("two ring requirements on one bond")
            ring = c == "@"
            r.i += 1 if c == "@" else 2
        elif c in ("/", "\\"):
            r.fail("bond stereo is not supported")
        elif c == "!":
            r.fail(_UNSUPPORTED["!"])
        else:
            break
        any_read = True
    return (codes if codes is not None else ANY_CODES, ring) if any_read else None


def parse(smarts: str, name: str = "") -> Pattern:
    """A pattern from a SMALL, LABELLED SUBSET of SMARTS - not SMARTS:
      bare atoms   B C N O F P S Cl Br I: the element, not aromatic; b c n o p s: the element, aromatic; * any; a any
                   aromatic atom; A any atom that is not aromatic.
      brackets     element alternatives joined by "," - the symbols above and Si Se As se as, or #<Z> (no aromaticity
                   requirement), or one of * a A - all with ONE aromaticity requirement; then any of D<n> (degree), H<n>
                   (hydrogens; a bare H means 1), R (in a ring), R0 or !R (not in a ring), with optional ";" or "&" between.
      bonds        - = # : (codes 1 2 3 4), ~ (any), @ (a ring bond), !@ (a chain bond), an order and a ring requirement
                   may be combined (-@, =!@); an omitted bond is single or aromatic.
      structure    branches, ring closures 1-9 and %nn, "." between components.
    Anything else is a ValueError naming the character position and the reason: charges ("no charges in this package"),
    $(), a general "!", X, v, isotopes, chirality, atom maps.  Aromaticity is never perceived: "aromatic" means the atom
    has a code-4 bond in the graph at hand."""
    if not isinstance(smarts, str):
        raise ValueError(f"a pattern string is needed, got {type(smarts).__name__}")
    r = _Reader(smarts)
    atoms: List[QueryAtom] = []
    bonds: Dict[Tuple[int, int], Tuple[Tuple[int, ...], Optional[bool]]] = {}
    stack: List[int] = []
    closures: Dict[int, Tuple[int, Optional[tuple], int]] = {}
    prev: Optional[int] = None
    pending, pending_at = None, 0

    def join(a: int, b: int, spec, at: int):
        if a == b:
            r.fail("a bond from an atom to itself", at)
        key = (min(a, b), max(a, b))
        if key in bonds:
            r.fail(f"two bonds between the pattern atoms {key[0]} and {key[1]}", at)
        bonds[key] = spec if spec is not None else ((1, 4), None)

    while r.i < len(r.s):
        at, c = r.i, r.peek()
        if c == "(":
            if prev is None:
                r.fail("a branch needs an atom in front of it")
            if pending is not None:
                r.fail("a bond symbol in front of a branch")
            stack.append(prev)
            r.i += 1
            continue
        if c == ")":
            if not stack:
                r.fail("a ')' without its '('")
            if pending is not None:
                r.fail("a bond symbol without an atom behind it", pending_at)
            prev = stack.pop()
            r.i += 1
            continue
        if c == ".":
            if prev is None or pending is not None:
                r.fail("a '.' needs an atom in front of it")
            prev = None
            r.i += 1
            continue
        if c.isdigit() or c == "%":
            if prev is None:
                r.fail("a ring closure needs an atom in front of it")
            if c == "%":
                if not (r.peek(3)[1:].isdigit() and len(r.peek(3)) == 3):
                    r.fail("two digits are needed behind '%'")
                num = int(r.peek(3)[1:])
                r.i += 3
            else:
                num = int(c)
                r.i += 1
            if num in closures:
                other, spec, opened = closures.pop(num)
                if spec is not None and pending is not None and spec != pending:
                    r.fail(f"the two ends of ring closure {num} name different bonds", at)
                join(other, prev, pending if pending is not None else spec, at)
            else:
                closures[num] = (prev, pending, at)
            pending = None
            continue
        spec = _bond_symbol(r)
        if spec is not None:
            if prev is None:
                r.fail("a bond symbol needs an atom in front of it", at)
            if pending is not None:
                r.fail("two bond symbols in a row", at)
            pending, pending_at = spec, at
            continue
        if c == "[":
            q = _bracket_atom(r)
        else:
            for sym in _BARE:
                if smarts.startswith(sym, r.i):
                    q = atom(_SYMBOLS[sym], aromatic=False)
                    r.i += len(sym)
                    break
            else:
                if c in _BARE_AROMATIC:
                    q = atom(_BARE_AROMATIC[c], aromatic=True)
                elif c in ("*", "a", "A"):
                    q = atom(aromatic={"*": None, "a": True, "A": False}[c])
                else:
                    r.fail(_UNSUPPORTED.get(c, "this character is not part of the subset"))
                r.i += 1
        if len(atoms) == MAX_PATTERN_ATOMS:
            r.fail(f"a pattern has at most {MAX_PATTERN_ATOMS} query atoms", at)
        atoms.append(q)
        if prev is not None:
            join(prev, len(atoms) - 1, pending, at)
        prev, pending = len(atoms) - 1, None
    if pending is not None:
        r.fail("a bond symbol without an atom behind it", pending_at)
    if stack:
        r.fail("a '(' is not closed")
    if closures:
        num, (_, _, opened) = sorted(closures.items())[0]
        r.fail(f"ring closure {num} is not closed", opened)
    if not atoms:
        r.fail("an empty pattern")
    return Pattern(tuple(atoms), tuple(bond(a, b, codes, ring) for (a, b), (codes, ring) in bonds.items()),
                   name or smarts)


# ----------------------------------------------------------------------------------------------- compiling
def matching_order(n_atoms: int, pairs: Sequence[Tuple[int, int]]) -> List[int]:
    """The matching order of a pattern of `n_atoms` atoms with query bonds between `pairs`: position k -> atom index.  Per
    component breadth-first from its lowest-index atom, neighbours in ascending index, components in ascending order of
    their lowest atom."""
    nbrs = [[] for _ in range(n_atoms)]
    for a, b in pairs:
        nbrs[a].append(b)
        nbrs[b].append(a)
    order, seen = [], [False] * n_atoms
    for start in range(n_atoms):
        if seen[start]:
            continue
        seen[start] = True
        queue = [start]
        while queue:
            a = queue.pop(0)
            order.append(a)
            for j in sorted(nbrs[a]):
                if not seen[j]:
                    seen[j] = True
                    queue.append(j)
    return order


@dataclasses.dataclass(frozen=True, eq=False)
class Compiled:
    """`compile_patterns`' result: the patterns, their packed host tensors in matching order (`pat_n` [P] int32,
    `pat_atoms` [P,32,2] int64 holding the unsigned bit patterns, `pat_bonds` [P,32,32] uint8), per pattern `order`
    (position -> the caller's atom index) and `inverse` (the caller's atom index -> position), and whether any pattern
    constrains hydrogens.  Compared by identity: it holds tensors."""
    patterns: Tuple[Pattern, ...]
    pat_n: torch.Tensor
    pat_atoms: torch.Tensor
    pat_bonds: torch.Tensor
    order: Tuple[Tuple[int, ...], ...]
    inverse: Tuple[Tuple[int, ...], ...]
    needs_hydrogens: bool

    @property
    def max_atoms(self) -> int:
        return max([len(p.atoms) for p in self.patterns] + [0])


def _signed(v: int) -> int:
    return v - (1 << 64) if v >= 1 << 63 else v


def as_pattern(obj, where: str = "patterns", k: Optional[int] = None) -> Pattern:
    """`obj` as a `Pattern`: a `Pattern`, a string (`parse`) or a graph source (`from_graph`).  ValueError naming `where`
    and the entry's position `k`."""
    if isinstance(obj, Pattern):
        return obj
    label = where if k is None else f"{where}[{k}]"
    try:
        return parse(obj) if isinstance(obj, str) else from_graph(obj)
    except ValueError as e:
        raise ValueError(f"{label}: {e}") from None


def compile_patterns(patterns, where: str = "patterns") -> Compiled:
    """Strings (`parse`), `Pattern`s and graph sources (`from_graph`) -> `Compiled`: each pattern renumbered into its
    matching order (`matching_order`) and packed as `mcg_substructure_match` reads it - word 0 of an atom the element
    mask, word 1 the bytes dmin, dmax, hmin, hmax, ring, arom (0 any, 1 yes, 2 no); a bond byte 0 for no query bond, else
    the code mask in the low nibble and the ring requirement (0 any, 1 ring, 2 chain) in bits 4-5.  Host work only.
    ValueError naming `where` and the entry's position: an entry that is unreadable or breaks a limit, and an argument
    that is no iterable of patterns.  A `Compiled` is returned as it is."""
    if isinstance(patterns, Compiled):
        return patterns
    if isinstance(patterns, (str, bytes, Pattern)) or not hasattr(patterns, "__iter__"):
        raise ValueError(f"{where} must be an iterable of pattern strings, Patterns or graphs, got "
                         f"{type(patterns).__name__}")
    pats = tuple(as_pattern(obj, where, k) for k, obj in enumerate(patterns))
    P = len(pats)
    pat_n = torch.tensor([len(p.atoms) for p in pats], dtype=torch.int32).reshape(P)
    pat_atoms = torch.zeros(P, MAX_PATTERN_ATOMS, 2, dtype=torch.int64)
    pat_bonds = torch.zeros(P, MAX_PATTERN_ATOMS, MAX_PATTERN_ATOMS, dtype=torch.uint8)
    orders, inverses = [], []
    tri = {None: 0, True: 1, False: 2}
    for p, pat in enumerate(pats):
        order = matching_order(len(pat.atoms), [(q.a, q.b) for q in pat.bonds])
        inverse = [0] * len(order)
        for k, a in enumerate(order):
            inverse[a] = k
        for k, a in enumerate(order):
            q = pat.atoms[a]
            mask = ANY_ELEMENT if q.elements is None else sum(1 << z for z in q.elements)
            word = q.dmin | q.dmax << 8 | q.hmin << 16 | q.hmax << 24 | tri[q.ring] << 32 | tri[q.aromatic] << 40
            pat_atoms[p, k, 0], pat_atoms[p, k, 1] = _signed(mask), word
        for q in pat.bonds:
            byte = sum(1 << (c - 1) for c in q.codes) | tri[q.ring] << 4
            pat_bonds[p, inverse[q.a], inverse[q.b]] = pat_bonds[p, inverse[q.b], inverse[q.a]] = byte
        orders.append(tuple(order))
        inverses.append(tuple(inverse))
    return Compiled(pats, pat_n, pat_atoms, pat_bonds, tuple(orders), tuple(inverses), any(p.needs_hydrogens for p in pats))


def first_in_caller_order(first: torch.Tensor, compiled: Compiled) -> torch.Tensor:
    """[.., P, 32] embeddings in matching order -> [.., P, M] in the caller's pattern atom order, M the largest pattern of
    the set; -1 beyond a pattern's atoms.  One gather on the tensor's device."""
    P, M = len(compiled.patterns), compiled.max_atoms
    idx = torch.zeros(P, M, dtype=torch.long)
    keep = torch.zeros(P, M, dtype=torch.bool)
    for p, inverse in enumerate(compiled.inverse):
        idx[p, : len(inverse)] = torch.tensor(inverse, dtype=torch.long)
        keep[p, : len(inverse)] = True
    idx, keep = idx.to(first.device), keep.to(first.device)
    lead = first.shape[:-2]
    out = first.gather(-1, idx.expand(*lead, P, M))
    return torch.where(keep.expand(*lead, P, M), out, torch.full_like(out, -1))


# ----------------------------------------------------------------------------------------------- device
@torch.no_grad()
def match_substructures(atomic_numbers: torch.Tensor, bond_orders: torch.Tensor, n_nodes: torch.Tensor, patterns,
                        hydrogens=None, device=None, check: bool = True) -> Dict[str, torch.Tensor]:
    """Every embedding of each of P patterns in each of B molecular graphs by this module's definition,
    `mcg_substructure_match` launches over chunks of `MAX_B` rows and `MAX_PATTERNS` patterns: `atomic_numbers` [B, >= W],
    `bond_orders` [B,W,W] (symmetric codes 0 none / 1 / 2 / 3 / 4 aromatic), `n_nodes` [B] real atoms each; the diagonal
    and everything at or beyond a molecule's atom count is ignored, whatever it holds.  `patterns`: what
    `compile_patterns` takes, or its result.  `hydrogens`: None - `hydrogens.implicit_counts(...)` (host work: its ring
    search) is passed where a pattern constrains hydrogens, nothing otherwise; a [B, >= W] integer tensor - each atom's
    hydrogens as given; False - nothing is passed and the kernel counts max(0, (2 v0 - v2) / 2), the count rule without
    the aromatic N-H.  Device tensors:
      count [B,P]     int32: the embeddings found (a lower bound where status is BUDGET)
      status [B,P]    int32: 0 or STATUS_BUDGET (`describe_status`)
      first [B,P,M]   int32: the embedding found first, in the CALLER's pattern atom order - entry i is the molecule's atom
                      that pattern atom i lands on; M the largest pattern; -1 beyond a pattern's atoms and where count is 0
      covered [B,P]   int64 holding the unsigned bit pattern: bit a set where atom a lies in any embedding found
    Every output is exact: the same bits whatever the batch, the row, the padded width and the other patterns.
    ValueError before the kernel: as `canonical.canonical_order` (W > 64, shapes that do not fit, atom counts outside
    [0, W], and with `check=True` a code outside 0..4, a matrix that is not symmetric over the real atoms, an atomic number
    < 1 on a real atom), what `compile_patterns` refuses, an empty pattern list, a `hydrogens` of another shape."""
    compiled = compile_patterns(patterns)
    P, M = len(compiled.patterns), compiled.max_atoms
    if P == 0:
        raise ValueError("match_substructures needs at least one pattern")
    z, bonds, B, W = _args.graph_arguments(atomic_numbers, bond_orders, n_nodes, MAX_ATOMS,
                                           f"substructure matches take molecules of at most {MAX_ATOMS} atoms")
    nh = None
    if hydrogens is not None and hydrogens is not False:
        nh = torch.as_tensor(hydrogens)
        if nh.dim() != 2 or nh.shape[0] != B or nh.shape[1] < W or nh.dtype.is_floating_point:
            raise ValueError(f"hydrogens must be an integer tensor [B, >= W] = [{B}, >= {W}], got {list(nh.shape)} of type "
                             f"{nh.dtype}")
    elif hydrogens is None and compiled.needs_hydrogens and B > 0 and W > 0:
        from .hydrogens import implicit_counts
        nh = implicit_counts(z[:, :W], bonds, n_nodes)
    dev = _args.resolve_device(device, bonds)
    if W == 0:                                  # no atoms anywhere: B empty graphs at the kernel's smallest width
        z, bonds, W, nh = torch.zeros(B, 1, dtype=torch.int32), torch.zeros(B, 1, 1, dtype=torch.int8), 1, None
    if B == 0:
        return dict(count=torch.zeros(0, P, dtype=torch.int32, device=dev), status=torch.zeros(0, P, dtype=torch.int32, device=dev),
                    first=torch.full((0, P, M), -1, dtype=torch.int32, device=dev),
                    covered=torch.zeros(0, P, dtype=torch.int64, device=dev))
    zd, bd, nn = _args.device_graph(z, bonds, n_nodes, B, W, dev)
    nhd = None if nh is None else nh[:, :W].to(dev, torch.int32).contiguous()
    if check:
        _args.check_graphs(zd, bonds.to(dev), nn, W)
    pn, pa, pb = compiled.pat_n.to(dev), compiled.pat_atoms.to(dev), compiled.pat_bonds.to(dev)
    parts = []
    for plo in range(0, P, MAX_PATTERNS):
        phi = min(P, plo + MAX_PATTERNS)
        Pc = phi - plo
        count = torch.zeros(B, Pc, dtype=torch.int32, device=dev)
        status = torch.zeros(B, Pc, dtype=torch.int32, device=dev)
        first = torch.full((B, Pc, MAX_PATTERN_ATOMS), -1, dtype=torch.int32, device=dev)
        covered = torch.zeros(B, Pc, dtype=torch.int64, device=dev)
        for lo in range(0, B, MAX_B):
            hi = min(B, lo + MAX_B)
            _lib.check(_lib.lib().mcg_substructure_match(
                _lib.dptr(zd[lo:hi]), _lib.dptr(bd[lo:hi]), _lib.dptr(nn[lo:hi]), None if nhd is None else _lib.dptr(nhd[lo:hi]),
                hi - lo, W, _lib.dptr(pn[plo:phi]), _lib.dptr(pa[plo:phi]), _lib.dptr(pb[plo:phi]), Pc,
                _lib.dptr(count[lo:hi]), _lib.dptr(status[lo:hi]), _lib.dptr(first[lo:hi]), _lib.dptr(covered[lo:hi]),
                _lib.current_stream_ptr(dev)), "mcg_substructure_match")
        parts.append((count, status, first, covered))
    count, status, first, covered = (parts[0] if len(parts) == 1 else tuple(torch.cat(t, dim=1) for t in zip(*parts)))
    return dict(count=count, status=status, first=first_in_caller_order(first, compiled), covered=covered)


# ----------------------------------------------------------------------------------------------- the catalogue
_CATALOGUE_SOURCE = (
    ("peroxide", "O-O"),
    ("acyl halide", "C(=O)[Cl,Br,I,F]"),
    ("aldehyde", "[CH1](=O)[#6]"),
    ("azo", "[#6]N=N[#6]"),
    ("thiol", "[SH1]"),
    ("isocyanate", "N=C=O"),
    ("isothiocyanate", "N=C=S"),
    ("Michael-acceptor enone", "C=CC(=O)[#6]"),
    ("alkyl halide", "C[Cl,Br,I]"),
    ("epoxide", "C1OC1"),
    ("aziridine", "C1NC1"),
    ("sulfonyl halide", "S(=O)(=O)[Cl,Br,I,F]"),
    ("disulfide", "SS"),
    ("nitroso", "[#6]N=O"),
    ("ring larger than 8", "*@*@*@*@*@*@*@*@*"),
)
# The package's OWN short list of groups a medicinal chemist usually does not want - NOT PAINS, NOT the Brenk filters, NOT
# RDKit's FilterCatalog, and no claim to cover what those cover.  Every entry is written in `parse`'s subset.  "ring larger
# than 8" is a chain of nine atoms joined by ring bonds: a single ring of up to 8 atoms has no such path, a larger one has;
# a fused system of nine or more ring atoms (naphthalene) has one too, so use it on its own only where that is wanted.
CATALOGUE: Dict[str, Pattern] = {name: parse(text, name) for name, text in _CATALOGUE_SOURCE}
