"""Class -> element decisions of the generator (`MLConformerGenerator(atom_decoder=...)`).

The reference writes `atom_decoder[argmax(h)]` into the XYZ block of every generated molecule
(`samples_to_rdkit_mol`, utils/mol_utils.py:41-45); from there RDKit's atomic number is what the GCN embeds
(`MolGraph.elements_vector`), what its connectivity is perceived from and what its validity gate judges.  Here the
decoder becomes one class -> Z map that the device hand-off reads (`mcg_handoff_elements`); everything downstream follows
Z and the table `config.ELEMENTS`.
"""
from __future__ import annotations

from typing import Dict, Tuple

from .config import ELEMENTS, GCN_NUM_EMBEDDINGS, N_ATOM_CLASSES

SYMBOL_TO_Z: Dict[str, int] = {sym: z for z, (sym, _, _) in ELEMENTS.items()}
Z_TO_SYMBOL: Dict[int, str] = {z: sym for z, (sym, _, _) in ELEMENTS.items()}


def class_z_from_decoder(atom_decoder: dict) -> Tuple[int, ...]:
    """(Z of class 0, ..., Z of class 7) for an `atom_decoder` {class index: element symbol}.

    Raises ValueError unless the keys are exactly 0..7 and every value names an element of `config.ELEMENTS` whose Z the
    GCN can embed (< GCN_NUM_EMBEDDINGS; the reference would fail later with an IndexError inside `nn.Embedding`).
    Hydrogen is refused: every count in this API is a heavy-atom count.  Two classes may name the same element."""
    if not isinstance(atom_decoder, dict):
        raise ValueError(f"atom_decoder must be a dict {{class index: element symbol}}, got {type(atom_decoder).__name__}")
    keys = set(atom_decoder)
    want = set(range(N_ATOM_CLASSES))
    if keys != want:
        missing, extra = sorted(want - keys), sorted(keys - want, key=repr)
        raise ValueError(f"atom_decoder must map exactly the classes 0..{N_ATOM_CLASSES - 1}"
                         + (f"; missing {missing}" if missing else "") + (f"; unexpected keys {extra}" if extra else ""))
    out = []
    for k in range(N_ATOM_CLASSES):
        sym = atom_decoder[k]
        if sym == "H":
            raise ValueError("atom_decoder: hydrogen cannot be a generated atom (every count of this API is heavy atoms)")
        z = SYMBOL_TO_Z.get(sym) if isinstance(sym, str) else None
        if z is None:
            raise ValueError(f"atom_decoder[{k}] = {sym!r} is not one of the supported elements "
                             f"{sorted(SYMBOL_TO_Z, key=SYMBOL_TO_Z.get)}")
        if z >= GCN_NUM_EMBEDDINGS:
            raise ValueError(f"atom_decoder[{k}] = {sym!r}: Z = {z} is outside the GCN's element embedding "
                             f"(Z < {GCN_NUM_EMBEDDINGS})")
        out.append(z)
    return tuple(out)
