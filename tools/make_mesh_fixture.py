#!/usr/bin/env python3
"""Write tests/golden/pocket_6q8k_mesh.npz from the reference project's demo pocket (`assets/demo_files/6q8k_pocket.stl`).

Data only: the welded vertices `v` fp32 [V,3] and the outward faces `f` int16 [F,3], as `mesh.load_mesh` returns them; the
STL itself is not committed.  Prints the figures the host tests pin (tests/test_mesh_host.py).
Usage:  python tools/make_mesh_fixture.py path/to/6q8k_pocket.stl [--out tests/golden/pocket_6q8k_mesh.npz]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from ml_conformer_generator_amd import mesh as M            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stl")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "pocket_6q8k_mesh.npz"))
    args = ap.parse_args()
    with open(args.stl, "rb") as fh:
        data = fh.read()
    corners = M._read_stl(data)
    mesh = M.load_mesh(data)
    assert mesh.faces.max() < 2 ** 15
    np.savez_compressed(args.out, v=mesh.vertices.astype(np.float32), f=mesh.faces.astype(np.int16))
    props = M.mass_properties(mesh)
    print(f"{corners.shape[0] * 3} corner records weld to {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces")
    print(f"volume {props['volume']:.3f}  principal inertia at density {M.DEFAULT_DENSITY}: "
          f"{np.round(props['principal_inertia_components'], 3).tolist()}")
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
