"""The stream contract of include/mlconfgen_hip_search.h on the MI355X: `stream_probe`'s arrangements A ("busy default
stream") and B ("late producer") applied to both entries of the fourth header, with bit equality against the same call on
the default stream.  `COVERAGE` is what tests/test_pose_search_host.py holds against the header's `void* stream` prototypes,
as tests/test_pose_flex_host.py holds the second header's."""
import numpy as np
import pytest
import torch

import flex_cases as FC
import interactions_ref as IR
import stream_probe as SP

DEV = torch.device("cuda:0")
FLEX_HEADER = SP.HEADER.replace("mlconfgen_hip.h", "mlconfgen_hip_flex.h")
SEARCH_HEADER = SP.HEADER.replace("mlconfgen_hip.h", "mlconfgen_hip_search.h")
# entry -> (the GPU test below that runs it, the arrangements it applies)
COVERAGE = {
    "mcg_pose_starts": ("test_search_entries_on_a_side_stream", "AB"),
    "mcg_pose_search_select": ("test_search_entries_on_a_side_stream", "AB"),
}


def _show(res):
    print(f"\nSTREAM {res.label}: baseline {res.t_call_ms:.2f} ms, spin {res.delay_ms:.0f} ms, "
          f"{'default stream still busy' if res.busy else 'side stream still busy at return' if res.pending else 'NOT busy'}, "
          f"{'equal' if res.equal else 'DIFFERENT'}, entries {sorted({n for n, _ in res.calls})}")
    return res


@pytest.mark.gpu
def test_search_entries_on_a_side_stream(monkeypatch):
    from ml_conformer_generator_amd import interactions as IX
    every = SP.stream_entries() + SP.stream_entries(FLEX_HEADER) + SP.stream_entries(SEARCH_HEADER)
    monkeypatch.setattr(SP, "stream_entries", lambda header=None: every)         # the recorder notes the new entries too
    by = FC.by_name()
    pool = [by[k] for k in ("hexane", "isopentylbenzene", "biphenyl", "folded_heptane", "butane", "toluene")]
    z, bonds, n, x = FC.padded(pool, 14)
    real = np.arange(14)[None, :, None] < n[:, None, None]
    x = x - x.sum(axis=1, keepdims=True) / np.maximum(n, 1)[:, None, None] * real
    x = (x + np.array([0.6, -0.3, 0.2], dtype=np.float32) * real).astype(np.float32)
    true = dict(coords=torch.from_numpy(x).to(DEV), n=torch.from_numpy(n).to(DEV), z=torch.from_numpy(z).to(DEV),
                bonds=torch.from_numpy(bonds).to(DEV))
    tree = IX.torsion_tree(true["z"], true["bonds"], true["n"], DEV, check=False)
    typed = dict(coords=true["coords"], n=true["n"], atoms=tree["torsion_atoms"], side=tree["side_mask"],
                 counts=tree["counts"])
    ids = torch.arange(len(pool)) + 40                                           # host ids: every device input is poisoned
    torch.cuda.synchronize()
    prepared = IX.prepare_receptor(IR.cases()[2].receptor)
    held = {"A": set(), "B": set()}
    calls = (
        (lambda i: IX.pose_starts(i["coords"], i["n"], dict(torsion_atoms=i["atoms"], side_mask=i["side"], counts=i["counts"]),
                                  ids, seed=5, starts=3, device=DEV, params=True),
         "pose_starts", ["mcg_pose_starts"], typed),
        (lambda i: IX.search_pose(prepared, i["coords"], i["n"], i["z"], i["bonds"], starts=3, steps=4, seed=5,
                                  sample_ids=ids, device=DEV),
         "search_pose", ["mcg_torsion_tree", "mcg_pose_starts", "mcg_receptor_optimise_flex", "mcg_pose_search_select"], true),
    )
    for call, label, entries, inputs in calls:
        _show(SP.arrangement_a(lambda: call(inputs), label + " [A]")).ok(entries)
        held["A"].update(entries)
        _show(SP.arrangement_b(call, inputs, SP.rolled(inputs), label + " [B]")).ok(entries)
        held["B"].update(entries)
    for entry, (_, arrangements) in COVERAGE.items():
        for a in arrangements:
            assert entry in held[a], (entry, a)
