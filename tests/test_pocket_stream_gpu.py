"""The stream contract of include/mlconfgen_hip_pocket.h on the MI355X: `stream_probe`'s arrangements A ("busy default
stream") and B ("late producer") applied to `mcg_pocket_masks`, with bit equality against the same call on the default
stream.  The call is made with more than one split, so the zeroing of the output in front of the kernel is part of what is
arranged: a memset that went to stream 0 would, under A, not have run when the side stream ORs into the sentinel-filled
buffer.  `COVERAGE` is what tests/test_pocket_host.py holds against the header's `void* stream` prototypes."""
import numpy as np
import pytest
import torch

import pocket_cases as PC
import stream_probe as SP

DEV = torch.device("cuda:0")
POCKET_HEADER = SP.HEADER.replace("mlconfgen_hip.h", "mlconfgen_hip_pocket.h")
# entry -> (the GPU test below that runs it, the arrangements it applies)
COVERAGE = {
    "mcg_pocket_masks": ("test_pocket_masks_on_a_side_stream", "AB"),
}


def _show(res):
    print(f"\nSTREAM {res.label}: baseline {res.t_call_ms:.2f} ms, spin {res.delay_ms:.0f} ms, "
          f"{'default stream still busy' if res.busy else 'side stream still busy at return' if res.pending else 'NOT busy'}, "
          f"{'equal' if res.equal else 'DIFFERENT'}, entries {sorted({n for n, _ in res.calls})}")
    return res


@pytest.mark.gpu
def test_pocket_masks_on_a_side_stream(monkeypatch):
    from ml_conformer_generator_amd import _lib
    from ml_conformer_generator_amd import receptor as RC
    both = SP.stream_entries() + SP.stream_entries(POCKET_HEADER)
    monkeypatch.setattr(SP, "stream_entries", lambda header=None: both)          # the recorder notes the new entry too
    xyz, z = PC.block()
    xyzr = RC.sort_receptor(torch.from_numpy(xyz).to(torch.float32), torch.from_numpy(PC.radii(z)))
    R, n, splits = int(xyzr.shape[0]), 21, 4
    true = dict(rec=xyzr.to(DEV), spheres=RC.tile_spheres(xyzr).to(DEV))
    # the poison: the same atoms moved by 1.5 A, with the spheres that hold them - a valid receptor with other masks
    moved = xyzr + torch.tensor([1.5, 0.0, 0.0, 0.0])
    poison = dict(rec=moved.to(DEV), spheres=RC.tile_spheres(moved).to(DEV))
    out = torch.zeros(n ** 3, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def call(i):
        _lib.check(_lib.lib().mcg_pocket_masks(_lib.dptr(i["rec"]), R, _lib.dptr(i["spheres"]), n, 1.0, 1.4, 8.0, splits,
                                               _lib.dptr(out), _lib.current_stream_ptr(DEV)), "mcg_pocket_masks")
        return out

    base = call(true).clone()
    torch.cuda.synchronize()
    assert int((base != 0).sum()) > n ** 3 // 2 and not torch.equal(base, call(poison))
    torch.cuda.synchronize()
    held = set()
    _show(SP.arrangement_a(lambda: call(true), "pocket_masks [A]", refill=[out])).ok(["mcg_pocket_masks"], raw=True)
    held.add("A")
    res = _show(SP.arrangement_b(call, true, poison, "pocket_masks [B]", raw=True, refill=[out])).ok(["mcg_pocket_masks"], raw=True)
    held.add("B")
    assert torch.equal(res.got[0], base)
    for entry, (_, arrangements) in COVERAGE.items():
        assert set(arrangements) <= held, entry

    from ml_conformer_generator_amd import pocket as PK                          # the wrapper: the same bits, on its stream
    wrapped = SP.arrangement_a(lambda: PK.ray_masks((xyz, z), (0.0, 0.0, 0.0), device=DEV), "ray_masks [A]")
    _show(wrapped).ok(["mcg_pocket_masks"])
    assert np.array_equal(wrapped.got[0].cpu().numpy(), base.cpu().numpy())
