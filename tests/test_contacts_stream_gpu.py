"""The stream contract of include/mlconfgen_hip_contacts.h on the MI355X: `stream_probe`'s arrangements A ("busy default
stream") and B ("late producer") applied to the entry of the fifth header, with bit equality against the same call on the
default stream.  `COVERAGE` is what tests/test_contacts_host.py holds against the header's `void* stream` prototype."""
import pytest
import torch

import contacts_cases as CC
import stream_probe as SP
from test_contacts_gpu import _pad, _prepared

DEV = torch.device("cuda:0")
CONTACTS_HEADER = SP.HEADER.replace("mlconfgen_hip.h", "mlconfgen_hip_contacts.h")
# entry -> (the GPU test below that runs it, the arrangements it applies)
COVERAGE = {"mcg_receptor_contacts": ("test_contacts_entry_on_a_side_stream", "AB")}


def _show(res):
    print(f"\nSTREAM {res.label}: baseline {res.t_call_ms:.2f} ms, spin {res.delay_ms:.0f} ms, "
          f"{'default stream still busy' if res.busy else 'side stream still busy at return' if res.pending else 'NOT busy'}, "
          f"{'equal' if res.equal else 'DIFFERENT'}, entries {sorted({n for n, _ in res.calls})}")
    return res


@pytest.mark.gpu
def test_contacts_entry_on_a_side_stream(monkeypatch):
    from ml_conformer_generator_amd import contacts as CT
    every = SP.stream_entries() + SP.stream_entries(CONTACTS_HEADER)
    monkeypatch.setattr(SP, "stream_entries", lambda header=None: every)         # the recorder notes the new entry too
    cases = [CC.cases()[1], CC.cases()[2], CC.cases()[3], CC.cases()[1], CC.cases()[3], CC.cases()[2]]
    prepared = _prepared(cases[0])
    x, r, t, n = (a.to(DEV) for a in _pad(cases, 32))
    inputs = dict(x=x, r=r, t=t, n=n)
    ref = cases[0].expected()["entries"][:6]
    reference = ([g for g, _ in ref], [k for _, k in ref])                       # host lists: every device input is poisoned
    torch.cuda.synchronize()

    def call(i):
        return CT.fingerprint_typed(prepared, i["x"], i["n"], i["r"], i["t"], reference=reference, device=DEV)
    held = {"A": set(), "B": set()}
    _show(SP.arrangement_a(lambda: call(inputs), "contact fingerprint [A]")).ok(["mcg_receptor_contacts"])
    held["A"].add("mcg_receptor_contacts")
    _show(SP.arrangement_b(call, inputs, SP.rolled(inputs), "contact fingerprint [B]")).ok(["mcg_receptor_contacts"])
    held["B"].add("mcg_receptor_contacts")
    for entry, (_, arrangements) in COVERAGE.items():
        for a in arrangements:
            assert entry in held[a], (entry, a)
