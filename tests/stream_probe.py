"""The stream contract of include/mlconfgen_hip.h, made testable: "`stream` is the hipStream_t the work goes to", "one handle
must not run on two streams at once, different handles are independent", "one mcg_egnn may be shared by several plans".

Every other test of the suite runs on the default stream, where a launch, memset or copy that goes to stream 0 instead of the
caller's stream, an internal stream that is not ordered behind the caller's, and a blocking call that ties a side stream to the
legacy default stream all give the right answer.  The two arrangements here make them give a wrong one, or make them visible:

  A, "busy default stream"  the call runs on a side stream S while the default stream spins.  Work misplaced onto stream 0
                            has not run when S is read (S's clones hold the sentinel), and anything that waited for the
                            legacy stream finds it idle afterwards (`busy` is False).
  B, "late producer"        the call's device inputs hold a different, valid batch ("poison") until a copy on S, queued
                            behind a spin on S, brings the true inputs in.  Work that ran ahead of S, on any stream not
                            ordered behind it, computed the poison's answer.

All comparisons are bit equality with the same call on the default stream (which the other test files hold to fp64 or
bit-exact restatements); no tolerance is introduced.  Nothing here faults: the poison is valid data, a spin is at most
MAX_DELAY_MS long, every arrangement ends in a device synchronise.

`COVERAGE` is the table `tests/test_stream_contract_host.py` holds against the header: every prototype with a `void* stream`
parameter is a key of it (with the GPU test that runs it and the arrangements that test applies), an alias of a key, or one of
the `EXCLUDED` hooks.  Importing this module needs no GPU."""
import gc
import os
import re
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mlconfgen_hip.h")

MAX_DELAY_MS = 250.0          # no single spin is longer
MIN_DELAY_MS = 20.0
A_MARGIN, B_MARGIN = 5.0, 10.0          # x the baseline's wall time (A) / the unsynchronised call's host time (B)
SENTINEL_BYTE = 0x5B          # every output byte before an arranged call: fp32 6.2e16, int32 1 532 713 819 - never an answer

# ---- the table ----------------------------------------------------------------------------------------------------------
# entry -> (GPU test in test_stream_contract_gpu.py, arrangements, why only A where B is left out)
_DENOISER, _SAMPLER, _GCN, _SHAPE = ("test_denoiser_on_a_side_stream", "test_sampler_entries_on_a_side_stream",
                                     "test_gcn_and_handoff_on_a_side_stream", "test_shape_entries_on_a_side_stream")
_MESH, _RECEPTOR, _GRAPHS, _IDENTITY = ("test_mesh_entries_on_a_side_stream", "test_receptor_entries_on_a_side_stream",
                                        "test_graph_preparation_and_scores_on_a_side_stream",
                                        "test_graph_identity_entries_on_a_side_stream")
COVERAGE = {
    "mcg_egnn_dynamics": (_DENOISER, "AB", None),
    "mcg_plan_peek": (_DENOISER, "A", "it copies out what the call in front of it left in the plan: it has no input to poison"),
    "mcg_sampler_noise": (_SAMPLER, "AB", None),
    "mcg_sampler_noise_keyed": (_SAMPLER, "AB", None),
    "mcg_sampler_step": (_SAMPLER, "AB", None),
    "mcg_sampler_decode": (_SAMPLER, "AB", None),
    "mcg_sampler_blend": (_SAMPLER, "AB", None),
    "mcg_egnn_aggregate": (_GCN, "AB", None),
    "mcg_gcn_forward": (_GCN, "AB", None),
    "mcg_gcn_peek": (_GCN, "A", "it copies out what the forward in front of it left in the workspace: it has no input to poison"),
    "mcg_handoff_ex": (_GCN, "AB", None),
    "mcg_bond_writeback": (_GCN, "AB", None),
    "mcg_ifm_merge": (_GCN, "AB", None),
    "mcg_shape_tanimoto": (_SHAPE, "AB", None),
    "mcg_shape_moments": (_SHAPE, "AB", None),
    "mcg_shape_frames": (_SHAPE, "AB", None),
    "mcg_shape_frames_tf": (_SHAPE, "AB", None),
    "mcg_shape_overlay": (_SHAPE, "AB", None),
    "mcg_shape_overlay_refined": (_SHAPE, "AB", None),
    "mcg_shape_pair_tanimoto": (_SHAPE, "AB", None),
    "mcg_shape_tanimoto_field": (_MESH, "AB", None),
    "mcg_shape_overlay_field": (_MESH, "AB", None),
    "mcg_mesh_winding": (_MESH, "AB", None),
    "mcg_mesh_occupancy": (_MESH, "AB", None),
    "mcg_mesh_atoms_outside": (_MESH, "AB", None),
    "mcg_receptor_overlap": (_RECEPTOR, "AB", None),
    "mcg_receptor_relieve": (_RECEPTOR, "AB", None),
    "mcg_receptor_interactions": (_RECEPTOR, "AB", None),
    "mcg_receptor_optimise": (_RECEPTOR, "AB", None),
    "mcg_geometry_relax_ex": (_GRAPHS, "AB", None),
    "mcg_pharm_perceive": (_GRAPHS, "AB", None),
    "mcg_pharm_score": (_GRAPHS, "AB", None),
    "mcg_hydrogens_place": (_GRAPHS, "AB", None),
    "mcg_standardize_graphs": (_GRAPHS, "AB", None),
    "mcg_charges_peoe": (_GRAPHS, "AB", None),
    "mcg_esp_overlap": (_GRAPHS, "AB", None),
    "mcg_graph_fingerprint": (_IDENTITY, "AB", None),
    "mcg_fingerprint_tanimoto": (_IDENTITY, "AB", None),
    "mcg_fingerprint_pair_tanimoto": (_IDENTITY, "AB", None),
    "mcg_canonical_order": (_IDENTITY, "AB", None),
    "mcg_stereo_order": (_IDENTITY, "AB", None),
    "mcg_substructure_match": (_IDENTITY, "AB", None),
    "mcg_ring_scaffold": (_IDENTITY, "AB", None),
    "mcg_induced_subgraph": (_IDENTITY, "AB", None),
}
# thin forwarders -> the entry whose launches they make
ALIASES = {"mcg_handoff": "mcg_handoff_ex", "mcg_handoff_elements": "mcg_handoff_ex", "mcg_geometry_relax": "mcg_geometry_relax_ex"}
# entries the header documents as synchronising their stream, and pure test / measurement hooks: no more than these seven
EXCLUDED = {
    "mcg_debug_gemm": "test hook; the header: it 'synchronises `stream`' before it frees its operands and returns",
    "mcg_bench_edge": "measurement hook: launches one edge kernel on the plan's current state, no result to compare",
    "mcg_bench_edge_incall": "measurement hook; the header: 'Synchronises `stream`'",
    "mcg_egnn_gcl_debug": "test hook: one GCL layer on compact arrays, the result stays in the plan",
    "mcg_egnn_gcl_debug_ex": "test hook: mcg_egnn_gcl_debug with the choice of keep_agg",
    "mcg_egnn_block_debug": "test hook: one EquivariantBlock on compact arrays",
    "mcg_egnn_equiv_debug": "test hook: the coordinate layer of one block on compact arrays",
}


def stream_entries(header=HEADER):
    """The names of every prototype of the header with a `void* stream` parameter, in the header's order."""
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    names = []
    for m in re.finditer(r"\b(?:int|void)\s+(mcg_\w+)\s*\(([^;{}()]*)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            names.append(m.group(1))
    return names


def covered_by(test_name):
    """The table's entries whose GPU test is `test_name`."""
    return sorted(k for k, v in COVERAGE.items() if v[0] == test_name)


# ---- the spin -----------------------------------------------------------------------------------------------------------
_RATE = []                    # `torch.cuda._sleep` cycles per millisecond, measured once per process
LARGEST = {"delay_ms": 0.0, "entry": None}


def cycles_per_ms():
    """`torch.cuda._sleep` counts cycles of a clock this module does not assume: one call, timed by a pair of events."""
    if not _RATE:
        cycles = 5_000_000
        torch.cuda._sleep(1000)                              # the kernel's code object is loaded outside the timed call
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.05, f"a spin of {cycles} cycles took {ms} ms: no rate to calibrate by"
        _RATE.append(cycles / ms)
        print(f"\nSTREAM-PROBE calibration: torch.cuda._sleep({cycles}) took {ms:.3f} ms: {_RATE[0]:.0f} cycles per ms")
    return _RATE[0]


def delay(stream, ms, what=None):
    """A bounded spin of min(ms, MAX_DELAY_MS) enqueued on `stream`; returns the milliseconds asked of the device."""
    ms = min(float(ms), MAX_DELAY_MS)
    rate = cycles_per_ms()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * rate))
    if ms > LARGEST["delay_ms"]:
        LARGEST.update(delay_ms=ms, entry=what)
    return ms


# ---- tensors by their bits ----------------------------------------------------------------------------------------------
def flat(outputs):
    """The tensors of a call's result - a tensor, a dict, a tuple or a list of them, None left out - as a list."""
    if outputs is None:
        return []
    if torch.is_tensor(outputs):
        return [outputs]
    if isinstance(outputs, dict):
        return [t for k in outputs for t in flat(outputs[k])]
    if isinstance(outputs, (list, tuple)):
        return [t for o in outputs for t in flat(o)]
    return []                                                 # a count, a flag: host values are compared by the caller


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    """Two lists of tensors: the same number, dtypes, shapes and bits (a NaN equals itself)."""
    if len(a) != len(b):
        return False
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bytes(x), _bytes(y)) for x, y in zip(a, b))


def fill_sentinel(t):
    if t.numel():
        _bytes_view(t).fill_(SENTINEL_BYTE)


def _bytes_view(t):
    assert t.is_contiguous()
    return t.view(-1).view(torch.uint8)


def is_sentinel(t):
    return bool((_bytes(t) == SENTINEL_BYTE).all())


# ---- which entry ran on which stream ------------------------------------------------------------------------------------
class Recorder:
    """While active, every call of a stream-taking C entry through `_lib.lib()` is noted as (name, stream argument)."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        from ml_conformer_generator_amd import _lib
        self._lib, self._real = _lib, _lib.lib()
        names = set(stream_entries())
        calls = self.calls
        real = self._real

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if name not in names:
                    return fn

                def noted(*args):
                    s = args[-1]
                    calls.append((name, int(getattr(s, "value", s) or 0)))
                    return fn(*args)
                return noted
        _lib._lib = Proxy()
        return self

    def __exit__(self, *exc):
        self._lib._lib = self._real
        return False

    def names(self):
        return {n for n, _ in self.calls}

    def streams(self):
        return {s for _, s in self.calls}


class Result:
    """What an arrangement saw: `base` / `got` the default-stream and the arranged outputs (clones), `equal` their bit
    equality, `busy` (A) whether the default stream was still spinning when S had finished, `pending` (B) whether S was still
    busy when the call returned to the host, `calls` the (entry, stream) pairs of the arranged call, `stream` S's handle."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def ok(self, entries=(), raw=False):
        """The contract held: the named entries ran, every stream-taking entry was given S, the outputs are the baseline's."""
        ran = {n for n, _ in self.calls}
        assert set(entries) <= ran, f"{self.label}: {sorted(set(entries) - ran)} did not run (ran: {sorted(ran)})"
        wrong = sorted({(n, s) for n, s in self.calls if s != self.stream})
        assert not wrong, f"{self.label}: entries given another stream than the current one ({self.stream:#x}): {wrong}"
        if self.busy is not None:
            assert self.busy, (f"{self.label}: the default stream's {self.delay_ms:.0f} ms spin was over when the side stream "
                               f"had finished (baseline call {self.t_call_ms:.2f} ms): something waited for stream 0")
        if raw and self.pending is not None:
            assert self.pending, f"{self.label}: the entry blocked the host until its stream's {self.delay_ms:.0f} ms spin was over"
        assert self.equal, f"{self.label}: outputs differ from the default-stream run"
        return self


def _ms(t0):
    return (time.perf_counter() - t0) * 1e3


def quiet_host(on):
    """An arrangement measures what the CALL waits for.  A handle of an earlier test that the cyclic garbage collector
    happens to finalise in the middle of it returns driver memory (`hipFree` of a model's weights), which waits for the whole
    device - the spin included.  So: collect first, then keep the collector off until the arrangement is over."""
    if on:
        gc.collect()
        gc.disable()
    else:
        gc.enable()


def independent_stream(dev, tries=8):
    """A side stream on which the arrangements can discriminate: work on it runs while the default stream spins, and work on
    the default stream runs while it spins, also with a copy queued behind the spin (measured with torch's own fills and
    copies, nothing of the library's).  Streams share the device's hardware queues, and two that share one run in turn;
    the next stream of the pool is tried then.
    What this does NOT guarantee: that a launch the LIBRARY makes on stream 0 runs beside the spinning side stream.  Behind
    some of the suite's files it does not, in a process where every check here passes
    (`test_control_b_work_on_stream_0_computes_the_poison` holds the measurement); why the two differ is not known."""
    default = torch.cuda.default_stream(dev)
    probe, late, seen = (torch.zeros(16, device=dev) for _ in range(3))
    rate = cycles_per_ms()
    for _ in range(tries):
        S = torch.cuda.Stream(dev)
        with torch.cuda.stream(S):
            probe.fill_(1.0)                                  # (a stream sets itself up at its first use)
        torch.cuda.synchronize()
        torch.cuda._sleep(int(3 * rate))
        with torch.cuda.stream(S):
            probe.fill_(2.0)
            S.synchronize()
        side_runs = not default.query()
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            torch.cuda._sleep(int(3 * rate))
        probe.fill_(3.0)
        default.synchronize()
        default_runs = not S.query()
        torch.cuda.synchronize()
        # ... and what arrangement B sets up: a device-to-device copy queued behind S's spin, then default-stream work
        # that reads the copy's destination (the runtime may park the copy's wait for the spin in a queue other streams share)
        with torch.cuda.stream(S):
            torch.cuda._sleep(int(3 * rate))
            late.copy_(probe)
        seen.copy_(late)
        default.synchronize()
        default_runs = default_runs and not S.query()
        torch.cuda.synchronize()
        if side_runs and default_runs:
            return S
    raise AssertionError(f"none of {tries} side streams runs beside the default stream on this device")


def arrangement_a(call, label, stream=None, baseline=None, refill=()):
    """Arrangement A of this module's docstring.  `call()` makes the call on the CURRENT stream and returns its output
    tensors (`flat`); `refill`: output buffers the caller owns and `call` writes into, filled with the sentinel in front of
    the arranged call (outputs a wrapper allocates itself are met by sentinel-filled blocks left in S's allocator pool).
    `baseline` = (outputs, wall ms) of an earlier default-stream run, where the arranged call must not be preceded by one."""
    dev = torch.cuda.current_device()
    default = torch.cuda.default_stream(dev)
    S = stream if stream is not None else independent_stream(dev)
    try:
        quiet_host(True)
        if baseline is None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = flat(call())
            torch.cuda.synchronize()
            t_call = _ms(t0)
            base = [o.clone() for o in out]
            del out
        else:
            base, t_call = [o.clone() for o in flat(baseline[0])], float(baseline[1])
        for t in refill:
            fill_sentinel(t)
        with torch.cuda.stream(S):                            # blocks of the outputs' sizes, holding the sentinel, for S's allocations
            seeds = [torch.empty_like(b) for b in base]
            for t in seeds:
                fill_sentinel(t)
            del seeds
        with torch.cuda.stream(S):                            # (S's first use is not part of what is arranged)
            torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        asked = delay(default, max(MIN_DELAY_MS, A_MARGIN * t_call), label)
        with torch.cuda.stream(S), Recorder() as rec:
            got = [o.clone() for o in flat(call())]
            S.synchronize()
        busy = not default.query()
        return Result(label=label, base=base, got=got, equal=same_bits(base, got), busy=busy, pending=None, calls=rec.calls,
                      stream=S.cuda_stream, delay_ms=asked, t_call_ms=t_call, enqueue_ms=None)
    finally:
        torch.cuda.synchronize()
        quiet_host(False)


def arrangement_b(call, true, poison, label, stream=None, raw=False, refill=()):
    """Arrangement B of this module's docstring.  `call(inputs)` makes the call on the current stream from the dict of
    device tensors `inputs` and returns its output tensors; `true` / `poison`: two such dicts of the same keys, shapes and
    dtypes, both valid, that differ.  `raw`: `call` is one C entry (no wrapper around it).  `refill`: output buffers the
    caller owns, filled with the sentinel in front of the arranged call (so that a call that has not run yet is not taken
    for the baseline's answer, which those buffers would still hold)."""
    dev = torch.cuda.current_device()
    S = stream if stream is not None else independent_stream(dev)
    try:
        quiet_host(True)
        assert set(true) == set(poison)
        for k in true:
            assert true[k].shape == poison[k].shape and true[k].dtype == poison[k].dtype and true[k].is_cuda, k
        assert any(not torch.equal(_bytes(true[k]), _bytes(poison[k])) for k in true), f"{label}: the poison is the true input"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = flat(call(true))
        t_host = _ms(t0)                                      # the host time of the unsynchronised call
        torch.cuda.synchronize()
        base = [o.clone() for o in out]
        del out
        work = {k: v.clone() for k, v in poison.items()}
        for t in refill:
            fill_sentinel(t)
        torch.cuda.synchronize()
        with torch.cuda.stream(S):                            # S's first copy, kernel and spin are not part of what is arranged:
            torch.cuda._sleep(1000)                           # a stream sets itself up at its first use, on the host's time
            for k in work:
                work[k].copy_(poison[k])
            S.synchronize()
        with torch.cuda.stream(S), Recorder() as rec:
            t0 = time.perf_counter()
            asked = delay(S, max(MIN_DELAY_MS, B_MARGIN * t_host), label)
            for k in work:
                work[k].copy_(true[k])
            out = flat(call(work))
            pending = not S.query()
            enqueue_ms = _ms(t0)
            got = [o.clone() for o in out]
            S.synchronize()
        return Result(label=label, base=base, got=got, equal=same_bits(base, got), busy=None, pending=pending, calls=rec.calls,
                      stream=S.cuda_stream, delay_ms=asked, t_call_ms=t_host, enqueue_ms=enqueue_ms)
    finally:
        torch.cuda.synchronize()
        quiet_host(False)


def rolled(inputs, keys=None):
    """The poison of a batch: every per-molecule tensor of `inputs` (all of them, or those named) rolled by one row, so that
    each row holds its neighbour's molecule - valid data of the same shapes and dtypes, a different batch."""
    return {k: (v.roll(1, 0).contiguous() if keys is None or k in keys else v.clone()) for k, v in inputs.items()}
