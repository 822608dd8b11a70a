"""The stream contract of the C ABI, made testable: run a case of poison_cases.CASES where a launch on the wrong stream shows.

Nearly every test runs on the default stream, where a launch is ordered after its inputs wherever it was enqueued.  Two runs
take that cover away:

run_delayed   the case on a fresh side stream, behind a delay and a copy that only then brings the real inputs: until the delay is
              over the inputs hold a decoy (zeros) and outputs, intermediates and scratch are fresh zero-filled arenas.  A kernel or
              memset that went to another stream runs at once, on the decoy or on the zeros, and the result differs.  A proxy around
              the library notes, for every launching C call, whether the delay was still pending when the call returned: a call that
              waited for the stream, and a delay too short to prove anything, both show there.
run_captured  the case captured into a graph on a side stream after one eager warm-up there, every output and every cached scratch
              buffer zeroed, then replayed, twice.  A launch that went to another stream during capture ran eagerly and is missing
              from the graph: its output stays zero.  The second replay finds scratch that is only clean when it is allocated.

split_pack(w) without a scale reads max |w| on the host (ops.py, split_pack: "scale defaults to the power of two ...") -- a
convenience of the wrapper, outside the C ABI, whose entry point takes the scale as a host number.  `ScaleMemo` records the scales
of the eager run and hands them to the later runs, which then make the same C calls with the same arguments and no host read.

Plain helper module (like poison.py): no fixture is registered and nothing is patched on import.
"""
from __future__ import annotations

import ctypes
import time

import torch

import poison
import poison_cases
import stream_cases

# delay in front of a case = max(FLOOR_MS, FACTOR * the host time of the case's eager enqueue), see docs/experiments.md
# ("Stream contract (tests)"): the delayed run enqueues the same calls plus one copy per input, in about the eager run's time
FACTOR, FLOOR_MS = 4.0, 40.0

# every per-(device, stream) cache of ops.py: the uninitialised scratch (poison.SCRATCH_CACHES) and the ones that hold state
STATE_CACHES = ("_SCALE_SLOTS", "_OVERFLOW", "_DETECT_PINNED")

LAUNCHING = frozenset(sym for c in poison_cases.CASES for sym in c.covers)      # the entry points that enqueue work

_RATE = {}


def _timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _calibrate():
    """Once per session: how many torch.cuda._sleep cycles make a millisecond (two events around a spin of a known length); where
    the spin kernel does not scale with its argument, the milliseconds of one 2048^3 matmul of a chain instead."""
    if _RATE:
        return _RATE
    _timed(lambda: torch.cuda._sleep(1_000_000))                               # (loads the kernel)
    short, long = _timed(lambda: torch.cuda._sleep(2_000_000)), _timed(lambda: torch.cuda._sleep(20_000_000))
    if long > 4.0 * short and long > 1.0:
        _RATE.update(kind="sleep", cycles_per_ms=18_000_000 / (long - short))
    else:
        m = torch.ones(2048, 2048, device="cuda")
        _timed(lambda: m @ m)
        _RATE.update(kind="matmul", ms_each=_timed(lambda: [m @ m for _ in range(20)]) / 20, operand=m)
    return _RATE


def delay(stream, ms: float):
    """Enqueue device-only work on `stream` that keeps it busy for at least `ms`; returns an event recorded right behind it
    (event.query() == False: the delay is still pending)."""
    rate = _calibrate()
    with torch.cuda.stream(stream):
        if ms > 0:
            if rate["kind"] == "sleep":
                torch.cuda._sleep(int(ms * rate["cycles_per_ms"]) + 1)
            else:
                m = rate["operand"]
                for _ in range(int(ms / rate["ms_each"]) + 1):
                    m @ m
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


PROBE_MS = 5.0
_PROBE = []


def independent_stream(others=()):
    """A new side stream whose work the device runs beside the default stream's and beside that of `others`.  The runtime folds its
    streams onto a few hardware queues, and a launch that went to a stream on the same queue still runs in the order of submission:
    a quarter of the wrong-stream launches would pass a delayed run unseen.  So a candidate is tried: behind a short delay on it, a
    one-element kernel on each other stream must finish while the delay is pending."""
    if not _PROBE:
        _PROBE.append(torch.zeros(1, device="cuda"))
    for _ in range(32):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ev, beside = delay(s, PROBE_MS), True
        for o in (torch.cuda.default_stream(), *others):
            with torch.cuda.stream(o):
                _PROBE[0].add_(1.0)
                done = torch.cuda.Event()
                done.record(o)
            done.synchronize()
            beside = beside and not ev.query()
        ev.synchronize()
        if beside:
            return s
    raise RuntimeError("no side stream runs beside the default stream: 32 candidates all shared its hardware queue")


def delay_ms_for(host_ms: float) -> float:
    return max(FLOOR_MS, FACTOR * host_ms)


# ------------------------------------------------------------------------------------------------ inputs, decoys, outputs
def _map(obj, fn):
    if isinstance(obj, torch.Tensor):
        return fn(obj)
    if isinstance(obj, dict):
        return {k: _map(v, fn) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and obj and all(isinstance(v, torch.Tensor) for v in obj):
        return type(obj)(fn(v) for v in obj)
    return obj


def tensors_of(obj):
    out = []
    _map(obj, lambda t: out.append(t) or t)
    return out


def decoy_inputs(case) -> dict:
    """CPU inputs of build()'s structure that are a valid call and NOT the real inputs: zeros, or the case's own decoy."""
    own = stream_cases.OWN_DECOY.get(case.name)
    return own() if own is not None else _map(case.build(), torch.zeros_like)


def host(outputs):
    torch.cuda.synchronize()
    return [None if t is None else t.detach().cpu().clone() for t in outputs]


def setup(case, monkeypatch):
    for k, v in (case.env or {}).items():
        monkeypatch.setenv(k, v)


class ScaleMemo:
    """ops.split_pack with the host read of max |w| taken out of the later runs: `record` notes the scale of every call that left
    the choice to split_pack, `replay` passes them back in the order of the calls."""

    def __init__(self, scales=None):
        self.scales = [] if scales is None else list(scales)

    def install(self, monkeypatch, replay: bool):
        from locov_amd import ops
        real, todo = ops.split_pack, list(self.scales)

        def split_pack(w, scale=None):
            if scale is not None:
                return real(w, scale)
            if replay:
                return real(w, todo.pop(0))
            packed = real(w)
            self.scales.append(packed.scale)
            return packed

        monkeypatch.setattr(ops, "split_pack", split_pack)
        return lambda: monkeypatch.setattr(ops, "split_pack", real)


class PendingRecorder:
    """Proxy around the ctypes library (as poison.Recorder): for every launching locov_* call made while `event` is set, whether the
    event was still pending when the call returned -- [(symbol, pending)] in the order of the calls -- and every non-null pointer the
    calls were given (device pointers and the stream handle)."""

    def __init__(self, lib):
        object.__setattr__(self, "_real", lib)
        object.__setattr__(self, "calls", [])
        object.__setattr__(self, "pointers", set())
        object.__setattr__(self, "event", None)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in LAUNCHING:
            return fn

        def call(*args):
            rc = fn(*args)
            if self.event is not None:
                self.calls.append((name, not self.event.query()))
                self.pointers.update(a.value for a in args if isinstance(a, ctypes.c_void_p) and a.value)
            return rc
        return call

    def __setattr__(self, name, value):
        if name == "event":
            object.__setattr__(self, name, value)
        else:
            setattr(self._real, name, value)


# ------------------------------------------------------------------------------------------------ the three runs
def run_eager(case, monkeypatch):
    """The case alone on the default stream, fresh zero-filled scratch: (host outputs, the host milliseconds of an enqueue -- taken
    before any synchronise --, the scales split_pack chose).  The outputs are the first run's; the time is a second run's, without
    what only a session's first call of an op pays (loading its kernels, starting the autograd engine: up to 0.7 s, which the
    delayed run does not pay again).  The caller has applied case.env (setup)."""
    inputs = poison_cases.to_device(case.build())
    torch.cuda.synchronize()
    memo = ScaleMemo()
    undo = memo.install(monkeypatch, replay=False)
    poison.fresh_scratch(monkeypatch)
    with poison.poisoned(0x00):
        torch.manual_seed(0)
        got = host(case.run(inputs))
    undo()
    undo = ScaleMemo(memo.scales).install(monkeypatch, replay=True)
    poison.fresh_scratch(monkeypatch)
    with poison.poisoned(0x00):
        torch.manual_seed(0)
        t0 = time.perf_counter()
        again = case.run(inputs)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        del again
    undo()
    return got, host_ms, memo.scales


def run_on_decoy(case, monkeypatch):
    """The case, eagerly, on the decoy inputs: what a kernel that ran before the real inputs arrived would have computed."""
    inputs = poison_cases.to_device(decoy_inputs(case))
    torch.cuda.synchronize()
    poison.fresh_scratch(monkeypatch)
    with poison.poisoned(0x00):
        torch.manual_seed(0)
        return host(case.run(inputs))


def delayed_inputs(case):
    """(real inputs, decoy inputs) on the device; the caller synchronises before it enqueues behind a delay."""
    return poison_cases.to_device(case.build()), poison_cases.to_device(decoy_inputs(case))


def run_delayed(case, monkeypatch, lib, ms: float, scales=()):
    """-> (host outputs, [(symbol, pending)]).  See the module docstring."""
    inputs = delayed_inputs(case)
    torch.cuda.synchronize()
    poison.fresh_scratch(monkeypatch)
    with poison.poisoned(0x00):
        side = independent_stream()
        job = enqueue_delayed(case, monkeypatch, lib, inputs, side, delay(side, ms), scales)
        return host(job["out"]), job["calls"]


def enqueue_delayed(case, monkeypatch, lib, inputs, side, event, scales=()):
    """The enqueueing part of run_delayed, inside the caller's fresh_scratch and poisoned(0x00): on `side`, behind the delay whose
    event is `event`, the copy of the real inputs over the decoy and the case.  Nothing is waited for here, so one thread can put
    two cases on two streams.  -> dict(out=device outputs, calls=[(symbol, pending)], pointers={every pointer the calls were given}); the caller reads `out` (host) before it
    leaves the poisoned context."""
    from locov_amd import _lib
    real, decoy = inputs
    rec = PendingRecorder(lib)
    monkeypatch.setattr(_lib, "_lib", rec)
    undo = ScaleMemo(scales).install(monkeypatch, replay=True)
    try:
        with torch.cuda.stream(side):
            torch.manual_seed(0)
            rec.event = event
            for d, r in zip(tensors_of(decoy), tensors_of(real)):
                d.copy_(r, non_blocking=True)
            out = case.run(decoy)
    finally:
        rec.event = None
        undo()
        monkeypatch.setattr(_lib, "_lib", lib)
    return dict(out=out, calls=rec.calls, pointers=rec.pointers)


def stream_scratch(stream):
    """Every cached device tensor the package keeps for `stream` (scratch, scale-slot ring, range-guard word)."""
    from locov_amd import ops
    found = []
    for name in poison.SCRATCH_CACHES + STATE_CACHES:
        for key, value in getattr(ops, name).items():
            if stream.cuda_stream in key:
                found += [t for t in (value if isinstance(value, (list, tuple)) else [value]) if isinstance(t, torch.Tensor) and t.is_cuda]
    return found


def run_captured(case, monkeypatch, scales=()):
    """-> [host outputs of the first replay, of the second].  See the module docstring.  The caches the case filled for its stream
    are gone when the test ends (monkeypatch, as poison.fresh_scratch)."""
    from locov_amd import ops
    inputs = poison_cases.to_device(case.build())
    torch.cuda.synchronize()
    poison.fresh_scratch(monkeypatch)
    for name in STATE_CACHES:
        monkeypatch.setattr(ops, name, dict(getattr(ops, name)))
    s = torch.cuda.Stream()
    undo = [ScaleMemo(scales).install(monkeypatch, replay=True)]
    torch.manual_seed(0)
    with torch.cuda.stream(s):
        case.run(inputs)                                                       # warm-up: sizes the caches of this stream
    s.synchronize()
    for u in undo:
        u()
    undo = [ScaleMemo(scales).install(monkeypatch, replay=True)]
    graph = torch.cuda.CUDAGraph()
    torch.manual_seed(0)
    try:
        with torch.cuda.graph(graph, stream=s):
            out = case.run(inputs)
    finally:
        for u in undo:
            u()
    given = {t.untyped_storage().data_ptr() for t in tensors_of(inputs)}
    replays = []
    for _ in range(2):
        for t in list(out) + stream_scratch(s):
            if t is not None and t.untyped_storage().data_ptr() not in given:
                t.detach().zero_()
        torch.cuda.synchronize()
        graph.replay()
        replays.append(host(out))
    del graph
    return replays
