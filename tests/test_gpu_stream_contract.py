"""Every op's stream contract (tests/stream_contract.py, tests/stream_cases.py): a call only enqueues work on the stream it is given.

The eager result of a case is the case alone on the default stream with fresh zero-filled scratch, computed once per session and
shared.  Against it, under the comparison rule of the poison tests (poison.compare: bit equality, the `unspecified` masks, the
NONREPRODUCIBLE gates of the atomic ROIAlign backward):

  behind a delay on a side stream   while the delay runs the inputs hold a decoy and everything else zeros, so a launch or memset
                                    that left the stream computes something else; every launching C call must return while the
                                    delay is pending (stream_cases.LATE_CALLS excepted, never the first call) -- which also fails a
                                    delay too short to prove anything
  the decoy                         run eagerly it must give other bytes than the real inputs, or the run above proves nothing
  capture and two replays           outputs and cached scratch zeroed before each replay: a launch that left the stream is missing
                                    from the graph, scratch that is only clean at allocation shows at the second replay
  two streams, one thread           two calls that use the same per-(device, stream) cache, each behind its own delay

The delay of a case is stream_contract.delay_ms_for(the host time of its eager enqueue), see docs/experiments.md."""
import pytest
import torch

import poison
import stream_cases
import stream_contract as sc
from poison_cases import CASES

pytestmark = pytest.mark.gpu

_EAGER = {}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import _lib
    return _lib.load()


def _eager(case, monkeypatch):
    """(host outputs, host ms of the enqueue, split_pack's scales) of the case's eager run: once per session, never changed."""
    if case.name not in _EAGER:
        _EAGER[case.name] = sc.run_eager(case, monkeypatch)
    return _EAGER[case.name]


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_results_behind_a_delay_on_a_side_stream_equal_eager(lib, monkeypatch, case):
    sc.setup(case, monkeypatch)
    want, host_ms, scales = _eager(case, monkeypatch)
    ms = sc.delay_ms_for(host_ms)
    got, calls = sc.run_delayed(case, monkeypatch, lib, ms, scales)
    print(f"{case.name}: eager enqueue {host_ms:.2f} ms, delay {ms:.0f} ms, calls {calls}")
    assert calls or not case.covers, f"{case.name} made no C call"
    late = [(i, sym) for i, (sym, pending) in enumerate(calls)
            if not pending and (i == 0 or (case.name, sym) not in stream_cases.LATE_CALLS)]
    assert not late, (f"{case.name}: calls that returned after the {ms:.0f} ms delay in front of them was over (a call that waits for "
                      f"its stream, or a delay too short for an enqueue of {host_ms:.2f} ms): {late}")
    poison.compare(case, got, want, "behind a delay on a side stream against eager")


SENSITIVE = [c for c in CASES if c.name not in stream_cases.INSENSITIVE]


@pytest.mark.parametrize("case", SENSITIVE, ids=_ids(SENSITIVE))
def test_the_decoy_would_have_been_noticed(lib, monkeypatch, case):
    sc.setup(case, monkeypatch)
    want = _eager(case, monkeypatch)[0]
    got = sc.run_on_decoy(case, monkeypatch)
    assert len(got) == len(want)
    differ = [i for i, (a, b) in enumerate(zip(got, want)) if a is not None and b is not None and not poison.same_bits(a, b)]
    assert differ, f"{case.name}: every output is the same bytes on the decoy inputs as on the real ones"


CAPTURED = stream_cases.capture_set(CASES)


@pytest.mark.parametrize("case", CAPTURED, ids=_ids(CAPTURED))
def test_capture_and_two_replays_equal_eager(lib, monkeypatch, case):
    sc.setup(case, monkeypatch)
    want, _, scales = _eager(case, monkeypatch)
    first, second = sc.run_captured(case, monkeypatch, scales)
    poison.compare(case, first, want, "first replay of the captured case against eager")
    poison.compare(case, second, want, "second replay of the captured case against eager")


def _larger(name):
    case = next(c for c in CASES if c.name == name)
    return case._replace(name=name, build=case.history, history=None)


def _case(name):
    return next(c for c in CASES if c.name == name)


# (first, second, the per-(device, stream) caches both use).  The larger call goes first: the smaller one would otherwise be handed a
# cache entry that a shared key had just replaced.  A case with a host read goes second (it waits for its own stream).
PAIRS = [
    (lambda: _larger("winograd_conv3x3_f32"), lambda: _case("winograd_conv3x3_f32"), "_WINO_WS"),
    (lambda: _larger("gemm_tn_split"), lambda: _case("gemm_tn_split"), "_WS, _SCALE_SLOTS"),
    (lambda: _larger("linear_split_segmean_128"), lambda: _case("linear_split_segmean_128"), "_SEGMEAN_WS, _OVERFLOW"),
    (lambda: _case("mha_3x2x17x32"), lambda: _case("linear_split_128"), "_OVERFLOW"),
    (lambda: _case("linear_split_128"), lambda: _case("nms_321"), "_WS"),
    (lambda: _case("mha_3x2x17x32"), lambda: _case("detect_postprocess"), "_WS, _DETECT_PINNED"),
]


@pytest.mark.parametrize("pair", PAIRS, ids=[p[2].replace(", ", "+") + f"-{i}" for i, p in enumerate(PAIRS)])
def test_two_streams_from_one_thread_do_not_share_a_cache(lib, monkeypatch, pair):
    """Extends test_gpu_winograd.test_concurrent_streams_do_not_share_the_workspace to the other per-stream caches: two calls,
    each behind its own delay on its own stream, enqueued one after the other from this thread, run side by side on the device."""
    a, b = pair[0](), pair[1]()
    for case in (a, b):
        sc.setup(case, monkeypatch)
    eager = [sc.run_eager(case, monkeypatch) for case in (a, b)]                   # (the larger builds are not in the shared table)
    ms = sum(sc.delay_ms_for(e[1]) for e in eager)
    inputs = [sc.delayed_inputs(case) for case in (a, b)]
    torch.cuda.synchronize()
    poison.fresh_scratch(monkeypatch)
    with poison.poisoned(0x00):
        streams = [sc.independent_stream()]
        streams.append(sc.independent_stream(streams))
        events = [sc.delay(s, ms) for s in streams]
        jobs = [sc.enqueue_delayed(case, monkeypatch, lib, inp, s, ev, e[2])
                for case, inp, s, ev, e in zip((a, b), inputs, streams, events, eager)]
        got = [sc.host(job["out"]) for job in jobs]
    # fresh inputs, fresh outputs, a scratch buffer and a state word per stream: the two calls may not have been given one pointer in
    # common (what a cache key that drops the stream does, whether or not the two calls happened to overlap on the device)
    shared = jobs[0]["pointers"] & jobs[1]["pointers"]
    assert not shared, f"{a.name} and {b.name} on two streams were given the same memory: {sorted(hex(p) for p in shared)}"
    for case, job, g, e in zip((a, b), jobs, got, eager):
        assert job["calls"] and all(pending for _, pending in job["calls"]), f"{case.name}: calls that returned after the delay: {job['calls']}"
        poison.compare(case, g, e[0], "beside another call on a second stream against eager")
