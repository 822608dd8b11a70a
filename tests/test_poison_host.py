"""CPU tests of the poisoned-allocation harness (tests/poison.py) on CPU tensors, and of the case table's coverage of the C ABI."""
import pytest
import torch

import poison
import poison_cases
from locov_amd import _lib

CPU = dict(device_types=("cpu",))


def _with_a_hole(n, hole):
    """A 'kernel' that leaves one output element unwritten."""
    out = torch.empty(n, dtype=torch.float32, device="cpu")
    for i in range(n):
        if i != hole:
            out[i] = float(i)
    return out


def _three_patterns(fn):
    runs = []
    for pattern in poison.PATTERNS:
        with poison.poisoned(pattern, **CPU) as st:
            runs.append(fn().clone())
            assert st.guards_intact() and st.passed_through == 0
    return runs


def test_a_function_with_a_hole_is_caught_and_a_complete_one_is_not():
    a, b, c = _three_patterns(lambda: _with_a_hole(37, 36))               # (the last element: a skipped ragged tail)
    assert not poison.same_bits(a, b) or not poison.same_bits(a, c)
    assert torch.isnan(c[36]) and a[36] == 0 and torch.isfinite(b[36]) and b[36] > 1e35
    a, b, c = _three_patterns(lambda: _with_a_hole(37, -1))
    assert poison.same_bits(a, b) and poison.same_bits(a, c)
    keep = torch.ones(37, dtype=torch.bool)
    keep[36] = False
    a, b, c = _three_patterns(lambda: _with_a_hole(37, 36))
    assert poison.same_bits(a, c, keep) and poison.same_bits(a, b, keep)  # the hole under an `unspecified` mask


def test_nan_payloads_and_signed_zeros_count_as_differences():
    assert not poison.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    nan = torch.tensor([float("nan")])
    assert poison.same_bits(nan, nan.clone())
    other = (nan.view(torch.int32) ^ 1).view(torch.float32)
    assert torch.isnan(other).all() and not poison.same_bits(nan, other)
    assert not poison.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
    assert poison.same_bits(torch.zeros(0), torch.zeros(0)) and poison.same_bits(torch.tensor(1.5), torch.tensor(1.5))


@pytest.mark.parametrize("side", ["front", "back"])
def test_a_one_byte_overrun_on_either_side_breaks_the_guards(side):
    with poison.poisoned(0x7B, **CPU) as st:
        t = torch.empty((3, 5), dtype=torch.int16, device="cpu")
        t.zero_()
        assert poison.guards_intact()
        raw, nbytes = st.arenas[-1]
        assert raw.numel() == nbytes + 2 * poison.GUARD and nbytes == 30
        at = poison.GUARD - 1 if side == "front" else poison.GUARD + nbytes
        raw[at] = 0
        assert not poison.guards_intact() and st.broken_guards() == [(0, 30, side)]
        poison.repoison()
        assert poison.guards_intact() and bool((t == 0x7B7B).all())       # (the body is refilled too)


def test_the_scratch_refill_touches_the_scratch_arenas_alone(monkeypatch):
    from locov_amd import ops
    assert poison.repoison_scratch() == 0                                 # outside a context: nothing to do
    with monkeypatch.context() as m, poison.poisoned(0x7B, **CPU):
        poison.fresh_scratch(m)
        out = torch.empty(4, dtype=torch.uint8, device="cpu").zero_()
        ops._WS["k"] = torch.empty(8, dtype=torch.uint8, device="cpu").zero_()
        own = torch.empty(8, dtype=torch.uint8, device="cpu").zero_()
        assert poison.repoison_scratch() == 1 and bool((ops._WS["k"] == 0x7B).all()) and bool((out == 0).all()) and bool((own == 0).all())
        assert poison.repoison_scratch(own, None) == 2 and bool((own == 0x7B).all()) and bool((out == 0).all())


def test_shapes_dtypes_and_the_three_entry_points():
    with poison.poisoned(0xFF, **CPU) as st:
        z = torch.empty(0, dtype=torch.float32, device="cpu")
        s = torch.empty((), dtype=torch.float32, device="cpu")
        h = torch.empty(2, 3, dtype=torch.bfloat16, device="cpu")
        i = torch.empty([4], dtype=torch.int64, device=torch.device("cpu"), requires_grad=False)
        like = torch.empty_like(h, memory_format=torch.contiguous_format)
        like64 = torch.empty_like(i, dtype=torch.float64)
        new = i.new_empty((2, 2))
        new8 = i.new_empty(5, dtype=torch.uint8)
        assert z.shape == (0,) and s.shape == () and torch.isnan(s) and torch.isnan(h.float()).all() and h.shape == (2, 3)
        assert bool((i == -1).all()) and like.dtype == torch.bfloat16 and like.shape == (2, 3) and torch.isnan(like64).all()
        assert new.dtype == torch.int64 and bool((new == -1).all()) and new8.dtype == torch.uint8 and bool((new8 == 255).all())
        for t in (z, s, h, i, like, like64, new, new8):
            assert t.is_contiguous() and t.data_ptr() % 2 == 0 and t._base is None
        assert len(st.arenas) == 8 and st.passed_through == 0 and st.guards_intact()
        g = torch.empty(3, dtype=torch.float32, device="cpu", requires_grad=True)
        assert g.requires_grad and g.is_leaf
        assert torch.empty(3).shape == (3,) and len(st.arenas) == 9       # no device given: the default device, left alone here


def test_other_devices_and_pinned_memory_pass_through_untouched():
    with poison.poisoned(0xFF) as st:                                     # (the default: device tensors only)
        t = torch.empty(5, dtype=torch.int32, device="cpu")
        u = torch.empty_like(t)
        v = t.new_empty(3)
        assert st.arenas == [] and st.passed_through == 0 and (t.shape, u.shape, v.shape) == ((5,), (5,), (3,))


def test_an_unusual_keyword_passes_through_and_is_counted():
    with poison.poisoned(0x00, **CPU) as st:
        a = torch.empty(2, 3, 4, 5, device="cpu", memory_format=torch.channels_last)
        assert st.passed_through == 1 and "channels_last" in st.passed_through_calls[0] and a.shape == (2, 3, 4, 5)
        b = torch.empty_like(torch.zeros(4, 6).t())                       # preserve_format of a transposed tensor: strides kept
        assert st.passed_through == 2 and b.stride() == (1, 6)
        out = torch.zeros(3)
        torch.empty(3, device="cpu", out=out)
        assert st.passed_through == 3 and st.arenas == []


def test_the_original_functions_are_back_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    with pytest.raises(RuntimeError, match="inside"):
        with poison.poisoned(0xFF, **CPU):
            assert torch.empty is not before[0]
            with poison.poisoned(0x00, **CPU) as inner:                   # nested: the innermost one is the active one
                assert bool((torch.empty(2, device="cpu") == 0).all()) and len(inner.arenas) == 1
            assert torch.isnan(torch.empty(2, device="cpu")).all()
            raise RuntimeError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__) == before
    with pytest.raises(RuntimeError, match="no poisoned"):
        poison.guards_intact()


def test_fresh_scratch_empties_the_scratch_caches_and_only_those(monkeypatch):
    from locov_amd import ops
    marker = object()
    kept = {name: getattr(ops, name) for name in ("_OVERFLOW", "_SCALE_SLOTS", "_DETECT_PINNED")}
    with monkeypatch.context() as m:
        for name in ("_WS", "_WINO_WS", "_SEGMEAN_WS"):
            m.setitem(getattr(ops, name), "stale", marker)
        poison.fresh_scratch(m)
        assert ops._WS == {} and ops._WINO_WS == {} and ops._SEGMEAN_WS == {}
        assert all(getattr(ops, name) is d for name, d in kept.items())
    assert ops._WS.get("stale") is None


def test_the_recorder_notes_the_symbols_a_case_called():
    class Fake:
        def locov_one(self):
            return 1
        other = 7
    rec = poison.Recorder(Fake())
    assert rec.locov_one() == 1 and rec.other == 7 and rec.called == {"locov_one"}
    with pytest.raises(AttributeError):
        rec.locov_missing


# ---------------------------------------------------------------------------------------------------------------------- coverage
# Entry points without a case.  Allowed here only: a body that launches nothing and writes no device memory (a hipMemsetAsync
# counts as writing).
_SIZE = "host arithmetic on its arguments: returns a byte count, launches nothing, touches no device memory"
_RULE = "the library's own yes / no rule on host integers: launches nothing, touches no device memory"
EXCLUDED = {
    "locov_abi_version": "returns a constant",
    "locov_last_error": "returns the thread's last error string (host memory)",
    "locov_launch_count": "reads a host-side counter",
    "locov_device_info": "hipGetDeviceProperties into three host ints",
    "locov_gemm_timing_enable": "sets the process-global measurement switch and clears the recorded host-side event list; no launch",
    "locov_gemm_timing_read": "waits for recorded events and sums their durations into host doubles (measurement aid)",
    "locov_gemm_timing_read_ex": "the same, plus the algorithmic byte count (host arithmetic)",
    "locov_roi_align_plan_bytes": _SIZE,
    "locov_gemm_segmean_supported": _RULE,
    "locov_resize_supported": _RULE,
    "locov_augment_supported": _RULE,
    **{name: _SIZE for name in _lib.SIGNATURES if name.endswith("_workspace_bytes") or name.endswith("_workspace_bytes_for")},
}


def test_every_entry_point_has_a_case_or_a_stated_reason():
    covered = set().union(*(c.covers for c in poison_cases.CASES))
    everything = set(_lib.SIGNATURES)
    assert covered <= everything, sorted(covered - everything)
    assert not covered & set(EXCLUDED), sorted(covered & set(EXCLUDED))
    assert covered | set(EXCLUDED) == everything, f"entry points without a poison case: {sorted(everything - covered - set(EXCLUDED))}"
    assert all(reason.strip() for reason in EXCLUDED.values())


def test_the_table_is_well_formed_and_builds_on_the_cpu():
    names = [c.name for c in poison_cases.CASES]
    assert len(set(names)) == len(names)
    for c in poison_cases.CASES:
        assert c.covers, c.name
        for build in (c.build, c.history):
            if build is None:
                continue
            d = build()
            assert isinstance(d, dict) and all(not t.is_cuda for t in d.values() if isinstance(t, torch.Tensor)), c.name
        for index, mask, sentence in c.unspecified:
            assert isinstance(index, int) and callable(mask) and len(sentence) > 20, c.name
        assert all(k.startswith("LOCOV_") for k in (c.env or {})), c.name
        assert c.tier is None or callable(c.tier), c.name
    # a dispatch switch without a proof of what it selected would let a case silently duplicate its neighbour
    assert all(c.tier is not None for c in poison_cases.CASES if c.env), [c.name for c in poison_cases.CASES if c.env and c.tier is None]
