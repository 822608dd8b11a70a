"""Every op on poisoned outputs and scratch (tests/poison.py, tests/poison_cases.py): no result may depend on memory the call did
not write.

History comparison (cases with a `history`): a larger call first, then the case, in ONE set of caches -- the scratch the case
works in still holds a real earlier call's data (valid indices, plausible values) -- against the case run alone.
Pattern comparison (every case): the case under 0x00, 0x7B and 0xFF in every output and every scratch byte, fresh scratch each
time.  Every returned tensor must be the same bytes in the three runs, the guard bands around every allocation intact, no
allocation left unpoisoned, and the C symbols the case claims to cover must have been called.

Each case chains its ops inside one `poisoned` context, in which nothing is recycled (every arena is kept alive), so the second
op of a case cannot be handed the first one's freed block.  Cached scratch is another matter: a case that makes two calls on the
same scratch calls `poison.repoison_scratch()` between them, which refills the scratch arenas alone (`repoison()` refills the
outputs too, which are the later op's inputs), so that the second call does not work in the first call's data.

A case with a `tier` also proves which kernel it ran: the library's GEMM launch record of the first run (or, where the choice is
made elsewhere, the library's rule restated on the case's inputs) must show the tier the case's name claims.

poison.NONREPRODUCIBLE lists the outputs that already differ between two runs under the SAME pattern, with the reason read from the
kernel; they are compared with the gate of the op's own reference test plus equal NaN / inf positions."""
import pytest
import torch

import poison
import poison_cases
from poison import compare as _compare
from poison_cases import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import _lib
    return _lib.load()


def _host(outputs):
    torch.cuda.synchronize()
    return [None if t is None else t.detach().cpu().clone() for t in outputs]


def _setup(case, monkeypatch):
    for k, v in (case.env or {}).items():
        monkeypatch.setenv(k, v)


def _gemm_launches(lib, fn):
    """(fn(), {class: launches}): the library's own record of the GEMM kernels fn launched (locov_gemm_timing_*)."""
    import ctypes
    from locov_amd import _lib
    torch.cuda.synchronize()
    lib.locov_gemm_timing_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        n = {}
        for cls in poison_cases.GEMM_CLASSES:
            c, ms, fl = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            _lib.check(lib.locov_gemm_timing_read(cls, ctypes.byref(c), ctypes.byref(ms), ctypes.byref(fl)), "locov_gemm_timing_read")
            n[cls] = c.value
    finally:
        lib.locov_gemm_timing_enable(0)
    return out, n


HISTORY = [c for c in CASES if c.history is not None]


@pytest.mark.parametrize("case", HISTORY, ids=[c.name for c in HISTORY])
def test_a_larger_call_before_leaves_nothing_behind(lib, monkeypatch, case):
    _setup(case, monkeypatch)
    inputs, larger = poison_cases.to_device(case.build()), poison_cases.to_device(case.history())
    poison.fresh_scratch(monkeypatch)
    torch.manual_seed(0)
    _host(case.run(larger))
    torch.manual_seed(0)
    after = _host(case.run(inputs))
    poison.fresh_scratch(monkeypatch)
    torch.manual_seed(0)
    alone = _host(case.run(inputs))
    _compare(case, after, alone, "after the larger call")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_results_do_not_depend_on_what_outputs_and_scratch_held(lib, monkeypatch, case):
    from locov_amd import _lib
    _setup(case, monkeypatch)
    rec = poison.Recorder(lib)
    monkeypatch.setattr(_lib, "_lib", rec)
    host_inputs = case.build()
    inputs = poison_cases.to_device(host_inputs)
    runs = {}
    for pattern in poison.PATTERNS:
        poison.fresh_scratch(monkeypatch)
        with poison.poisoned(pattern) as st:
            torch.manual_seed(0)
            if case.tier is not None and pattern == poison.PATTERNS[0]:
                out, launched = _gemm_launches(lib, lambda: case.run(inputs))
                case.tier(launched, host_inputs)
                runs[pattern] = _host(out)
            else:
                runs[pattern] = _host(case.run(inputs))
            broken = st.broken_guards()
            assert not broken, f"{case.name} under 0x{pattern:02X}: guard bands written (arena, body bytes, side): {broken[:8]}"
            assert st.passed_through == 0, f"{case.name}: allocations that were not poisoned: {st.passed_through_calls}"
    first = poison.PATTERNS[0]
    for pattern in poison.PATTERNS[1:]:
        _compare(case, runs[pattern], runs[first], f"under 0x{pattern:02X} against 0x{first:02X}")
    missing = set(case.covers) - rec.called
    assert not missing, f"{case.name} did not reach {sorted(missing)}"
