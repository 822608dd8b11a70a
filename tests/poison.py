"""Poisoned allocations: run an op on outputs and scratch that hold a chosen byte pattern, with guard bands.

ops.py allocates its outputs and its cached scratch with torch.empty, so a test cannot hand an op a canary buffer, and a
second call usually gets back the block the first one freed -- with the right answer in it.  `poisoned(pattern)` replaces
torch.empty / torch.empty_like / Tensor.new_empty for device tensors while it is active: every allocation is the middle
of a larger uint8 arena filled with `pattern`, kept alive until the context ends.  A result that differs between
patterns depends on memory the call never wrote; a guard byte that changed was written out of bounds.

Plain helper module (like split_ref.py): no fixture is registered and nothing is patched on import.
"""
from __future__ import annotations

import contextlib

import torch

PATTERNS = (0x00, 0x7B, 0xFF)     # zeros (fresh hipMalloc) / a large finite float, a large int / NaN in every float type, -1 in every int
GUARD = 4096                      # bytes on each side: a multiple of 256, so the caller-visible pointer keeps the allocator's alignment

_ACTIVE = []                      # innermost last


class Arenas:
    """What one `poisoned` context recorded."""

    def __init__(self, pattern: int, guard: int, device_types):
        if not 0 <= int(pattern) <= 255 or guard < 0 or guard % 256:
            raise ValueError("pattern is one byte; guard a multiple of 256")
        self.pattern, self.guard, self.device_types = int(pattern), int(guard), tuple(device_types)
        self.arenas = []                  # (raw uint8 tensor, body bytes): strong references, nothing is recycled inside a case
        self.passed_through = 0           # allocations on a poisoned device type that went to the real function
        self.passed_through_calls = []    # ... and what they were

    def allocate(self, real_empty, shape, dtype, device):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        nbytes = n * dtype.itemsize       # (not from a torch.empty(...) call: that would come back here)
        raw = real_empty(nbytes + 2 * self.guard, dtype=torch.uint8, device=device)
        raw.fill_(self.pattern)
        self.arenas.append((raw, nbytes))
        # not a view of raw: a tensor of its own on raw's storage, so autograd sees no view inside a Function.forward
        return real_empty(0, dtype=dtype, device=device).set_(raw.untyped_storage(), self.guard // dtype.itemsize, shape)

    def note(self, what: str):
        self.passed_through += 1
        self.passed_through_calls.append(what)

    def guards_intact(self) -> bool:
        return not self.broken_guards()

    def broken_guards(self):
        """[(arena index, body bytes, 'front' | 'back')] of every guard band that no longer holds the pattern."""
        bad = []
        for i, (raw, nbytes) in enumerate(self.arenas):
            g = self.guard
            if g and not bool((raw[:g] == self.pattern).all()):
                bad.append((i, nbytes, "front"))
            if g and not bool((raw[g + nbytes:] == self.pattern).all()):
                bad.append((i, nbytes, "back"))
        return bad

    def repoison(self) -> None:
        for raw, _ in self.arenas:
            raw.fill_(self.pattern)

    def repoison_tensors(self, tensors) -> int:
        """Refill the arenas that back `tensors` (guards and body); returns how many were found."""
        wanted = {t.untyped_storage().data_ptr() for t in tensors if t is not None}
        n = 0
        for raw, _ in self.arenas:
            if raw.untyped_storage().data_ptr() in wanted:
                raw.fill_(self.pattern)
                n += 1
        return n


def _active() -> Arenas:
    if not _ACTIVE:
        raise RuntimeError("no poisoned() context is active")
    return _ACTIVE[-1]


def guards_intact() -> bool:
    """Every guard byte of every arena of the innermost active context still equals its pattern."""
    return _active().guards_intact()


def repoison() -> None:
    """Refill every recorded arena of the innermost active context, guards and body, with its pattern (between two calls of a
    case, after the first call's results were cloned to the host)."""
    _active().repoison()


_MISSING = object()
_HANDLED = {"dtype", "device", "memory_format", "requires_grad"}


def _size_of(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(args[0])
    if all(isinstance(a, int) or (isinstance(a, torch.Tensor) and a.dim() == 0) for a in args):
        return tuple(int(a) for a in args)
    return None


@contextlib.contextmanager
def poisoned(pattern: int, guard: int = GUARD, device_types=("cuda",)):
    """While active, torch.empty / torch.empty_like / Tensor.new_empty on `device_types` return the middle of a uint8 arena of
    nbytes + 2 * guard bytes filled with the byte `pattern`.  Other devices (CPU, pinned) pass through untouched.  Yields the
    Arenas record: `.guards_intact()`, `.repoison()`, `.passed_through` (allocations with a keyword this helper does not
    model, which went to the real function unpoisoned)."""
    st = Arenas(pattern, guard, device_types)
    real_empty, real_empty_like = torch.empty, torch.empty_like
    real_new_empty = torch.Tensor.new_empty
    own_new_empty = torch.Tensor.__dict__.get("new_empty", _MISSING)

    def wanted(device) -> bool:
        return device is not None and torch.device(device).type in st.device_types

    def finish(kwargs, shape, dtype, device):
        t = st.allocate(real_empty, shape, dtype, device)
        return t.requires_grad_(True) if kwargs.get("requires_grad") else t

    def plain(kwargs) -> bool:
        return set(kwargs) <= _HANDLED and kwargs.get("memory_format", torch.contiguous_format) is torch.contiguous_format

    def empty(*args, **kwargs):
        if not wanted(kwargs.get("device")) or kwargs.get("pin_memory"):
            return real_empty(*args, **kwargs)
        size = _size_of(args)
        if size is None or not plain(kwargs):
            st.note(f"torch.empty{args} {kwargs}")
            return real_empty(*args, **kwargs)
        return finish(kwargs, size, kwargs.get("dtype") or torch.get_default_dtype(), torch.device(kwargs["device"]))

    def empty_like(inp, *args, **kwargs):
        device = kwargs.get("device", inp.device)
        if not wanted(device):
            return real_empty_like(inp, *args, **kwargs)
        mf = kwargs.get("memory_format", torch.preserve_format)
        dense = mf is torch.contiguous_format or (mf is torch.preserve_format and inp.is_contiguous())
        if args or not set(kwargs) <= _HANDLED or not dense:
            st.note(f"torch.empty_like({tuple(inp.shape)}, {inp.dtype}, strides {inp.stride()}) {args} {kwargs}")
            return real_empty_like(inp, *args, **kwargs)
        return finish(kwargs, inp.shape, kwargs.get("dtype") or inp.dtype, torch.device(device))

    def new_empty(self, *args, **kwargs):
        device = kwargs.get("device", self.device)
        if not wanted(device) or kwargs.get("pin_memory"):
            return real_new_empty(self, *args, **kwargs)
        size = _size_of(args) if args else (tuple(kwargs["size"]) if "size" in kwargs else None)
        kw = {k: v for k, v in kwargs.items() if k != "size"}
        if size is None or not set(kw) <= (_HANDLED - {"memory_format"}):
            st.note(f"Tensor.new_empty{args} {kwargs}")
            return real_new_empty(self, *args, **kwargs)
        return finish(kw, size, kw.get("dtype") or self.dtype, torch.device(device))

    _ACTIVE.append(st)
    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield st
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like
        if own_new_empty is _MISSING:
            del torch.Tensor.new_empty
        else:
            torch.Tensor.new_empty = own_new_empty
        _ACTIVE.remove(st)
        st.arenas.clear()


SCRATCH_CACHES = ("_WS", "_WINO_WS", "_SEGMEAN_WS")


def repoison_scratch(*more) -> int:
    """Between two scratch-using calls of ONE case: refill the arenas behind the package's cached scratch (and behind the tensors
    in `more`, e.g. a call site's own workspace) with the active pattern, so that the second call starts on poisoned scratch and
    not on the first call's data -- which are the same bytes under every pattern and would hide a hole.  Outputs are left as
    they are (a later op's inputs).  Outside a `poisoned` context (the history comparison) nothing is done.  Returns the number
    of arenas refilled."""
    if not _ACTIVE:
        return 0
    from locov_amd import ops
    tensors = [t for name in SCRATCH_CACHES for t in getattr(ops, name).values()] + [t for t in more if t is not None]
    return _ACTIVE[-1].repoison_tensors(tensors)


def fresh_scratch(monkeypatch) -> None:
    """Empty every cache of uninitialised device scratch of the package for the duration of a test, so that the next request
    allocates again -- through the patched torch.empty when a `poisoned` context is active.  Caches that hold state (the range
    guard words of _OVERFLOW, the zeroed ring of _SCALE_SLOTS, the pinned mirror of _DETECT_PINNED, the weight banks) stay.  So
    does poolers._BATCH_INDEX_COLUMNS, the one other module-level dict of the package that a torch.empty fills: it is no scratch
    but a finished result, every row of which torch fills write before it is stored, and no C entry point receives it unwritten.
    (SgdTable's norm-clipping workspace belongs to the table object, which a case makes anew.)"""
    from locov_amd import ops
    for name in SCRATCH_CACHES:
        monkeypatch.setattr(ops, name, {})


class Recorder:
    """Proxy around the ctypes library that records which locov_* symbols were called:
    monkeypatch.setattr(_lib, "_lib", Recorder(_lib.load()))."""

    def __init__(self, lib):
        object.__setattr__(self, "_real", lib)
        object.__setattr__(self, "called", set())

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.startswith("locov_"):
            self.called.add(name)
        return fn

    def __setattr__(self, name, value):
        setattr(self._real, name, value)


def same_bits(a: torch.Tensor, b: torch.Tensor, mask=None) -> bool:
    """Bit equality of two host tensors (NaN payloads count); mask: boolean tensor of a's shape, True = compare."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if mask is not None:
        a, b = a[mask], b[mask]
    a, b = a.contiguous(), b.contiguous()
    if a.numel() == 0:
        return True
    return bool(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))


# case name -> {output index: (gate, reason)}: max |a - b| <= gate * max(max |a|, 1), the gate of tests/test_gpu_roi_align_bwd.py
_ATOMIC = ("the ROIAlign backward kernels add into the zero-filled map gradient with fp32 atomics (ops.roi_align_nhwc_bwd: 'fp32 atomics'; "
           "csrc/roi_align.hip, roi_align_nhwc_bwd.hip): the order of the additions is the order of arrival")
NONREPRODUCIBLE = {
    "roi_align_plan_path": {1: (1e-5, _ATOMIC)},
    "roi_align_exact_nhwc_copy": {1: (1e-5, _ATOMIC)},
    "roi_align_nchw": {1: (1e-5, _ATOMIC)},
    "roi_align_nhwc_even_bins_pos_major": {2: (1e-5, _ATOMIC)},
    "roi_align_nhwc_all_bins_bf16_map": {2: (1e-5, _ATOMIC)},
}


def _close(a, b, gate):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.double(), b.double()
    if not (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))):
        return False
    fin = torch.isfinite(a)
    if not fin.any():
        return True
    return float((a[fin] - b[fin]).abs().max()) <= gate * max(float(a[fin].abs().max()), 1.0)


def compare(case, got, want, what):
    """The rule by which two runs of a case are the same result: bit equality of every output (inside its `unspecified` mask), the
    NONREPRODUCIBLE outputs by their gate instead; raises AssertionError naming the outputs that differ."""
    assert len(got) == len(want), f"{case.name}: {len(got)} outputs {what}, {len(want)} before"
    masks = {i: (build, why) for i, build, why in case.unspecified}
    loose = NONREPRODUCIBLE.get(case.name, {})
    bad = []
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            if a is not b:
                bad.append(f"output {i}: present in one run only")
            continue
        mask = masks[i][0](want) if i in masks else None
        if i in loose:
            ok = _close(a if mask is None else a[mask], b if mask is None else b[mask], loose[i][0])
        else:
            ok = same_bits(a, b, mask)
        if not ok:
            diff = (a.reshape(-1).view(torch.uint8) != b.reshape(-1).view(torch.uint8)) if a.shape == b.shape and a.dtype == b.dtype else None
            where = "" if diff is None else f", {int(diff.sum())} of {diff.numel()} bytes differ, first at byte {int(diff.nonzero()[0])}"
            bad.append(f"output {i} {tuple(a.shape)} {a.dtype}{where}")
    assert not bad, f"{case.name} {what}: " + "; ".join(bad)
