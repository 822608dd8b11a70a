"""locov_resize_flip_images / locov_resize_supported (csrc/image_resize.hip): argument errors are reported before any HIP call, so
they can be checked without a GPU; the header, the binding and the build agree about the new symbols."""
import ctypes
import os
import re

import pytest

import resize_cases
import resize_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_resize_is_declared_bound_and_built_without_contraction(lib):
    from locov_amd import build, _lib
    header = open(os.path.join(ROOT, "include", "locov_hip.h")).read()
    for name in ("locov_resize_flip_images", "locov_resize_supported"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(re.findall(r"\b%s\b" % name, header)) >= 2                       # the "later, additively" list and the declaration
    assert "#define LOCOV_ABI_VERSION 8" in header and lib.locov_abi_version() == _lib.ABI_VERSION == 8     # additive
    assert re.search(r"#define LOCOV_RESIZE_MAX_TAPS %d\b" % _lib.RESIZE_MAX_TAPS, header) and _lib.RESIZE_MAX_TAPS == resize_cases.MAX_TAPS
    assert (_lib.FLIP_NONE, _lib.FLIP_HORIZONTAL, _lib.FLIP_VERTICAL) == (0, 1, 2)
    assert "-ffp-contract=off" in build.FILE_FLAGS["image_resize.hip"]


def test_resize_supported_is_the_tap_rule(lib):
    ok = lib.locov_resize_supported
    assert ok(480, 640, 800, 1067, 3) == 1 and ok(3000, 4000, 800, 1067, 3) == 1 and ok(1, 1, 3000, 2000, 1) == 1      # every upscale
    for _, (h, w), (nh, nw) in resize_cases.SMALL_CASES + [resize_cases.REALISTIC]:
        want = max(resize_ref.taps(h, nh), resize_ref.taps(w, nw)) <= resize_cases.MAX_TAPS
        assert ok(h, w, nh, nw, 3) == int(want), (h, w, nh, nw)
    assert ok(64, 64, 8, 8, 4) == 1 and ok(65, 64, 8, 8, 4) == 0 and ok(64, 65, 8, 8, 4) == 0       # a factor of 8 per axis, no more
    assert ok(64, 64, 8, 8, 0) == 0 and ok(64, 64, 8, 8, 5) == 0 and ok(0, 64, 8, 8, 3) == 0 and ok(64, 64, 8, -1, 3) == 0
    assert ok(1 << 15, 1 << 15, 1 << 15, 1 << 15, 3) == 0                                            # 3 * 2^30 bytes: past int32


def test_resize_flip_images_validates_its_arguments(lib):
    from locov_amd import _lib
    p, ints = ctypes.c_void_p, lambda *v: (ctypes.c_int * len(v))(*v)
    src, dst = (p * 2)(4096 + 1, 1 << 20), (p * 2)((1 << 21) + 3, 1 << 22)           # one byte of alignment is all that is asked
    hs, ws, ohs, ows, flips = ints(37, 48), ints(53, 64), ints(61, 13), ints(87, 17), ints(0, 1)

    def call(n=2, channels=3, src=src, hs=hs, ws=ws, dst=dst, ohs=ohs, ows=ows, flips=flips):
        return lib.locov_resize_flip_images(src, hs, ws, dst, ohs, ows, flips, n, channels, None)

    assert lib.locov_resize_flip_images(None, None, None, None, None, None, None, 0, 9, None) == 0          # no images: a no-op
    assert call(n=_lib.LABEL_MAX_IMAGES + 1) == -1 and b"images per call" in lib.locov_last_error()
    assert call(n=-1) == -1
    assert call(channels=0) == -1 and b"channels" in lib.locov_last_error()
    assert call(channels=_lib.IMAGE_MAX_CHANNELS + 1) == -1 and b"channels" in lib.locov_last_error()
    for kw in ({"src": None}, {"hs": None}, {"ws": None}, {"dst": None}, {"ohs": None}, {"ows": None}, {"flips": None},
               {"src": (p * 2)(4096, None)}, {"dst": (p * 2)(None, 4096)}):
        assert call(**kw) == -1 and b"null pointer" in lib.locov_last_error(), kw
    for kw in ({"hs": ints(37, 0)}, {"ws": ints(-1, 64)}, {"ohs": ints(0, 13)}, {"ows": ints(87, -3)}):
        assert call(**kw) == -1 and b"must be positive" in lib.locov_last_error(), kw
    assert call(flips=ints(0, 3)) == -1 and b"unknown flip" in lib.locov_last_error()
    assert call(hs=ints(37, 65), ohs=ints(61, 8)) == -1 and b"over the limit of 17" in lib.locov_last_error()      # 65 -> 8: 19 taps
    assert call(ws=ints(53, 145), ows=ints(87, 16)) == -1 and b"over the limit" in lib.locov_last_error()
    big = 1 << 15
    assert call(n=1, hs=ints(big), ws=ints(big), ohs=ints(big), ows=ints(big)) == -1 and b"int32" in lib.locov_last_error()
    assert call(n=1, hs=ints(4), ws=ints(4), ohs=ints(big), ows=ints(big)) == -1 and b"int32" in lib.locov_last_error()


def test_ops_wrapper_refuses_cpu_tensors_and_bad_batches():
    import torch
    from locov_amd import ops
    from locov_amd._lib import LocovError
    assert ops.resize_flip_images([], []) == []
    with pytest.raises(LocovError, match="no CPU fallback"):
        ops.resize_flip_images([torch.zeros(4, 4, 3, dtype=torch.uint8)], [(8, 8)])
    assert ops.resize_supported((64, 64), (8, 8)) and not ops.resize_supported((65, 64), (8, 8)) and ops.RESIZE_MAX_TAPS == 17
