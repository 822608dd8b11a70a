"""locov_preprocess_images / locov_detector_rescale (csrc/image_batch.hip): argument errors are reported before any HIP call, so
they can be checked without a GPU."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_preprocess_images_validates_its_arguments(lib):
    from locov_amd import _lib
    p = ctypes.c_void_p
    ptrs, hs, ws = (p * 2)(4096, 8192 + 1), (ctypes.c_int * 2)(37, 40), (ctypes.c_int * 2)(53, 41)
    mean, std = (ctypes.c_float * 4)(1, 2, 3, 4), (ctypes.c_float * 4)(1, 1, 1, 1)
    out = p(1 << 20)

    def call(n=2, dtype=_lib.IMAGE_U8, channels=3, images=ptrs, heights=hs, out=out, hb=40, wb=53, mean=mean):
        return lib.locov_preprocess_images(images, heights, ws, n, dtype, channels, mean, std, 0.0, out, hb, wb, None)

    assert lib.locov_preprocess_images(None, None, None, 0, 7, 9, None, None, 0.0, None, 0, 0, None) == 0     # no images: a no-op
    assert call(n=_lib.LABEL_MAX_IMAGES + 1) == -1 and b"images per call" in lib.locov_last_error()
    assert call(n=-1) == -1
    assert call(dtype=2) == -1 and b"unknown dtype" in lib.locov_last_error()
    assert call(channels=0) == -1 and b"channels" in lib.locov_last_error()
    assert call(channels=_lib.IMAGE_MAX_CHANNELS + 1) == -1 and b"channels" in lib.locov_last_error()
    assert call(images=None) == -1 and b"null pointer" in lib.locov_last_error()
    assert call(mean=None) == -1 and b"null pointer" in lib.locov_last_error()
    assert call(out=None) == -1 and b"null pointer" in lib.locov_last_error()
    assert call(images=(p * 2)(4096, None)) == -1 and b"null pointer" in lib.locov_last_error()
    assert call(hb=39) == -1 and b"larger than the batch" in lib.locov_last_error()                       # image 1 is 40 high
    assert call(wb=52) == -1 and b"larger than the batch" in lib.locov_last_error()                       # image 0 is 53 wide
    assert call(heights=(ctypes.c_int * 2)(37, -1)) == -1
    assert call(hb=1 << 16, wb=1 << 16) == -1 and b"batch size" in lib.locov_last_error()                 # a plane must index in 31 bits
    assert call(out=p((1 << 20) + 4)) == -1 and b"16-byte aligned" in lib.locov_last_error()
    assert call(dtype=_lib.IMAGE_F32) == -1 and b"element size" in lib.locov_last_error()                 # an fp32 image at an odd byte


def test_detector_rescale_validates_its_arguments(lib):
    from locov_amd import _lib
    p = ctypes.c_void_p
    roff, sx, sy = (ctypes.c_int * 3)(0, 100, 250), (ctypes.c_float * 2)(0.6, 2.0), (ctypes.c_float * 2)(0.6, 2.0)
    oh, ow = (ctypes.c_int * 2)(480, 640), (ctypes.c_int * 2)(640, 480)
    boxes, out, src, counts = p(4096), p(8192), p(16384), p(32768)

    def call(n=2, boxes=boxes, roff=roff, sx=sx, out=out, src=src, counts=counts):
        return lib.locov_detector_rescale(boxes, roff, sx, sy, oh, ow, n, out, src, counts, None)

    assert lib.locov_detector_rescale(None, None, None, None, None, None, 0, None, None, None, None) == 0       # no images: a no-op
    assert call(n=_lib.LABEL_MAX_IMAGES + 1) == -1 and b"images per call" in lib.locov_last_error()
    assert call(n=-1) == -1
    for kw in ({"boxes": None}, {"roff": None}, {"sx": None}, {"out": None}, {"src": None}, {"counts": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.locov_last_error(), kw
    assert call(roff=(ctypes.c_int * 3)(0, 100, 50)) == -1 and b"must not decrease" in lib.locov_last_error()
    assert call(roff=(ctypes.c_int * 3)(1, 100, 250)) == -1 and b"roff[0]" in lib.locov_last_error()
    assert call(boxes=p(4096 + 4)) == -1 and b"aligned" in lib.locov_last_error()
    assert call(out=boxes) == -1 and b"must not be boxes" in lib.locov_last_error()
