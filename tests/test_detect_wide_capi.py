"""CPU-side checks of locov_detect_postprocess_wide (csrc/detect_wide.hip): the exports, argument errors before any HIP call, and the
workspace formula documented in include/locov_hip.h (no compute: there is no GPU here)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def _offs(sizes):
    vals = [0]
    for n in sizes:
        vals.append(vals[-1] + n)
    return (ctypes.c_int * len(vals))(*vals)


def _documented_bytes(sizes, K, per_class_above):
    """include/locov_hip.h: 16 R + 16 n K + 180 352 n + 8 (sum R_i W_i + sum cap_i W_i + R K)."""
    n, R = len(sizes), sum(sizes)
    if n == 0 or R == 0:
        return 0
    words = sum(r * ((r + 63) // 64) for r in sizes)
    caps = sum(max(0, min(per_class_above - 1, r * K)) * ((r + 63) // 64) for r in sizes)
    return 16 * R + 16 * n * K + 180352 * n + 8 * (words + caps + R * K)


def test_exports(lib):
    from locov_amd import _lib
    for name in ("locov_detect_postprocess_wide", "locov_detect_postprocess_wide_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.locov_abi_version() == 8


@pytest.mark.parametrize("sizes,K,pca", [
    ([1000], 1203, 40000), ([1000] * 8, 1203, 40000), ([300, 0, 1, 517], 80, 40000), ([1000, 20], 1203, 1),
    ([16383], 3, 0), ([37] * 64, 20, 10 ** 9), ([64, 65], 7, 100),
])
def test_workspace_formula(lib, sizes, K, pca):
    got = lib.locov_detect_postprocess_wide_workspace_bytes(_offs(sizes), len(sizes), K, pca)
    assert got == _documented_bytes(sizes, K, pca) > 0


def test_workspace_is_zero_for_empty_input(lib):
    assert lib.locov_detect_postprocess_wide_workspace_bytes(None, 0, 1203, 40000) == 0
    assert lib.locov_detect_postprocess_wide_workspace_bytes(_offs([0, 0]), 2, 1203, 40000) == 0


def _call(lib, sizes=(1000,), K=1203, topk=300, pca=40000, ws_bytes=None, n_images=None, offs=None, probs=256, counts=512):
    offs = _offs(sizes) if offs is None else offs
    n = len(sizes) if n_images is None else n_images
    hw = (ctypes.c_float * (2 * max(n, 1)))(*([800.0, 1333.0] * max(n, 1)))
    if ws_bytes is None:
        ws_bytes = lib.locov_detect_postprocess_wide_workspace_bytes(offs, n, K, pca)
    p = ctypes.c_void_p
    return lib.locov_detect_postprocess_wide(p(probs), K + 1, K, p(1024), p(2048), offs, hw, n, 10.0, 10.0, 5.0, 5.0, 4.135, 1e-4, 0.5,
                                             topk, pca, p(4096), ws_bytes, p(8192), p(8192), p(8192), p(8192), p(counts), None)


@pytest.mark.parametrize("kw,msg", [
    ({"n_images": 65, "sizes": [10] * 65}, b"too many images"),
    ({"offs": ctypes.POINTER(ctypes.c_int)()}, b"null row_offsets"),
    ({"sizes": [16384]}, b"too many rows"),
    ({"K": 0}, b"too many classes"),
    ({"K": 32768}, b"too many classes"),
    ({"topk": 0}, b"topk out of range"),
    ({"topk": 8193}, b"topk out of range"),
    ({"ws_bytes": 1024}, b"workspace too small"),
    ({"probs": 0}, b"null pointer"),
    ({"counts": 0}, b"null pointer"),
])
def test_argument_errors_are_reported(lib, kw, msg):
    rc = _call(lib, **kw)
    assert rc < 0
    assert msg in lib.locov_last_error(), lib.locov_last_error()
    if "ws_bytes" not in kw and "offs" not in kw:
        return
    assert lib.locov_detect_postprocess_wide_workspace_bytes(ctypes.POINTER(ctypes.c_int)(), 1, 1203, 40000) < 0
