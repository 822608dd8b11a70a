"""CPU-side checks of the class-specific detection entry points (csrc/detect.hip, csrc/detect_wide.hip: locov_detect_postprocess_cs,
locov_detect_postprocess_wide_cs and their workspace functions): the exports, argument errors before any HIP call, and the workspace
formulas documented in include/locov_hip.h (no compute: there is no GPU here)."""
import ctypes

import pytest

NAMES = ("locov_detect_postprocess_cs_workspace_bytes", "locov_detect_postprocess_cs", "locov_detect_postprocess_wide_cs_workspace_bytes",
         "locov_detect_postprocess_wide_cs")


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


def _lds_bytes(R, n, B):
    """include/locov_hip.h: align16(R (16 B + 8) + 4 ceil4(n)) + 4 522 000 n + 64."""
    if R <= 0 or n <= 0:
        return 0
    head = (R * (16 * B + 8) + 4 * ((n + 3) // 4 * 4) + 15) // 16 * 16
    return head + 4522000 * n + 64


def _wide_bytes(sizes, K, per_class_above, B):
    """include/locov_hip.h: 16 R B + 16 n K + 180 352 n + 8 (M + sum cap_i W_i + R K), M = sum R_i W_i for B = 1, 0 for B = K > 1."""
    n, R = len(sizes), sum(sizes)
    if n == 0 or R == 0:
        return 0
    words = sum(r * ((r + 63) // 64) for r in sizes) if B == 1 else 0
    caps = sum(max(0, min(per_class_above - 1, r * K)) * ((r + 63) // 64) for r in sizes)
    return 16 * R * B + 16 * n * K + 180352 * n + 8 * (words + caps + R * K)


def test_exports(lib):
    from locov_amd import _lib
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.locov_abi_version() == 8


CASES = [([1000], 1203, 40000), ([1000] * 8, 1203, 40000), ([300, 0, 1, 517], 80, 40000), ([1000, 20], 1203, 1), ([16383], 3, 0),
         ([37] * 64, 20, 10 ** 9), ([64, 65], 7, 100)]


@pytest.mark.parametrize("sizes,K,pca", CASES)
def test_class_agnostic_workspaces_equal_the_existing_functions(lib, sizes, K, pca):
    R, n = sum(sizes), len(sizes)
    for ld in (4, 8):
        assert lib.locov_detect_postprocess_cs_workspace_bytes(R, n, K, ld, 1) == lib.locov_detect_postprocess_workspace_bytes(R, n) > 0
        assert (lib.locov_detect_postprocess_wide_cs_workspace_bytes(_offs(sizes), n, K, pca, ld, 1)
                == lib.locov_detect_postprocess_wide_workspace_bytes(_offs(sizes), n, K, pca) > 0)


@pytest.mark.parametrize("sizes,K,pca", CASES)
def test_class_specific_workspace_formulas(lib, sizes, K, pca):
    R, n = sum(sizes), len(sizes)
    assert lib.locov_detect_postprocess_cs_workspace_bytes(R, n, K, 4 * K, K) == _lds_bytes(R, n, K) > 0
    assert lib.locov_detect_postprocess_wide_cs_workspace_bytes(_offs(sizes), n, K, pca, 4 * K, K) == _wide_bytes(sizes, K, pca, K) > 0
    assert lib.locov_detect_postprocess_wide_cs_workspace_bytes(_offs(sizes), n, K, pca, 4 * K + 4, K) == _wide_bytes(sizes, K, pca, K)
    # (the decoded boxes grow K-fold; the row x row matrices are gone)
    assert _lds_bytes(R, n, K) - _lds_bytes(R, n, 1) == 16 * R * (K - 1)


def test_workspaces_are_zero_for_empty_input(lib):
    assert lib.locov_detect_postprocess_cs_workspace_bytes(0, 1, 80, 320, 80) == 0
    assert lib.locov_detect_postprocess_cs_workspace_bytes(10, 0, 80, 320, 80) == 0
    assert lib.locov_detect_postprocess_wide_cs_workspace_bytes(None, 0, 1203, 40000, 4812, 1203) == 0
    assert lib.locov_detect_postprocess_wide_cs_workspace_bytes(_offs([0, 0]), 2, 1203, 40000, 4812, 1203) == 0


@pytest.mark.parametrize("K,ld,box_classes,msg", [
    (80, 320, 2, b"box_classes must be 1 or num_classes"),
    (80, 320, 0, b"box_classes must be 1 or num_classes"),
    (80, 320, 81, b"box_classes must be 1 or num_classes"),
    (80, 316, 80, b"ld_deltas"),
    (80, 322, 80, b"ld_deltas"),
    (80, 0, 1, b"ld_deltas"),
])
def test_workspace_argument_errors(lib, K, ld, box_classes, msg):
    assert lib.locov_detect_postprocess_cs_workspace_bytes(300, 1, K, ld, box_classes) < 0
    assert msg in lib.locov_last_error(), lib.locov_last_error()
    assert lib.locov_detect_postprocess_wide_cs_workspace_bytes(_offs([300]), 1, K, 40000, ld, box_classes) < 0
    assert msg in lib.locov_last_error(), lib.locov_last_error()


def test_wide_workspace_rejects_bad_offsets(lib):
    f = lib.locov_detect_postprocess_wide_cs_workspace_bytes
    assert f(ctypes.POINTER(ctypes.c_int)(), 1, 80, 40000, 320, 80) < 0 and b"null row_offsets" in lib.locov_last_error()
    assert f((ctypes.c_int * 3)(0, 10, 5), 2, 80, 40000, 320, 80) < 0 and b"non-decreasing" in lib.locov_last_error()
    assert f((ctypes.c_int * 2)(1, 10), 1, 80, 40000, 320, 80) < 0 and b"offsets start at 0" in lib.locov_last_error()
    assert f(_offs([16384]), 1, 80, 40000, 320, 80) < 0 and b"too many rows" in lib.locov_last_error()
    assert f(_offs([16383] * 5), 5, 32767, 40000, 4 * 32767, 32767) < 0 and b"2^31" in lib.locov_last_error()


def _call(lib, wide, sizes=(300,), K=80, ld=None, box_classes=None, topk=100, ws_bytes=None, probs=256, counts=512):
    offs, n = _offs(sizes), len(sizes)
    ld = 4 * K if ld is None else ld
    box_classes = K if box_classes is None else box_classes
    hw = (ctypes.c_float * (2 * n))(*([800.0, 1333.0] * n))
    p = ctypes.c_void_p
    if wide:
        if ws_bytes is None:
            ws_bytes = max(lib.locov_detect_postprocess_wide_cs_workspace_bytes(offs, n, K, 40000, ld, box_classes), 0)
        return lib.locov_detect_postprocess_wide_cs(p(probs), K + 1, K, p(1024), ld, box_classes, p(2048), offs, hw, n, 10.0, 10.0, 5.0, 5.0,
                                                    4.135, 1e-4, 0.5, topk, 40000, p(4096), ws_bytes, p(8192), p(8192), p(8192), p(8192),
                                                    p(counts), None)
    if ws_bytes is None:
        ws_bytes = max(lib.locov_detect_postprocess_cs_workspace_bytes(sum(sizes), n, K, ld, box_classes), 0)
    return lib.locov_detect_postprocess_cs(p(probs), K + 1, K, p(1024), ld, box_classes, p(2048), offs, hw, n, 10.0, 10.0, 5.0, 5.0, 4.135,
                                           0.05, 0.5, topk, p(4096), ws_bytes, p(8192), p(8192), p(8192), p(8192), p(counts), None)


@pytest.mark.parametrize("wide", [False, True], ids=["lds", "wide"])
@pytest.mark.parametrize("kw,msg", [
    ({"box_classes": 2}, b"box_classes must be 1 or num_classes"),
    ({"box_classes": 79}, b"box_classes must be 1 or num_classes"),
    ({"ld": 319}, b"ld_deltas"),
    ({"ld": 4}, b"ld_deltas"),
    ({"box_classes": 1, "ld": 6}, b"ld_deltas"),
    ({"topk": 0}, b"topk"),
    ({"ws_bytes": 1024}, b"workspace too small"),
    ({"probs": 0}, b"null pointer"),
    ({"counts": 0}, b"null pointer"),
])
def test_argument_errors_are_reported_before_any_launch(lib, wide, kw, msg):
    rc = _call(lib, wide, **kw)
    assert rc < 0
    assert msg in lib.locov_last_error(), lib.locov_last_error()
    name = b"locov_detect_postprocess_wide_cs" if wide else b"locov_detect_postprocess_cs"
    assert lib.locov_last_error().startswith(name)
