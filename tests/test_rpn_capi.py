"""CPU-side checks of the RPN entry points (csrc/rpn.hip: locov_rpn_proposals and its workspace function): the exports, every
argument error before any HIP call, the empty-input no-op and the workspace formula documented in include/locov_hip.h (no compute:
there is no GPU here)."""
import ctypes

import pytest

NAMES = ("locov_rpn_proposals_workspace_bytes", "locov_rpn_proposals")


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def _bytes(n, hwa, pre):
    """include/locov_hip.h: n_images (512 W^2 + 1 544 W), W = ceil(min(hwa, pre_nms_topk) / 64)."""
    if n == 0 or hwa == 0:
        return 0
    W = (min(hwa, pre) + 63) // 64
    return n * (512 * W * W + 1544 * W)


def test_exports(lib):
    from locov_amd import _lib, ops
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.locov_abi_version() == 8
    assert callable(ops.rpn_proposals)
    assert (_lib.RPN_FLAG_NONFINITE, _lib.RPN_MAX_PRE_NMS_TOPK, _lib.RPN_MAX_ANCHORS) == (1, 16384, 2 ** 22 - 1)


@pytest.mark.parametrize("n,hwa,pre", [(1, 63000, 6000), (4, 63000, 12000), (1, 1, 1), (3, 63, 100), (2, 64, 64), (2, 65, 100),
                                       (64, 2 ** 22 - 1, 16384), (7, 16384, 16384), (1, 70000, 12000)])
def test_workspace_formula(lib, n, hwa, pre):
    assert lib.locov_rpn_proposals_workspace_bytes(n, hwa, pre) == _bytes(n, hwa, pre) > 0


def test_workspace_at_12000_boxes_is_18_mb_per_image(lib):
    assert 18.0e6 < lib.locov_rpn_proposals_workspace_bytes(1, 63000, 12000) < 18.5e6


def test_workspace_is_zero_for_empty_input(lib):
    assert lib.locov_rpn_proposals_workspace_bytes(0, 63000, 6000) == 0
    assert lib.locov_rpn_proposals_workspace_bytes(3, 0, 6000) == 0


def _call(lib, n=1, hwa=100, pre=50, post=10, w=(1.0, 1.0, 1.0, 1.0), ptr=64, ws_bytes=1 << 30, hw=None, logits=None):
    """Pointers are never dereferenced on the host: an argument error must come back before any HIP call."""
    hw = (ctypes.c_float * max(2 * n, 2))(*([800.0, 1333.0] * max(n, 1))) if hw is None else hw
    p = ctypes.c_void_p(ptr)
    return lib.locov_rpn_proposals(p if logits is None else logits, p, p, hwa, hw, n, w[0], w[1], w[2], w[3], 4.135, pre, post, 0.0, 0.7, p,
                                   ws_bytes, p, p, p, p, None)


@pytest.mark.parametrize("kwargs,text", [
    (dict(n=65), "too many images"), (dict(n=-1), "too many images"),
    (dict(hwa=2 ** 22), "too many anchors"), (dict(hwa=-1), "too many anchors"),
    (dict(pre=0), "pre_nms_topk out of range"), (dict(pre=16385, post=10), "pre_nms_topk out of range"),
    (dict(post=0), "post_nms_topk out of range"), (dict(pre=50, post=51), "post_nms_topk out of range"),
    (dict(w=(1.0, 0.0, 1.0, 1.0)), "zero box weight"),
    (dict(logits=ctypes.c_void_p(0)), "null pointer"),
    (dict(ws_bytes=1000), "workspace too small"),
    (dict(ptr=72), "16-byte aligned"),
])
def test_argument_errors_come_before_any_hip_call(lib, kwargs, text):
    assert _call(lib, **kwargs) == -1
    assert text in lib.locov_last_error().decode()


def test_workspace_function_reports_the_same_limits(lib):
    for args in ((65, 100, 50), (1, 2 ** 22, 50), (1, 100, 0), (1, 100, 16385)):
        assert lib.locov_rpn_proposals_workspace_bytes(*args) == -1


def test_empty_input_is_a_no_op(lib):
    """n_images == 0 or hwa == 0: success without touching a pointer (all null here) or the device."""
    null = ctypes.c_void_p(0)
    for n, hwa in ((0, 100), (2, 0), (0, 0)):
        assert lib.locov_rpn_proposals(null, null, null, hwa, None, n, 1.0, 1.0, 1.0, 1.0, 4.135, 50, 10, 0.0, 0.7, null, 0, null, null, null,
                                       null, None) == 0


def test_ops_wrapper_has_no_cpu_fallback():
    """CPU tensors are an error, not a quiet torch computation."""
    import torch
    from locov_amd import ops
    from locov_amd._lib import LocovError
    with pytest.raises(LocovError):
        ops.rpn_proposals(torch.zeros(1, 10), torch.zeros(1, 10, 4), torch.zeros(10, 4), [(8, 8)], (1, 1, 1, 1), 4.0, 5, 5, 0.0, 0.7)
