"""The C ABI of the RPN's training half (csrc/rpn_train.hip), without a GPU: the symbols are exported and bound, every argument error
of every entry point is reported before any HIP call, empty input is a no-op, and the workspace sizes are the header's formulas."""
import ctypes

import pytest

NAMES = ["locov_rpn_label_anchors_workspace_bytes", "locov_rpn_label_anchors", "locov_rpn_sample_anchors", "locov_rpn_loss_workspace_bytes",
         "locov_rpn_loss"]
p = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def err(lib):
    return lib.locov_last_error()


def test_symbols_are_exported_and_bound(lib):
    from locov_amd import _lib, ops
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert all(hasattr(ops, n) for n in ("rpn_label_anchors", "rpn_sample_anchors", "rpn_loss"))
    assert lib.locov_abi_version() == 8 and _lib.RPN_LOSS_FLAG_DEGENERATE == 1


def test_workspace_sizes(lib):
    from locov_amd import _lib
    lab, loss = lib.locov_rpn_label_anchors_workspace_bytes, lib.locov_rpn_loss_workspace_bytes
    assert lab(4, 63000, 37) == 16 * 10 and lab(1, 189, 4) == 16 and lab(1, 189, 0) == 0            # 16 ceil(n_gt / 4)
    assert lab(0, 189, 5) == 0 and lab(2, 0, 5) == 0
    assert lab(_lib.LABEL_MAX_IMAGES + 1, 189, 5) < 0 and b"images" in err(lib)
    assert lab(1, 1 << 22, 5) < 0 and b"anchors" in err(lib)
    assert lab(1, 189, -1) < 0 and b"ground-truth" in err(lib)
    assert loss(4, 63000) == 16 * 4 * 247 and loss(1, 256) == 16 and loss(1, 257) == 32             # 16 n ceil(hwa / 256)
    assert loss(0, 189) == 0 and loss(3, 0) == 0
    assert loss(_lib.LABEL_MAX_IMAGES + 1, 189) < 0 and loss(1, 1 << 22) < 0 and loss(1, -1) < 0


def label_call(lib, n_images=1, hwa=189, offsets=(0, 2), n_thr=3, boundary=-1.0, ptrs=True, ws_bytes=1 << 20, anchors=4096, labels=8192):
    off = (ctypes.c_int * len(offsets))(*offsets)
    hw = (ctypes.c_float * (2 * max(n_images, 1)))(*([32.0, 48.0] * max(n_images, 1)))
    lo, hi = (ctypes.c_float * 6)(-1e30, 0.3, 0.7), (ctypes.c_float * 6)(0.3, 0.7, 1e30)
    lab = (ctypes.c_int * 6)(0, -1, 1)
    d = (lambda v: p(v)) if ptrs else (lambda v: None)
    return lib.locov_rpn_label_anchors(d(anchors), hwa, d(256), off, hw, n_images, lo, hi, lab, n_thr, 1, boundary, d(512), ws_bytes, d(labels),
                                       d(1024), d(2048), None)


def test_label_anchors_validates_its_arguments(lib):
    from locov_amd import _lib
    assert label_call(lib, n_images=0, ptrs=False) == 0 and label_call(lib, hwa=0, ptrs=False) == 0          # empty: a no-op
    assert label_call(lib, n_images=_lib.LABEL_MAX_IMAGES + 1) == -1 and b"images" in err(lib)
    assert label_call(lib, hwa=1 << 22) == -1 and b"anchors" in err(lib)
    assert label_call(lib, n_thr=_lib.LABEL_MAX_THRESHOLDS + 1) == -1 and b"matcher intervals" in err(lib)
    assert label_call(lib, offsets=(0, -1)) == -1 and b"non-decreasing" in err(lib)
    assert label_call(lib, offsets=(1, 2)) == -1 and b"start at 0" in err(lib)
    assert label_call(lib, ptrs=False) == -1 and b"null pointer" in err(lib)
    assert label_call(lib, ws_bytes=8) == -1 and b"workspace too small" in err(lib)
    assert label_call(lib, anchors=4100) == -1 and b"16-byte aligned" in err(lib)
    assert lib.locov_rpn_label_anchors(p(4096), 189, p(256), None, None, 1, None, None, None, 0, 1, -1.0, p(512), 64, p(8192), p(1024), p(2048),
                                       None) == -1 and b"null host array" in err(lib)


def test_sample_anchors_validates_its_arguments(lib):
    from locov_amd import _lib
    f = lib.locov_rpn_sample_anchors
    assert f(None, None, 189, 0, 16, 8, None, None, None) == 0 and f(None, None, 0, 2, 16, 8, None, None, None) == 0
    assert f(p(256), p(512), 189, _lib.LABEL_MAX_IMAGES + 1, 16, 8, p(1024), p(2048), None) == -1 and b"images" in err(lib)
    assert f(p(256), p(512), 1 << 22, 1, 16, 8, p(1024), p(2048), None) == -1 and b"anchors" in err(lib)
    assert f(p(256), p(512), 189, 1, 16, 17, p(1024), p(2048), None) == -1 and b"max_pos <= budget" in err(lib)
    assert f(p(256), p(512), 189, 1, -1, 0, p(1024), p(2048), None) == -1
    assert f(None, p(512), 189, 1, 16, 8, p(1024), p(2048), None) == -1 and b"null pointer" in err(lib)
    assert f(p(256), p(512), 189, 1, 16, 8, p(1024), p(256), None) == -1 and b"alias" in err(lib)


def loss_call(lib, n_images=1, hwa=189, beta=0.0, ptrs=True, ws_bytes=1 << 20, deltas=512):
    d = (lambda v: p(v)) if ptrs else (lambda v: None)
    return lib.locov_rpn_loss(d(256), d(deltas), d(768), d(1024), d(2048), hwa, n_images, 1.0, 1.0, 1.0, 1.0, beta, 1.0, 1.0, d(4096), ws_bytes,
                              d(8192), d(12288), d(16384), d(20480), None)


def test_loss_validates_its_arguments(lib):
    from locov_amd import _lib
    assert loss_call(lib, n_images=0, ptrs=False) == 0 and loss_call(lib, hwa=0, ptrs=False) == 0
    assert loss_call(lib, n_images=_lib.LABEL_MAX_IMAGES + 1) == -1 and b"images" in err(lib)
    assert loss_call(lib, hwa=1 << 22) == -1 and b"anchors" in err(lib)
    assert loss_call(lib, beta=-0.5) == -1 and b"smooth_l1_beta" in err(lib)
    assert loss_call(lib, ptrs=False) == -1 and b"null pointer" in err(lib)
    assert loss_call(lib, ws_bytes=8) == -1 and b"workspace too small" in err(lib)
    assert loss_call(lib, deltas=516) == -1 and b"16-byte aligned" in err(lib)


def test_wrappers_reject_cpu_tensors_and_bad_shapes():
    import torch
    from locov_amd import ops
    from locov_amd._lib import LocovError
    with pytest.raises(LocovError, match="no CPU fallback"):
        ops.rpn_label_anchors(torch.zeros(8, 4), None, [0], [(32, 48)], [-1e30, 0.3, 0.7, 1e30], [0, -1, 1])
    with pytest.raises(LocovError, match="no CPU fallback"):
        ops.rpn_sample_anchors(torch.zeros(1, 8, dtype=torch.int8), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(2, 1, 8, dtype=torch.float64), 4, 2)
    with pytest.raises(ValueError, match="rpn_loss"):
        ops.rpn_loss(torch.zeros(1, 8), torch.zeros(1, 8, 4), torch.zeros(1, 7, dtype=torch.int8), torch.zeros(8, 4), torch.zeros(1, 8, 4),
                     (1, 1, 1, 1), 0.0, 1.0, 1.0)
