"""locov_coco_match / locov_coco_accumulate: every argument error is reported before any HIP call (no GPU needed), in the style
of tests/test_capi_exports.py; the workspace function's values; the wrappers refuse CPU tensors."""
import ctypes
import os
import re

import pytest

P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_constants_agree_with_the_header():
    from locov_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "locov_hip.h")).read()
    defs = dict(re.findall(r"#define LOCOV_(COCO_[A-Z_]+) (\d+)", src))
    assert len(defs) == 6 and all(getattr(_lib, k) == int(v) for k, v in defs.items()), defs
    assert _lib.COCO_MAX_AREAS * _lib.COCO_MAX_THRESHOLDS <= 64 and _lib.ABI_VERSION == 8      # one lane per (range, threshold)


def _match(lib, det_off=P(256), gt_off=P(512), cells=10, n_det=5, n_gt=3, max_det=100, det_boxes=P(1024), gt_boxes=P(2048), gt_area=P(4096),
           gt_crowd=P(8192), areas=(0, 1e10, 0, 1024), n_areas=2, thrs=(0.5, 0.75), n_thrs=2, bits=P(1 << 14), gt_ignore=P(1 << 15),
           ws=P(1 << 16), ws_bytes=1 << 30):
    ar = (ctypes.c_double * len(areas))(*areas) if areas is not None else None
    th = (ctypes.c_double * len(thrs))(*thrs) if thrs is not None else None
    return lib.locov_coco_match(det_off, gt_off, cells, n_det, n_gt, max_det, det_boxes, gt_boxes, gt_area, gt_crowd, ar, n_areas, th, n_thrs,
                                bits, gt_ignore, ws, ws_bytes, None)


def test_coco_match_validates_its_arguments(lib):
    from locov_amd import _lib
    err = lib.locov_last_error
    assert _match(lib, cells=0) == 0                                                                    # no cells: a no-op
    assert _match(lib, n_det=0, n_gt=0, det_off=None, gt_off=None) == 0                                 # no det and no gt: a no-op
    for kw in (dict(cells=-1), dict(n_det=-1), dict(n_gt=-1), dict(ws_bytes=-8)):
        assert _match(lib, **kw) == -1 and b"negative" in err()
    assert _match(lib, max_det=0) == -1 and b"max_det" in err()
    assert _match(lib, n_areas=0) == -1 and b"area ranges" in err()
    assert _match(lib, n_areas=_lib.COCO_MAX_AREAS + 1) == -1 and b"area ranges" in err()
    assert _match(lib, n_thrs=0) == -1 and b"IoU thresholds" in err()
    assert _match(lib, n_thrs=_lib.COCO_MAX_THRESHOLDS + 1) == -1 and b"IoU thresholds" in err()
    assert _match(lib, areas=None) == -1 and b"null area range" in err()
    assert _match(lib, thrs=None) == -1 and b"null area range or threshold" in err()
    assert _match(lib, areas=(0, 1e10, 1024, 0)) == -1 and b"not ascending" in err()
    assert _match(lib, max_det=_lib.COCO_MAX_DET + 1) == -3 and b"dets per cell" in err()               # LOCOV_ERR_UNSUPPORTED: never a truncation
    assert _match(lib, cells=4 * _lib.COCO_MAX_BLOCKS + 1) == -3
    assert _match(lib, det_off=None) == -1 and b"null offsets" in err()
    assert _match(lib, gt_off=None) == -1 and b"null offsets" in err()
    for name in ("det_boxes", "bits"):
        assert _match(lib, **{name: None}) == -1 and b"null det pointer" in err()
    for name in ("gt_boxes", "gt_area", "gt_crowd", "gt_ignore"):
        assert _match(lib, **{name: None}) == -1 and b"null gt pointer" in err()
    assert _match(lib, gt_boxes=P(2052)) == -1 and b"misaligned" in err()
    assert _match(lib, det_off=P(258)) == -1 and b"misaligned" in err()
    assert _match(lib, ws=None) == -1 and b"workspace" in err()
    assert _match(lib, ws=P((1 << 16) + 4)) == -1 and b"workspace" in err()
    need = lib.locov_coco_match_workspace_bytes(3, 100)
    assert need == 3 * (100 * 8 + 64)                                                                   # per gt: an IoU column and 64 matched flags
    assert lib.locov_coco_match_workspace_bytes(0, 100) == 0 and lib.locov_coco_match_workspace_bytes(3, 0) == 0
    assert lib.locov_coco_match_workspace_bytes(1, 1) == 72
    assert _match(lib, ws_bytes=need - 1) == -1 and b"too small" in err()
    with pytest.raises(_lib.LocovError, match="null offsets"):
        _lib.check(_match(lib, det_off=None), "locov_coco_match")


def _acc(lib, cat_off=P(256), K=4, idx=P(512), rank=P(1024), score=P(2048), n_det=5, bits=P(4096), npig=P(8192), A=4, T=10, caps=(1, 10, 100),
         M=None, rec=(0.0, 0.5, 1.0), R=None, precision=P(1 << 14), recall=P(1 << 15), scores=P(1 << 16)):
    c = (ctypes.c_int * max(len(caps), 1))(*caps) if caps is not None else None
    r = (ctypes.c_double * max(len(rec), 1))(*rec) if rec is not None else None
    return lib.locov_coco_accumulate(cat_off, K, idx, rank, score, n_det, bits, npig, A, T, c, len(caps) if M is None else M, r,
                                     len(rec) if R is None else R, precision, recall, scores, None)


def test_coco_accumulate_validates_its_arguments(lib):
    from locov_amd import _lib
    err = lib.locov_last_error
    assert _acc(lib, K=0) == 0                                                                          # no categories: a no-op
    assert _acc(lib, K=-1) == -1 and b"negative" in err()
    assert _acc(lib, n_det=-1) == -1 and b"negative" in err()
    assert _acc(lib, A=0) == -1 and _acc(lib, A=_lib.COCO_MAX_AREAS + 1) == -1 and b"area ranges" in err()
    assert _acc(lib, T=0) == -1 and _acc(lib, T=_lib.COCO_MAX_THRESHOLDS + 1) == -1 and b"IoU thresholds" in err()
    assert _acc(lib, caps=(1, 2, 3, 4)) == -1 and b"detection caps" in err()                            # M > 3
    assert _acc(lib, caps=(), M=0) == -1 and b"detection caps" in err()
    assert _acc(lib, caps=(10, 1)) == -1 and b"ascending" in err()
    assert _acc(lib, caps=(1, 1)) == -1 and b"ascending" in err()
    assert _acc(lib, caps=(0, 1)) == -1 and b"positive" in err()
    assert _acc(lib, rec=(), R=0) == -1 and b"recall thresholds" in err()
    assert _acc(lib, rec=(0.0,), R=_lib.COCO_MAX_RECALL_THRESHOLDS + 1) == -1 and b"recall thresholds" in err()
    assert _acc(lib, rec=(0.5, 0.25)) == -1 and b"recall thresholds must be ascending" in err()
    assert _acc(lib, caps=None, M=3) == -1 and b"null cap" in err()
    assert _acc(lib, rec=None, R=3) == -1 and b"null cap or recall" in err()
    assert _acc(lib, K=_lib.COCO_MAX_BLOCKS // 100) == -3 and b"above" in err()                         # LOCOV_ERR_UNSUPPORTED
    for name in ("cat_off", "npig", "precision", "recall"):
        assert _acc(lib, **{name: None}) == -1 and b"null pointer" in err()
    for name in ("idx", "rank", "score", "bits"):
        assert _acc(lib, **{name: None}) == -1 and b"null det pointer" in err()
    assert _acc(lib, precision=P((1 << 14) + 4)) == -1 and b"misaligned" in err()
    assert _acc(lib, cat_off=P(258)) == -1 and b"misaligned" in err()


def test_the_wrappers_refuse_cpu_tensors():
    import torch
    from locov_amd import ops
    from locov_amd._lib import LocovError
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(LocovError, match="only run on a ROCm GPU"):
        ops.coco_order(z, z, torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4), 2, 2)
    o = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(LocovError, match="only run on a ROCm GPU"):
        ops.coco_match(o, o, torch.zeros(4, 4), torch.zeros(1, 4, dtype=torch.float64), torch.zeros(1, dtype=torch.float64),
                       torch.zeros(1, dtype=torch.uint8), [[0, 1e10]], [0.5], 100)
    with pytest.raises(LocovError, match="only run on a ROCm GPU"):
        ops.coco_accumulate(o, o, o, torch.zeros(5, dtype=torch.float64), torch.zeros(5, 4, dtype=torch.uint8),
                            torch.zeros(4, 4, dtype=torch.int32), 1, (1, 10), [0.0, 1.0])
