"""locov_lvis_match: declared in the header, bound and exported; every argument error is reported before any HIP call (no GPU
needed), in the style of tests/test_cocoeval_capi.py; the wrappers refuse CPU tensors."""
import ctypes
import os
import re

import pytest

P = ctypes.c_void_p
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "locov_hip.h")


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_the_export_is_declared_bound_and_present(lib):
    from locov_amd import _lib
    src = open(HEADER).read()
    decl = re.search(r"^int locov_lvis_match\(([^;]*)\);", src, re.M)
    assert decl, "locov_lvis_match is not declared in include/locov_hip.h"
    n_params = len(decl.group(1).split(","))
    restype, argtypes = _lib.SIGNATURES["locov_lvis_match"]
    assert restype is ctypes.c_int and len(argtypes) == n_params == 20
    assert argtypes == _lib.SIGNATURES["locov_coco_match"][1][:2] + [P] + _lib.SIGNATURES["locov_coco_match"][1][2:]   # + cell_flags
    assert lib.locov_lvis_match.argtypes == argtypes                                  # (a missing symbol fails load() itself)


def test_constants_agree_with_the_header(lib):
    from locov_amd import _lib
    src = open(HEADER).read()
    defs = dict(re.findall(r"#define LOCOV_(LVIS_[A-Z_]+) (\d+)", src))
    assert defs == {"LVIS_CELL_NEG": "1", "LVIS_CELL_NOT_EXHAUSTIVE": "2"}
    assert all(getattr(_lib, k) == int(v) for k, v in defs.items())
    assert _lib.ABI_VERSION == 8 and lib.locov_abi_version() == 8 and "#define LOCOV_ABI_VERSION 8" in src   # additive


def _match(lib, det_off=P(256), gt_off=P(512), flags=P(768), cells=10, n_det=5, n_gt=3, max_det=300, det_boxes=P(1024), gt_boxes=P(2048),
           gt_area=P(4096), gt_ignore_in=P(8192), areas=(0, 1e10, 0, 1024), n_areas=2, thrs=(0.5, 0.75), n_thrs=2, bits=P(1 << 14),
           gt_ignore=P(1 << 15), ws=P(1 << 16), ws_bytes=1 << 30):
    ar = (ctypes.c_double * len(areas))(*areas) if areas is not None else None
    th = (ctypes.c_double * len(thrs))(*thrs) if thrs is not None else None
    return lib.locov_lvis_match(det_off, gt_off, flags, cells, n_det, n_gt, max_det, det_boxes, gt_boxes, gt_area, gt_ignore_in, ar, n_areas,
                                th, n_thrs, bits, gt_ignore, ws, ws_bytes, None)


def test_lvis_match_validates_its_arguments(lib):
    from locov_amd import _lib
    err = lib.locov_last_error
    assert _match(lib, cells=0) == 0                                                                    # no cells: a no-op
    assert _match(lib, n_det=0, n_gt=0, det_off=None, gt_off=None, flags=None) == 0                     # no det and no gt: a no-op
    for kw in (dict(cells=-1), dict(n_det=-1), dict(n_gt=-1), dict(ws_bytes=-8)):
        assert _match(lib, **kw) == -1 and b"locov_lvis_match: negative" in err()
    assert _match(lib, max_det=0) == -1 and b"max_det" in err()
    assert _match(lib, n_areas=0) == -1 and b"area ranges" in err()
    assert _match(lib, n_areas=_lib.COCO_MAX_AREAS + 1) == -1 and b"area ranges" in err()
    assert _match(lib, n_thrs=0) == -1 and b"IoU thresholds" in err()
    assert _match(lib, n_thrs=_lib.COCO_MAX_THRESHOLDS + 1) == -1 and b"IoU thresholds" in err()
    assert _match(lib, areas=None) == -1 and b"null area range" in err()
    assert _match(lib, thrs=None) == -1 and b"null area range or threshold" in err()
    assert _match(lib, areas=(0, 1e10, 1024, 0)) == -1 and b"not ascending" in err()
    assert _match(lib, max_det=_lib.COCO_MAX_DET + 1) == -3 and b"dets per cell" in err()               # LOCOV_ERR_UNSUPPORTED
    assert _match(lib, cells=4 * _lib.COCO_MAX_BLOCKS + 1) == -3 and b"locov_lvis_match" in err()
    assert _match(lib, det_off=None) == -1 and b"null offsets" in err()
    assert _match(lib, gt_off=None) == -1 and b"null offsets" in err()
    assert _match(lib, flags=None) == -1 and b"null cell flags" in err()
    for name in ("det_boxes", "bits"):
        assert _match(lib, **{name: None}) == -1 and b"null det pointer" in err()
    for name in ("gt_boxes", "gt_area", "gt_ignore_in", "gt_ignore"):
        assert _match(lib, **{name: None}) == -1 and b"null gt pointer" in err()
    assert _match(lib, gt_boxes=P(2052)) == -1 and b"misaligned" in err()
    assert _match(lib, det_off=P(258)) == -1 and b"misaligned" in err()
    assert _match(lib, ws=None) == -1 and b"workspace" in err()
    assert _match(lib, ws=P((1 << 16) + 4)) == -1 and b"workspace" in err()
    need = lib.locov_coco_match_workspace_bytes(3, 300)                                                 # the COCO entry's workspace rule
    assert need == 3 * (300 * 8 + 64)
    assert _match(lib, ws_bytes=need - 1) == -1 and b"too small" in err()
    with pytest.raises(_lib.LocovError, match="null cell flags"):
        _lib.check(_match(lib, flags=None), "locov_lvis_match")


def test_the_wrappers_refuse_cpu_tensors():
    import torch
    from locov_amd import ops
    from locov_amd._lib import LocovError
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(LocovError, match="only run on a ROCm GPU"):
        ops.lvis_limit(z, z, torch.zeros(4, dtype=torch.float64), 2, 2, 300)
    o = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(LocovError, match="only run on a ROCm GPU"):
        ops.lvis_match(o, o, torch.zeros(4, dtype=torch.uint8), torch.zeros(4, 4), torch.zeros(1, 4, dtype=torch.float64),
                       torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.uint8), [[0, 1e10]], [0.5], 300)
