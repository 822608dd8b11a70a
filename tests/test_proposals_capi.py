"""locov_map_proposals (csrc/proposal_map.hip): argument errors are reported before any HIP call, so they can be checked without a GPU;
the header, the binding and the build agree about the new symbol."""
import ctypes
import os
import re

import pytest

import proposal_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_map_proposals_is_declared_bound_and_built_without_contraction(lib):
    from locov_amd import build, _lib
    header = open(os.path.join(ROOT, "include", "locov_hip.h")).read()
    assert "locov_map_proposals" in _lib.SIGNATURES and hasattr(lib, "locov_map_proposals")
    assert len(re.findall(r"\blocov_map_proposals\b", header)) >= 2                   # the "later, additively" list and the declaration
    assert "#define LOCOV_ABI_VERSION 8" in header and lib.locov_abi_version() == _lib.ABI_VERSION == 8     # additive
    for name, value in (("F32", _lib.PROPOSAL_F32), ("F64", _lib.PROPOSAL_F64)):
        assert re.search(r"#define LOCOV_PROPOSAL_%s %d\b" % (name, value), header)
    assert _lib.LABEL_MAX_IMAGES == pc.MAX_IMAGES
    assert "-ffp-contract=off" in build.FILE_FLAGS["proposal_map.hip"]
    # Boxes.clip's clamp has one copy, in a header both users include
    csrc = os.path.join(ROOT, "locov_amd", "csrc")
    defined = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip")) and re.search(r"float clamp_like_torch\(", open(os.path.join(csrc, f)).read())]
    assert defined == ["box_clip_common.h"]
    for user in ("image_batch.hip", "proposal_map.hip"):
        assert '#include "box_clip_common.h"' in open(os.path.join(csrc, user)).read()


def test_map_proposals_validates_its_arguments(lib):
    from locov_amd import _lib
    p = ctypes.c_void_p
    ints, longs, doubles = (lambda *v: (ctypes.c_int * len(v))(*v)), (lambda *v: (ctypes.c_int64 * len(v))(*v)), (lambda *v: (ctypes.c_double * len(v))(*v))
    many = _lib.LABEL_MAX_IMAGES + 1
    good = dict(rows=p(1 << 20), R=100, dtype=_lib.PROPOSAL_F64, starts=longs(40, 0), counts=ints(60, 40), fx=doubles(1.5, 1.0), fy=doubles(2.0, 1.0),
                flips=ints(1, 2), hs=ints(800, 37), ws=ints(1067, 53), n=2, topk=1000, thr=0.7,
                outs=[p(1 << 21), p(1 << 22), p(1 << 23), p(1 << 24), p(1 << 25), p(1 << 26), p(1 << 27)], counts_out=p(1 << 28))

    def call(**kw):
        a = dict(good, **kw)
        return lib.locov_map_proposals(a["rows"], a["R"], a["dtype"], a["starts"], a["counts"], a["fx"], a["fy"], a["flips"], a["hs"], a["ws"],
                                       a["n"], a["topk"], a["thr"], *a["outs"], a["counts_out"], None)

    def outs_with(k, value):
        outs = list(good["outs"])
        outs[k] = value
        return outs

    assert lib.locov_map_proposals(None, 0, 9, None, None, None, None, None, None, None, 0, -1, 0.7, *[None] * 8, None) == 0       # no images: a no-op
    assert call(n=many) == -1 and b"images per call" in lib.locov_last_error()
    assert call(n=-1) == -1
    for dtype in (-1, 2):
        assert call(dtype=dtype) == -1 and b"unknown dtype" in lib.locov_last_error()
    assert call(topk=-1) == -1 and b"topk" in lib.locov_last_error()
    for kw in ({"starts": None}, {"counts": None}, {"fx": None}, {"fy": None}, {"flips": None}, {"hs": None}, {"ws": None}, {"counts_out": None},
               {"rows": None}, *[{"outs": outs_with(k, None)} for k in range(7)]):
        assert call(**kw) == -1 and b"null pointer" in lib.locov_last_error(), kw
    assert call(counts=ints(60, -1)) == -1 and b"negative row count" in lib.locov_last_error()
    for flip in (-1, 3):
        assert call(flips=ints(0, flip)) == -1 and b"unknown flip" in lib.locov_last_error()
    assert call(hs=ints(800, -37)) == -1 and b"negative size" in lib.locov_last_error()
    for kw in ({"starts": longs(41, 0)}, {"starts": longs(40, -1)}, {"R": 99}, {"R": -1}, {"starts": longs(1 << 62, 0)}):
        assert call(**kw) == -1 and b"store" in lib.locov_last_error(), kw
    assert call(rows=p((1 << 20) + 4)) == -1 and b"element size" in lib.locov_last_error()                  # fp64 rows on a 4-byte boundary
    assert call(rows=p((1 << 20) + 2), dtype=_lib.PROPOSAL_F32) == -1 and b"element size" in lib.locov_last_error()
    for k, off in ((0, 8), (3, 8), (1, 2), (4, 2), (2, 4), (5, 4), (6, 4)):
        assert call(outs=outs_with(k, p(good["outs"][k].value + off))) == -1 and b"aligned" in lib.locov_last_error(), k
    assert call(counts_out=p((1 << 28) + 2)) == -1 and b"aligned" in lib.locov_last_error()
    big = (1 << 31) - 1
    assert call(R=1 << 40, starts=longs(0, 0), counts=ints(big, 1)) == -1 and b"int32" in lib.locov_last_error()


def test_ops_wrapper_refuses_cpu_tensors_and_bad_batches():
    import torch
    from locov_amd import ops
    from locov_amd._lib import LocovError
    assert ops.PROPOSAL_DTYPES == (torch.float32, torch.float64)
    with pytest.raises(LocovError, match="no CPU fallback"):
        ops.map_proposals(torch.zeros(4, 5), [0], [4], [(1.0, 1.0)], [0], [(8, 8)], 10, 0.7)
