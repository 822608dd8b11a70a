"""CPU-side checks of the fused attention core's C entry points (locov_mha_fwd / locov_mha_bwd, csrc/mha.hip): declared, bound and
exported with matching signatures under ABI version 8, and every unsupported or invalid argument reported by name before any HIP
call (the pointers below are never dereferenced: a call that got as far as a launch would fail differently)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["locov_mha_fwd", "locov_mha_bwd"]
P = ctypes.c_void_p
INVALID, UNSUPPORTED = -1, -3
CTYPE_OF = {"const float *": P, "float *": P, "const uint8_t *": P, "int64_t": ctypes.c_int64, "int": ctypes.c_int,
            "float": ctypes.c_float, "locov_stream_t": P}


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locov_hip.h")).read(), flags=re.S)


def test_exports_are_declared_bound_and_exported_with_matching_signatures(lib):
    from locov_amd import _lib, ops
    src = _header()
    for name in NEW:
        m = re.search(rf"\bint {name}\s*\((.*?)\);", src, flags=re.S)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [CTYPE_OF[re.match(r"(.*?)\b\w+$", p).group(1).strip()] for p in params]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes == types, (name, params)
        assert hasattr(lib, name), name
    assert re.search(rf"#define LOCOV_MHA_MAX_S {_lib.MHA_MAX_S}\b", src) and _lib.MHA_MAX_S >= 512
    assert re.search(rf"#define LOCOV_MHA_MAX_GRID {_lib.MHA_MAX_GRID}\b", src)
    assert ops.MHA_MAX_S == _lib.MHA_MAX_S and ops.MHA_HEAD_DIMS == (32, 64, 96, 128)
    assert lib.locov_abi_version() == 8 and _lib.ABI_VERSION == 8 and re.search(r"#define LOCOV_ABI_VERSION 8\b", src)
    mha = open(os.path.join(ROOT, "locov_amd", "csrc", "mha.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in mha                      # the products run on the f32-input MFMA


def _calls(lib):
    q, k, v, bias, keep, ctx, lse, dctx, delta, dq, dk, dv = (P(4096 * i) for i in range(1, 13))

    def fwd(S=17, d=32, H=2, nseq=3, q=q, ld=64, keep=None, p=0.0, lse=lse, ldo=64):
        return lib.locov_mha_fwd(q, ld, k, 64, v, 64, bias, keep, p, 0.125, nseq, S, H, d, ctx, ldo, lse, None)

    def bwd(S=17, d=32, H=2, nseq=3, q=q, ld=64, keep=None, p=0.0, lse=lse, ldo=64, dq=dq, lddq=64):
        return lib.locov_mha_bwd(q, ld, k, 64, v, 64, bias, keep, p, 0.125, nseq, S, H, d, dctx, ldo, lse, delta, dq, lddq, dk, 64,
                                 dv, 64, None)
    return fwd, bwd, keep


def test_rejections_name_the_condition_before_any_device_call(lib):
    from locov_amd import _lib
    fwd, bwd, keep = _calls(lib)
    err = lambda: lib.locov_last_error()
    for f in (fwd, bwd):
        for d in (48, 16, 0, 256):
            assert f(d=d, ld=4 * max(d, 1), ldo=4 * max(d, 1)) == UNSUPPORTED and b"head dim d must be 32, 64, 96 or 128" in err(), d
        assert f(S=0) == UNSUPPORTED and b"sequence length S must be in [1, 4096] (got 0)" in err()
        assert f(S=-3) == UNSUPPORTED and b"sequence length" in err()
        assert f(S=_lib.MHA_MAX_S + 1) == UNSUPPORTED and b"(got 4097)" in err()
        assert f(H=0) == UNSUPPORTED and b"Nseq and H" in err()
        assert f(nseq=70000) == UNSUPPORTED and b"Nseq and H" in err()
        assert f(q=None) == INVALID and b"null pointer q" in err()
        assert f(lse=None) == INVALID and b"null pointer" in err()
        assert f(q=P(4096 + 4)) == INVALID and b"q is not 16-byte aligned" in err()
        assert f(ld=66) == INVALID and b"pitch of q must be a multiple of 4 floats" in err()
        assert f(ld=60) == INVALID and b"pitch of q" in err() and b">= H*d = 64" in err()
        assert f(ldo=62) == INVALID and (b"pitch of ctx" in err() or b"pitch of dctx" in err())
        for p in (1.0, -0.1, float("nan")):
            assert f(keep=keep, p=p) == INVALID and b"p_drop must be in [0, 1)" in err()
    assert bwd(dq=None) == INVALID and b"null pointer dq" in err()
    assert bwd(lddq=63) == INVALID and b"pitch of dq" in err()


def test_ops_wrappers_check_their_arguments():
    from locov_amd import ops, transformer_head as th
    from locov_amd._lib import LocovError
    q, bias = torch.zeros(6, 64), torch.zeros(2, 3)
    with pytest.raises(TypeError, match="must be torch.Tensors"):
        ops.mha(q, None, q, bias, 2)
    for call in (lambda: ops.mha(q, q, q, bias, 2), lambda: ops.mha_packed(torch.zeros(6, 192), bias, 2),
                 lambda: th.attention_core(q, q, q, bias, 2)):
        with pytest.raises(LocovError, match="no CPU fallback"):      # a missing device is an error, not eager torch
            call()
