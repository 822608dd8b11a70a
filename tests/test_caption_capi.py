"""CPU-side checks of the caption kernels' C entry points (locov_caption_embed_fwd / _bwd, csrc/caption.hip): declared, bound and
exported with matching signatures under ABI version 8, and every unsupported or invalid argument reported before any HIP call (the
pointers below are never dereferenced: a call that got as far as a launch would fail differently)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["locov_caption_embed_fwd", "locov_caption_embed_bwd_workspace_bytes", "locov_caption_embed_bwd"]
P = ctypes.c_void_p
INVALID, UNSUPPORTED = -1, -3
CTYPE_OF = {"const float *": P, "float *": P, "const uint8_t *": P, "const int *": P, "const double *": P, "const int64_t *": P,
            "int64_t *": P, "void *": P, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
            "locov_stream_t": P}


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_exports_are_declared_bound_and_exported_with_matching_signatures(lib):
    from locov_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locov_hip.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(rf"\b(int|int64_t) {name}\s*\((.*?)\);", src, flags=re.S)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        types = [CTYPE_OF[re.match(r"(.*?)\b\w+$", p).group(1).strip()] for p in params]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is CTYPE_OF[m.group(1)] and argtypes == types, (name, params)
        assert hasattr(lib, name), name
    assert re.search(rf"#define LOCOV_CAPTION_MAX_TOKENS {_lib.CAPTION_MAX_TOKENS}\b", src)
    assert re.search(rf"#define LOCOV_CAPTION_MAX_HIDDEN {_lib.CAPTION_MAX_HIDDEN}\b", src)
    assert (ops.CAPTION_MAX_TOKENS, ops.CAPTION_MAX_HIDDEN) == (8192, 4096)
    assert lib.locov_abi_version() == 8 and _lib.ABI_VERSION == 8


def _calls(lib):
    packed, draws, W, Pe, Tt, ga, be, keep, ints, emb, enc, mean, rstd, g, dW, ws = (P(4096 * i) for i in range(1, 17))

    def fwd(N=21, T=7, H=64, V=50, packed=packed, draws=draws, Pe=None, keep=None, p_drop=0.1, p=0.15, mask_id=4, len_tok=48, rows=6,
            max_pos=32, enc=enc):
        return lib.locov_caption_embed_fwd(packed, draws, N, T, H, V, W, Pe, max_pos, Tt, 2, ga, be, 1e-12, keep, p_drop, p, 0.9, 0.95, mask_id,
                                           len_tok, rows, ints, emb, enc, mean, rstd, None)

    def bwd(N=21, T=7, H=64, V=50, ints=ints, Pe=None, g_enc=None, g_in=g, dW=dW, ws=ws, ws_bytes=1 << 20):
        return lib.locov_caption_embed_bwd(ints, N, T, H, V, W, Pe, Tt, ga, mean, rstd, None, 0.0, g_enc, g_in, dW, ws, ws_bytes, None)
    return fwd, bwd, Pe, keep, g


def test_rejections_name_the_condition_before_any_device_call(lib):
    from locov_amd import _lib
    fwd, bwd, Pe, keep, g = _calls(lib)
    err = lambda: lib.locov_last_error()
    assert fwd(packed=None) == INVALID and b"null pointer" in err()
    assert fwd(N=_lib.CAPTION_MAX_TOKENS + 7, T=7) == UNSUPPORTED and b"over the limits" in err()
    assert fwd(H=_lib.CAPTION_MAX_HIDDEN + 4) == UNSUPPORTED and b"over the limits" in err()
    assert fwd(mask_id=50) == INVALID and b"mask_id 50 outside the word table" in err()
    assert fwd(mask_id=-1) == INVALID and b"mask_id" in err()
    assert fwd(len_tok=51) == INVALID and b"len_tok 51" in err()
    assert fwd(N=20) == INVALID and b"not a multiple of T" in err()
    assert fwd(rows=5) == INVALID and b"int_rows" in err()
    assert fwd(rows=4) == INVALID and b"draws need int_rows == 6" in err()
    assert fwd(p=0.0) == INVALID and b"MLM probabilities" in err()
    assert fwd(Pe=Pe, enc=None) == INVALID and b"LayerNorm path" in err()
    assert fwd(Pe=Pe, T=7, max_pos=6) == INVALID and b"exceeds the 6 position embeddings" in err()
    assert fwd(Pe=Pe, keep=keep, p_drop=1.0) == INVALID and b"p_drop must be in [0, 1)" in err()
    assert fwd(N=-1) == INVALID and b"negative count" in err()
    assert fwd(N=0) == 0 and fwd(N=0, packed=None, draws=None) == 0                # an empty input is a no-op
    assert bwd(dW=None) == INVALID and b"null pointer (dW)" in err()
    assert bwd(ints=None) == INVALID and b"null pointer" in err()
    assert bwd(g_in=None) == INVALID and b"no gradient given" in err()
    assert bwd(g_enc=g) == INVALID and b"g_enc without the LayerNorm path" in err()
    assert bwd(ws_bytes=16) == INVALID and b"too small" in err()
    assert bwd(N=_lib.CAPTION_MAX_TOKENS + 7) == UNSUPPORTED and bwd(H=_lib.CAPTION_MAX_HIDDEN + 4) == UNSUPPORTED
    assert bwd(V=0) == 0
    assert lib.locov_caption_embed_bwd_workspace_bytes(21, 64, 0) == 176 and lib.locov_caption_embed_bwd_workspace_bytes(21, 64, 1) == 176 + 21 * 64 * 4
    assert lib.locov_caption_embed_bwd_workspace_bytes(0, 64, 1) == 0


def test_ops_wrapper_checks_its_arguments():
    from locov_amd import ops
    from locov_amd._lib import LocovError
    with pytest.raises(LocovError, match="no CPU fallback"):      # a missing device is an error, not eager torch
        ops.caption_embed(torch.zeros(4, 6, dtype=torch.int32), None, 3, torch.zeros(10, 8))
