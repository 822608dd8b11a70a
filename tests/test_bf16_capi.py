"""CPU-side checks of the bf16 entry points (locov_gemm_nt_bf16, locov_conv3x3_nhwc_bf16, locov_f32_to_bf16,
locov_sim_gemm_bf16, locov_pack_conv3x3_weight): argument errors are reported, with their documented text, before any HIP
call, and empty problems return LOCOV_OK without a launch (no GPU here).  Every call below fails a check, or is empty: none
of the fake pointers reaches a kernel."""
import ctypes

import pytest

P = ctypes.c_void_p
A, B, C, D = P(1 << 12), P(2 << 12), P(3 << 12), P(4 << 12)          # 16-byte aligned fake device addresses


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def _fails(lib, rc, text):
    assert rc == -1, rc
    msg = lib.locov_last_error()
    assert text.encode() in msg, msg


def test_gemm_nt_bf16_rejects_bad_arguments(lib):
    def call(x=A, lda=64, w=B, y=C, ldc=48, M=32, N=48, K=64):
        return lib.locov_gemm_nt_bf16(x, lda, w, None, None, None, y, ldc, M, N, K, 0, None)
    for M, N, K in ((-1, 48, 64), (32, 0, 64), (32, 48, 0), (32, -5, 64)):
        _fails(lib, call(M=M, N=N, K=K), "locov_gemm_nt_bf16: bad shape")
    assert call(M=0, x=None, w=None, y=None) == 0                               # empty: OK, nothing launched
    for kw in ({"x": None}, {"w": None}, {"y": None}):
        _fails(lib, call(**kw), "locov_gemm_nt_bf16: null pointer")
    for K, lda in ((60, 64), (68, 72), (4, 8)):
        _fails(lib, call(K=K, lda=lda), "K and lda must be multiples of 8")
    _fails(lib, call(K=64, lda=68), "K and lda must be multiples of 8")
    _fails(lib, call(K=64, lda=56), "lda < K or ldc < N")
    _fails(lib, call(N=48, ldc=44), "lda < K or ldc < N")
    for x, w in ((P(A.value + 8), B), (A, P(B.value + 2)), (P(A.value + 4), P(B.value + 8))):
        _fails(lib, call(x=x, w=w), "x / W must be 16-byte aligned")


def test_conv3x3_nhwc_bf16_rejects_bad_arguments(lib):
    def call(x=A, R=4, H=7, W=7, Cin=64, w=B, y=C, N=40, pos_major=0):
        return lib.locov_conv3x3_nhwc_bf16(x, R, H, W, Cin, pos_major, w, None, None, None, y, N, 0, None)
    for kw in ({"R": -1}, {"H": 0}, {"W": 0}, {"Cin": 0}, {"N": 0}, {"H": -7}):
        _fails(lib, call(**kw), "locov_conv3x3_nhwc_bf16: bad shape")
    for pm in (0, 1):
        assert call(R=0, x=None, w=None, y=None, pos_major=pm) == 0
    for kw in ({"x": None}, {"w": None}, {"y": None}):
        _fails(lib, call(**kw), "locov_conv3x3_nhwc_bf16: null pointer")
    for Cin in (32, 8, 96, 200):
        _fails(lib, call(Cin=Cin), "Cin must be a multiple of 64")
    for kw in ({"x": P(A.value + 2)}, {"w": P(B.value + 8)}):
        _fails(lib, call(**kw), "locov_conv3x3_nhwc_bf16: misaligned pointer")
    for pm in (0, 1):
        _fails(lib, call(R=0x7FFFFFFF // 49 + 1, pos_major=pm), "locov_conv3x3_nhwc_bf16: R too large")
        _fails(lib, call(R=1 << 40, H=1, W=1, pos_major=pm), "locov_conv3x3_nhwc_bf16: R too large")


def test_f32_to_bf16_rejects_bad_arguments(lib):
    _fails(lib, lib.locov_f32_to_bf16(A, -1, B, None), "locov_f32_to_bf16: n < 0")
    assert lib.locov_f32_to_bf16(None, 0, None, None) == 0
    for x, y in ((None, B), (A, None)):
        _fails(lib, lib.locov_f32_to_bf16(x, 5, y, None), "locov_f32_to_bf16: null pointer")
    for x, y in ((P(A.value + 4), B), (P(A.value + 8), B), (A, P(B.value + 2)), (A, P(B.value + 4))):
        _fails(lib, lib.locov_f32_to_bf16(x, 5, y, None), "locov_f32_to_bf16: misaligned pointer")


def test_sim_gemm_bf16_rejects_bad_arguments(lib):
    def call(e=A, b=B, R=10, D=64, K1=9, out=C, ldc=9):
        return lib.locov_sim_gemm_bf16(e, b, R, D, K1, out, ldc, None)
    for kw in ({"R": -1}, {"D": 0}, {"K1": 0}):
        _fails(lib, call(**kw), "locov_sim_gemm_bf16: bad shape")
    assert call(R=0, e=None, b=None, out=None) == 0
    for kw in ({"e": None}, {"b": None}, {"out": None}):
        _fails(lib, call(**kw), "locov_sim_gemm_bf16: null pointer")
    for D in (4, 12, 100, 1020):
        _fails(lib, call(D=D), "D must be a multiple of 8")
    _fails(lib, call(K1=9, ldc=8), "locov_sim_gemm_bf16: ldc < K1")
    for kw in ({"e": P(A.value + 8)}, {"b": P(B.value + 2)}):
        _fails(lib, call(**kw), "emb / bank must be 16-byte aligned")


def test_pack_conv3x3_weight_rejects_bad_arguments(lib):
    from locov_amd import _lib
    _fails(lib, lib.locov_pack_conv3x3_weight(A, 0, 64, B, _lib.BF16, None), "locov_pack_conv3x3_weight: bad shape")
    _fails(lib, lib.locov_pack_conv3x3_weight(A, 8, 0, B, _lib.BF16, None), "locov_pack_conv3x3_weight: bad shape")
    _fails(lib, lib.locov_pack_conv3x3_weight(None, 8, 64, B, _lib.BF16, None), "locov_pack_conv3x3_weight: null pointer")
    _fails(lib, lib.locov_pack_conv3x3_weight(A, 8, 64, None, _lib.F32, None), "locov_pack_conv3x3_weight: null pointer")
    for dt in (2, -1):
        _fails(lib, lib.locov_pack_conv3x3_weight(A, 8, 64, B, dt, None), "locov_pack_conv3x3_weight: bad dtype")
