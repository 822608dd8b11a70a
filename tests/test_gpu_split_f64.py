"""Every launch form of the fp32-in / fp32-out GEMMs against float64, element by element (split_ref.py): the f32-MFMA NT GEMM at each
tile the dispatcher picks, the f16x2 split GEMM (128 x 128 and 256 x 256 tiles; split-layout A / output / residual; masked with a
device scale; mean-fused; batched), the Winograd convolution (f32 and split, both row orders, split-layout output, fused with conv1
and with the pooler, masked data gradient) and the weight gradients (TN GEMM f32 / split, Winograd, from the forward's kept V).

Inputs follow a magnitude ladder inside each tensor -- rows of A at ~1, 2^-6, 2^-12, 2^-18, 2^-26 and all-zero rows, rows of W from 1
down to 2^-12 -- so an error confined to the small rows (a flushed lo half, a dropped cross product on one tile) is not hidden by
the tensor's maximum, which is all a normwise check sees.  tests/test_split_gates.py shows on the CPU that the gate rejects those bugs.
Each case prints its worst err / bound (SPLITGATE lines with pytest -s).

The last test measures the head's logits at the evaluation scale (logit sigma = 3) against a float64 head."""
import numpy as np
import pytest
import torch

import split_ref as sr

pytestmark = pytest.mark.gpu

LADDER = (1.0, 2.0 ** -6, 2.0 ** -12, 2.0 ** -18, 2.0 ** -26, 0.0)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (run with -m 'not gpu' on CPU-only hosts)")
    from locov_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def _report(name, q):
    print(f"SPLITGATE {name} {q:.4f}")


def _ladder_rows(M, g, cols, heavy=True):
    """[M, cols] with row magnitudes cycling through LADDER; heavy: post-ReLU with a heavy tail (up to 8x)."""
    x = torch.randn(M, cols, generator=g)
    if heavy:
        x = x.relu() * torch.rand(M, cols, generator=g).pow(-0.5).clamp_max(8.0)
    mag = torch.tensor([LADDER[m % len(LADDER)] for m in range(M)])
    return x * mag[:, None]


def _ladder_w(N, K, g, amp=0.05):
    """[N, K] with rows from amp down to amp * 2^-12."""
    return torch.randn(N, K, generator=g) * amp * (2.0 ** -torch.linspace(0, 12, N)).view(-1, 1)


def _epi(g, M, N, kind):
    sc = torch.rand(N, generator=g) + 0.5 if "affine" in kind else None
    sh = torch.randn(N, generator=g) * 1e-2 if ("affine" in kind or "bias" in kind) else None
    res = _ladder_rows(M, g, N, heavy=False) * 1e-2 if "residual" in kind else None
    return sc, sh, res, "relu" in kind


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


# kernel classes of the library's launch record (locov_gemm_timing_*, include/locov_hip.h): which kernel a call ran
CLS_F32_128, CLS_F32_OTHER, CLS_SPLIT128, CLS_TN, CLS_TN_SPLIT = 0, 2, 5, 6, 7
CLS_WINO_FUSED, CLS_BIG, CLS_BATCHED_BIG, CLS_SEGMEAN_BIG = 8, 9, 10, 11
CLASSES = (0, 2, 5, 6, 7, 8, 9, 10, 11)


def _launched(fn):
    """(fn(), {class: launches}) -- the GEMM kernels fn launched, so that a case cannot pass on a silent fallback to another form."""
    import ctypes
    from locov_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.locov_gemm_timing_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        n = {}
        for cls in CLASSES:
            c, ms, fl = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            _lib.check(lib.locov_gemm_timing_read(cls, ctypes.byref(c), ctypes.byref(ms), ctypes.byref(fl)), "locov_gemm_timing_read")
            n[cls] = c.value
    finally:
        lib.locov_gemm_timing_enable(0)
    return out, n


# ------------------------------------------------------------------ f32 MFMA NT GEMM
def _tile(M, N):
    from test_gpu_bf16 import _tile as t
    return t(M, N)


F32_CASES = ([(301, N, 200, "affine+residual+relu") for N in (4, 32)]                 # 128x32; K = 200: not a multiple of 32
             + [(301, N, 264, "affine+residual+relu") for N in (36, 64, 132)]         # 128x64
             + [(801, 768, 136, "affine+residual+relu"), (801, 768, 96, "bias")]      # 64x64
             + [(6001, 768, 160, "affine+residual+relu"), (6001, 512, 128, "none")])  # 128x128


@pytest.mark.parametrize("M,N,K,epi", F32_CASES, ids=[f"f32nt-{_tile(M, N)}-M{M}-N{N}-K{K}-{e}" for M, N, K, e in F32_CASES])
def test_f32_nt_gemm(ops, M, N, K, epi):
    g = torch.Generator().manual_seed(M + 7 * N + K)
    wide = _ladder_rows(M, g, K + 12)
    x = wide[:, 4:4 + K]                                     # strided A (lda = K + 12)
    w = _ladder_w(N, K, g)
    sc, sh, res, relu = _epi(g, M, N, epi)
    xd = wide.cuda()[:, 4:4 + K]
    shd, scd, resd = _cuda(sh, sc, res)
    got, n = _launched(lambda: ops.linear(xd, w.cuda(), shd, scale=scd, residual=resd, relu=relu))
    assert n[CLS_F32_128 if _tile(M, N) == "128x128" else CLS_F32_OTHER] == 1, n
    r = sr.epilogue(sr.gemm(x, w), sc, sh, res, relu)
    q = sr.assert_gate(got, r, f"f32 NT {M}x{N}x{K} {epi}")
    _report(f"f32nt[{_tile(M, N)} M{M} N{N} K{K} {epi} strided]", q)


@pytest.mark.parametrize("M,N,K", [(301, 32, 96), (801, 768, 200), (6001, 512, 128)], ids=["masked-128x32", "masked-64x64", "masked-128x128"])
def test_f32_nt_gemm_masked(ops, M, N, K):
    g = torch.Generator().manual_seed(M + N)
    x, w = _ladder_rows(M, g, K, heavy=False), _ladder_w(N, K, g)
    act = torch.randn(M, N, generator=g)
    got, n = _launched(lambda: ops.linear_ex(x.cuda(), w.cuda(), mask=act.cuda()))
    assert n[CLS_F32_128 if _tile(M, N) == "128x128" else CLS_F32_OTHER] == 1, n
    r = sr.epilogue(sr.gemm(x, w), mask=act)
    assert bool((got.cpu()[act <= 0] == 0).all())
    _report(f"f32nt-masked[{_tile(M, N)} M{M} N{N} K{K}]", sr.assert_gate(got, r, "masked f32 NT"))


# ------------------------------------------------------------------ split GEMM, 128 x 128 tile
SPLIT_K = (160, 256)                                         # an odd multiple of 32 (a ragged tile count) and a multiple of 64


@pytest.mark.parametrize("K", SPLIT_K)
@pytest.mark.parametrize("epi", ["none", "affine+residual+relu"])
def test_split_gemm_128(ops, monkeypatch, epi, K):
    monkeypatch.setenv("LOCOV_SPLIT_BIG", "0")
    M, N = 1037, 388
    g = torch.Generator().manual_seed(K + len(epi))
    wide = _ladder_rows(M, g, K + 32)
    x = wide[:, 32:]
    w = _ladder_w(N, K, g)
    sc, sh, res, relu = _epi(g, M, N, epi)
    wp = ops.split_pack(w.cuda())
    shd, scd, resd = _cuda(sh, sc, res)
    got, n = _launched(lambda: ops.linear_split(wide.cuda()[:, 32:], wp, shd, scale=scd, residual=resd, relu=relu))
    assert n[CLS_SPLIT128] == 1 and n[CLS_BIG] == 0, n
    r = sr.epilogue(sr.gemm(x, w, (16.0, wp.scale)), sc, sh, res, relu)
    _report(f"split128[M{M} N{N} K{K} {epi} strided]", sr.assert_gate(got, r, f"split 128 {epi} K{K}"))


@pytest.mark.parametrize("K", SPLIT_K)
def test_split_gemm_split_layouts(ops, monkeypatch, K):
    """A given in the split layout (x_is_split), the output written in it (out_split) and a residual read from it (residual_is_split).
    The reference takes the values the split tensors hold, split_unpack."""
    monkeypatch.setenv("LOCOV_SPLIT_BIG", "0")
    M, N = 733, 160
    g = torch.Generator().manual_seed(K)
    x, w = _ladder_rows(M, g, K), _ladder_w(N, K, g)
    sc, sh, res, relu = _epi(g, M, N, "affine+residual+relu")
    xs = ops.split_pack(x.cuda(), 16.0).data
    rs = ops.split_pack(res.cuda(), 16.0).data
    xv, rv = ops.split_unpack(xs, 16.0).cpu(), ops.split_unpack(rs, 16.0).cpu()
    wp = ops.split_pack(w.cuda())
    r = sr.epilogue(sr.gemm(xv, w, (16.0, wp.scale)), sc, sh, rv, relu)
    y = ops.linear_split(xs, wp, sh.cuda(), scale=sc.cuda(), residual=rs, relu=True, x_is_split=True, residual_is_split=True)
    _report(f"split128-a_split-res_split[M{M} N{N} K{K}]", sr.assert_gate(y, r, "x_is_split + residual_is_split"))
    ys = ops.linear_split(xs, wp, sh.cuda(), scale=sc.cuda(), residual=rs, relu=True, x_is_split=True, residual_is_split=True,
                          out_split=True)
    q = sr.assert_gate(ops.split_unpack(ys, 16.0), sr.stored_split(r, 16.0), "out_split")
    _report(f"split128-out_split[M{M} N{N} K{K}]", q)


@pytest.mark.parametrize("K", SPLIT_K)
def test_split_gemm_masked_device_scale(ops, monkeypatch, K):
    """The data-gradient form: x (a gradient) with its operand scale chosen on the device, the ReLU-backward mask, max |y| out."""
    monkeypatch.setenv("LOCOV_SPLIT_BIG", "0")
    M, N = 911, 132
    g = torch.Generator().manual_seed(K + 1)
    x = _ladder_rows(M, g, K, heavy=False) * 3e-3
    w = _ladder_w(N, K, g)
    act = torch.randn(M, N, generator=g)
    xd = x.cuda()
    slot = ops.split_scale_from_amax(xd)
    amax = ops.scale_slot(xd)
    wp = ops.split_pack(w.cuda())
    got = ops.linear_split_ex(xd, wp, mask=act.cuda(), x_scale_dev=slot, amax_out=amax)
    sa = sr.slot_scale(slot)
    assert sa == 2.0 ** (13 - np.frexp(float(x.abs().max()))[1])
    r = sr.epilogue(sr.gemm(x, w, (sa, wp.scale)), mask=act)
    _report(f"split128-masked-devscale[M{M} N{N} K{K} s_a=2^{int(np.log2(sa))}]", sr.assert_gate(got, r, "masked split"))
    assert float(amax.cpu()[2]) == float(got.abs().max())


# ------------------------------------------------------------------ split GEMM, 256 x 256 tile and the mean-fused form
# The 256 x 256 kernel (gemm_split_big.hip) only takes a PRE-SPLIT A (x_is_split), K % 64 == 0, N % 8 == 0, no mask / device scale;
# LOCOV_SPLIT_BIG=1 lifts the size heuristic only.  Every case asserts the kernel class that ran (_launched).
def _presplit(ops, x):
    """x in the split layout at 16 (what the producing GEMM writes with out_split) and the values it holds."""
    xs = ops.split_pack(x.cuda(), 16.0).data
    return xs, ops.split_unpack(xs, 16.0).cpu()


@pytest.mark.parametrize("K", (256, 192), ids=lambda k: f"K{k}")
def test_split_gemm_256(ops, monkeypatch, K):
    monkeypatch.setenv("LOCOV_SPLIT_BIG", "1")
    M, N = 1301, 544                                          # ragged M and N tiles
    g = torch.Generator().manual_seed(K + 2)
    x, w = _ladder_rows(M, g, K), _ladder_w(N, K, g)
    sc, sh, res, relu = _epi(g, M, N, "affine+residual+relu")
    xs, xv = _presplit(ops, x)
    wp = ops.split_pack(w.cuda())
    got, n = _launched(lambda: ops.linear_split(xs, wp, sh.cuda(), scale=sc.cuda(), residual=res.cuda(), relu=True, x_is_split=True))
    assert n[CLS_BIG] == 1 and n[CLS_SPLIT128] == 0, n
    r = sr.epilogue(sr.gemm(xv, w, (16.0, wp.scale)), sc, sh, res, relu)
    _report(f"split256-forced[M{M} N{N} K{K} a_split affine+residual+relu]", sr.assert_gate(got, r, "split 256"))
    # conv3 of Res5 blocks 0-1: the residual read from and the output written in the split layout
    rs, rv = _presplit(ops, res)
    ys, n = _launched(lambda: ops.linear_split(xs, wp, sh.cuda(), scale=sc.cuda(), residual=rs, relu=True, x_is_split=True,
                                               residual_is_split=True, out_split=True))
    assert n[CLS_BIG] == 1 and n[CLS_SPLIT128] == 0, n
    r = sr.stored_split(sr.epilogue(sr.gemm(xv, w, (16.0, wp.scale)), sc, sh, rv, relu), 16.0)
    _report(f"split256-forced[M{M} N{N} K{K} a_split res_split out_split]", sr.assert_gate(ops.split_unpack(ys, 16.0), r, "split 256 split layouts"))


def test_split_gemm_natural_size(ops, monkeypatch):
    """Res5's conv3 shape at the size where the dispatcher itself picks the 256 x 256 tile (>= 1024 tiles, N % 256 == 0); the bound is
    checked on a sample of rows (every 29th and the ragged last tile)."""
    monkeypatch.delenv("LOCOV_SPLIT_BIG", raising=False)
    M, N, K = 49 * 669, 2048, 512
    g = torch.Generator().manual_seed(9)
    x, w = _ladder_rows(M, g, K), _ladder_w(N, K, g)
    sh = torch.randn(N, generator=g) * 1e-2
    xs, xv = _presplit(ops, x)
    wp = ops.split_pack(w.cuda())
    got, n = _launched(lambda: ops.linear_split(xs, wp, sh.cuda(), relu=True, x_is_split=True))
    assert n[CLS_BIG] == 1 and n[CLS_SPLIT128] == 0, n
    rows = torch.cat([torch.arange(0, M - 256, 29), torch.arange(M - 256, M)])
    r = sr.epilogue(sr.gemm(xv[rows], w, (16.0, wp.scale)), shift=sh, relu=True)
    _report(f"split256-natural[M{M} N{N} K{K} a_split]", sr.assert_gate(got[rows.cuda()], r, "split natural size"))


SEGMEAN = [("128", "pos-major-res", False), ("128", "roi-major-res", False), ("256", "roi-major-res", True)]


@pytest.mark.parametrize("tile,order,presplit", SEGMEAN, ids=[f"segmean-{t}-{o}" for t, o, _ in SEGMEAN])
def test_split_segmean(ops, monkeypatch, tile, order, presplit):
    """The mean-fused form; the 256 x 256 one needs a pre-split A and the ROI-major residual."""
    monkeypatch.setenv("LOCOV_SPLIT_BIG", "1" if tile == "256" else "0")
    R, seg, N, K = 53, 49, 264, 160 if tile == "128" else 192
    M = R * seg
    g = torch.Generator().manual_seed(R + len(order) + int(presplit))
    mag = torch.tensor([LADDER[q % len(LADDER)] for q in range(R)]).repeat_interleave(seg)      # per-ROI magnitude ladder
    x = torch.randn(M, K, generator=g).relu() * mag[:, None]
    w = _ladder_w(N, K, g)
    sc, sh = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 1e-3
    res_rm = torch.randn(M, N, generator=g) * 1e-2 * mag[:, None]
    res_pm = res_rm.view(R, seg, N).permute(1, 0, 2).reshape(M, N).contiguous()
    wp = ops.split_pack(w.cuda())
    if presplit:
        xd, x = _presplit(ops, x)
    else:
        xd = x.cuda()
    rm = order == "roi-major-res"
    got, n = _launched(lambda: ops.linear_split_segmean(xd, wp, sh.cuda(), (res_rm if rm else res_pm).cuda(), seg, scale=sc.cuda(),
                                                        residual_roi_major=rm, x_is_split=presplit))
    assert (n[CLS_SEGMEAN_BIG], n[CLS_SPLIT128]) == ((1, 0) if tile == "256" else (0, 1)), n
    r = sr.segmean(sr.epilogue(sr.gemm(x, w, (16.0, wp.scale)), sc, sh, res_rm, True), seg)
    _report(f"segmean{tile}[{order}{' a_split' if presplit else ''} R{R} N{N} K{K}]", sr.assert_gate(got, r, f"segmean {tile} {order}"))


def test_split_batched(ops):
    """gemm_nt_batched_split (fp32 A: always the 128 x 128 tile) and the f32-MFMA batched GEMM on 121 problems; the batched 256 x 256
    tile is reached through the Winograd convolution (test_winograd_conv, split-*-big)."""
    B, M, N, K = 121, 133, 68, 160
    g = torch.Generator().manual_seed(121)
    x = torch.stack([_ladder_rows(M, g, K) for _ in range(B)]) * 4
    w = torch.stack([_ladder_w(N, K, g) for _ in range(B)])
    wp = ops.split_pack(w.cuda())
    got, n = _launched(lambda: ops.gemm_nt_batched_split(x.cuda(), wp, x_scale=0.25))
    assert n[CLS_SPLIT128] == 1 and n[CLS_BATCHED_BIG] == 0, n
    _report(f"batched-split128[B{B} M{M} N{N} K{K}]", sr.assert_gate(got, sr.gemm_batched(x, w, (0.25, wp.scale)), "batched split"))
    got32 = ops.gemm_nt_batched(x.cuda(), w.cuda())
    _report(f"batched-f32[B{B} M{M} N{N} K{K}]", sr.assert_gate(got32, sr.gemm_batched(x, w), "batched f32"))


# ------------------------------------------------------------------ Winograd convolution
def _tiles(R, C, g):
    """d [R,C,7,7]: ROIs cycle through the ladder, post-ReLU heavy-tailed."""
    d = _ladder_rows(R, g, C * 49).view(R, C, 7, 7)
    return d


def _pos_rows(d):
    R, C = d.shape[:2]
    return d.permute(2, 3, 0, 1).reshape(49 * R, C).contiguous()


def _roi_rows(d):
    R, C = d.shape[:2]
    return d.permute(0, 2, 3, 1).reshape(49 * R, C).contiguous()


def _from_rows(y, R, roi_major):
    N = y.shape[1]
    return (y.reshape(R, 7, 7, N).permute(0, 3, 1, 2) if roi_major else y.reshape(7, 7, R, N).permute(2, 3, 0, 1)).cpu()


def _wino_epi(r, sc, sh, relu=True):
    v = lambda t: t.view(1, -1, 1, 1)
    return sr.epilogue(r, v(sc), v(sh), relu=relu)


@pytest.mark.parametrize("form", ["f32-pos", "f32-roi", "split-pos", "split-roi", "split-roi-outsplit", "split-pos-big", "split-roi-big"])
def test_winograd_conv(ops, monkeypatch, form):
    """*-big: the 121 transform-domain GEMMs on the batched 256 x 256 tile (V is written pre-split; LOCOV_SPLIT_BIG=1 lifts the size
    heuristic), otherwise on the 128 x 128 one."""
    monkeypatch.setenv("LOCOV_SPLIT_BIG", "1" if form.endswith("big") else "0")
    R, C, N = 67, 128, 96                                    # N % 32 == 0: the split-layout output
    g = torch.Generator().manual_seed(len(form) + R)
    d = _tiles(R, C, g)
    w = torch.randn(N, C, 3, 3, generator=g) * 0.05
    sc, sh = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 1e-3
    roi = "roi" in form
    x = (_roi_rows(d) if roi else _pos_rows(d)).cuda()
    U = ops.winograd_pack_weight(w.cuda())
    if form.startswith("f32"):
        y = ops.winograd_conv3x3(x, U, scale=sc.cuda(), shift=sh.cuda(), relu=True, roi_major=roi, in_roi_major=roi)
        r = _wino_epi(sr.wino_conv(d, w), sc, sh)
    else:
        Up = ops.split_pack(U)
        oss = 16.0 if "outsplit" in form else None
        y, n = _launched(lambda: ops.winograd_conv3x3(x, Up, scale=sc.cuda(), shift=sh.cuda(), relu=True, roi_major=roi, in_roi_major=roi,
                                                      out_split_scale=oss))
        assert (n[CLS_BATCHED_BIG], n[CLS_SPLIT128]) == ((1, 0) if form.endswith("big") else (0, 1)), n
        if oss:
            y = ops.split_unpack(y, oss)
        r = _wino_epi(sr.wino_conv(d, w, (0.25, Up.scale)), sc, sh)
        if oss:
            r = sr.stored_split(r, oss)
    _report(f"winograd[{form} R{R} C{C} N{N}]", sr.assert_gate(_from_rows(y, R, roi), r, f"winograd {form}"))


def _compose(r1: "sr.Ref", w, split):
    """Winograd convolution of a computed input: the reference of the float64 input r1.ref, with r1's own bound carried through the
    magnitude of the transforms."""
    r2 = sr.wino_conv(r1.ref, w, split)
    carried = sr.wino_conv(sr.bound(r1), w.abs()).S
    return sr.Ref(r2.ref, r2.S, r2.E + carried, r2.K)


@pytest.mark.parametrize("fuse", ["1", "0"], ids=["conv1-wino-fused", "conv1-wino-unfused"])
def test_conv1x1_winograd(ops, monkeypatch, fuse):
    monkeypatch.setenv("LOCOV_WINO_FUSE", fuse)
    monkeypatch.setenv("LOCOV_SPLIT_BIG", "1")
    R, K, C, N = 23, 192, 256, 64                             # K % 64 == 0, C % 256 == 0: the fused form qualifies
    g = torch.Generator().manual_seed(23 + int(fuse))
    mag = torch.tensor([LADDER[q % (len(LADDER) - 1)] for q in range(R)]).repeat_interleave(49)
    x = torch.randn(49 * R, K, generator=g).relu() * mag[:, None]
    xs = ops.split_pack(x.cuda(), 16.0).data
    xv = ops.split_unpack(xs, 16.0).cpu()
    w1 = torch.randn(C, K, generator=g) * 0.05
    s1, b1 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 1e-3
    w2 = torch.randn(N, C, 3, 3, generator=g) * 0.03
    s2, b2 = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 1e-3
    w1p = ops.split_pack(w1.cuda())
    Up = ops.split_pack(ops.winograd_pack_weight(w2.cuda()))
    y, n = _launched(lambda: ops.conv1x1_winograd_conv3x3(xs, w1p, b1.cuda(), Up, scale1=s1.cuda(), scale2=s2.cuda(), shift2=b2.cuda(),
                                                          relu=True, x_scale=16.0))
    # fused: conv1 on the 256 x 256 tile with the input transform in its epilogue; unfused: conv1 on the 256 x 256 tile writing the
    # pixels, then the transform; either way the batched 256 x 256 tile for the 121 GEMMs
    assert (n[CLS_WINO_FUSED], n[CLS_BIG], n[CLS_BATCHED_BIG], n[CLS_SPLIT128]) == ((1, 0, 1, 0) if fuse == "1" else (0, 1, 1, 0)), n
    r1 = sr.epilogue(sr.gemm(xv, w1, (16.0, w1p.scale)), s1, b1, relu=True)
    to_tiles = lambda t: t.view(R, 7, 7, -1).permute(0, 3, 1, 2)
    r1 = sr.Ref(to_tiles(r1.ref), to_tiles(r1.S), to_tiles(r1.E), r1.K)
    r = _wino_epi(_compose(r1, w2, (0.25, Up.scale)), s2, b2)
    _report(f"conv1x1-winograd[fuse={fuse} R{R} K{K} C{C} N{N}]", sr.assert_gate(_from_rows(y, R, True), r, "conv1x1 + winograd"))


@pytest.mark.parametrize("fuse", ["1", "0"], ids=["pooler-wino-fused", "pooler-wino-unfused"])
def test_roi_align_winograd(ops, monkeypatch, fuse):
    """Block 0's pooler + FrozenBN + ReLU + conv2; the reference starts from roi_align_nhwc's output (checked against the oracle
    elsewhere) and runs the convolution in float64."""
    monkeypatch.setenv("LOCOV_WINO_FUSE", fuse)
    Nimg, H, W, C, R, N = 2, 25, 38, 128, 37, 64
    g = torch.Generator().manual_seed(5 + int(fuse))
    feat = torch.randn(Nimg, H, W, C, generator=g) * torch.tensor([LADDER[c % 5] for c in range(C)])
    wh = torch.rand(R, 2, generator=g) * torch.tensor([W * 16.0, H * 16.0]) * 0.9 + 4.0
    xy = torch.rand(R, 2, generator=g) * torch.tensor([W * 16.0, H * 16.0]) - 20.0
    rois = torch.cat([torch.randint(0, Nimg, (R, 1), generator=g).float(), xy, xy + wh], dim=1).cuda()
    s1, b1 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 1e-4
    w2 = torch.randn(N, C, 3, 3, generator=g) * 0.03
    s2, b2 = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 1e-3
    Up = ops.split_pack(ops.winograd_pack_weight(w2.cuda()))
    fd = feat.cuda()
    pooled = ops.roi_align_nhwc(fd, rois, 14, 1.0 / 16, 0, True, bin_stride=2, ch_scale=s1.cuda(), ch_shift=b1.cuda(), relu=True)
    y = ops.roi_align_winograd_conv3x3(fd, rois, 14, 1.0 / 16, 0, True, Up, ch_scale=s1.cuda(), ch_shift=b1.cuda(), scale2=s2.cuda(),
                                       shift2=b2.cuda(), relu=True)
    d = pooled.view(R, 7, 7, C).permute(0, 3, 1, 2).cpu()
    r = _wino_epi(sr.wino_conv(d, w2, (0.25, Up.scale)), s2, b2)
    _report(f"pooler-winograd[fuse={fuse} R{R} C{C} N{N}]", sr.assert_gate(_from_rows(y, R, True), r, "pooler + winograd"))


@pytest.mark.parametrize("form", ["f32", "split"], ids=["wino-dgrad-f32", "wino-dgrad-split"])
def test_winograd_masked_data_gradient(ops, form):
    R, C, N = 41, 64, 96
    g = torch.Generator().manual_seed(41 + len(form))
    d = _tiles(R, C, g) * 1e-3                                # a gradient: small, signed
    d = d * torch.sign(torch.randn(d.shape, generator=g))
    w = torch.randn(N, C, 3, 3, generator=g) * 0.05
    act = torch.randn(R, N, 7, 7, generator=g)
    x, mask = _roi_rows(d).cuda(), _roi_rows(act).cuda()
    U = ops.winograd_pack_weight(w.cuda())
    if form == "f32":
        y = ops.winograd_conv3x3_ex(x, U, mask=mask)
        r = sr.epilogue(sr.wino_conv(d, w), mask=act)
    else:
        Up = ops.split_pack(U)
        amax = ops.scale_slot(x)
        y = ops.winograd_conv3x3_split_ex(x, Up, mask=mask, amax_out=amax)
        sv = sr.slot_scale(ops.winograd_scale_slot(x, R, C, N))
        r = sr.epilogue(sr.wino_conv(d, w, (sv, Up.scale)), mask=act)
        assert float(amax.cpu()[2]) == float(y.abs().max())
        form += f" s_v=2^{int(np.log2(sv))}"
    _report(f"wino-dgrad-masked[{form} R{R} C{C} N{N}]", sr.assert_gate(_from_rows(y, R, True), r, "masked winograd dgrad"))


# ------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("form", ["f32", "split", "split-b_split"])
def test_tn_weight_gradient(ops, form):
    M, N, K = 49 * 31, 132, 96
    g = torch.Generator().manual_seed(M + len(form))
    a = _ladder_rows(M, g, N, heavy=False) * 1e-3            # the gradient
    b = _ladder_rows(M, g, K)                                 # the activation
    rs = torch.rand(N, generator=g) + 0.5
    ad, bd = a.cuda(), b.cuda()
    if form == "f32":
        got, n = _launched(lambda: ops.gemm_tn(ad, bd, rs.cuda()))
        assert n[CLS_TN] == 1 and n[CLS_TN_SPLIT] == 0, n
        r = sr.tn(a, b, None, rs)
    else:
        slot = ops.split_scale_from_amax(ad)
        if form == "split-b_split":
            bs = ops.split_pack(bd, 16.0).data
            got, n = _launched(lambda: ops.gemm_tn_split(ad, bs, rs.cuda(), slot, 16.0, b_is_split=True))
            assert n[CLS_TN_SPLIT] == 1 and n[CLS_TN] == 0, n
            b = ops.split_unpack(bs, 16.0).cpu()
        else:
            got, n = _launched(lambda: ops.gemm_tn_split(ad, bd, rs.cuda(), slot, 16.0))
        assert n[CLS_TN_SPLIT] == 1 and n[CLS_TN] == 0, n
        r = sr.tn(a, b, (sr.slot_scale(slot), 16.0), rs)
    _report(f"tn-wgrad[{form} M{M} N{N} K{K}]", sr.assert_gate(got, r, f"TN {form}"))


@pytest.mark.parametrize("form", ["f32", "split", "split-v_split"])
def test_winograd_weight_gradient(ops, form):
    R, C, N = 37, 64, 96
    g = torch.Generator().manual_seed(R + len(form))
    d = _tiles(R, C, g)
    gr = _tiles(R, N, g) * 1e-3 * torch.sign(torch.randn(R, N, 7, 7, generator=g))
    rs = torch.rand(N, generator=g) + 0.5
    x, gy = _roi_rows(d).cuda(), _roi_rows(gr).cuda()
    if form == "f32":
        dw, n = _launched(lambda: ops.winograd_wgrad(x, gy, rs.cuda()))
        assert n[CLS_TN] == 1 and n[CLS_TN_SPLIT] == 0, n
        r = sr.wino_wgrad(d, gr, None, rs)
    else:
        kw = {}
        if form == "split-v_split":
            U = ops.split_pack(ops.winograd_pack_weight((torch.randn(N, C, 3, 3, generator=g) * 0.05).cuda()))
            fws = torch.empty(ops.winograd_workspace_bytes(R, C, N), dtype=torch.uint8, device="cuda")
            ops.winograd_conv3x3(x, U, in_roi_major=True, roi_major=True, workspace=fws)
            kw["v_split"] = fws
        dw, n = _launched(lambda: ops.winograd_wgrad(x, gy, rs.cuda(), split=True, **kw))
        assert n[CLS_TN_SPLIT] == 1 and n[CLS_TN] == 0, n
        sm = sr.slot_scale(ops.winograd_scale_slot(x, R, C, N, wgrad=True))
        r = sr.wino_wgrad(d, gr, (sm, 0.25), rs)
        form += f" s_dM=2^{int(np.log2(sm))}"
    _report(f"wino-wgrad[{form} R{R} C{C} N{N}]", sr.assert_gate(dw, r, "winograd wgrad"))


# ------------------------------------------------------------------ the logit gate at the evaluation scale
# device error (either Res5 arithmetic) against the float64 head <= LOGIT_MULT x the torch-fp32 oracle's own error + LOGIT_FLOOR x max |logit|.
# Both constants were CHOSEN BY HAND before the first measurement, not derived: the device's head runs more fp32 roundings than the
# oracle's (Winograd transforms, the split operands, the fused mean) and LOGIT_FLOOR (~1e-5 at |logit| 10.5, a tenth of the 1e-4 logit
# gate) dominates the allowance.  Measured on an MI355X: 6.4e-6 / 1.8e-5 (f16x2, small / coco_lsm), 7.4e-6 / 1.5e-5 (fp32), the oracle
# 2.1e-6 / 2.7e-6 -- the device is ~3-7x the oracle, and the coco_lsm f16x2 case passes its 2.1e-5 allowance by ~15 %.
LOGIT_MULT = 4.0
LOGIT_FLOOR = 2.0 ** -20


@pytest.mark.parametrize("size", ["small", "coco_lsm"])
def test_logits_at_sigma3_against_a_float64_head(ops, size):
    """The bank rescaled so that the logits have sigma = 3 over the proposals (bench.eval_heads); the head recomputed in float64 from
    the device's pooled rows; f16x2 and fp32 device logits and the CPU fp32 oracle (torch arithmetic) measured against it."""
    import locov_amd as pkg
    from oracle import lsm_oracle as oracle
    import test_gpu_roi_heads as T
    oracle.build()
    heads, seed = {}, 1992
    for dtype in ("f16x2", "fp32"):
        if size == "small":
            cfg = T._small_cfg(pkg)
        else:
            cfg = pkg.config.get_cfg()
            cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
            cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
            cfg.MODEL.ROI_HEADS.NAME = "EmbeddingProposalsRes5ROIHeads"
        cfg.MODEL.ROI_BOX_HEAD.RES5_DTYPE = dtype
        heads[dtype], params, h = T._make_heads(pkg, oracle, cfg, 80, seed)
    c_in = heads["fp32"].res5.state_dict()["0.conv1.weight"].shape[1]
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((2, c_in, 50, 84)).astype(np.float32)
    props, boxes = T._proposals(pkg, oracle, rng, 2, 60)
    rois = T.dev(oracle.boxes_to_pooler_format(boxes))

    def device_logits(dtype):
        with torch.no_grad():
            bf = heads[dtype]._shared_roi_transform([T.dev(feat)], [p.proposal_boxes for p in props])
            return heads[dtype].box_predictor(heads[dtype]._pooled_mean(bf))[0].double().cpu()

    std = float(device_logits("fp32")[:, :-1].std())
    h = dict(h, cls_w=(h["cls_w"] * np.float32(3.0 / std)).astype(np.float32))
    for hd in heads.values():
        hd.box_predictor.set_class_embeddings(h["cls_w"])
    with torch.no_grad():
        pooled = ops.roi_align_nhwc(ops.nchw_to_nhwc(T.dev(feat)), rois, 14, 1.0 / 16, 0, True).permute(0, 3, 1, 2).double().cpu()
    r5 = oracle.res5_stage(pooled, params, dtype=torch.float64)
    d64 = lambda a: torch.as_tensor(a).double()
    emb = r5.mean(dim=(2, 3)) @ d64(h["emb_w"]).t() + d64(h["emb_b"])
    want = emb @ d64(h["cls_w"]).t()
    sigma = float(want[:, :-1].std())
    top = float(want.abs().max())
    err = {k: float((device_logits(k) - want).abs().max()) for k in ("f16x2", "fp32")}
    err["oracle"] = float((torch.from_numpy(oracle.roi_head_forward(feat, boxes, params, h)["scores"]).double() - want).abs().max())
    print(f"SPLITGATE logits-sigma3[{size}] sigma {sigma:.3f} max|logit| {top:.2f} "
          f"f16x2 {err['f16x2']:.3e} fp32 {err['fp32']:.3e} torch-fp32-oracle {err['oracle']:.3e}")
    assert abs(sigma - 3.0) < 0.05, sigma
    for k in ("f16x2", "fp32"):
        assert err[k] <= LOGIT_MULT * err["oracle"] + LOGIT_FLOOR * top, (k, err)
