"""CPU proof that the per-element gate of the fp32 / f16x2-split GEMM and Winograd tests (split_ref.assert_gate, used by
tests/test_gpu_split_f64.py) bites.  A torch emulation of the split arithmetic -- hi = fp16(s x), lo = fp16(s x - hi) with subnormals
kept, the three products summed in fp32 per 32-column K-tile -- passes it for the plain GEMM, the epilogue, the mean-fused GEMM and
the Winograd path; each plausible kernel bug exceeds it by at least 10x: a subnormal lo flushed to zero, the hi.lo or the lo.hi
product dropped on a tile, a K-tile dropped (the last one and one in the middle), a split residual unsplit with twice the inverse
scale, a ROI straddling two M-tiles losing one partial sum of its mean, a wrong output tap of the F(3,3) segment (row / column 6).

The first two bugs only touch rows far below the tensor's maximum: the normwise check of tests/test_gpu_split_gemm.py
(_rel <= 3e-6) accepts them on the magnitude-ladder input, which is the gap this gate closes.  Most cases use inputs whose rounding
residuals share one sign (_lo_heavy); the last test repeats the lo / cross-product bugs on the natural ladder inputs of the GPU file
(no constructed residuals), where the gate still rejects them by >= 10x (12-63x)."""
import math

import pytest
import torch

import split_ref as sr

MARGIN = 10.0
SA, K = 16.0, 160                       # the activations' operand scale; K = 5 K-tiles of 32 (an odd multiple of 32)
LADDER = (1.0, 2.0 ** -6, 2.0 ** -12, 2.0 ** -18, 2.0 ** -26, 0.0)


def _rel(y, ref):
    return float((y.double() - ref).abs().max() / ref.abs().max())


def _lo_heavy(t, s):
    """t (>= 0) moved onto values whose split has lo = hi * 2^-13 exactly (hi = fp16(s t)): the rounding residuals of all elements
    share one sign, so a lost lo half is not averaged away."""
    hi = (t * s).half().float()
    return (hi * (1 + 2.0 ** -13) / s).float()


def _ladder(M=256, N=96, seed=0):
    """x [M,K] >= 0 (post-ReLU, heavy-tailed): rows 0..127 (the first M-tile) at magnitude ~1, rows 128.. cycle through the ladder
    2^-6 .. 2^-26 and all-zero rows; w [N,K] >= 0 with rows from 1 down to 2^-12."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).relu() * torch.rand(M, K, generator=g).pow(-0.5).clamp_max(8.0)
    mag = torch.tensor([1.0 if m < 128 else LADDER[1 + (m - 128) % (len(LADDER) - 1)] for m in range(M)])
    x = _lo_heavy(x * mag[:, None], SA)
    w = torch.rand(N, K, generator=g) * 0.05 * (2.0 ** -torch.linspace(0, 12, N)).view(-1, 1)
    sw = 2.0 ** (12 - math.floor(math.log2(float(w.abs().max()))))
    w = _lo_heavy(w, sw)
    return x, w, sw


def test_split_emulation_passes_the_plain_gemm_and_the_epilogue():
    x, w, sw = _ladder()
    assert torch.all(x[128:][4::5] == 0) and float(x[128:][3::5].max()) < 2.0 ** -20
    for epi in ({}, {"scale": True, "shift": True, "residual": True, "relu": True}):
        g = torch.Generator().manual_seed(1)
        N = w.shape[0]
        sc = torch.rand(N, generator=g) + 0.5 if epi else None
        sh = torch.randn(N, generator=g) * 1e-3 if epi else None
        res = torch.randn(x.shape[0], N, generator=g) * 1e-3 if epi else None
        r = sr.epilogue(sr.gemm(x, w, (SA, sw)), sc, sh, res, bool(epi))
        acc = sr.emulate_split_gemm(x, w, SA, sw)
        got = acc if not epi else torch.relu(acc * sc + sh + res)
        assert sr.gate_ratio(got, r) <= 1.0
    # the f32 MFMA (fp32 accumulation of the fp32 operands) passes its own gate
    assert sr.gate_ratio(x @ w.t(), sr.gemm(x, w)) <= 1.0


def test_a_flushed_subnormal_lo_is_rejected_and_invisible_to_the_normwise_check():
    x, w, sw = _ladder()
    ref = sr.gemm(x, w, (SA, sw))
    bad = sr.emulate_split_gemm(x, w, SA, sw, flush_lo=True)
    q = sr.gate_ratio(bad, ref)
    print(f"SPLITGATE-CPU flush_lo ratio {q:.1f} normwise {_rel(bad, ref.ref):.2e}")
    assert q >= MARGIN
    assert _rel(bad, ref.ref) <= 3e-6                       # the normwise check of test_gpu_split_gemm.py accepts it


@pytest.mark.parametrize("kept", [("hh", "lh"), ("hh", "hl")], ids=["hi.lo-dropped", "lo.hi-dropped"])
def test_a_cross_product_dropped_on_the_small_row_tile_is_rejected(kept):
    """The product dropped on the second M-tile (rows 128..255: the ladder rows below the tensor's max)."""
    x, w, sw = _ladder()
    ref = sr.gemm(x, w, (SA, sw))
    bad = sr.emulate_split_gemm(x, w, SA, sw)
    bad[128:] = sr.emulate_split_gemm(x[128:], w, SA, sw, products=kept)
    q = sr.gate_ratio(bad, ref)
    print(f"SPLITGATE-CPU {kept} ratio {q:.1f} normwise {_rel(bad, ref.ref):.2e}")
    assert q >= MARGIN
    assert _rel(bad, ref.ref) <= 3e-6                       # invisible to the normwise check


@pytest.mark.parametrize("tile", [4, 2], ids=["last-k-tile", "middle-k-tile"])
def test_a_dropped_k_tile_is_rejected(tile):
    x, w, sw = _ladder()
    ref = sr.gemm(x, w, (SA, sw))
    assert sr.gate_ratio(sr.emulate_split_gemm(x, w, SA, sw, skip_tile=tile), ref) >= MARGIN


def test_a_split_residual_unsplit_with_twice_the_inverse_scale_is_rejected():
    x, w, sw = _ladder()
    g = torch.Generator().manual_seed(2)
    res = torch.randn(x.shape[0], w.shape[0], generator=g) * x.abs().amax(1, keepdim=True) * 1e-2
    hi, lo = sr.split_halves(res, SA)
    held = (hi.float() + lo.float()) / SA                  # what the split residual holds
    r = sr.epilogue(sr.gemm(x, w, (SA, sw)), residual=held, relu=True)
    acc = sr.emulate_split_gemm(x, w, SA, sw)
    assert sr.gate_ratio(torch.relu(acc + held), r) <= 1.0
    bad = torch.relu(acc + (hi.float() + lo.float()) * (2.0 / SA))
    assert sr.gate_ratio(bad, r) >= MARGIN


def test_mean_fused_gemm_and_a_lost_partial_sum():
    """seg = 49 ROI-major rows per ROI; ROI 2 (rows 98..146) straddles the 128-row M-tiles: losing the partial of rows 128..146
    is rejected; the fp32 mean of the emulated rows passes."""
    x, w, sw = _ladder(M=49 * 6)
    g = torch.Generator().manual_seed(3)
    N = w.shape[0]
    sh = torch.randn(N, generator=g) * 1e-3
    res = torch.randn(x.shape[0], N, generator=g) * 1e-3
    r = sr.segmean(sr.epilogue(sr.gemm(x, w, (SA, sw)), shift=sh, residual=res, relu=True), 49)
    y = torch.relu(sr.emulate_split_gemm(x, w, SA, sw) + sh + res)
    good = torch.stack([y[q * 49:(q + 1) * 49].sum(0) / 49 for q in range(6)])
    assert sr.gate_ratio(good, r) <= 1.0
    bad = good.clone()
    bad[2] = y[98:128].sum(0) / 49
    assert sr.gate_ratio(bad, r) >= MARGIN


def _wino_emulation(d, w, out_mats=None):
    """fp32 Winograd convolution: transforms and the 121 GEMMs in fp32 (the f32 MFMA form).  out_mats: the (left, right) output
    transforms, A^T twice unless a bug replaces one."""
    BT, G, AT = sr.wino_mats()
    L, Rm = out_mats or (AT, AT)
    V = torch.einsum("ai,rcij,bj->rcab", BT.float(), d.float(), BT.float())
    Ut = torch.einsum("ai,ncij,bj->ncab", G.float(), w.float(), G.float())
    M = torch.einsum("rcab,ncab->rnab", V, Ut)
    return torch.einsum("ya,rnab,xb->rnyx", L.float(), M, Rm.float())


def _wino_split_emulation(d, w, sv):
    BT, G, AT = sr.wino_mats()
    V = torch.einsum("ai,rcij,bj->rcab", BT.float(), d.float(), BT.float())
    Ut = torch.einsum("ai,ncij,bj->ncab", G.float(), w.float(), G.float())
    su = 2.0 ** (12 - math.floor(math.log2(float(Ut.abs().max()))))
    R, C, N = d.shape[0], d.shape[1], w.shape[0]
    Vm = V.permute(2, 3, 0, 1).reshape(121, R, C)
    Um = Ut.permute(2, 3, 0, 1).reshape(121, N, C)
    M = torch.stack([sr.emulate_split_gemm(Vm[i], Um[i], sv, su) for i in range(121)]).view(11, 11, R, N).permute(2, 3, 0, 1)
    return torch.einsum("ya,rnab,xb->rnyx", AT.float(), M, AT.float()), su


def test_winograd_emulation_passes_and_a_wrong_f33_tap_is_rejected():
    g = torch.Generator().manual_seed(4)
    R, C, N = 6, 64, 24
    d = torch.randn(R, C, 7, 7, generator=g).relu() * torch.tensor([1.0, 2.0 ** -6, 2.0 ** -12, 2.0 ** -18, 2.0 ** -26, 0.0]).view(-1, 1, 1, 1)
    w = torch.randn(N, C, 3, 3, generator=g) * 0.05
    _, _, AT = sr.wino_mats()
    assert sr.gate_ratio(_wino_emulation(d, w), sr.wino_conv(d, w)) <= 1.0
    ys, su = _wino_split_emulation(d, w, 0.25)
    rs = sr.wino_conv(d, w, (0.25, su))
    assert sr.gate_ratio(ys, rs) <= 1.0
    # output row 6 (the last output of the F(3,3) segment) with its point-at-infinity term lost; column 6 likewise
    bad_at = AT.clone()
    bad_at[6, 10] = 0
    ref = sr.wino_conv(d, w)
    for axis in ("row", "col"):
        q = sr.gate_ratio(_wino_emulation(d, w, (bad_at, AT) if axis == "row" else (AT, bad_at)), ref)
        assert q >= MARGIN, (axis, q)


@pytest.mark.parametrize("K_", [160, 256])
def test_the_gate_also_bites_on_the_gpu_tests_natural_ladder(K_):
    """The inputs of test_gpu_split_f64.py's split cases -- heavy-tailed post-ReLU rows cycling through the ladder, signed weights
    from 1 down to 2^-12, no constructed rounding residuals: the emulation passes, a flushed subnormal lo and a dropped cross
    product are still rejected by >= 10x."""
    g = torch.Generator().manual_seed(K_)
    M, N = 1037, 388
    x = torch.randn(M, K_, generator=g).relu() * torch.rand(M, K_, generator=g).pow(-0.5).clamp_max(8.0)
    x = x * torch.tensor([LADDER[m % len(LADDER)] for m in range(M)])[:, None]
    w = torch.randn(N, K_, generator=g) * 0.05 * (2.0 ** -torch.linspace(0, 12, N)).view(-1, 1)
    sw = 2.0 ** (12 - math.floor(math.log2(float(w.abs().max()))))
    ref = sr.gemm(x, w, (SA, sw))
    assert sr.gate_ratio(sr.emulate_split_gemm(x, w, SA, sw), ref) <= 1.0
    for bug, kw in (("flush_lo", {"flush_lo": True}), ("hi.lo-dropped", {"products": ("hh", "lh")}),
                    ("lo.hi-dropped", {"products": ("hh", "hl")})):
        q = sr.gate_ratio(sr.emulate_split_gemm(x, w, SA, sw, **kw), ref)
        print(f"SPLITGATE-CPU natural K{K_} {bug} ratio {q:.1f}")
        assert q >= MARGIN, (bug, q)
