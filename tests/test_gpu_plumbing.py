"""The small HBM-bound kernels that move, select and rescale data around the heavy ones, each against tests/plumbing_ref.py:
csrc/res5_bwd.hip (weight_transpose_scale, conv3x3_weight_flip, im2col3x3, conv3x3_wgrad_unpack, relu_mask, spatial_mean_bwd,
rows_stride2), the transpose of csrc/roi_align_nhwc.hip in both roles, the three spatial_mean kernels and rownorm of
csrc/head.hip, pack_conv3x3_weight and frozen_bn_fold of csrc/gemm_nt.hip.

Copies, selects and single fp32 multiplies are held to BIT equality (int patterns: -0.0 is not +0.0) at the tile and border
edges, and once per kernel past the grid cap, where every thread takes a second, partial grid-stride trip.  The operand-scale
slots (amax_out=) are read back word by word.  The short reductions are toleranced with bounds that follow from their operation
order; each prints its worst err / bound (PLUMBING lines with pytest -s).  tests/test_plumbing_ref.py shows on the CPU that the
references are right and that these comparisons reject the bugs they exist for, on these inputs."""
import math

import numpy as np
import pytest
import torch

import plumbing_ref as pr

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (run with -m 'not gpu' on CPU-only hosts)")
    from locov_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dgen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _specials_over(t):
    """t with the bf16 rounding edge values of tests/test_gpu_bf16.py over its first elements."""
    from test_gpu_bf16 import _special_fp32_bits, _to_f32
    sp = _to_f32(_special_fp32_bits())
    t = t.clone()
    n = min(sp.numel(), t.numel())
    t.view(-1)[:n] = sp[:n]
    return t


# ------------------------------------------------------------------------------------------------ tile and border edges
@pytest.mark.parametrize("N,K", pr.TRANSPOSE_CASES)
def test_weight_transpose_scale_at_tile_edges(ops, N, K):
    """(63,65) .. (130,129): ragged tiles on both axes and tiles with k0 > 0 / n0 > 0 on their own; (2048,512): the Res5 size."""
    w, s = pr.transpose_inputs(N, K)
    pr.assert_scale_specials(s)
    pr.assert_bits(ops.weight_transpose_scale(w.cuda(), s.cuda()).cpu(), pr.transpose_scale(w, s), "scaled")
    pr.assert_bits(ops.weight_transpose_scale(w.cuda()).cpu(), pr.transpose_scale(w), "plain")


@pytest.mark.parametrize("N,C,HW", pr.LAYOUT_CASES)
def test_layout_transposes_at_tile_edges(ops, N, C, HW):
    """nchw_to_nhwc with fp32 and bf16 stores (torch's rounding, bit for bit, on the rounding edge values) and the same kernel
    with the roles swapped (nhwc_to_nchw)."""
    x = pr.layout_inputs(N, C, HW)
    H, W = x.shape[2:]
    pr.assert_bits(ops.nchw_to_nhwc(x.cuda()).cpu(), pr.to_nhwc(x), "nhwc fp32")
    pr.assert_bits(ops.nchw_to_nhwc(x.cuda(), dtype=BF16).cpu(), pr.to_nhwc(x).to(BF16), "nhwc bf16 == x.to(bfloat16)")
    y = pr.to_nhwc(x)
    assert tuple(y.shape) == (N, H, W, C)
    pr.assert_bits(ops.nhwc_to_nchw(y.cuda()).cpu(), pr.to_nchw(y), "nchw")
    pr.assert_bits(pr.to_nchw(y), x, "round trip of the reference")


@pytest.mark.parametrize("N,Cin", pr.CONV_W_CASES)
def test_conv3x3_weight_layouts(ops, N, Cin):
    w, s, p = pr.conv_w_inputs(N, Cin)
    pr.assert_scale_specials(s)
    pr.assert_bits(ops.conv3x3_weight_flip(w.cuda(), s.cuda()).cpu(), pr.weight_flip(w, s), "flip scaled")
    pr.assert_bits(ops.conv3x3_weight_flip(w.cuda()).cpu(), pr.weight_flip(w), "flip")
    pr.assert_bits(ops.conv3x3_wgrad_unpack(p.cuda(), s.cuda()).cpu(), pr.wgrad_unpack(p, s), "unpack scaled")
    pr.assert_bits(ops.conv3x3_wgrad_unpack(p.cuda()).cpu(), pr.wgrad_unpack(p), "unpack")
    ws = _specials_over(w)
    pr.assert_bits(ops.pack_conv3x3_weight(ws.cuda()).cpu(), pr.pack3x3(ws), "pack fp32")
    pr.assert_bits(ops.pack_conv3x3_weight(ws.cuda(), dtype=BF16).cpu(), pr.pack3x3(ws, BF16), "pack bf16")


@pytest.mark.parametrize("R,H,W,C", pr.IM2COL_CASES)
def test_im2col3x3_at_the_borders(ops, R, H, W, C):
    """One-pixel, one-row and one-column tiles (every tap but the centre is padding somewhere), and tiles whose neighbours in
    memory belong to another ROI."""
    rows = pr.im2col_inputs(R, H, W, C)
    pr.assert_bits(ops.im2col3x3(rows.cuda(), H, W).cpu(), pr.im2col(rows, H, W))


@pytest.mark.parametrize("N,H,W,C", pr.STRIDE2_CASES)
def test_rows_stride2_both_directions(ops, N, H, W, C):
    m, r = pr.stride2_inputs(N, H, W, C)
    pr.assert_bits(ops.rows_stride2(m.cuda(), N, H, W, True).cpu(), pr.stride2(m), "forward")
    back = ops.rows_stride2(r.cuda(), N, H, W, False).cpu()
    pr.assert_bits(back, pr.stride2_adjoint(r, N, H, W), "adjoint")
    odd = torch.ones(H, W, dtype=torch.bool)
    odd[::2, ::2] = False
    assert int((pr.bits(back)[:, odd] != 0).sum()) == 0, "the odd pixels of the adjoint must be exact +0.0"


@pytest.mark.parametrize("hw", pr.MASK_HW)
def test_relu_mask_and_mean_bwd_on_special_values(ops, hw):
    """act holds +0.0, -0.0, NaN (masked) and a positive subnormal and +inf (kept); the gradient under every masked position is
    NaN or inf and must come out +0.0.  spatial_mean_bwd also without a mask."""
    R, C = 3, 8
    act = pr.mask_inputs(R * hw, C, pr.gen(hw))
    pr.assert_act_specials(act)
    g = pr.poison_masked(torch.randn(R * hw, C, generator=pr.gen(1)), act)
    got = ops.relu_mask(g.cuda(), act.cuda()).cpu()
    pr.assert_bits(got, pr.relu_mask(g, act), "relu_mask")
    assert int((pr.bits(got)[~(act > 0)] != 0).sum()) == 0 and bool(torch.isfinite(got).all())
    gp, act = pr.mean_bwd_inputs(R, hw, C, pr.gen(hw))
    pr.assert_act_specials(act)
    got = ops.spatial_mean_bwd(gp.cuda(), act.cuda(), hw).cpu()
    pr.assert_bits(got, pr.mean_bwd(gp, act, hw), "spatial_mean_bwd")
    assert int((pr.bits(got)[~(act > 0)] != 0).sum()) == 0 and bool(torch.isfinite(got).all())
    gq = torch.randn(R, C, generator=pr.gen(hw + 100))
    pr.assert_bits(ops.spatial_mean_bwd(gq.cuda(), None, hw).cpu(), pr.mean_bwd(gq, None, hw), "spatial_mean_bwd(act=None)")


# ------------------------------------------------------------------------------------------------ past the grid cap
# Inputs are drawn on the device and the reference is evaluated there by torch: every step of it is a copy, a select or one fp32
# multiply.  The gate is still bit equality.  (relu_mask and spatial_mean_bwd past the cap: with their slots, below.)
def test_im2col3x3_past_the_grid_cap(ops):
    R, H, W, C = pr.CAP_IM2COL
    assert pr.work_items("im2col", pr.CAP_IM2COL) > pr.CAP
    rows = torch.randn(R * H * W, C, device="cuda", generator=dgen(1))
    pr.assert_bits(ops.im2col3x3(rows, H, W), pr.im2col(rows, H, W))


def test_rows_stride2_past_the_grid_cap(ops):
    N, H, W, C = pr.CAP_STRIDE2_FWD
    assert pr.work_items("stride2_fwd", pr.CAP_STRIDE2_FWD) > pr.CAP and pr.work_items("stride2_adj", pr.CAP_STRIDE2_ADJ) > pr.CAP
    m = torch.randn(N, H, W, C, device="cuda", generator=dgen(2))
    pr.assert_bits(ops.rows_stride2(m, N, H, W, True), pr.stride2(m), "forward")
    del m
    torch.cuda.empty_cache()
    N, H, W, C = pr.CAP_STRIDE2_ADJ
    r = torch.randn(N * ((H + 1) // 2) * ((W + 1) // 2), C, device="cuda", generator=dgen(3))
    pr.assert_bits(ops.rows_stride2(r, N, H, W, False), pr.stride2_adjoint(r, N, H, W), "adjoint")


def test_conv3x3_weight_layouts_past_the_grid_cap(ops):
    N, Cin = pr.CAP_FLIP
    assert pr.work_items("flip", pr.CAP_FLIP) > pr.CAP and pr.work_items("pack", pr.CAP_PACK) > pr.PACK_CAP
    w = torch.randn(N, Cin, 3, 3, device="cuda", generator=dgen(4))
    s = pr.special_scale(N, pr.gen(5)).cuda()
    pr.assert_bits(ops.conv3x3_weight_flip(w, s), pr.weight_flip(w, s), "flip")
    p = w.view(N, 9 * Cin)
    pr.assert_bits(ops.conv3x3_wgrad_unpack(p, s), pr.wgrad_unpack(p, s), "unpack")
    N, Cin = pr.CAP_PACK
    w = _specials_over(w.view(-1)[:N * Cin * 9].view(N, Cin, 3, 3))
    pr.assert_bits(ops.pack_conv3x3_weight(w), pr.pack3x3(w), "pack fp32")
    pr.assert_bits(ops.pack_conv3x3_weight(w, dtype=BF16).cpu(), pr.pack3x3(w.cpu(), BF16), "pack bf16")


@pytest.mark.parametrize("code", [1, 2])
def test_channels_last_mean_past_the_grid_cap(ops, code):
    """ROI-major [R,h,w,C] (1) and position-major [h,w,R,C] (2): 524 800 quads on a grid of 524 288 threads."""
    R, C, hw = pr.CAP_MEAN_NHWC
    assert pr.work_items("mean_nhwc", pr.CAP_MEAN_NHWC) > pr.MEAN_NHWC_CAP
    x = torch.randn((R, hw, 1, C) if code == 1 else (hw, 1, R, C), device="cuda", generator=dgen(6))
    xc = x.cpu()
    per_row = xc.view(R, hw, C).permute(0, 2, 1) if code == 1 else xc.view(hw, R, C).permute(1, 2, 0)
    pr.assert_bits(ops.spatial_mean(x, channels_last=code).cpu(), pr.mean_rows_sequential(per_row))


# ------------------------------------------------------------------------------------------------ operand-scale slots
S0, S1, S3 = 0x11111111, 0x22222222, 0x33333333          # sentinels of the words the producers must leave alone


def _words(slot):
    return [int(v) & 0xFFFFFFFF for v in slot.view(torch.int32).cpu().tolist()]


def _set_words(slot, words):
    slot.view(torch.int32).copy_(torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32).copy()))


def _relu_inputs(kind, shape, device):
    """(g, act) with |g| <= 1 but for the one planted maximum."""
    on_dev = device == "cuda"
    g = torch.rand(shape, device=device, generator=dgen(7) if on_dev else pr.gen(7)) * 2 - 1
    act = torch.randn(shape, device=device, generator=dgen(8) if on_dev else pr.gen(8))
    i = 0 if kind == "first" else -1
    g.view(-1)[i] = float("inf") if kind == "inf" else -7.0
    act.view(-1)[i] = 1.0
    if kind == "masked":
        act = -act.abs()
    return g, act


def _mean_bwd_inputs(kind, R, hw, C, device):
    """(g, act): the planted maximum g[r, c] reaches the output at ONE position (the first / the last element), every other
    position of that (r, c) is masked."""
    on_dev = device == "cuda"
    g = torch.rand(R, C, device=device, generator=dgen(9) if on_dev else pr.gen(9)) * 2 - 1
    act = torch.randn(R * hw, C, device=device, generator=dgen(10) if on_dev else pr.gen(10))
    r, c, p = (0, 0, 0) if kind == "first" else (R - 1, C - 1, hw - 1)
    g[r, c] = float("inf") if kind == "inf" else -7.0 * hw
    act[r * hw:(r + 1) * hw, c] = -1.0
    act[r * hw + p, c] = 1.0
    if kind == "masked":
        act = -act.abs()
    return g, act


def _slot_scenarios(ops, make, run, ref, tag):
    """make(kind) -> inputs; run(inputs, slot) -> device result; ref(inputs) -> reference on the inputs' device.
    NaN gradients are out of scope: fmaxf drops a NaN operand, so a NaN that is KEPT never reaches the slot."""
    slot = ops.scale_slot(torch.empty(1, device="cuda"))
    try:
        for where in ("first", "last"):                        # word 2 = max |out| wherever it sits; words 0, 1, 3 untouched
            inp = make(where)
            want = ref(inp)
            pr.assert_amax_at(want, where)
            amax = pr.amax_bits(want)
            _set_words(slot, [S0, S1, 0, S3])
            pr.assert_bits(run(inp, slot).cpu(), want.cpu(), f"{tag} max at the {where} element")
            assert _words(slot) == [S0, S1, amax, S3], (tag, where, [hex(v) for v in _words(slot)], hex(amax))
        larger, smaller = pr.amax_bits(torch.tensor(2.0 * pr.f32(amax))), pr.amax_bits(torch.tensor(0.25 * pr.f32(amax)))
        _set_words(slot, [0, 0, larger, 0])                    # a larger value already there: unchanged
        run(inp, slot)
        assert _words(slot) == [0, 0, larger, 0], tag
        _set_words(slot, [0, 0, smaller, 0])                   # a smaller one: raised
        run(inp, slot)
        assert _words(slot) == [0, 0, amax, 0], tag
        inp = make("masked")                                   # nothing kept: a zeroed slot stays zero
        want = ref(inp)
        assert pr.amax_bits(want) == 0
        _set_words(slot, [0, 0, 0, 0])
        pr.assert_bits(run(inp, slot).cpu(), want.cpu(), f"{tag} all masked")
        assert _words(slot) == [0, 0, 0, 0], tag
        inp = make("inf")                                      # a kept +inf
        want = ref(inp)
        assert pr.amax_bits(want) == 0x7F800000
        pr.assert_bits(run(inp, slot).cpu(), want.cpu(), f"{tag} kept inf")
        assert _words(slot) == [0, 0, 0x7F800000, 0], tag
    finally:
        slot.zero_()


@pytest.mark.parametrize("size", ["small", "past the cap"])
def test_relu_mask_result_and_slot(ops, size):
    """600 elements, and 4 194 563 quads on a grid of 4 194 304 threads: the last 259 quads are second trips."""
    shape, device = ((50, 12), "cpu") if size == "small" else ((pr.CAP_RELU_N,), "cuda")
    assert size == "small" or pr.work_items("relu_mask", pr.CAP_RELU_N) > pr.CAP
    _slot_scenarios(ops, lambda kind: _relu_inputs(kind, shape, device),
                    lambda inp, slot: ops.relu_mask(inp[0].cuda(), inp[1].cuda(), amax_out=slot),
                    lambda inp: pr.relu_mask(*inp), f"relu_mask {size}")


@pytest.mark.parametrize("size", ["small", "past the cap"])
def test_spatial_mean_bwd_result_and_slot(ops, size):
    (R, hw, C), device = ((7, 9, 12), "cpu") if size == "small" else (pr.CAP_MEAN_BWD, "cuda")
    assert size == "small" or pr.work_items("mean_bwd", pr.CAP_MEAN_BWD) > pr.CAP
    _slot_scenarios(ops, lambda kind: _mean_bwd_inputs(kind, R, hw, C, device),
                    lambda inp, slot: ops.spatial_mean_bwd(inp[0].cuda(), inp[1].cuda(), hw, amax_out=slot),
                    lambda inp: pr.mean_bwd(inp[0], inp[1], hw), f"spatial_mean_bwd {size}")
    if size == "small":                                        # ... and without a mask
        slot = ops.scale_slot(torch.empty(1, device="cuda"))
        g = torch.randn(R, C, generator=pr.gen(11))
        want = pr.mean_bwd(g, None, hw)
        pr.assert_bits(ops.spatial_mean_bwd(g.cuda(), None, hw, amax_out=slot).cpu(), want, "act=None with a slot")
        assert _words(slot) == [0, 0, pr.amax_bits(want), 0]
        slot.zero_()


def test_the_scale_a_split_gemm_derives_from_the_slot(ops):
    """The slot relu_mask filled, fed to linear_split_ex(x_scale_dev=): the scale split_scale_of derives puts max |x| in
    [2^12, 2^13), the range guard stays clear and the product is the float64 one."""
    g = pr.gen(12)
    M, K, N = 256, 64, 32
    gr, act = torch.randn(M, K, generator=g) * 3e-3, torch.randn(M, K, generator=g)
    slot = ops.scale_slot(torch.empty(1, device="cuda"))
    x = ops.relu_mask(gr.cuda(), act.cuda(), amax_out=slot)
    want_x = pr.relu_mask(gr, act)
    pr.assert_bits(x.cpu(), want_x)
    assert _words(slot) == [0, 0, pr.amax_bits(want_x), 0]                       # a LAZY slot: consumers derive the scale
    amax = pr.f32(pr.amax_bits(want_x))
    s = 2.0 ** (13 - math.frexp(amax)[1])
    assert 2.0 ** 12 <= s * amax < 2.0 ** 13
    w = ops.split_pack((torch.randn(N, K, generator=g) * 0.1).cuda())
    ops.split_overflow_reset("cuda")
    y = ops.linear_split_ex(x, w, x_scale_dev=slot)
    assert not ops.split_overflow_raised("cuda")
    want = want_x.double() @ ops.split_unpack(w.data, w.scale).double().cpu().t()
    assert float((y.double().cpu() - want).abs().max() / want.abs().max()) < 3e-6
    slot.zero_()


# ------------------------------------------------------------------------------------------------ short reductions
@pytest.mark.parametrize("hw", pr.MEAN_HW)
def test_spatial_mean_rows_kernel_is_the_sequential_sum(ops, hw):
    """256 rows per workgroup staged in LDS: one row, one short of / one past a tile, two tiles and one row; hw = 64 is the last
    size whose tile fits 64 KB.  The channels-last kernels define the same sum."""
    for rows in pr.MEAN_ROWS:
        x = torch.randn(1, rows, hw, 1, generator=pr.gen(rows + hw))
        pr.assert_bits(ops.spatial_mean(x.cuda()).cpu(), pr.mean_rows_sequential(x.view(1, rows, hw)), f"rows={rows}")
    R, C = 5, 12
    x = torch.randn(R, hw, 1, C, generator=pr.gen(hw))
    pr.assert_bits(ops.spatial_mean(x.cuda(), channels_last=1).cpu(), pr.mean_rows_sequential(x.view(R, hw, C).permute(0, 2, 1)), "ROI-major")
    x = torch.randn(hw, 1, R, C, generator=pr.gen(hw + 1))
    pr.assert_bits(ops.spatial_mean(x.cuda(), channels_last=2).cpu(), pr.mean_rows_sequential(x.view(hw, R, C).permute(1, 2, 0)), "position-major")


def test_spatial_mean_of_one_position_is_a_copy(ops):
    x = _specials_over(torch.randn(3, 8, 1, 1, generator=pr.gen(13)))
    pr.assert_bits(ops.spatial_mean(x.cuda()).cpu(), x.view(3, 8))
    pr.assert_bits(ops.spatial_mean(x.view(3, 1, 1, 8).cuda(), channels_last=1).cpu(), x.view(3, 8))
    pr.assert_bits(ops.spatial_mean(x.view(1, 1, 3, 8).cuda(), channels_last=2).cpu(), x.view(3, 8))


@pytest.mark.parametrize("hw", pr.WAVE_HW)
def test_spatial_mean_wave_kernel_vs_float64(ops, hw):
    """hw > 64: one wave per row.  ceil(hw/64) adds per lane, six butterfly levels, one division:
    |err| <= (ceil(hw/64) + 7) 2^-24 sum|x| / hw + 2^-24 |ref| per element."""
    R, C = 3, 43                                               # 129 rows: the last workgroup holds one
    x = torch.randn(R, C, hw, 1, generator=pr.gen(hw)) + 0.25
    ref = pr.mean_f64(x.view(R, C, hw))
    got = ops.spatial_mean(x.cuda()).cpu()
    ratio = float(((got.double() - ref).abs() / pr.wave_mean_bound(x.view(R, C, hw), ref)).max())
    print(f"PLUMBING spatial_mean_wave hw={hw}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("C", pr.BN_CASES)
def test_frozen_bn_fold_vs_float64(ops, C):
    """add, sqrt, reciprocal, multiply: |scale - ref| <= 4 2^-24 |ref|; then multiply, subtract:
    |shift - ref| <= 2^-24 (|bias| + 6 |mean scale|)."""
    w, b, m, v = pr.bn_inputs(C, pr.gen(C))
    pr.assert_bn_specials(w, b, m, v)
    scale, shift = ops.frozen_bn_fold(w.cuda(), b.cuda(), m.cuda(), v.cuda(), eps=1e-5)
    sr, hr = pr.bn_fold_f64(w, b, m, v, np.float32(1e-5))
    sb, hb = pr.bn_fold_bounds(b, m, sr)
    rs, rh = float(((scale.cpu().double() - sr).abs() / sb).max()), float(((shift.cpu().double() - hr).abs() / hb).max())
    print(f"PLUMBING frozen_bn_fold C={C}: worst err / bound scale {rs:.3f} shift {rh:.3f}")
    assert rs <= 1.0 and rh <= 1.0


ROWNORM_PARAMS = [(R, D, mode) for (R, D) in pr.ROWNORM_CASES for mode in (pr.NORM_L2, pr.NORM_STANDARDIZE)
                  if not (D == 1 and mode == pr.NORM_STANDARDIZE)]


@pytest.mark.parametrize("R,D,mode", ROWNORM_PARAMS)
def test_rownorm_forward_and_backward_vs_float64(ops, R, D, mode):
    """Per row, the error against float64 may be at most 2 x the error of the same chain in torch fp32 on the CPU plus
    1e-6 x max |float64| (the factor 2: another summation order at the same precision).  Excluded by construction, never by the
    outcome: standardise of the zero row, and the backward of standardise on the constant row (float64 has no value there); for
    them the documented behaviour is asserted -- finite output, and g / eps on the clamped L2 row."""
    eps = pr.ROWNORM_EPS
    x, g, rows = pr.rownorm_inputs(R, D, pr.gen(R * D))
    pr.assert_rownorm_rows(x, rows)
    want = pr.rownorm_f64(x, mode, eps, g)
    cpu32 = pr.rownorm_f32(x, mode, eps, g)
    xd = x.cuda().requires_grad_(True)
    y = ops.rownorm_autograd(xd, mode, eps)
    y.backward(g.cuda())
    got = (y.detach().cpu(), xd.grad.cpu())
    pr.assert_bits(ops.rownorm(x.cuda(), mode, eps).cpu(), got[0], "forward with and without autograd")
    for i, name in ((0, "forward"), (1, "backward")):
        excluded = pr.rownorm_excluded(rows, mode, backward=bool(i))
        by_construction = [] if mode == pr.NORM_L2 or R < 3 else [0] + ([3] if i and R >= 5 else [])
        assert excluded == by_construction, "nothing else may be excluded"
        keep = torch.ones(R, dtype=torch.bool)
        keep[excluded] = False
        assert bool(torch.isfinite(want[i][keep]).all()), "a row outside the exclusions has no float64 value"
        assert bool(torch.isfinite(got[i]).all()), f"{name}: the kernel documents a finite result on every row"
        ratio = float(pr.rownorm_gate(got[i], want[i], cpu32[i])[keep].max())
        print(f"PLUMBING rownorm mode={mode} {name} ({R},{D}): worst err / bound {ratio:.3f}")
        assert ratio <= 1.0, name
    if mode == pr.NORM_L2 and "clamped" in rows:
        r = rows["clamped"]
        pr.assert_bits(got[1][r], g[r] / torch.tensor(np.float32(eps)), "the clamped row's gradient is g / eps")
