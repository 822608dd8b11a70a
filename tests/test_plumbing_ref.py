"""CPU proof for tests/test_gpu_plumbing.py: the references of plumbing_ref.py are pinned to something independent (autograd in
float64), the edge cases are present in the inputs the GPU file uses, and every comparison rejects the bug it exists to catch --
each mutant of a reference is run on those same inputs and reported by name (MUTANT lines with pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plumbing_ref as pr

MARGIN = 10.0


# ------------------------------------------------------------------------------------------------ independent pins
def test_weight_flip_is_the_filter_of_the_data_gradient():
    g = pr.gen(1)
    x = torch.randn(2, 3, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64)
    s = torch.randn(4, generator=g, dtype=torch.float64)
    gy = torch.randn(2, 4, 5, 6, generator=g, dtype=torch.float64)
    (dx,) = torch.autograd.grad(F.conv2d(x, w, padding=1) * s[None, :, None, None], x, gy)
    got = F.conv2d(gy, pr.weight_flip(w, s), padding=1)
    assert float((got - dx).abs().max()) <= 1e-12 * float(dx.abs().max())
    (dx,) = torch.autograd.grad(F.conv2d(x, w, padding=1), x, gy)
    assert float((F.conv2d(gy, pr.weight_flip(w), padding=1) - dx).abs().max()) <= 1e-12 * float(dx.abs().max())


def test_wgrad_unpack_of_the_im2col_product_is_the_weight_gradient():
    g = pr.gen(2)
    R, H, W, C, N = 3, 4, 5, 6, 7
    x = torch.randn(R, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(N, C, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(R, N, H, W, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, padding=1)
    (dw,) = torch.autograd.grad(y, w, gy)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    grows = gy.permute(0, 2, 3, 1).reshape(-1, N)
    got = pr.wgrad_unpack(grows.t() @ pr.im2col(rows, H, W))
    assert float((got - dw).abs().max()) <= 1e-12 * float(dw.abs().max())
    # ... and the packed weight is the operand whose product with the patches is the convolution
    yrows = pr.im2col(rows, H, W) @ pr.pack3x3(w.detach(), torch.float64).t()
    assert float((yrows - y.detach().permute(0, 2, 3, 1).reshape(-1, N)).abs().max()) <= 1e-12 * float(y.detach().abs().max())
    assert torch.equal(pr.wgrad_unpack(pr.pack3x3(w.detach(), torch.float64)), w.detach())


def test_stride2_adjoint_is_the_autograd_adjoint():
    for (N, H, W, C) in ((2, 5, 7, 4), (1, 6, 1, 4), (3, 2, 2, 8)):
        m, r = pr.stride2_inputs(N, H, W, C)
        m = m.double().requires_grad_(True)
        (dm,) = torch.autograd.grad(pr.stride2(m), m, r.double())
        assert torch.equal(dm, pr.stride2_adjoint(r.double(), N, H, W))


def test_mean_bwd_is_the_autograd_of_the_mean_within_one_ulp():
    for hw in pr.MASK_HW:
        g = pr.gen(hw)
        R, C = 5, 8
        x = (torch.rand(R, hw, C, generator=g) + 0.5).requires_grad_(True)
        gp = torch.randn(R, C, generator=g)
        (dx,) = torch.autograd.grad(x.mean(1), x, gp)
        got = pr.mean_bwd(gp, x.detach().view(R * hw, C), hw)
        ulps = (pr.bits(got).to(torch.int64) - pr.bits(dx.reshape(R * hw, C)).to(torch.int64)).abs()
        assert int(ulps.max()) <= 1, hw
        assert pr.bits_equal(pr.mean_bwd(gp, None, hw), got)


def test_the_reciprocal_of_hw_is_unambiguous():
    hw = np.arange(1, 5000)
    assert np.array_equal((1.0 / hw).astype(np.float32), np.float32(1) / hw.astype(np.float32))


def test_sequential_mean_and_rownorm_pins():
    x = torch.randn(6, 49, generator=pr.gen(3))
    s = np.zeros(6, np.float32)
    for k in range(49):
        s = s + x[:, k].numpy()
    assert np.array_equal(pr.mean_rows_sequential(x).numpy(), s / np.float32(49))
    xd = torch.randn(5, 33, generator=pr.gen(4), dtype=torch.float64)
    assert torch.equal(pr.rownorm_chain(xd, pr.NORM_L2, 1e-12), F.normalize(xd, dim=1))
    want = (xd - xd.mean(1, keepdim=True)) / (torch.sqrt(((xd - xd.mean(1, keepdim=True)) ** 2).sum(1, keepdim=True) / 32) + 1e-12)
    assert float((pr.rownorm_chain(xd, pr.NORM_STANDARDIZE, 1e-12) - want).abs().max()) < 1e-13


def test_bits_tell_signed_zeros_and_nan_payloads_apart():
    a = torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0])
    assert torch.equal(*a) and not pr.bits_equal(*a)
    n = torch.from_numpy(np.array([0x7FC00000, 0x7FC00001], dtype=np.uint32).view(np.float32).copy())
    assert not pr.bits_equal(n[:1], n[1:]) and pr.bits_equal(n, n.clone())
    with pytest.raises(AssertionError, match="1 of 2 elements differ"):
        pr.assert_bits(*a)
    assert pr.amax_bits(torch.tensor([-3.0, 2.0])) == 0x40400000 and pr.amax_bits(torch.tensor([float("inf"), 0.0])) == 0x7F800000
    assert pr.f32(0x40400000) == 3.0


# ------------------------------------------------------------------------------------------------ the inputs keep their edges
def test_past_the_cap_cases_take_a_partial_second_trip():
    for kernel, case, cap in (("relu_mask", pr.CAP_RELU_N, pr.CAP), ("mean_bwd", pr.CAP_MEAN_BWD, pr.CAP),
                              ("im2col", pr.CAP_IM2COL, pr.CAP), ("stride2_fwd", pr.CAP_STRIDE2_FWD, pr.CAP),
                              ("stride2_adj", pr.CAP_STRIDE2_ADJ, pr.CAP), ("flip", pr.CAP_FLIP, pr.CAP),
                              ("pack", pr.CAP_PACK, pr.PACK_CAP), ("mean_nhwc", pr.CAP_MEAN_NHWC, pr.MEAN_NHWC_CAP)):
        n = pr.work_items(kernel, case)
        assert cap < n < 1.02 * cap, (kernel, n, cap)
    assert pr.work_items("relu_mask", pr.CAP_RELU_N) == 4194563 and pr.work_items("mean_bwd", pr.CAP_MEAN_BWD) == 4201750
    assert pr.work_items("im2col", pr.CAP_IM2COL) == 4225221 and pr.work_items("stride2_fwd", pr.CAP_STRIDE2_FWD) == 4215456
    assert pr.work_items("stride2_adj", pr.CAP_STRIDE2_ADJ) == 4265640 and pr.work_items("flip", pr.CAP_FLIP) == 4198401
    assert pr.work_items("pack", pr.CAP_PACK) == 1052676 and pr.work_items("mean_nhwc", pr.CAP_MEAN_NHWC) == 524800


def test_mask_inputs_hold_the_special_values():
    for hw in pr.MASK_HW:
        act = pr.mask_inputs(3 * hw, 8, pr.gen(hw))
        pr.assert_act_specials(act)
        kept = act.view(-1)[:5] > 0
        assert kept.tolist() == [False, False, False, True, True]
        g = pr.poison_masked(torch.randn(3 * hw, 8, generator=pr.gen(1)), act)
        assert bool(torch.isnan(g).any()) and bool(torch.isinf(g).any()) and bool(torch.isfinite(g[act > 0]).all())
        out = pr.relu_mask(g, act)
        assert bool(torch.isfinite(out).all()) and int((pr.bits(out)[~(act > 0)] != 0).sum()) == 0      # +0.0, never -0.0
        gp, act = pr.mean_bwd_inputs(3, hw, 8, pr.gen(hw))
        pr.assert_act_specials(act)
        out = pr.mean_bwd(gp, act, hw)
        assert bool(torch.isfinite(out).all()) and int((pr.bits(out)[~(act > 0)] != 0).sum()) == 0
    with pytest.raises(AssertionError, match="lost its special values"):
        pr.assert_act_specials(torch.randn(4, 8))
    for where in ("first", "last"):
        t = torch.rand(5, 8, generator=pr.gen(2))
        t.view(-1)[0 if where == "first" else -1] = -7.0
        pr.assert_amax_at(t, where)
        with pytest.raises(AssertionError):
            pr.assert_amax_at(t, "last" if where == "first" else "first")


def test_rownorm_and_bn_inputs_hold_their_special_rows():
    for R, D in pr.ROWNORM_CASES:
        x, _, rows = pr.rownorm_inputs(R, D, pr.gen(R * D))
        pr.assert_rownorm_rows(x, rows)
        assert (R >= 3) == ("zero" in rows) and (R >= 5) == ("constant" in rows)
    assert pr.rownorm_excluded({"zero": 0, "clamped": 1, "above": 2, "constant": 3}, pr.NORM_STANDARDIZE, True) == [0, 3]
    assert pr.rownorm_excluded({"zero": 0, "clamped": 1, "above": 2, "constant": 3}, pr.NORM_STANDARDIZE, False) == [0]
    assert pr.rownorm_excluded({"zero": 0, "clamped": 1, "above": 2, "constant": 3}, pr.NORM_L2, True) == []
    for C in pr.BN_CASES:
        pr.assert_bn_specials(*pr.bn_inputs(C, pr.gen(C)))
    for n in (1, 3, 64):
        pr.assert_scale_specials(pr.special_scale(n, pr.gen(n)))


# ------------------------------------------------------------------------------------------------ mutants
def _report(name, rejected, total):
    print(f"MUTANT {name}: rejected on {rejected} of {total} cases")


def test_mutant_taps_not_flipped_is_rejected():
    def mutant(w, s):
        return (w * s[:, None, None, None]).permute(1, 0, 2, 3).contiguous()
    n = 0
    for case in pr.CONV_W_CASES:
        w, s, _ = pr.conv_w_inputs(*case)
        assert not pr.bits_equal(mutant(w, s), pr.weight_flip(w, s)), case
        n += 1
    _report("taps t instead of 8 - t", n, len(pr.CONV_W_CASES))


def test_mutant_scale_on_the_wrong_axis_is_rejected():
    n = total = 0
    for (N, K) in pr.TRANSPOSE_CASES:
        w, s = pr.transpose_inputs(N, K)
        bad = (w * s[torch.arange(K) % N][None, :]).t().contiguous()
        rejected = not pr.bits_equal(bad, pr.transpose_scale(w, s))
        assert rejected or N == 1, (N, K)                       # one row: one scale, whichever axis indexes it
        n, total = n + rejected, total + 1
    for (N, Cin) in pr.CONV_W_CASES:
        w, s, p = pr.conv_w_inputs(N, Cin)
        sc = s[torch.arange(Cin) % N]
        bad_flip = (w * sc[None, :, None, None]).flip(2, 3).permute(1, 0, 2, 3).contiguous()
        bad_unpack = pr.wgrad_unpack(p) * sc[None, :, None, None]
        for bad, good in ((bad_flip, pr.weight_flip(w, s)), (bad_unpack, pr.wgrad_unpack(p, s))):
            rejected = not pr.bits_equal(bad, good)
            assert rejected or N == 1, (N, Cin)
            n, total = n + rejected, total + 1
    _report("scale indexed by the wrong axis", n, total)


def test_mutant_act_ge_zero_is_rejected():
    n = 0
    for hw in pr.MASK_HW:
        act = pr.mask_inputs(3 * hw, 8, pr.gen(hw))
        g = pr.poison_masked(torch.randn(3 * hw, 8, generator=pr.gen(1)), act)
        assert not pr.bits_equal(torch.where(act >= 0, g, torch.zeros_like(g)), pr.relu_mask(g, act)), hw
        gp, act = pr.mean_bwd_inputs(3, hw, 8, pr.gen(hw))
        v = pr.mean_bwd(gp, None, hw)
        assert not pr.bits_equal(torch.where(act >= 0, v, torch.zeros_like(v)), pr.mean_bwd(gp, act, hw)), hw
        n += 2
    _report("act >= 0 instead of > 0", n, 2 * len(pr.MASK_HW))


def test_mutant_dropped_tile_edge_is_rejected():
    """The last row / column of a 64 x 64 tile left unwritten (zero): every case with a dimension of 64 or more must notice."""
    n = total = 0
    for (N, K) in pr.TRANSPOSE_CASES:
        w, s = pr.transpose_inputs(N, K)
        good = pr.transpose_scale(w, s)
        for axis in (0, 1):
            bad = good.clone()
            bad.index_fill_(axis, torch.arange(good.shape[axis])[63::64], 0.0)
            rejected = not pr.bits_equal(bad, good)
            assert rejected == (good.shape[axis] >= 64), (N, K, axis)
            n, total = n + rejected, total + 1
    for (N, C, HW) in pr.LAYOUT_CASES:
        x = pr.layout_inputs(N, C, HW)
        for dtype in (torch.float32, torch.bfloat16):
            good = pr.to_nhwc(x, dtype).view(N, HW, C)
            for axis in (1, 2):
                bad = good.clone()
                bad.index_fill_(axis, torch.arange(good.shape[axis])[63::64], 0.0)
                rejected = not pr.bits_equal(bad, good)
                assert rejected == (good.shape[axis] >= 64), (N, C, HW, axis)
                n, total = n + rejected, total + 1
    _report("last row or column of a 64-tile dropped", n, total)


def _std_biased(x, mode, eps):
    if mode == pr.NORM_L2:
        return pr.rownorm_chain(x, mode, eps)
    return (x - x.mean(1, keepdim=True)) / (x.std(1, unbiased=False, keepdim=True) + eps)


def _eps_in_sqrt(x, mode, eps):
    if mode == pr.NORM_L2:
        return x / torch.sqrt((x * x).sum(1, keepdim=True) + eps)
    return (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=True, keepdim=True) + eps)


def _rownorm_ratios(mutant, R, D, mode):
    """Worst gate ratio (forward, backward) of a mutant chain evaluated in float64, over the rows the gate covers."""
    x, g, rows = pr.rownorm_inputs(R, D, pr.gen(R * D))
    out = []
    want = pr.rownorm_f64(x, mode, pr.ROWNORM_EPS, g)
    cpu32 = pr.rownorm_f32(x, mode, pr.ROWNORM_EPS, g)
    got = pr._rownorm_with_grad(mutant, x.double(), mode, pr.ROWNORM_EPS, g.double())
    for i, backward in ((0, False), (1, True)):
        ratio = pr.rownorm_gate(got[i], want[i], cpu32[i])
        keep = torch.ones(R, dtype=torch.bool)
        keep[pr.rownorm_excluded(rows, mode, backward)] = False
        assert bool(torch.isfinite(want[i][keep]).all()), "a row outside the exclusions has no float64 value"
        out.append(float(ratio[keep].max()))
    return out


def test_rownorm_gate_passes_the_fp32_chain_and_rejects_its_mutants():
    n_var = n_eps = 0
    for (R, D) in pr.ROWNORM_CASES:
        for mode in (pr.NORM_L2, pr.NORM_STANDARDIZE):
            if D == 1 and mode == pr.NORM_STANDARDIZE:
                continue
            x, g, rows = pr.rownorm_inputs(R, D, pr.gen(R * D))
            want = pr.rownorm_f64(x, mode, pr.ROWNORM_EPS, g)
            cpu32 = pr.rownorm_f32(x, mode, pr.ROWNORM_EPS, g)
            for i, backward in ((0, False), (1, True)):
                keep = torch.ones(R, dtype=torch.bool)
                keep[pr.rownorm_excluded(rows, mode, backward)] = False
                assert float(pr.rownorm_gate(cpu32[i], want[i], cpu32[i])[keep].max()) <= 0.5     # the yardstick itself
            if mode == pr.NORM_STANDARDIZE:
                fwd, bwd = _rownorm_ratios(_std_biased, R, D, mode)
                assert min(fwd, bwd) >= MARGIN, (R, D, fwd, bwd)
                n_var += 1
            if R >= 3:                                           # the rows at the scale of eps are what tells this one apart
                fwd, bwd = _rownorm_ratios(_eps_in_sqrt, R, D, mode)
                assert min(fwd, bwd) >= MARGIN, (R, D, mode, fwd, bwd)
                n_eps += 1
    _report("D instead of D - 1 in the standardise variance", n_var, len(pr.ROWNORM_CASES) - 1)
    _report("eps inside the square root", n_eps, 2 * (len(pr.ROWNORM_CASES) - 1))


def test_mutant_oh_rounded_down_is_rejected():
    n = total = 0
    for (N, H, W, C) in pr.STRIDE2_CASES:
        m, r = pr.stride2_inputs(N, H, W, C)
        OH, OW = H // 2, (W + 1) // 2                            # the mutant's OH
        fwd_bad = m[:, :2 * OH:2, ::2].reshape(-1, C)
        rejected = not pr.bits_equal(fwd_bad, pr.stride2(m))
        assert rejected == (H % 2 == 1), (N, H, W, C)
        n, total = n + rejected, total + 1
        # the adjoint reads rows[((n*OH + y/2)*OW + x/2)] with that OH
        y, x, img = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :], torch.arange(N)[:, None, None]
        src = ((img * OH + y // 2) * OW + x // 2).clamp_max(r.shape[0] - 1)
        adj_bad = torch.where(((y % 2 == 0) & (x % 2 == 0))[..., None], r[src], torch.zeros(()))
        rejected = not pr.bits_equal(adj_bad, pr.stride2_adjoint(r, N, H, W))
        assert rejected == (H % 2 == 1 and N * H * W > 1), (N, H, W, C)
        n, total = n + rejected, total + 1
    _report("OH = H // 2", n, total)


def test_mutant_im2col_reading_the_neighbouring_roi_is_rejected():
    n = 0
    for (R, H, W, C) in pr.IM2COL_CASES:
        rows = pr.im2col_inputs(R, H, W, C)
        bad = pr.im2col(rows, R * H, W)                          # no border between the ROIs: one tall tile
        rejected = not pr.bits_equal(bad, pr.im2col(rows, H, W))
        assert rejected == (R > 1), (R, H, W, C)
        n += rejected
    _report("the neighbouring ROI's pixel read across an im2col border", n, len(pr.IM2COL_CASES))


def test_wave_mean_and_bn_bounds_pass_fp32_and_reject_a_dropped_element():
    for hw in pr.WAVE_HW:
        x = torch.randn(300, hw, generator=pr.gen(hw)) + 0.5
        ref = pr.mean_f64(x)
        bound = pr.wave_mean_bound(x, ref)
        assert float(((x.mean(-1).double() - ref).abs() / bound).max()) <= 1.0
        dropped = x[:, :-1].double().sum(-1) / hw                # the last element of the row never added
        assert float(((dropped - ref).abs() / bound).median()) >= MARGIN
    for C in pr.BN_CASES:
        w, b, m, v = pr.bn_inputs(C, pr.gen(C))
        eps = np.float32(1e-5)
        sr, hr = pr.bn_fold_f64(w, b, m, v, eps)
        sb, hb = pr.bn_fold_bounds(b, m, sr)
        s32 = w * (1.0 / torch.sqrt(v + torch.tensor(eps)))
        h32 = b - m * s32
        assert float(((s32.double() - sr).abs() / sb).max()) <= 1.0 and float(((h32.double() - hr).abs() / hb).max()) <= 1.0
        s_bad = w.double() / torch.sqrt(v.double()).clamp_min(1e-30)            # eps left out
        assert float(((s_bad - sr).abs() / sb).max()) >= MARGIN
