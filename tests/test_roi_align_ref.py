"""The float64 ROIAlign reference (tests/roi_align_ref.py) against the fp32 CPU oracle (oracle/roi_ops_ref.c), its adjoint
identity, and -- per case of tests/test_gpu_roi_align_bwd.py -- the oracle's own distance from the reference: the yardstick
for that file's gate.  No GPU.

Oracle distance, max abs error / max(|reference|.max(), 1), worst case per group (the gate of the GPU tests is 1e-5):
  ownership cases 2.1e-6 (sampling_ratio 3 and 2 on the 5 x 3 map: every contribution is divided by the count on its own),
  list edges 2.0e-6 (R = 2100: ~2100 fp32 additions per pixel), footprint margin 3.4e-7, scatter cases 6.4e-7,
  accumulation 5.6e-7, strided rows 1.9e-7, NCHW 8.7e-7 (huge grids 2.8e-7).
Every case is inside 1e-5 by a factor of 4.7 or more, so no case of the GPU file has a gate of its own.

The same for the forward cases of tests/test_gpu_roi_align_fwd.py (tests/roi_align_fwd_cases.py; those without a bf16 map or an
affine, which the oracle does not have): worst oracle distance per group
  pooler settings 1.6e-7, table form 1.3e-7, on the fly 1.0e-7, channel slices 1.3e-7, option maps 9.7e-8, pooler contract 1.5e-7.
A forward case whose oracle distance is within a factor 3 of the gate has the wrong inputs for that gate and fails here.
"""
import numpy as np
import pytest

import roi_align_bwd_cases as cases
import roi_align_fwd_cases as fwd_cases
import roi_align_ref as ref


def _boxes(H, W, scale):
    s = 1.0 / scale
    return np.array([
        [0, 1.5 * s, 2.0 * s, 6.2 * s, 7.7 * s],
        [1, -3.0 * s, -2.0 * s, 4.0 * s, 3.5 * s],                 # partly outside
        [0, 4.0 * s, 4.0 * s, 4.0 * s, 4.0 * s],                   # empty
        [1, 9.0 * s, 2.0 * s, 3.0 * s, 8.0 * s],                   # inverted on x
        [0, 2.0 * s, 9.0 * s, 8.0 * s, 1.0 * s],                   # inverted on y
        [1, -2.0 * s, -2.0 * s, (W + 3.0) * s, (H + 2.0) * s],     # larger than the map
        [0, 5.1 * s, 0.2 * s, 5.4 * s, (H - 0.5) * s],             # narrower than a pixel
        [1, 0.4 * W * s, 0.3 * H * s, W * s, H * s],               # flush against the far edges
        [0, (W - 0.7) * s, (H - 0.2) * s, (W + 5.0) * s, (H + 4.0) * s],   # starts on the last pixel, leaves the map
    ], np.float32)


@pytest.mark.parametrize("P", [7, 13, 14])
@pytest.mark.parametrize("sr", [0, 2, 3])
@pytest.mark.parametrize("aligned", [True, False])
def test_reference_matches_the_oracle(oracle, aligned, sr, P):
    """Forward and backward, every bin and the even bins only, within 1e-5 of the largest entry of the fp32 oracle's result."""
    rng = np.random.default_rng(P * 10 + sr)
    N, C, H, W, scale = 2, 5, 11, 14, 1 / 16
    rois = _boxes(H, W, scale)
    feat = rng.standard_normal((N, H, W, C)).astype(np.float32)
    want_f = oracle.roi_align(feat.transpose(0, 3, 1, 2), rois, (P, P), scale, sr, aligned).transpose(0, 2, 3, 1)     # [R,P,P,C]
    for stride in (1, 2):
        got = ref.roi_align_fwd_f64(feat, rois, P, scale, sr, aligned, stride)
        want = want_f[:, ::stride, ::stride]
        assert got.shape == want.shape and np.abs(want).max() > 0
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
        g = rng.standard_normal(got.shape).astype(np.float32)
        full = np.zeros((len(rois), C, P, P), np.float32)
        full[:, :, ::stride, ::stride] = g.transpose(0, 3, 1, 2)
        want_b = oracle.roi_align_backward(full, (N, C, H, W), rois, scale, sr, aligned).transpose(0, 2, 3, 1)
        got_b = ref.roi_align_bwd_f64(g, (N, H, W, C), rois, P, scale, sr, aligned, stride)
        assert np.abs(want_b).max() > 0
        assert np.abs(got_b - want_b).max() <= 1e-5 * np.abs(want_b).max()


@pytest.mark.parametrize("P,stride,sr,aligned", [(14, 2, 0, True), (13, 2, 2, False), (7, 1, 3, True), (14, 1, 0, False), (1, 1, 0, True)])
def test_reference_adjoint_identity(P, stride, sr, aligned):
    """<fwd(F), G> == <F, bwd(G)> in float64, incl. a roi whose image index is out of range (zeros forward, nothing backward).
    The two sides agree to 1e-12 of ||fwd(F)|| ||G||, the scale of the sum's terms (Cauchy-Schwarz), and -- the inner product of these
    seeded inputs does not cancel -- to 1e-12 of the inner product itself as well."""
    rng = np.random.default_rng(P + sr)
    N, C, H, W, scale = 2, 3, 11, 14, 1 / 16
    rois = np.concatenate([_boxes(H, W, scale), [[7, 10.0, 10.0, 90.0, 90.0]]]).astype(np.float32)
    feat = rng.standard_normal((N, H, W, C))
    y = ref.roi_align_fwd_f64(feat, rois, P, scale, sr, aligned, stride)
    assert not y[-1].any()
    g = rng.standard_normal(y.shape)
    gf = ref.roi_align_bwd_f64(g, (N, H, W, C), rois, P, scale, sr, aligned, stride)
    lhs, rhs = float((y * g).sum()), float((feat * gf).sum())
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(y) * np.linalg.norm(g)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


def test_axis_weights_analytic():
    """Rows hold one unit of weight per sample inside [-1, extent], samples past either end none; the clamps put the weight
    of a sample in [-1, 0] on pixel 0 and of one in [extent - 1, extent] on the last pixel; the unaligned size clamp."""
    # aligned, scale 1: box [0.5, 4.5] -> start 0, bins of 2 with 2 samples at .5, 1.5, 2.5, 3.5
    w = ref.axis_weights(0.5, 4.5, 2, [0, 1], 0, True, 1.0, 6)
    np.testing.assert_allclose(w, [[0.5, 1.0, 0.5, 0, 0, 0], [0, 0, 0.5, 1.0, 0.5, 0]], atol=0, rtol=0)
    # samples at -1.5 (outside), -0.5 (clamped to pixel 0), 5.5 (clamped to the last pixel), 6.5 (outside)
    w = ref.axis_weights(-1.5, 7.5, 9, [0, 1, 7, 8], 1, True, 1.0, 6)
    np.testing.assert_allclose(w, [[0] * 6, [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], [0] * 6], atol=0, rtol=0)
    # not aligned: an empty box is one pixel wide; aligned: it has no samples at all
    assert ref.axis_weights(2.25, 2.25, 1, [0], 0, False, 1.0, 6).sum() == 1.0
    assert not ref.axis_weights(2.25, 2.25, 1, [0], 0, True, 1.0, 6).any()
    # an inverted box under a fixed sampling ratio samples backwards from its start; with the adaptive grid it has no samples
    w = ref.axis_weights(4.5, 2.5, 1, [0], 2, True, 1.0, 6)              # start 4, bin -2: samples at 3.5 and 2.5
    np.testing.assert_allclose(w, [[0, 0, 0.5, 1.0, 0.5, 0]], atol=0, rtol=0)
    assert not ref.axis_weights(4.5, 2.5, 1, [0], 0, True, 1.0, 6).any()
    gh, gw = ref.grid_sizes(np.array([[0, 4.5, 0.5, 2.5, 4.5]], np.float32), 2, 1.0, 0, True)
    assert (int(gh[0]), int(gw[0])) == (2, -1)


_ALL = cases.all_nhwc_cases() + cases.nchw_cases()


@pytest.mark.parametrize("case", _ALL, ids=[c["name"] for c in _ALL])
def test_oracle_distance_per_gpu_case(oracle, case):
    """Per case of the GPU file: the conditions that keep it from passing for the wrong reason, and the fp32 oracle's distance
    from the float64 reference on the case's inputs (its first 16 channels) -- printed, and asserted inside the GPU file's gate
    of 1e-5: were it not, the kernel could not be held to 1e-5 on that case either and the case would need 4 x this distance."""
    want = cases.check_conditions(case)
    got = cases.oracle_backward(oracle, case)
    ratio = cases.error_ratio(got, want[..., :got.shape[-1]])
    print(f"oracle distance {case['name']}: {ratio:.2e}")
    assert ratio <= 1e-5


_FWD = fwd_cases.plain_cases()


@pytest.mark.parametrize("case", _FWD, ids=[c["name"] for c in _FWD])
def test_oracle_distance_per_forward_gpu_case(oracle, case):
    """Per plain case of the forward GPU file: check_conditions (every marked proposal has the grid, taps or plan that select its
    branch; plan() runs on every proposal of a contract case), and the fp32 oracle's distance from reference(case) on the first 16
    channels, out-of-range rows dropped -- printed, and asserted a factor 3 inside the GPU file's gate."""
    want = fwd_cases.check_conditions(case)
    if case["entry"] == "contract":
        plans = [fwd_cases.plan(case, r) for r in range(len(case["rois"]))]
        assert all(p["fast"] == (p["why"] is None) for p in plans)
        if max(fwd_cases.pooled(case)) <= fwd_cases.K_TL_BINS:
            assert any(p["fast"] for p in plans), "no proposal of this case takes the staged form"
    got, keep = fwd_cases.oracle_forward(oracle, case)
    ratio = fwd_cases.error_ratio(got, want[keep][..., :got.shape[-1]])
    print(f"oracle distance {case['name']}: {ratio:.2e}")
    assert ratio <= fwd_cases.GATE / 3


def test_forward_case_helpers():
    """The restated slice rule, the bf16 rounding, and that every variant of the GPU file passes its conditions."""
    assert [fwd_cases.fwd_slices(C) for C in (8, 36, 508, 512, 516, 1024, 1028, 2048, 4096)] == \
        [(1, 2), (1, 9), (1, 127), (2, 64), (2, 65), (4, 64), (4, 65), (8, 64), (8, 128)]
    x = np.array([1.0, 1.00390625, 1.01171875, -3.1415927, 1e-30, 65504.0], np.float32)
    import torch
    assert np.array_equal(fwd_cases.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    names = [c["name"] for c in fwd_cases.all_cases()]
    assert len(set(names)) == len(names)
    for case in fwd_cases.affine_cases() + fwd_cases.sliced_affine_cases() + fwd_cases.misc_cases() + [c for c, _ in fwd_cases.dtype_cases()]:
        fwd_cases.check_conditions(case)
