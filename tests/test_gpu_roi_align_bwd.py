"""The ROIAlign backward kernels outside the one default pooler configuration, against a float64 reference of the operation
(tests/roi_align_ref.py) on the whole output, all channels.  The inputs live in tests/roi_align_bwd_cases.py:

  channels-last entry (locov_roi_align_nhwc_bwd, locov_amd/csrc/roi_align_nhwc_bwd.hip)
    ownership kernel  (P, bin_stride) x aligned x sampling_ratio x scale pairwise, maps inside one tile / exactly one tile / one pixel
                      into the next tile / several tiles, C = 128 and 256, gradient rows that are a column block of a wider matrix,
                      R = 1 / 257 / 2100 (a second pass of the 2048-entry list), boxes with an edge within 2.5 px of a tile boundary,
                      accumulation into an existing gradient; every case also through the scatter kernel (LOCOV_POOL_BWD_TILES=0)
    scatter kernel    every reason the dispatcher leaves the ownership form (C % 128, position-major rows, grids of 14, 4, 2, 1 rows),
                      ragged channel slices, the LDS gradient window and the direct scatter in one launch, the four-tap branch from
                      LDS tables (grid > 16; under a fixed sampling ratio the large boxes whose bins keep two samples 11 pixels
                      apart, where the separable build bails out -- those that keep one sample per bin scatter separably again),
                      weights computed on the fly (OH * grid > 192); every case also with LOCOV_POOL_BWD_WINDOW=0
  NCHW entry (locov_roi_align_bwd through ops.roi_align under autograd): P x sampling_ratio x aligned x C in {3, 4, 6}, a grid past the
    1024-entry tables, no rois

Every case appends one of each awkward box (partly outside, larger than the map, zero area, x2 < x1, narrower than a map pixel,
flush against the far edges), interleaves the image indices and has two of them out of range.  check_conditions asserts, from the
reference alone, that each roi marked for a branch has the grid size that selects it, that every image with a roi got a gradient,
and that rows without samples contributed exactly nothing.

Gate (the one tests/test_gpu_res5_train.py holds this kernel to against the fp32 oracle): max abs error <= 1e-5 x
max(|reference|.max(), 1).  The fp32 oracle itself is within 2.1e-6 of the reference on every case (tests/test_roi_align_ref.py), so
no case has a gate of its own.  Worst measured ratio max abs error / max(|reference|.max(), 1) per group, MI355X, over two runs (the forms
that add with atomics vary a little from run to run with the order of the additions):
  ownership kernel            1.5e-6 (R = 2100; 3.3e-7 on every other case)
  the same cases, scatter     1.5e-6 (R = 2100; 2.7e-7 on every other case)
  scatter cases, window       2.9e-7
  scatter cases, no window    4.9e-7
  accumulation, strided rows  1.8e-7
  NCHW                        9.4e-7

Found by these cases and fixed with them: the ownership kernel's listing took [start, start + size] for a proposal's footprint, so
an inverted box (x2 < x1) under aligned=True and a fixed sampling ratio -- negative bin size, samples running from the start BACK
-- was listed by no tile its samples reach and its gradient was dropped (tiles-P13s2-aligned-sr2-scale32-map20x30 and
tiles-P13s2-aligned-sr3-scale16-map9x17 were 0.17 and 0.26 of the largest entry off; the scatter kernel was right).
"""
import numpy as np
import pytest
import torch

import roi_align_bwd_cases as cases

pytestmark = pytest.mark.gpu

GATE = 1e-5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grad_rows(case, grad):
    """[R, OH, OW, C] -> the rows the entry reads: ROI-major [R*OH*OW, C] or position-major [OH*OW*R, C]."""
    if case["pos_major"]:
        grad = grad.transpose(1, 2, 0, 3)
    return dev(grad.reshape(-1, case["C"]))


def run_nhwc(ops, case, rows, monkeypatch, tiles=None, window=None, accumulate_into=None):
    for name, value in (("LOCOV_POOL_BWD_TILES", tiles), ("LOCOV_POOL_BWD_WINDOW", window)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    shape = (case["N"], case["H"], case["W"], case["C"])
    out = ops.roi_align_nhwc_bwd(rows, shape, dev(case["rois"]), case["P"], case["scale"], case["sr"], case["aligned"],
                                 bin_stride=case["bin_stride"], pos_major=case["pos_major"], accumulate_into=accumulate_into)
    torch.cuda.synchronize()
    return out


def gate(case, form, got, want):
    ratio = cases.error_ratio(got.cpu().numpy(), want)
    print(f"error ratio {case['name']} [{form}]: {ratio:.2e}")
    assert ratio <= GATE, f"{case['name']} [{form}]: {ratio:.3e} of the largest entry"


_TILES = cases.tiles_cases() + cases.tiles_list_cases() + cases.tiles_margin_cases()
_SCATTER = cases.scatter_cases()
_ACC = cases.accumulate_cases()
_NCHW = cases.nchw_cases()
ids = lambda cs: [c["name"] for c in cs]


@pytest.mark.parametrize("case", _TILES, ids=ids(_TILES))
def test_ownership_form(ops, case, monkeypatch):
    """By default these reach the ownership kernel: the whole map gradient against float64, the same bits on a second run, and the
    same inputs through the scatter kernel."""
    assert cases.dispatches_to_tiles(case)
    grad = cases.gradient(case)
    want = cases.check_conditions(case, grad=grad)
    rows = grad_rows(case, grad)
    got = run_nhwc(ops, case, rows, monkeypatch)
    gate(case, "ownership", got, want)
    assert torch.equal(got, run_nhwc(ops, case, rows, monkeypatch)), "the ownership form must be reproducible bit for bit"
    gate(case, "scatter", run_nhwc(ops, case, rows, monkeypatch, tiles="0"), want)


def test_ownership_form_strided_gradient_rows(ops, monkeypatch):
    """The 128-channel gradient rows as a column block of a 160-wide matrix (grad_ld = 160, the pointer 64 bytes into a row): the
    bits of the contiguous call; the scatter kernel reads the same rows."""
    case = cases.strided_case()
    assert cases.dispatches_to_tiles(case)
    grad = cases.gradient(case)
    want = cases.check_conditions(case, grad=grad)
    rows = grad_rows(case, grad)
    wide = torch.randn(rows.shape[0], 160, generator=torch.Generator().manual_seed(9)).cuda()
    wide[:, 16:144] = rows
    block = wide[:, 16:144]
    assert block.stride(0) == 160 and not block.is_contiguous() and block.data_ptr() % 16 == 0 and ops._rows(block, "g") is block
    got = run_nhwc(ops, case, block, monkeypatch)
    gate(case, "ownership, strided rows", got, want)
    assert torch.equal(got, run_nhwc(ops, case, rows, monkeypatch))
    gate(case, "scatter, strided rows", run_nhwc(ops, case, block, monkeypatch, tiles="0"), want)
    gate(case, "scatter, strided rows, no window", run_nhwc(ops, case, block, monkeypatch, tiles="0", window="0"), want)


@pytest.mark.parametrize("case", _ACC, ids=ids(_ACC))
def test_accumulation_into_an_existing_gradient(ops, case, monkeypatch):
    grad = cases.gradient(case)
    want = cases.check_conditions(case, grad=grad)
    rows = grad_rows(case, grad)
    seed = torch.randn(want.shape, generator=torch.Generator().manual_seed(4))
    total = seed.double().numpy() + want
    forms = [("ownership", None, None), ("scatter", "0", None)] if cases.dispatches_to_tiles(case) else [("window", None, None), ("no window", None, "0")]
    for form, tiles, window in forms:
        got = run_nhwc(ops, case, rows, monkeypatch, tiles=tiles, window=window, accumulate_into=seed.clone().cuda())
        gate(case, form + ", accumulate", got, total)


@pytest.mark.parametrize("case", _SCATTER, ids=ids(_SCATTER))
def test_scatter_form(ops, case, monkeypatch):
    """Cases the dispatcher sends to the scatter kernel, with the default gradient window and without one."""
    assert not cases.dispatches_to_tiles(case)
    grad = cases.gradient(case)
    want = cases.check_conditions(case, grad=grad)
    rows = grad_rows(case, grad)
    gate(case, "window", run_nhwc(ops, case, rows, monkeypatch), want)
    gate(case, "no window", run_nhwc(ops, case, rows, monkeypatch, window="0"), want)


@pytest.mark.parametrize("case", _NCHW, ids=ids(_NCHW))
def test_nchw_backward(ops, case):
    grad = cases.gradient(case)                                      # [R, P, P, C]
    want = cases.check_conditions(case, grad=grad)                   # [N, H, W, C]
    feat = torch.zeros(case["N"], case["C"], case["H"], case["W"], device="cuda", requires_grad=True)
    out = ops.roi_align(feat, dev(case["rois"]), case["P"], case["scale"], case["sr"], case["aligned"])
    out.backward(dev(grad.transpose(0, 3, 1, 2)))
    torch.cuda.synchronize()
    gate(case, "nchw", feat.grad.permute(0, 2, 3, 1), want)


@pytest.mark.parametrize("C", [3, 4])
def test_nchw_backward_without_rois(ops, C):
    feat = torch.randn(2, C, 9, 17, device="cuda", requires_grad=True)
    out = ops.roi_align(feat, torch.zeros(0, 5, device="cuda"), 7, 1 / 16, 2, False)
    assert out.shape == (0, C, 7, 7)
    out.backward(torch.zeros_like(out))
    assert feat.grad is not None and feat.grad.shape == feat.shape and not bool(feat.grad.any())
