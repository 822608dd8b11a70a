"""Float64 reference of ROIAlign (torchvision semantics) and of its adjoint on a channels-last map: plain numpy, nothing
imported from the package under test.

The GEOMETRY is the contract's (locov_amd/csrc/roi_align_common.h, oracle/roi_ops_ref.c), every step one rounded float32
operation: the box edges `x * scale - 0.5` (aligned) or `x * scale`, the size clamped to 1 when not aligned, the bin size, the
sampling grid `sampling_ratio or ceil(bin)`, the sample positions `start + p * bin + ((i + .5) * bin) / grid`, the [-1, extent]
rule and the clamps at 0 and at the last pixel.  A different rounding there would move a sample across a pixel boundary, which is
a different operation, not an error of the arithmetic.  The WEIGHTS (`v - floor(v)`, `1 - that`), their per-pixel sums, the
products with the data and every sum after them are float64.

The validity of a sample is a product of a y and an x condition and so is its bilinear weight, so the operation is separable: per
roi  out = Wy . F . Wx^T / count  and the adjoint  dF += Wy^T . G . Wx / count,  with Wy [bins, H], Wx [bins, W] from axis_weights.
"""
import numpy as np

_f = np.float32


def _axis_geometry(lo, hi, pooled, sampling_ratio, aligned, scale):
    """(start, bin size, raw grid) of one axis of one box, float32 step by step.  lo / hi: the box's two edges, image pixels."""
    off = _f(0.5) if aligned else _f(0.0)
    start = _f(_f(lo) * _f(scale)) - off
    end = _f(_f(hi) * _f(scale)) - off
    size = _f(end - start)
    if not aligned:
        size = max(size, _f(1.0))
    bin_size = _f(size / _f(pooled))
    grid = int(sampling_ratio) if sampling_ratio > 0 else int(np.ceil(bin_size))
    return start, bin_size, grid


def axis_taps(start, end, pooled, bins, sampling_ratio, aligned, scale, extent):
    """The samples of the bins `bins` on one axis: (valid, low, high, frac), each [len(bins), grid] -- whether the sample lies in
    [-1, extent], its two tap pixels after the clamps, and the float64 weight of the high tap (the low tap has 1 - frac)."""
    s, b, grid = _axis_geometry(start, end, pooled, sampling_ratio, aligned, scale)
    bins = np.asarray(bins, dtype=np.int64)
    grid = max(grid, 0)
    p = bins.astype(np.float32)[:, None]
    i = np.arange(grid, dtype=np.float32)[None, :]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = (s + p * b) + ((i + _f(0.5)) * b) / _f(max(grid, 1))                # float32 [bins, grid]
    assert v.dtype == np.float32
    valid = ~((v < _f(-1.0)) | (v > _f(extent))) & np.isfinite(v)
    v = np.where(valid, v, _f(0.0))
    v = np.where(v <= 0, _f(0.0), v)
    low = v.astype(np.int64)
    last = low >= extent - 1
    low = np.where(last, extent - 1, low)
    high = np.where(last, low, low + 1)
    v = np.where(last, low.astype(np.float32), v)
    return valid, low, high, v.astype(np.float64) - low                          # float64 from here on


def axis_weights(start, end, pooled, bins, sampling_ratio, aligned, scale, extent):
    """float64 [len(bins), extent]: entry [o, p] = the sum over the samples of bin bins[o] of the bilinear weight the sample puts
    on pixel p of an axis of `extent` pixels.  start / end: the box's two edges on this axis in image pixels (both edges, not a
    size: the contract forms the size from the two SCALED edges in float32).  Not divided by the sample count."""
    valid, low, high, frac = axis_taps(start, end, pooled, bins, sampling_ratio, aligned, scale, extent)
    out = np.zeros((valid.shape[0], extent), np.float64)
    rows = np.broadcast_to(np.arange(valid.shape[0])[:, None], valid.shape)
    np.add.at(out, (rows[valid], low[valid]), (1.0 - frac)[valid])
    np.add.at(out, (rows[valid], high[valid]), frac[valid])
    return out


def _pooled(P):
    """(PH, PW) of a pooled size given as one int (square) or as a pair."""
    return (int(P), int(P)) if np.isscalar(P) else (int(P[0]), int(P[1]))


def grid_sizes(rois, P, scale, sr, aligned):
    """(gh, gw): int64 [R] each, the contract's RAW sampling grid per roi (<= 0: the roi has no samples), float32 geometry.
    P: the pooled size, an int or (PH, PW)."""
    PH, PW = _pooled(P)
    rois = np.asarray(rois, np.float32).reshape(-1, 5)
    gh = np.array([_axis_geometry(r[2], r[4], PH, sr, aligned, scale)[2] for r in rois], np.int64)
    gw = np.array([_axis_geometry(r[1], r[3], PW, sr, aligned, scale)[2] for r in rois], np.int64)
    return gh, gw


def _roi_matrices(roi, H, W, P, scale, sr, aligned, bin_stride):
    PH, PW = _pooled(P)
    wy = axis_weights(roi[2], roi[4], PH, np.arange(0, PH, bin_stride), sr, aligned, scale, H)
    wx = axis_weights(roi[1], roi[3], PW, np.arange(0, PW, bin_stride), sr, aligned, scale, W)
    gh = _axis_geometry(roi[2], roi[4], PH, sr, aligned, scale)[2]
    gw = _axis_geometry(roi[1], roi[3], PW, sr, aligned, scale)[2]
    return wy, wx, float(max(gh * gw, 1))


def roi_align_fwd_f64(feat_nhwc, rois, P, scale, sr, aligned, bin_stride=1):
    """feat [N,H,W,C], rois [R,5] (image, x1, y1, x2, y2) -> float64 [R, OH, OW, C], OH = ceil(PH / bin_stride), OW = ceil(PW /
    bin_stride): the bins 0, bin_stride, 2 bin_stride, ... of a PH x PW pooler (P: an int, or the pair).  A roi whose image index
    is outside [0, N) gives zeros."""
    feat = np.asarray(feat_nhwc, np.float64)
    rois = np.asarray(rois, np.float32).reshape(-1, 5)
    N, H, W, C = feat.shape
    PH, PW = _pooled(P)
    OH, OW = len(range(0, PH, bin_stride)), len(range(0, PW, bin_stride))
    out = np.zeros((len(rois), OH, OW, C), np.float64)
    for r, roi in enumerate(rois):
        b = int(roi[0])
        if not 0 <= b < N:
            continue
        wy, wx, count = _roi_matrices(roi, H, W, P, scale, sr, aligned, bin_stride)
        t = (wy @ feat[b].reshape(H, W * C)).reshape(OH, W, C)
        out[r] = np.matmul(wx, t) / count
    return out


def roi_align_bwd_f64(grad, feat_shape, rois, P, scale, sr, aligned, bin_stride=1):
    """grad [R, OH, OW, C] -> float64 [N,H,W,C]: per roi  Wy^T . G . Wx / max(gh * gw, 1)  added into image int(roi[0]); a roi
    whose image index is outside [0, N) contributes nothing."""
    N, H, W, C = feat_shape
    rois = np.asarray(rois, np.float32).reshape(-1, 5)
    O = len(range(0, P, bin_stride))
    grad = np.asarray(grad, np.float64).reshape(len(rois), O, O, C)
    out = np.zeros((N, H, W, C), np.float64)
    for r, roi in enumerate(rois):
        b = int(roi[0])
        if not 0 <= b < N:
            continue
        wy, wx, count = _roi_matrices(roi, H, W, P, scale, sr, aligned, bin_stride)
        t = np.matmul(wx.T, grad[r])                                         # [OH, W, C]
        out[b] += (wy.T @ t.reshape(O, W * C)).reshape(H, W, C) / count
    return out
