"""A second restatement of Pillow's 8-bit bilinear resampling (public Resample.c), written independently of locov_amd/data.py:
Python floats and ints only for the coefficients, a plain loop over every output index of the resampled axis and over its taps,
one tap added at a time.  (The other axis and the channels ride along as a numpy row, so that the realistic shapes take a second,
not minutes; no coefficient table, gather or clip of data.py is shared.)  The GPU tests compare bytes against this module."""
import math

import numpy as np


def taps(in_size, out_size):
    """ksize of precompute_coeffs: the width of a coefficient row."""
    fs = max(in_size / out_size, 1.0)
    return int(math.ceil(1.0 * fs)) * 2 + 1


def coefficients(in_size, out_size, xx):
    """(xmin, [k0, k1, ...]) of output index xx: the integer taps normalize_coeffs_8bpc leaves."""
    scale = in_size / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    center = (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = int(center - support + 0.5)
    if xmin < 0:
        xmin = 0
    xmax = int(center + support + 0.5)
    if xmax > in_size:
        xmax = in_size
    xmax -= xmin
    ws, ww = [], 0.0
    for x in range(xmax):
        t = (x + xmin - center + 0.5) * ss
        if t < 0.0:
            t = -t
        w = 1.0 - t if t < 1.0 else 0.0
        ws.append(w)
        ww += w
    ks = []
    for w in ws:
        if ww != 0.0:
            w /= ww
        ks.append(int(-0.5 + w * 4194304.0) if w < 0 else int(0.5 + w * 4194304.0))
    return xmin, ks


def _pass(lines, out_size):
    """lines: uint8 [in_size, ...]; resamples the first axis."""
    in_size = lines.shape[0]
    wide = lines.astype(np.int64)
    out = np.empty((out_size,) + lines.shape[1:], dtype=np.uint8)
    for xx in range(out_size):
        xmin, ks = coefficients(in_size, out_size, xx)
        ss0 = np.full(lines.shape[1:], 1 << 21, dtype=np.int64)
        for x, k in enumerate(ks):
            ss0 = ss0 + wide[xmin + x] * k
        v = ss0 >> 22
        v[v < 0] = 0
        v[v > 255] = 255
        out[xx] = v
    return out


def resize(img, new_h, new_w):
    """uint8 [H, W, C] -> [new_h, new_w, C]: the horizontal pass writes bytes, the vertical pass reads them."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    if new_w != img.shape[1]:
        img = _pass(img.transpose(1, 0, 2), new_w).transpose(1, 0, 2)
    if new_h != img.shape[0]:
        img = _pass(img, new_h)
    return np.ascontiguousarray(img)


def resize_flip_chw(img, new_h, new_w, flip=0):
    """What the kernel writes: resize, then flip (0 none, 1 horizontal, 2 vertical), then HWC -> CHW."""
    out = resize(img, new_h, new_w)
    if flip == 1:
        out = out[:, ::-1]
    elif flip == 2:
        out = out[::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1))
