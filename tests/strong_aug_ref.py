"""A second, independent restatement of the strong augmentation's bytes, close to Pillow's C and slow (small shapes only, but for
the per-pixel conversions, which take arrays so that all 2^24 colours can go through them).

Where locov_amd/strong_augment.py computes in native fp32, this file computes in float64 and rounds to fp32 explicitly after every
operation that Pillow does in fp32 (sums, products and quotients of two fp32 values rounded from their float64 result are the
fp32 operation's result: 53 >= 2 * 24 + 2 bits).  The box blur is Pillow's running accumulator over one line with its edgeA / edgeB
cases (BoxBlur.c: ImagingLineBoxBlur8), not the clamped-index sum of the definition."""
import math

import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 3, 4


def r32(x):
    """Round float64 value(s) to fp32, kept as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def luma(rgb):
    v = rgb.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 32768) // 65536).astype(np.uint8)


def rgb_to_hsv(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    mx, mn = np.max(rgb, axis=-1).astype(np.int64), np.min(rgb, axis=-1).astype(np.int64)
    out = np.zeros(rgb.shape, dtype=np.uint8)
    out[..., 2] = mx
    m = mx != mn
    r, g, b, mx, mn = r[m], g[m], b[m], mx[m], mn[m]
    cr = (mx - mn).astype(np.float64)
    s = r32(cr / mx)
    rc, gc, bc = r32((mx - r) / cr), r32((mx - g) / cr), r32((mx - b) / cr)
    h = np.empty(cr.shape, dtype=np.float64)
    is_r, is_g = r == mx, (r != mx) & (g == mx)
    is_b = ~is_r & ~is_g
    h[is_r] = (bc - gc)[is_r]
    h[is_g] = (2.0 + rc - bc)[is_g]
    h[is_b] = (4.0 + gc - rc)[is_b]
    h = r32(h)
    h = r32(np.fmod(h / 6.0 + 1.0, 1.0))
    hs = np.zeros((cr.size, 2), dtype=np.uint8)
    hs[:, 0] = np.clip(np.trunc(h * 255.0), 0, 255)
    hs[:, 1] = np.clip(np.trunc(s * 255.0), 0, 255)
    out[..., 0][m], out[..., 1][m] = hs[:, 0], hs[:, 1]
    return out


def hsv_to_rgb(hsv):
    h, s, v = (hsv[..., k].astype(np.int64) for k in range(3))
    sector = (h * 6) // 255
    f = h * 6.0 / 255.0 - sector
    fs = s / 255.0
    vf = v.astype(np.float64)
    p = np.floor(vf * (1.0 - fs) + 0.5).astype(np.int64)
    q = np.floor(vf * (1.0 - fs * f) + 0.5).astype(np.int64)
    t = np.floor(vf * (1.0 - fs * (1.0 - f)) + 0.5).astype(np.int64)
    lut = np.stack([np.stack(x, -1) for x in ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))], -2)   # [..., 6, 3]
    out = np.take_along_axis(lut, (sector % 6)[..., None, None].repeat(3, -1), axis=-2)[..., 0, :]
    out = np.where((s == 0)[..., None], v[..., None], out)
    return np.clip(out, 0, 255).astype(np.uint8)


def blend(degenerate, image, factor):
    a = float(np.float32(factor))
    d = np.broadcast_to(degenerate, image.shape).astype(np.float64)
    x = image.astype(np.float64)
    t = r32(d + r32(a * (x - d)))
    if 0.0 <= a <= 1.0:
        return np.trunc(t).astype(np.uint8)
    return np.trunc(np.where(t <= 0.0, 0.0, np.where(t >= 255.0, 255.0, t))).astype(np.uint8)


def adjust(rgb, op, value):
    if op == BRIGHTNESS:
        return blend(0, rgb, value)
    if op == CONTRAST:
        l = luma(rgb).reshape(-1).tolist()
        return blend(int(sum(l) / len(l) + 0.5), rgb, value)
    if op == SATURATION:
        return blend(luma(rgb)[..., None], rgb, value)
    assert op == HUE
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + int(value)) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


def box_radius(sigma):
    radius = float(np.float32(sigma))
    s2 = float(r32(float(r32(radius * radius)) / 3.0))
    L = float(r32(math.sqrt(12.0 * s2 + 1.0)))
    l = float(r32(math.floor((L - 1.0) / 2.0)))
    num = float(r32(float(r32(float(r32(2.0 * l)) + 1.0)) * float(r32(float(r32(l * float(r32(l + 1.0)))) - float(r32(3.0 * s2))))))
    den = float(r32(6.0 * float(r32(s2 - float(r32(float(r32(l + 1.0)) * float(r32(l + 1.0))))))))
    return float(r32(l + float(r32(num / den))))


def line_box_blur(line, fr):
    """ImagingLineBoxBlur8 on a list of ints."""
    radius = int(fr)
    ww = int(float(r32(16777216.0 / float(r32(float(r32(fr * 2.0)) + 1.0)))))
    fw = ((1 << 24) - (radius * 2 + 1) * ww) // 2
    length, lastx = len(line), len(line) - 1
    edge_a, edge_b = min(radius + 1, length), max(length - radius - 1, 0)
    out = [0] * length
    acc = line[0] * (radius + 1)
    for x in range(edge_a - 1):
        acc += line[x]
    acc += line[lastx] * (radius - edge_a + 1)

    def save(x, left, right):
        out[x] = ((acc * ww + (line[left] + line[right]) * fw + (1 << 23)) >> 24) & 255

    if edge_a <= edge_b:
        for x in range(edge_a):
            acc += line[x + radius] - line[0]
            save(x, 0, x + radius + 1)
        for x in range(edge_a, edge_b):
            acc += line[x + radius] - line[x - radius - 1]
            save(x, x - radius - 1, x + radius + 1)
        for x in range(edge_b, length):
            acc += line[lastx] - line[x - radius - 1]
            save(x, x - radius - 1, lastx)
    else:
        for x in range(edge_b):
            acc += line[x + radius] - line[0]
            save(x, 0, x + radius + 1)
        for x in range(edge_b, edge_a):
            acc += line[lastx] - line[0]
            save(x, 0, lastx)
        for x in range(edge_a, length):
            acc += line[lastx] - line[x - radius - 1]
            save(x, x - radius - 1, lastx)
    return out


def gaussian_blur(img, sigma):
    fr = box_radius(sigma)
    cur = img.astype(np.int64)
    h, w, c = cur.shape
    for _ in range(3):
        for y in range(h):
            for k in range(c):
                cur[y, :, k] = line_box_blur(cur[y, :, k].tolist(), fr)
    for _ in range(3):
        for x in range(w):
            for k in range(c):
                cur[:, x, k] = line_box_blur(cur[:, x, k].tolist(), fr)
    return cur.astype(np.uint8)


def erase(img, rects, noise):
    """The torch expression of the reference: ToTensor, the three writes of RandomErasing, ToPILImage."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).float().div(255)
    at = 0
    for rect in rects:
        if rect is None:
            continue
        i, j, eh, ew = rect
        t[:, i:i + eh, j:j + ew] = torch.from_numpy(np.asarray(noise[at:at + 3 * eh * ew], dtype=np.float32)).view(3, eh, ew)
        at += 3 * eh * ew
    return t.mul(255).byte().numpy().transpose(1, 2, 0)


def apply(img, d, noise=None):
    """The whole chain for StrongAugmentation.draw's dict."""
    if d["jitter"]:
        value = {BRIGHTNESS: d["brightness"], CONTRAST: d["contrast"], SATURATION: d["saturation"], HUE: int(d["hue"] * 255)}
        for op in d["order"]:
            img = adjust(img, op, value[op])
    if d["gray"]:
        img = np.repeat(luma(img)[..., None], 3, axis=2)
    if d["blur"]:
        img = gaussian_blur(img, d["sigma"])
    if any(e is not None for e in d["erase"]):
        img = erase(img, d["erase"], noise)
    return np.ascontiguousarray(img)
