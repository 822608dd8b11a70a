"""The reference's strong augmentation (ovr/data/detection_utils.py:60-100, applied at basic_mappers.py:171-180), Pillow-exact.

The reference builds a torchvision Compose over a PIL image: RandomApply([ColorJitter(cj, cj, cj, 0.1)], 0.8), RandomGrayscale(0.2),
RandomApply([GaussianBlur([0.1, 2.0])], 0.5) (its own class over ImageFilter.GaussianBlur) and three RandomErasing between ToTensor
and ToPILImage.  Every byte of that chain comes from Pillow's C (ImageEnhance = Image.blend, convert, GaussianBlur = three box
blurs per axis) or from the two torch expressions, so the chain is restated here bit for bit:

  * apply_host is the DEFINITION, in numpy, with fp32 / fp64 / integers exactly where Pillow's C has them.
  * the device path (ops.augment_images: csrc/image_augment.hip) gives the same bytes for a whole batch in at most two launches.

The parts, each checked against a live Pillow by tests/test_strong_aug_host.py and pinned by tests/golden/g13_pil_strong_aug.npz:

  L          (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16
  RGB -> HSV v = max; max == min: h = s = 0.  Else, in fp32, cr = max - min, s = cr / max, rc = (max - r) / cr (gc, bc alike);
             h = bc - gc | 2 + rc - bc | 4 + gc - rc (r, g or b the maximum, in that order of tests), summed in DOUBLE from the fp32
             terms and rounded to fp32; h = fmod(h / 6 + 1, 1) in double, rounded to fp32; the bytes are (int)((double)x * 255).
  HSV -> RGB in double: s == 0: grey v.  Else fs = s / 255, i = floor(h * 6 / 255), f = h * 6 / 255 - i, p = round(v * (1 - fs)),
             q = round(v * (1 - fs * f)), t = round(v * (1 - fs * (1 - f))), round(x) = floor(x + 0.5); i % 6 selects
             (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q).
  enhance(f) Image.blend(degenerate, image, f): in fp32 t = d + (float)f * (x - d); for 0 <= f <= 1 the byte is (int)t, otherwise
             t clipped to [0, 255] and truncated.  d: 0 (Brightness), the pixel's L (Color), int(sum(L) / n + 0.5) of the whole
             image (Contrast).
  blur       box radius (fp32 unless stated): s2 = sigma * sigma / 3; L = sqrt(12 * s2 + 1) in double, rounded; l = floor((L - 1)
             / 2) in double, rounded; a = (2l + 1)(l(l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)); fr = l + a.  Three horizontal box
             passes, then three vertical, each writing rounded bytes: radius = (int)fr, ww = (uint32)(2^24 / (fr * 2 + 1)),
             fw = (2^24 - (2 radius + 1) ww) / 2, out[x] = (ww * sum(in[x - radius .. x + radius]) + fw * (in[x - radius - 1] +
             in[x + radius + 1]) + 2^23) >> 24, indices clamped to the line.
  erasing    ToTensor -> ToPILImage is the identity on bytes; an erased byte is trunc(v * 255) (fp32 product) modulo 256.

[TV-upstream] (restated from torchvision's public sources, unverified here: torchvision is not installed): RandomApply,
ColorJitter.get_params / forward and the PIL branches of adjust_brightness / _contrast / _saturation / _hue, RandomGrayscale,
RandomErasing.get_params / forward, ToTensor, ToPILImage.  The draws come from a random.Random, not from torch's global generator:
the distribution is upstream's, the stream is this project's (as with the mapper's other draws).
"""
from __future__ import annotations

import math
import random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 1, 2, 3, 4     # LOCOV_AUG_OP_*; ColorJitter's fn_id + 1
JITTER_OPS = (OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE)
MAX_ERASERS = 3                                                    # LOCOV_AUG_MAX_ERASERS
BLUR_PASSES = 3

_f32 = np.float32


# ---- Pillow's conversions ------------------------------------------------------------------------------------------------------

def luma(rgb: np.ndarray) -> np.ndarray:
    """convert("L") of uint8 [..., 3]: uint8 [...]."""
    v = rgb.astype(np.uint32)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def rgb_to_hsv(rgb: np.ndarray) -> np.ndarray:
    """convert("HSV") of uint8 [..., 3]."""
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    flat = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(_f32)
        s = cr / maxc.astype(_f32)
        rc, gc, bc = ((maxc - c).astype(_f32) / cr for c in (r, g, b))
        d = np.float64
        h = np.where(r == maxc, bc.astype(d) - gc.astype(d),
                     np.where(g == maxc, 2.0 + rc.astype(d) - bc.astype(d), 4.0 + gc.astype(d) - rc.astype(d))).astype(_f32)
        h = np.fmod(h.astype(d) / 6.0 + 1.0, 1.0).astype(_f32)
        uh = np.clip(np.nan_to_num(h.astype(d) * 255.0).astype(np.int32), 0, 255)
        us = np.clip(np.nan_to_num(s.astype(d) * 255.0).astype(np.int32), 0, 255)
    out = np.empty(rgb.shape, dtype=np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = np.where(flat, 0, uh), np.where(flat, 0, us), maxc
    return out


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """convert("RGB") of a uint8 [..., 3] HSV image."""
    h, s, v = (hsv[..., k].astype(np.float64) for k in range(3))
    fs = s / 255.0
    hh = h * 6.0 / 255.0
    i = np.floor(hh)
    f = hh - i
    rnd = lambda x: np.floor(x + 0.5)
    p, q, t = rnd(v * (1.0 - fs)), rnd(v * (1.0 - fs * f)), rnd(v * (1.0 - fs * (1.0 - f)))
    k = i.astype(np.int32) % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.empty(hsv.shape, dtype=np.uint8)
    for c in range(3):
        x = np.select([k == n for n in range(6)], [table[n][c] for n in range(6)])
        out[..., c] = np.where(hsv[..., 1] == 0, v, np.clip(x, 0, 255)).astype(np.uint8)
    return out


def blend(degenerate: np.ndarray, image: np.ndarray, factor: float) -> np.ndarray:
    """Image.blend(degenerate, image, factor) of uint8 arrays (degenerate broadcast to image)."""
    a = _f32(factor)
    d, x = np.broadcast_to(degenerate, image.shape).astype(np.int32), image.astype(np.int32)
    t = d.astype(_f32) + a * (x - d).astype(_f32)
    if not (a >= 0 and a <= 1):
        t = np.clip(t, _f32(0), _f32(255))
    return t.astype(np.int32).astype(np.uint8)


def contrast_mean(rgb: np.ndarray) -> int:
    """ImageEnhance.Contrast's grey level: int(ImageStat.Stat(image.convert("L")).mean[0] + 0.5)."""
    l = luma(rgb)
    return int(int(l.sum(dtype=np.int64)) / l.size + 0.5)


def adjust(rgb: np.ndarray, op: int, value) -> np.ndarray:
    """One ColorJitter operation on uint8 [H, W, 3]: value is the enhancement factor, or for OP_HUE the byte shift of H."""
    if op == OP_BRIGHTNESS:
        return blend(np.zeros((), np.uint8), rgb, value)
    if op == OP_CONTRAST:
        return blend(np.uint8(contrast_mean(rgb)), rgb, value)
    if op == OP_SATURATION:
        return blend(luma(rgb)[..., None], rgb, value)
    if op == OP_HUE:
        hsv = rgb_to_hsv(rgb)
        hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(value)) & 255
        return hsv_to_rgb(hsv)
    raise ValueError(f"unknown jitter operation {op}")


def hue_shift(hue_factor: float) -> int:
    """[TV-upstream] adjust_hue's np.uint8(hue_factor * 255): the truncated product modulo 256."""
    return int(hue_factor * 255) & 255


# ---- Pillow's Gaussian blur ----------------------------------------------------------------------------------------------------

def box_radius(sigma: float) -> np.float32:
    """_gaussian_blur_radius(sigma, 3): the fp32 box radius."""
    r = _f32(sigma)
    s2 = r * r / _f32(BLUR_PASSES)
    L = _f32(math.sqrt(12.0 * float(s2) + 1.0))
    l = _f32(math.floor((float(L) - 1.0) / 2.0))
    a = (_f32(2) * l + _f32(1)) * (l * (l + _f32(1)) - _f32(3) * s2)
    a = a / (_f32(6) * (s2 - (l + _f32(1)) * (l + _f32(1))))
    return _f32(l + a)


def box_weights(fr) -> Tuple[int, int, int]:
    """(radius, ww, fw) of one box pass of fp32 radius fr."""
    fr = _f32(fr)
    radius = int(fr)
    ww = int(_f32(1 << 24) / (fr * _f32(2) + _f32(1)))
    fw = ((1 << 24) - (2 * radius + 1) * ww) // 2
    return radius, ww, fw


def _box_pass(img: np.ndarray, radius: int, ww: int, fw: int) -> np.ndarray:
    """One box pass along axis 1 of uint8 [H, W, ...]."""
    n = img.shape[1]
    x = np.arange(n)
    v = img.astype(np.uint32)
    acc = np.zeros(img.shape, dtype=np.uint32)
    for k in range(-radius, radius + 1):
        acc += v[:, np.clip(x + k, 0, n - 1)]
    far = v[:, np.clip(x - radius - 1, 0, n - 1)] + v[:, np.clip(x + radius + 1, 0, n - 1)]
    return ((acc * np.uint32(ww) + far * np.uint32(fw) + np.uint32(1 << 23)) >> np.uint32(24)).astype(np.uint8)


def gaussian_blur(img: np.ndarray, sigma: float) -> np.ndarray:
    """np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius=sigma))) for uint8 [H, W, C]."""
    if _f32(sigma) == 0:
        return img.copy()
    radius, ww, fw = box_weights(box_radius(sigma))
    for _ in range(BLUR_PASSES):
        img = _box_pass(img, radius, ww, fw)
    img = np.swapaxes(img, 0, 1)
    for _ in range(BLUR_PASSES):
        img = _box_pass(img, radius, ww, fw)
    return np.ascontiguousarray(np.swapaxes(img, 0, 1))


def blur_reach(sigma: float) -> int:
    """How far one box pass reads: (int)fr + 1."""
    return int(box_radius(sigma)) + 1


# ---- the erasers ---------------------------------------------------------------------------------------------------------------

def noise_bytes(values: np.ndarray) -> np.ndarray:
    """ToPILImage's pic.mul(255).byte() of fp32 normal draws: the truncated fp32 product modulo 256."""
    return ((values.astype(_f32) * _f32(255)).astype(np.int32) & 255).astype(np.uint8)


def noise_count(draws: dict) -> int:
    """How many fp32 values apply_host takes from `noise` for these draws."""
    return sum(3 * e[2] * e[3] for e in draws["erase"] if e is not None)


# ---- the augmentation ----------------------------------------------------------------------------------------------------------

class RandomErasing:
    """[TV-upstream] RandomErasing(p, scale, ratio, value="random")."""

    def __init__(self, p: float, scale: Tuple[float, float], ratio: Tuple[float, float]):
        self.p, self.scale, self.ratio = float(p), tuple(scale), tuple(ratio)

    def get_params(self, rng: random.Random, h: int, w: int) -> Optional[Tuple[int, int, int, int]]:
        """Ten attempts at a rectangle (i, j, eh, ew) strictly smaller than the image; None when none fits (upstream returns the
        image unchanged)."""
        area = h * w
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            erase_area = area * rng.uniform(self.scale[0], self.scale[1])
            aspect_ratio = math.exp(rng.uniform(log_ratio[0], log_ratio[1]))
            eh = int(round(math.sqrt(erase_area * aspect_ratio)))
            ew = int(round(math.sqrt(erase_area / aspect_ratio)))
            if not (eh < h and ew < w):
                continue
            i = rng.randint(0, h - eh)
            j = rng.randint(0, w - ew)
            return i, j, eh, ew
        return None


class StrongAugmentation:
    """What build_complete_augmentation returns.  color_jitter: cj or 0; gray_scale, gaussian_blur: bool; erasers: the
    RandomErasing list."""
    JITTER_P, HUE, GRAY_P, BLUR_P, SIGMA = 0.8, 0.1, 0.2, 0.5, (0.1, 2.0)

    def __init__(self, color_jitter: float = 0.0, gray_scale: bool = False, gaussian_blur: bool = False,
                 erasers: Sequence[RandomErasing] = ()):
        self.color_jitter, self.gray_scale, self.gaussian_blur = float(color_jitter), bool(gray_scale), bool(gaussian_blur)
        self.erasers = list(erasers)
        if len(self.erasers) > MAX_ERASERS:
            raise ValueError(f"at most {MAX_ERASERS} erasers")

    def draw(self, rng: random.Random, h: int, w: int) -> dict:
        """One image's draws, in the order the Compose makes them: {"jitter": bool, "order": the four operations in the order
        they run, "brightness" / "contrast" / "saturation" / "hue": the factors, "gray": bool, "blur": bool, "sigma": float,
        "erase": per eraser None or (i, j, eh, ew)}.  What is not applied is not drawn (factors 1, 1, 1, 0; sigma 0)."""
        d = {"jitter": False, "order": list(JITTER_OPS), "brightness": 1.0, "contrast": 1.0, "saturation": 1.0, "hue": 0.0,
             "gray": False, "blur": False, "sigma": 0.0, "erase": []}
        if self.color_jitter > 0 and not self.JITTER_P < rng.random():              # RandomApply skips when p < u
            cj = self.color_jitter
            lo, hi = max(0.0, 1.0 - cj), 1.0 + cj                                     # ColorJitter._check_input
            d["jitter"] = True
            d["order"] = rng.sample(JITTER_OPS, len(JITTER_OPS))                       # torch.randperm(4)
            d["brightness"], d["contrast"], d["saturation"] = rng.uniform(lo, hi), rng.uniform(lo, hi), rng.uniform(lo, hi)
            d["hue"] = rng.uniform(-self.HUE, self.HUE)
        if self.gray_scale:
            d["gray"] = rng.random() < self.GRAY_P
        if self.gaussian_blur and not self.BLUR_P < rng.random():
            d["blur"], d["sigma"] = True, rng.uniform(*self.SIGMA)
        for eraser in self.erasers:
            d["erase"].append(eraser.get_params(rng, h, w) if rng.random() < eraser.p else None)
        return d


def build_complete_augmentation(cfg, is_train: bool) -> Optional[StrongAugmentation]:
    """ovr/data/detection_utils.py:60-100: None when not training or when none of INPUT.COLOR_JITTER, RANDOM_GRAY_SCALE,
    GAUSSIAN_BLUR, RANDOM_ERASE is on."""
    if not is_train:
        return None
    inp = cfg.INPUT
    cj = float(getattr(inp, "COLOR_JITTER", 0.0))
    gray, blur, erase = (bool(getattr(inp, k, False)) for k in ("RANDOM_GRAY_SCALE", "GAUSSIAN_BLUR", "RANDOM_ERASE"))
    if not (cj > 0 or gray or blur or erase):
        return None
    erasers = [RandomErasing(0.7, (0.05, 0.2), (0.3, 3.3)), RandomErasing(0.5, (0.02, 0.2), (0.1, 6)),
               RandomErasing(0.3, (0.02, 0.2), (0.05, 8))] if erase else []
    return StrongAugmentation(cj if cj > 0 else 0.0, gray, blur, erasers)


def jitter_chain(draws: dict) -> List[Tuple[int, float]]:
    """The (operation, value) list of the draws' colour jitter: the factor, or for OP_HUE the byte shift."""
    if not draws["jitter"]:
        return []
    value = {OP_BRIGHTNESS: draws["brightness"], OP_CONTRAST: draws["contrast"], OP_SATURATION: draws["saturation"],
             OP_HUE: hue_shift(draws["hue"])}
    return [(int(op), value[int(op)]) for op in draws["order"]]


def apply_host(image, draws: dict, noise=None) -> np.ndarray:
    """The DEFINITION: the chain on a uint8 [H, W, 3] image (channel 0 plays R, as in the reference's Image.fromarray(..., "RGB")).
    noise: fp32 [>= noise_count(draws)], the erasers' normal draws: per eraser with a rectangle its [3, eh, ew] values,
    channel-major, eraser after eraser."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise TypeError(f"apply_host: a uint8 [H, W, 3] image, got {img.dtype} {img.shape}")
    img = img.copy()
    for op, value in jitter_chain(draws):
        img = adjust(img, op, value)
    if draws["gray"]:
        img = np.repeat(luma(img)[..., None], 3, axis=2)
    if draws["blur"]:
        img = gaussian_blur(img, draws["sigma"])
    need = noise_count(draws)
    if need:
        noise = np.asarray(noise.detach().cpu().numpy() if hasattr(noise, "detach") else noise, dtype=np.float32).reshape(-1)
        if noise.size < need:
            raise ValueError(f"apply_host: {need} noise values needed, {noise.size} given")
        at = 0
        for e in draws["erase"]:
            if e is None:
                continue
            i, j, eh, ew = e
            block = noise_bytes(noise[at:at + 3 * eh * ew]).reshape(3, eh, ew)
            img[i:i + eh, j:j + ew] = block.transpose(1, 2, 0)
            at += 3 * eh * ew
    return np.ascontiguousarray(img)
