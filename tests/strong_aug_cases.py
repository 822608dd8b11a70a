"""The shapes, contents and draws the strong-augmentation tests share: tests/golden/make_golden_g13.py records Pillow's own bytes for
OP_CASES and CHAIN_CASES, the host tests check both restatements (locov_amd/strong_augment.py and tests/strong_aug_ref.py) against
that record and against a live Pillow, the GPU tests run the kernel against locov_amd.strong_augment.apply_host."""
import itertools
import zlib

import numpy as np

TILE_H, TILE_W = 32, 64          # the kernel's output tile (csrc/image_augment.hip: kTH, kTW)
MAX_IMAGES, MAX_ERASERS = 64, 3
BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 3, 4

# the lines shorter than a box pass's reach, one tile, one pixel past it, several tiles with partial edges
SIZES = [(1, 1), (1, 7), (7, 1), (3, 5), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (70, 150)]
SIGMAS = [0.1, 0.45, 0.9, 1.3, 2.0]
FACTOR_SETS = [(0.6, 1.4, 0.6, -0.1), (1.4, 0.6, 1.4, 0.1), (1.0, 1.0, 1.0, 0.0)]
PERMUTATIONS = [list(p) for p in itertools.permutations((BRIGHTNESS, CONTRAST, SATURATION, HUE))]
BLUR_SIZES = [(23, 31), (1, 1), (1, 7), (7, 1)]
SMALL = (13, 17)                 # the fixture's image for single operations and chains


def content(h, w, key, kind="random"):
    """uint8 [h, w, 3]: "random" (uniform bytes seeded by `key`), "smooth" (a colour ramp plus small noise: saturated and grey
    regions, where the hue branches differ), or a constant byte given as an int."""
    if isinstance(kind, int):
        return np.full((h, w, 3), kind, dtype=np.uint8)
    rng = np.random.default_rng(zlib.crc32(str(key).encode()))
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert kind == "smooth"
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)], -1)
    return np.clip(base + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def draws(order=(), factors=(1.0, 1.0, 1.0, 0.0), gray=False, sigma=None, erase=()):
    """StrongAugmentation.draw's dict.  order: the jitter operations that run, in order (may be fewer than four)."""
    b, c, s, h = factors
    return {"jitter": len(order) > 0, "order": list(order), "brightness": float(b), "contrast": float(c), "saturation": float(s),
            "hue": float(h), "gray": bool(gray), "blur": sigma is not None, "sigma": 0.0 if sigma is None else float(sigma),
            "erase": list(erase)}


def noise(n, key):
    """fp32 [n] normal draws, with a few values past +-1 / 255 steps on purpose: every byte, negative and wrapped ones."""
    v = np.random.default_rng(zlib.crc32(str(key).encode()) ^ 0x5EED).standard_normal(n).astype(np.float32)
    v[::7] *= np.float32(3.0)
    return v


# what the fixture records: single operations on SMALL ...
OP_CASES = ([("L", None), ("HSV", None), ("RGB_from_HSV", None)]
            + [(name, f) for name in ("brightness", "contrast", "color") for f in (0.0, 0.35, 1.0, 1.4, 2.0)]
            + [("hue", s) for s in (-25, 0, 25)]
            + [("blur", s) for s in SIGMAS])
# ... and whole chains: (name, (h, w), content kind, draws)
CHAIN_CASES = [
    ("jitter_0", SMALL, "random", draws(PERMUTATIONS[0], FACTOR_SETS[0])),
    ("jitter_9", SMALL, "smooth", draws(PERMUTATIONS[9], FACTOR_SETS[1])),
    ("jitter_17", SMALL, "random", draws(PERMUTATIONS[17], FACTOR_SETS[1])),
    ("jitter_23", SMALL, "smooth", draws(PERMUTATIONS[23], FACTOR_SETS[2])),
    ("gray", SMALL, "random", draws(gray=True)),
    ("jitter_gray_blur", SMALL, "random", draws(PERMUTATIONS[5], FACTOR_SETS[0], gray=True, sigma=1.3)),
    ("jitter_blur", (23, 31), "smooth", draws(PERMUTATIONS[14], FACTOR_SETS[1], sigma=2.0)),
    ("blur_row", (1, 7), "random", draws(sigma=2.0)),
    ("blur_column", (7, 1), "random", draws(sigma=0.9)),
    ("blur_pixel", (1, 1), "random", draws(sigma=2.0)),
    ("white_blur", SMALL, 255, draws(sigma=2.0)),
]
