"""The shapes and contents the resize tests share: tests/golden/make_golden_g12.py records Pillow's output for SMALL_CASES, the host
tests check both restatements against that record (and against a live Pillow where it imports), the GPU tests run the kernel
over SMALL_CASES + [REALISTIC] against tests/resize_ref.py."""
import zlib

import numpy as np

TILE_H, TILE_W = 16, 64          # the kernel's output tile (csrc/image_resize.hip: kTH, kTW)
MAX_TAPS = 17                    # LOCOV_RESIZE_MAX_TAPS: ceil(in / out) <= 8 per axis

# (name, (h, w), (new_h, new_w)) -- the smallest shapes at which each part of the kernel can go wrong
SMALL_CASES = [
    ("pixel", (1, 1), (3, 2)),
    ("row", (1, 9), (3, 2)),
    ("column", (9, 1), (2, 3)),
    ("upscale", (37, 53), (61, 87)),                      # non-integer factors
    ("width_only", (37, 53), (37, 80)),                   # the vertical pass is the identity
    ("height_only", (37, 53), (19, 53)),                  # the horizontal pass is the identity
    ("identity", (37, 53), (37, 53)),
    ("many_taps", (48, 64), (13, 17)),                    # 9 taps per axis
    ("mixed", (97, 131), (31, 200)),                      # down in height, up in width
    ("tap_limit", (63, 128), (8, 16)),                    # 7.875 and 8: exactly MAX_TAPS taps
    ("tap_limit_bands", (320, 24), (40, 24)),             # ... over three bands: the longest strips the kernel holds
    ("over_limit", (65, 40), (8, 20)),                    # 8.125: 19 taps -- resize_supported is False, the host path answers
    ("one_tile", (10, 10), (TILE_H, TILE_W)),
    ("tile_plus_1", (20, 30), (TILE_H + 1, TILE_W + 1)),  # the second band / tile is one pixel; source row 18 is in both bands' strips
    ("two_tiles_minus_1", (40, 50), (2 * TILE_H - 1, 2 * TILE_W - 1)),
]
REALISTIC = ("realistic", (480, 640), (800, 1067))
CHANNEL_CASE = ("channels", (9, 13), (14, 7))             # run with 1 and 4 channels


def content(kind, h, w, c, key):
    """uint8 [h, w, c]: "random" (uniform bytes, seeded by `key`), "checker" (0 / 255 by pixel parity: the largest accumulators,
    sums on the rounding boundary) or "white" (all 255)."""
    if kind == "random":
        return np.random.default_rng(zlib.crc32(str(key).encode())).integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], c, axis=2)
    assert kind == "white"
    return np.full((h, w, c), 255, dtype=np.uint8)
