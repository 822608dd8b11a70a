"""Writes tests/golden/g12_pil_resize.npz: Pillow's own output for the small cases of tests/resize_cases.py.

    python tests/golden/make_golden_g12.py        (on the CPU, with Pillow installed)

Per case `<name>/<content>/<channels>`: `in:<key>` the uint8 [h, w, c] input and `out:<key>` the bytes of
Image.fromarray(img).resize((new_w, new_h), Image.BILINEAR).  Modes: "L" for one channel, "RGB" for three, "CMYK" for four ("RGBA"
would be resized with premultiplied alpha, which is not what the mapper does to an image array).  `pillow_version` records the
Pillow that produced the file."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_cases  # noqa: E402

MODES = {1: "L", 3: "RGB", 4: "CMYK"}


def pil_resize(img, new_h, new_w):
    c = img.shape[2]
    im = Image.fromarray(img[:, :, 0] if c == 1 else img, MODES[c])
    out = np.asarray(im.resize((new_w, new_h), Image.BILINEAR))
    return out[:, :, None] if c == 1 else out


def entries():
    """(key, name, (h, w), (new_h, new_w), content, channels) of every recorded case."""
    for name, size, new in resize_cases.SMALL_CASES:
        yield f"{name}/random/3", name, size, new, "random", 3
    for kind in ("checker", "white"):
        for name in ("upscale", "many_taps"):
            size, new = next((s, n) for nm, s, n in resize_cases.SMALL_CASES if nm == name)
            yield f"{name}/{kind}/3", name, size, new, kind, 3
    name, size, new = resize_cases.CHANNEL_CASE
    for c in (1, 4):
        yield f"{name}/random/{c}", name, size, new, "random", c


def main():
    arrays = {"pillow_version": np.array(PIL.__version__)}
    for key, name, (h, w), (nh, nw), kind, c in entries():
        img = resize_cases.content(kind, h, w, c, key)
        arrays["in:" + key] = img
        arrays["out:" + key] = pil_resize(img, nh, nw)
    path = os.path.join(HERE, "g12_pil_resize.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
