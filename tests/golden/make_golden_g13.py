"""Writes tests/golden/g13_pil_strong_aug.npz: Pillow's own bytes for the strong augmentation's parts and for whole chains, on the
small cases of tests/strong_aug_cases.py.

    python tests/golden/make_golden_g13.py        (on the CPU, with Pillow installed)

`op:<name>/<value>`: the operation on content(*SMALL, "ops") -- "L" / "HSV" / "RGB_from_HSV" are convert(), "brightness" /
"contrast" / "color" are ImageEnhance.<Name>(im).enhance(value), "hue" is torchvision's adjust_hue restated over Pillow (convert("HSV"),
H + value modulo 256, convert("RGB")), "blur" is filter(ImageFilter.GaussianBlur(radius=value)).  `chain:<name>`: the Compose of
the reference for the draws of CHAIN_CASES (no erasers: those are torch's bytes, which the host tests form with torch itself).
`blur_sizes:<h>x<w>/<sigma>`: the blur on the lines shorter than its reach.  `pillow_version` records the Pillow that produced
the file.  The inputs are not stored: the tests redraw them from strong_aug_cases.content."""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import strong_aug_cases as sc  # noqa: E402

ENHANCERS = {sc.BRIGHTNESS: ImageEnhance.Brightness, sc.CONTRAST: ImageEnhance.Contrast, sc.SATURATION: ImageEnhance.Color}


def pil_hue(im, shift):
    h, s, v = im.convert("HSV").split()
    np_h = ((np.asarray(h).astype(np.int64) + int(shift)) % 256).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pil_op(img, name, value):
    im = Image.fromarray(img, "RGB")
    if name == "L":
        return np.asarray(im.convert("L"))
    if name == "HSV":
        return np.asarray(im.convert("HSV"))
    if name == "RGB_from_HSV":
        return np.asarray(Image.fromarray(img, "HSV").convert("RGB"))
    if name in ("brightness", "contrast", "color"):
        return np.asarray(getattr(ImageEnhance, name.capitalize())(im).enhance(value))
    if name == "hue":
        return np.asarray(pil_hue(im, value))
    assert name == "blur"
    return np.asarray(im.filter(ImageFilter.GaussianBlur(radius=value)))


def pil_chain(img, d):
    """The reference's Compose without the erasers, for StrongAugmentation.draw's dict."""
    im = Image.fromarray(img, "RGB")
    if d["jitter"]:
        factor = {sc.BRIGHTNESS: d["brightness"], sc.CONTRAST: d["contrast"], sc.SATURATION: d["saturation"]}
        for op in d["order"]:
            im = pil_hue(im, int(d["hue"] * 255)) if op == sc.HUE else ENHANCERS[op](im).enhance(factor[op])
    if d["gray"]:
        l = np.asarray(im.convert("L"))
        im = Image.fromarray(np.dstack([l, l, l]), "RGB")
    if d["blur"]:
        im = im.filter(ImageFilter.GaussianBlur(radius=d["sigma"]))
    return np.asarray(im)


def main():
    arrays = {"pillow_version": np.array(PIL.__version__)}
    img = sc.content(*sc.SMALL, "ops")
    for name, value in sc.OP_CASES:
        arrays[f"op:{name}/{value}"] = pil_op(img, name, value)
    for name, (h, w), kind, d in sc.CHAIN_CASES:
        arrays[f"chain:{name}"] = pil_chain(sc.content(h, w, name, kind), d)
    for h, w in sc.BLUR_SIZES:
        for sigma in sc.SIGMAS:
            arrays[f"blur_sizes:{h}x{w}/{sigma}"] = pil_op(sc.content(h, w, f"blur{h}x{w}"), "blur", sigma)
    path = os.path.join(HERE, "g13_pil_strong_aug.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
