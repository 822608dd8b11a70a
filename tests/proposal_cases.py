"""Shared by tests/test_proposals_host.py, tests/test_proposals_capi.py and tests/test_gpu_proposals.py: the case table of the proposal
side of the dataset mapper (locov_amd/data.py: transform_proposals + change_proposals_as_gt; csrc/proposal_map.hip).  Small, because
the kernel can only go wrong at boundaries: a chunk is 256 rows, a wave 64, a call 64 images.

A case is a batch: images of n rows each (content by `kind`), a row dtype, a topk, and a store layout.  rows() redraws an image's
[n, 5] rows from the case's name; the first SPECIAL rows of an image with n >= SPECIAL are the edge rows listed at special_rows()."""
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np

THR = 0.7
THR_F32 = np.float32(0.7)                                   # what an fp32 tensor is compared with
THR_F32_NEXT = np.nextafter(THR_F32, np.float32(1.0))       # the only one of the three threshold logits that is kept
SPECIAL = 12
CHUNK, MAX_IMAGES = 256, 64
ROW_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


class Image(NamedTuple):
    n: int
    hw: Tuple[int, int]
    new_hw: Optional[Tuple[int, int]]                       # None: no resize (ResizeShortestEdge drew 0), factors of exactly 1
    flip: int                                               # 0 / 1 / 2
    kind: str = "random"                                    # "random" | "all_kept" | "all_dropped"


class Case(NamedTuple):
    name: str
    dtype: str
    topk: int
    images: Tuple[Image, ...]
    scattered: bool = True                                  # the store holds the images permuted, with filler rows between them


def special_rows(h: int, w: int, dtype) -> np.ndarray:
    """[SPECIAL, 5]: what the definition must get right one row at a time (before the transform; h, w the original size)."""
    inf, nan = np.inf, np.nan
    good = [0.25 * w, 0.25 * h, 0.5 * w, 0.75 * h]
    rows = np.array([
        [0.3 * w, 0.1 * h, 0.3 * w, 0.9 * h, 0.9],          # 0: x1 == x2: empty
        [1.5 * w, 0.1 * h, 1.9 * w, 0.9 * h, 0.9],          # 1: wholly outside: clipped to empty
        [0.6 * w, 0.8 * h, 0.2 * w, 0.3 * h, 0.9],          # 2: x1 > x2 and y1 > y2: apply_box orders the corners
        [-0.0, -0.0, 0.5 * w, 0.5 * h, 0.9],                # 3: negative zeros
        [0.1 * w, 0.1 * h, inf, 0.5 * h, 0.9],              # 4: +inf is clipped to the width
        [-inf, 0.1 * h, 0.4 * w, inf, 0.2],                 # 5: -inf to 0, below the threshold
        [nan, 0.1 * h, 0.4 * w, 0.5 * h, 0.9],              # 6: a NaN end makes the axis NaN: empty
        [0.1 * w, 0.1 * h, 0.4 * w, nan, 0.9],              # 7
        good + [0.0],                                       # 8: logit == fp32(0.7): not above it
        good + [0.0],                                       # 9: its fp32 successor: kept
        good + [0.0],                                       # 10: the DOUBLE 0.7 (above fp32(0.7) as a real number, equal to it once fp32)
        [-inf, -inf, inf, inf, 0.95],                       # 11: the whole image
    ], dtype=np.float64).astype(dtype)
    rows[8, 4], rows[9, 4], rows[10, 4] = THR_F32, THR_F32_NEXT, 0.7
    return rows


def rows(case: Case, i: int) -> np.ndarray:
    im = case.images[i]
    rng = np.random.default_rng(zlib.crc32(f"{case.name}/{i}".encode()))
    (h, w), n = im.hw, im.n
    if im.kind == "all_kept":
        x1, y1 = rng.uniform(0, 0.4 * w, n), rng.uniform(0, 0.4 * h, n)
        x2, y2 = x1 + rng.uniform(1, 0.5 * w, n), y1 + rng.uniform(1, 0.5 * h, n)
    elif im.kind == "all_dropped":
        x1, y1 = rng.uniform(1.01 * w, 2 * w, n), rng.uniform(0, h, n)
        x2, y2 = x1 + rng.uniform(0, w, n), y1.copy()       # outside the image, and of no height
    else:
        x1, y1 = rng.uniform(-0.2 * w, 1.1 * w, n), rng.uniform(-0.2 * h, 1.1 * h, n)
        x2, y2 = x1 + rng.uniform(-0.1 * w, 0.6 * w, n), y1 + rng.uniform(-0.1 * h, 0.6 * h, n)
    out = np.stack([x1, y1, x2, y2, rng.uniform(0.4, 1.0, n)], axis=1).astype(case.dtype)
    if im.kind == "random" and n >= SPECIAL:
        out[:SPECIAL] = special_rows(h, w, case.dtype)
    return out


def store(case: Case):
    """(store [R, 5], row_start per image, n_rows per image): packed in order, or permuted with three filler rows before each."""
    per_image = [rows(case, i) for i in range(len(case.images))]
    order = list(range(len(per_image)))
    if case.scattered:
        order = list(np.random.default_rng(len(per_image)).permutation(len(per_image)))
    parts, starts, at = [], [0] * len(per_image), 0
    for i in order:
        if case.scattered:
            parts.append(np.full((3, 5), 1e30, dtype=case.dtype))
            at += 3
        starts[i] = at
        parts.append(per_image[i])
        at += per_image[i].shape[0]
    parts.append(np.zeros((0, 5), dtype=case.dtype))
    return np.concatenate(parts), starts, [r.shape[0] for r in per_image]


def size_of(im: Image) -> Tuple[int, int]:
    return im.hw if im.new_hw is None else im.new_hw


def factors_of(im: Image) -> Tuple[float, float]:
    """(fx, fy) as ResizeTransform.apply_coords forms them, in double."""
    return (1.0, 1.0) if im.new_hw is None else (im.new_hw[1] * 1.0 / im.hw[1], im.new_hw[0] * 1.0 / im.hw[0])


def transforms_of(data, im: Image):
    """The TransformList the mapper builds for the image, from locov_amd.data's classes."""
    (h, w), (nh, nw) = im.hw, size_of(im)
    resize = data.NoOpTransform() if im.new_hw is None else data.ResizeTransform(h, w, nh, nw)
    flip = {0: data.NoOpTransform(), 1: data.HFlipTransform(nw), 2: data.VFlipTransform(nh)}[im.flip]
    return data.TransformList([resize, flip])


_A, _B, _C = ((480, 640), (800, 1067)), ((37, 53), (74, 90)), ((333, 500), (222, 333))        # fx != fy in _B; a downscale in _C


def _many(n_images: int):
    picks = (12, 0, 1, 63, 65, 30)
    return tuple(Image(picks[i % len(picks)], *(_A, _B, _C)[i % 3], flip=i % 3, kind=("random", "all_kept", "random", "all_dropped")[i % 4])
                 for i in range(n_images))


_SIZES = tuple(Image(n, *(_A, _B, _C)[i % 3], flip=(1, 0, 2)[i % 3]) for i, n in enumerate((63, 0, 1, 64, 65, 255, 256, 257, 1000)))

CASES = (
    Case("sizes_f32", "float32", 2000, _SIZES),                                  # every row count, n == 0 between two others; topk > n
    Case("sizes_f64", "float64", 2000, _SIZES),
    Case("one_image", "float32", 1000, (Image(257, *_A, flip=1),), scattered=False),
    Case("no_resize", "float32", 50, (Image(65, (37, 53), None, 1), Image(64, (37, 53), None, 2), Image(63, (37, 53), None, 0))),
    Case("no_resize_f64", "float64", 50, (Image(65, (37, 53), None, 2), Image(64, (37, 53), None, 1), Image(12, (37, 53), None, 0))),
    Case("topk_0", "float32", 0, (Image(257, *_A, flip=0), Image(12, *_B, flip=1), Image(0, *_C, flip=2))),
    Case("topk_1", "float64", 1, (Image(257, *_A, flip=1), Image(1, *_B, flip=0, kind="all_kept"), Image(65, *_C, flip=2, kind="all_dropped"))),
    Case("topk_in_chunk", "float32", 100, (Image(1000, *_A, flip=1, kind="all_kept"), Image(1000, *_C, flip=0), Image(63, *_B, flip=2))),
    Case("topk_chunk", "float32", CHUNK, (Image(600, *_A, flip=2, kind="all_kept"), Image(257, *_B, flip=1), Image(256, *_C, flip=0, kind="all_kept"))),
    Case("topk_past_chunk", "float64", 300, (Image(1000, *_A, flip=0, kind="all_kept"), Image(1000, *_B, flip=1), Image(300, *_C, flip=2, kind="all_dropped"))),
    Case("full_call", "float32", 40, _many(MAX_IMAGES)),
)
CHUNKED = Case("two_calls", "float32", 40, _many(MAX_IMAGES + 1))                # through ops only: 64 + 1 images
assert {im.n for c in CASES for im in c.images} >= set(ROW_COUNTS) and {len(c.images) for c in CASES} >= {1, 3, MAX_IMAGES}

_expected = {}


def expected(data, case: Case):
    """Per image, what the HOST DEFINITION gives (computed once per case and shared): prop_boxes / prop_logits / prop_src and
    gt_boxes / gt_logits / gt_classes / gt_src as CPU tensors.  The source rows come from the definition too: a second pass whose
    logits are the row numbers."""
    import torch
    if case.name not in _expected:
        out = []
        for i, im in enumerate(case.images):
            r = rows(case, i)
            d = {"proposal_boxes": r[:, :4], "proposal_bbox_mode": data.XYXY_ABS, "proposal_objectness_logits": r[:, 4]}
            numbered = dict(d, proposal_objectness_logits=np.arange(im.n, dtype=np.float64))
            for each in (d, numbered):
                data.transform_proposals(each, size_of(im), transforms_of(data, im), case.topk)
            src = numbered["proposals"].objectness_logits.to(torch.int64)
            props = d["proposals"]
            d["instances"] = "the annotated boxes"
            done = data.change_proposals_as_gt(d, THR)
            assert done["gt_obj"] == "the annotated boxes" and "proposals" not in done
            gt = done["instances"]
            out.append({"prop_boxes": props.proposal_boxes.tensor, "prop_logits": props.objectness_logits, "prop_src": src,
                        "gt_boxes": gt.gt_boxes.tensor, "gt_logits": gt.objectness_logits, "gt_classes": gt.gt_classes,
                        "gt_src": src[props.objectness_logits > float(THR)], "image_size": gt.image_size})
        _expected[case.name] = out
    return _expected[case.name]
