"""Seeded cases of the RPN's training half for tests/test_rpn_train_ref.py (CPU: the torch chain) and tests/test_gpu_rpn_train.py (the
kernels).  Every case names the conditions it exists for; check_conditions asserts each from the reference's record
(tests/rpn_train_ref.py), so a case that stops exercising its point fails loudly.

All coordinates lie on a quarter-pixel grid and are small: box areas, intersections and unions are exact in fp32 (check_exactness),
so a label depends on ONE correctly rounded division, and the device, the torch chain and the reference must agree bit for bit.

Grids: 7 x 9 cells with A = 3 (189 anchors: less than one block, not a multiple of 64) and 23 x 37 with A = 15 (12 765 anchors: many
blocks, several radix passes).  N in {1, 2, 3}; ground-truth counts 0, 1, 5 and 70 (more than a wave).
"""
import functools

import numpy as np

import rpn_train_ref as ref

STRIDE = 4
DEFAULT_THRESHOLDS, DEFAULT_LABELS = [0.3, 0.7], [0, -1, 1]
INF = float("inf")


def make_anchors(H, W, A):
    """(y, x, a) order; centres on the stride grid, extents on the half-pixel grid."""
    if A == 3:
        shapes = [(8, 8), (12, 6), (6, 12)]
    else:
        assert A == 15
        shapes = [s for size in (4, 8, 12, 16, 24) for s in ((size, size), (1.5 * size, 0.75 * size), (0.75 * size, 1.5 * size))]
    cell = np.array([[-w / 2, -h / 2, w / 2, h / 2] for w, h in shapes], dtype=np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32) * STRIDE, np.arange(W, dtype=np.float32) * STRIDE, indexing="ij")
    shifts = np.stack([xs, ys, xs, ys], axis=-1).reshape(-1, 1, 4)
    return (shifts + cell[None]).reshape(-1, 4).astype(np.float32)


def quarter(a):
    return (np.round(np.asarray(a, dtype=np.float64) * 4) / 4).astype(np.float32)


def make_gt(rng, anchors, count, extent):
    """Half of the boxes are anchors moved by up to a pixel and a half (high IoU: positives by threshold), half are random boxes
    inside the extent (low IoU: positives by the low-quality rule only)."""
    out = []
    for k in range(count):
        if k % 2 == 0:
            b = anchors[rng.integers(anchors.shape[0])].astype(np.float64) + rng.integers(-6, 7, size=4) / 4.0
        else:
            x0, y0 = rng.uniform(0, extent[1] - 6), rng.uniform(0, extent[0] - 6)
            b = np.array([x0, y0, x0 + rng.uniform(2, 30), y0 + rng.uniform(2, 30)])
        b = quarter(b)
        b[2], b[3] = max(b[2], b[0] + 1), max(b[3], b[1] + 1)
        out.append(b)
    return np.stack(out).astype(np.float32) if out else np.zeros((0, 4), dtype=np.float32)


def _case(name, seed, H, W, A, gt_counts, budget, fraction=0.5, thresholds=None, labels=None, boundary=-1.0, key_steps=0, marks=(),
          extra_gt=None):
    rng = np.random.default_rng(seed)
    anchors = make_anchors(H, W, A)
    hwa, N = anchors.shape[0], len(gt_counts)
    extent = (H * STRIDE, W * STRIDE)
    gt = [make_gt(rng, anchors, g, extent) for g in gt_counts]
    if extra_gt is not None:
        gt = extra_gt(gt)
    rnd = rng.random((2, N, hwa))
    if key_steps:                                                # few distinct keys: duplicates everywhere, so also at the cut
        rnd = np.floor(rnd * key_steps) / key_steps
    return {"name": name, "anchors": anchors, "gt": gt, "image_hw": [extent] * N, "budget": budget, "fraction": fraction,
            "thresholds": list(thresholds or DEFAULT_THRESHOLDS), "labels": list(labels or DEFAULT_LABELS), "boundary": boundary,
            "rnd": rnd, "weights": (1.0, 1.0, 1.0, 1.0), "beta": 0.0, "marks": tuple(marks),
            "logits": rng.normal(0, 2, size=(N, hwa)).astype(np.float32), "deltas": rng.normal(0, 0.5, size=(N, hwa, 4)).astype(np.float32),
            # predictions far from any target: every L1 gradient entry is exactly +- weight / normalizer
            "deltas_far": (rng.choice([-1.0, 1.0], size=(N, hwa, 4)) * (1000 + rng.random((N, hwa, 4)))).astype(np.float32)}


def _duplicate_first(gt):
    return [np.concatenate([g[:1], g[:1], g[1:]]) if g.shape[0] else g for g in gt]


def _add_far_box(gt):
    return [np.concatenate([g, np.array([[200, 200, 220, 230]], dtype=np.float32)]) for g in gt]


BUILDERS = {
    # image 0: 70 boxes, both populations above their budget; image 1: 5 boxes, fewer positives than int(B f): negatives fill the rest
    "big_over_and_fill": lambda: _case("big_over_and_fill", 1, 23, 37, 15, (70, 5), 32,
                                       marks=("both_over:0", "neg_fill:1", "promoted", "promoted_other_box")),
    # 189 anchors against a budget of 256: both populations short of it
    "small_short": lambda: _case("small_short", 2, 7, 9, 3, (1,), 256, marks=("both_short:0",)),
    # B = 7, f = 0.5: int() truncates to 3 positives; an image without ground truth inside a batch that has some
    "b7_with_empty": lambda: _case("b7_with_empty", 3, 7, 9, 3, (5, 0, 5), 7, marks=("max_pos=3", "empty:1", "pos_over:0")),
    "empty_alone": lambda: _case("empty_alone", 4, 7, 9, 3, (0,), 16, marks=("empty:0",)),
    # a box that touches no anchor: its row maximum is 0, every anchor with IoU 0 to it is promoted
    "outside_gt": lambda: _case("outside_gt", 5, 7, 9, 3, (1,), 16, extra_gt=_add_far_box, marks=("zero_max",)),
    # two identical boxes: they tie for an anchor's maximum, the first wins
    "tie_max": lambda: _case("tie_max", 6, 7, 9, 3, (5, 1), 16, extra_gt=_duplicate_first, marks=("tie_for_max",)),
    "boundary0": lambda: _case("boundary0", 7, 7, 9, 3, (5, 5), 16, boundary=0.0, marks=("outside",)),
    # keys on a grid of 8 / 64 values: duplicated keys at the cut, small and over several radix passes
    "dup_keys_small": lambda: _case("dup_keys_small", 8, 7, 9, 3, (5,), 16, key_steps=8, marks=("tie_at_cut",)),
    "dup_keys_big": lambda: _case("dup_keys_big", 9, 23, 37, 15, (70, 1, 5), 64, key_steps=64, marks=("tie_at_cut", "both_over:0")),
    # an interval list other than the default: four intervals, no ignore band next to the positives
    "intervals": lambda: _case("intervals", 10, 7, 9, 3, (5, 5), 16, thresholds=[0.25, 0.5, 0.75], labels=[0, -1, 0, 1],
                               marks=("label_mix",)),
}
NAMES = list(BUILDERS)
SMALL = [n for n in NAMES if not n.startswith(("big", "dup_keys_big"))]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per image the record of rpn_train_ref.label_and_sample (computed once per process; callers must not write to it)."""
    c = case(name)
    return ref.label_and_sample(c["anchors"], c["gt"], c["image_hw"], [-INF] + c["thresholds"] + [INF], c["labels"], True, c["boundary"],
                                c["rnd"], c["budget"], c["fraction"])


def check_exactness(c):
    """Areas, intersections and unions of every (box, anchor) pair are exact in fp32: the float64 values are fp32 numbers."""
    a = c["anchors"].astype(np.float64)
    assert np.array_equal(a * 4, np.round(a * 4))
    for g in c["gt"]:
        g = g.astype(np.float64)
        assert np.array_equal(g * 4, np.round(g * 4))
        if not g.shape[0]:
            continue
        area_g, area_a = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]), (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        w = np.clip(np.minimum(g[:, None, 2], a[None, :, 2]) - np.maximum(g[:, None, 0], a[None, :, 0]), 0, None)
        h = np.clip(np.minimum(g[:, None, 3], a[None, :, 3]) - np.maximum(g[:, None, 1], a[None, :, 1]), 0, None)
        inter = w * h
        union = area_g[:, None] + area_a[None] - inter
        for v in (area_g, area_a, inter, union):
            assert np.array_equal(v, v.astype(np.float32).astype(np.float64)) and float(np.abs(v).max()) * 16 < 2 ** 24


def check_conditions(c, recs):
    B, max_pos = c["budget"], int(c["budget"] * c["fraction"])
    for mark in c["marks"]:
        key, _, arg = mark.partition(":")
        r = recs[int(arg)] if arg else None
        if key == "both_over":
            assert r["pop_pos"] > max_pos and r["pop_neg"] > B - max_pos and r["num_pos"] + r["num_neg"] == B, mark
        elif key == "pos_over":
            assert r["pop_pos"] > max_pos, mark
        elif key == "neg_fill":
            assert 0 < r["pop_pos"] < max_pos and r["num_neg"] == B - r["pop_pos"] > B - max_pos, mark
        elif key == "both_short":
            assert 0 < r["pop_pos"] < max_pos and r["pop_neg"] < B - r["num_pos"] and r["num_pos"] + r["num_neg"] < B, mark
        elif key == "max_pos=3":
            assert max_pos == 3 and B * c["fraction"] == 3.5, mark
        elif key == "empty":
            assert r["n_gt"] == 0 and r["pop_pos"] == 0 and not r["labels"].any() and not r["matched_boxes"].any(), mark
        elif key == "zero_max":
            assert any(x["zero_max_boxes"] > 0 and x["promoted"] > 0 for x in recs), mark
        elif key in ("promoted", "promoted_other_box", "tie_for_max", "outside"):
            assert sum(x[key] for x in recs) > 0, mark
            if key == "outside":
                assert sum(x["outside_labelled"] for x in recs) > 0, mark
        elif key == "tie_at_cut":
            assert any(x["tie_at_cut"] for x in recs), mark
        elif key == "label_mix":
            assert all({-1, 0, 1} <= set(x["labels"].tolist()) for x in recs), mark
        else:
            raise AssertionError(f"unknown mark {mark}")


# ------------------------------------------------------------------------------------------------ the module under test on a case

def make_rpn(c, **overrides):
    """An RPN with the case's matcher, budget, fraction and boundary threshold (head and anchor generator are not used)."""
    from torch import nn
    from locov_amd.proposal_generator import RPN
    from locov_amd.roi_heads.box_emb_head import Box2BoxTransform
    from locov_amd.roi_heads.labelling import Matcher
    kw = dict(in_features=["res4"], head=nn.Identity(), anchor_generator=nn.Identity(), box2box_transform=Box2BoxTransform(c["weights"]),
              pre_nms_topk=(100, 100), post_nms_topk=(10, 10), anchor_matcher=Matcher(c["thresholds"], c["labels"], allow_low_quality_matches=True),
              batch_size_per_image=c["budget"], positive_fraction=c["fraction"], anchor_boundary_thresh=c["boundary"],
              smooth_l1_beta=c["beta"])
    kw.update(overrides)
    return RPN(**kw).train()


def inputs(c, device="cpu"):
    """(anchors: [Boxes], gt_instances, rnd) of a case as the module takes them."""
    import torch
    from locov_amd.structures import Boxes, Instances
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    gt = [Instances(tuple(hw), gt_boxes=Boxes(t(g))) for g, hw in zip(c["gt"], c["image_hw"])]
    return [Boxes(t(c["anchors"]))], gt, t(c["rnd"])
