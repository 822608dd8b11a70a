"""The inputs of the exact RPN proposal tests (tests/test_gpu_rpn.py runs the kernels on them, tests/test_rpn_ref.py checks each
case's condition from the reference alone and compares the reference with the CPU torch chain).  numpy only, built from seeds.

Every input is one on which fp32 arithmetic makes no rounding error, so the float64 reference (tests/rpn_ref.py) has to be met bit
for bit:
  - anchors have integer coordinates in [0, 2048) and widths and heights that are multiples of 8; the weights are (1, 1, 1, 1);
    dx, dy are multiples of 1/8, so dx * width is an integer and every decoded coordinate an integer;
  - dw = dh = 0 (exp gives exactly 1), or 100, far above the clamp log(1000 / 16): such an anchor lies so that the decoded box
    (half extent 31.25 x the anchor's side) covers its image on every side by a pixel and more, whatever the last bits of exp,
    and the clipped box is the whole image;
  - sides are at most 1 024, so areas, intersections and unions are integers below 2^22 and the IoU is ONE correctly rounded
    division, which compares with the dyadic thresholds 0.5 and 0.75 as the true ratio does; min_box_size is 0 or 4.

A case is a dict of the operation's inputs plus `marks`: what the case is meant to reach.  check_conditions asserts every mark from
the reference's record alone, never from a kernel's output.  Marks: P (selected per image), tie_cut (the logit at the cut equals the
next one), zeros (both +0.0 and -0.0 selected), counts (proposals per image), chain ((a, b, c) selection positions: a suppresses b,
b overlaps c, c survives), more_survivors / fewer_survivors (than post_nms_topk), filtered (at least that many positions dropped by
the size filter), dropped_suppressor ((s, k): s is filtered, overlaps k, k survives), whole_image (image whose every output box is
its whole image), nonfinite.
"""
import functools
import math

import numpy as np

import rpn_ref as ref

WEIGHTS = (1.0, 1.0, 1.0, 1.0)
CLAMP = math.log(1000.0 / 16)
IMAGE = (800, 1333)


def rand_anchors(rng, n, extent=2048, max_side=128):
    """n integer boxes inside [0, extent) with sides that are multiples of 8 up to max_side."""
    wh = 8 * rng.integers(1, max_side // 8 + 1, (n, 2))
    xy = rng.integers(0, extent - max_side, (n, 2))
    return np.concatenate([xy, xy + wh], axis=1).astype(np.float32)


def cells(n, size=16, per_row=80, y0=0):
    """n pairwise disjoint size x size boxes (touching at most), row-major."""
    i = np.arange(n)
    x, y = (i % per_row) * size, y0 + (i // per_row) * size
    return np.stack([x, y, x + size, y + size], axis=1).astype(np.float32)


def rand_deltas(rng, shape):
    d = np.zeros(shape + (4,), dtype=np.float32)
    d[..., :2] = rng.integers(-4, 5, shape + (2,)) / 8.0
    return d


def ranked_logits(rng, n, step=1.0):
    """Distinct logits on shuffled indices; position p of the selection is the index with logit -p * step."""
    perm = rng.permutation(n)
    v = np.empty(n, dtype=np.float32)
    v[perm] = -step * np.arange(n, dtype=np.float32)
    return v, perm


def make_case(name, logits, deltas, anchors, image_hw=None, pre=1000, post=100, nms_thresh=0.5, min_box_size=0.0, scale_clamp=CLAMP,
              marks=None):
    logits, deltas = np.asarray(logits, dtype=np.float32), np.asarray(deltas, dtype=np.float32)
    if logits.ndim == 1:
        logits, deltas = logits[None], deltas[None]
    N = logits.shape[0]
    return {"name": name, "logits": logits, "deltas": deltas, "anchors": np.asarray(anchors, dtype=np.float32),
            "image_hw": [tuple(hw) for hw in (image_hw or [IMAGE] * N)], "weights": WEIGHTS, "scale_clamp": scale_clamp, "pre": pre,
            "post": post, "min_box_size": float(min_box_size), "nms_thresh": float(nms_thresh), "marks": marks or {}}


def _small(hwa):
    rng = np.random.default_rng(hwa)
    anchors = rand_anchors(rng, hwa, extent=400, max_side=128)
    logits = rng.integers(-20, 20, hwa) / 4.0                    # (ties: the index decides)
    return make_case(f"hwa{hwa}", logits, rand_deltas(rng, (hwa,)), anchors, pre=100, post=100, marks={"P": [hwa]})


def _tie_cut():
    """HWA 60, pre 16, post 4.  Selection positions 0-11 are copies of box A (one survivor); 12-14 carry -0.0, +0.0, -0.0 in index
    order: box B, a copy of B, box C; 15-17 hold one logit, -1: the cut takes the lowest index of the three, box D.  The output is
    A, B, C, D with the bits of -0.0 on B and C; any other order of the zeros or of the tie changes an index."""
    rng = np.random.default_rng(60)
    hwa = 60
    perm = rng.permutation(hwa)
    top, zeros, tie, rest = perm[:12], np.sort(perm[12:15]), np.sort(perm[15:18]), perm[18:]
    logits = np.empty(hwa, dtype=np.float32)
    logits[top] = np.arange(12, 0, -1)
    logits[zeros] = [-0.0, 0.0, -0.0]
    logits[tie] = -1.0
    logits[rest] = -2.0 - np.arange(len(rest))
    anchors = cells(hwa, size=16, per_row=10, y0=200)            # everything disjoint, then the copies
    anchors[top] = [0, 0, 64, 64]
    anchors[zeros[1]] = anchors[zeros[0]]
    return make_case("tie_cut", logits, np.zeros((hwa, 4)), anchors, pre=16, post=4,
                     marks={"P": [16], "tie_cut": [0], "zeros": [0], "counts": [4], "index": [[int(top[0]), int(zeros[0]), int(zeros[2]), int(tie[0])]]})


def _all_equal():
    rng = np.random.default_rng(7)
    hwa = 200
    anchors = rand_anchors(rng, hwa, extent=300, max_side=96)
    logits = np.stack([np.full(hwa, 0.5), np.where(rng.integers(0, 2, hwa) > 0, 0.0, -0.0)]).astype(np.float32)
    return make_case("all_equal", logits, rand_deltas(rng, (2, hwa)), anchors, pre=50, post=20,
                     marks={"P": [50, 50], "tie_cut": [0, 1], "zeros": [1], "selected_is_index_order": [0, 1]})


def _batch():
    """HWA 2 000, pre 1 000, post 100, three images of different sizes; image 2 consists of copies of one box (every delta is the
    clamp case): count 1, trailing rows zero."""
    rng = np.random.default_rng(2000)
    hwa = 2000
    anchors = rand_anchors(rng, hwa, extent=256, max_side=64)
    logits = rng.integers(-400, 400, (3, hwa)) / 8.0
    deltas = rand_deltas(rng, (3, hwa))
    deltas[2] = [0, 0, 100, 100]
    return make_case("batch_2000", logits, deltas, anchors, image_hw=[(200, 240), (136, 176), (240, 104)], pre=1000, post=100,
                     marks={"P": [1000] * 3, "counts": [None, None, 1], "whole_image": [2], "distinct_counts_or_sizes": True})


def _chain():
    """P = 129.  A = [0, 80), B = [24, 104), C = [48, 128) along x (IoU 56/104 between neighbours, 32/128 between A and C): A
    suppresses B, B would have suppressed C, C survives -- at positions 63/64/65 and 126/127/128, across the 64-position chunks."""
    rng = np.random.default_rng(129)
    hwa = 129
    logits, perm = ranked_logits(rng, hwa)
    anchors = cells(hwa, size=16, per_row=40, y0=300)
    for a, y in ((63, 0), (126, 100)):
        for k in range(3):
            anchors[perm[a + k]] = [24 * k, y, 24 * k + 80, y + 80]
    return make_case("chain_129", logits, np.zeros((hwa, 4)), anchors, pre=200, post=129,
                     marks={"P": [129], "chain": [(0, 63, 64, 65), (0, 126, 127, 128)], "counts": [127]})


def _early_stop():
    rng = np.random.default_rng(300)
    hwa = 300
    logits, _ = ranked_logits(rng, hwa)
    return make_case("early_stop_64", logits, np.zeros((hwa, 4)), cells(hwa), pre=300, post=64, marks={"P": [300], "more_survivors": [0], "counts": [64]})


def _post_above_survivors():
    rng = np.random.default_rng(301)
    hwa = 300
    logits, _ = ranked_logits(rng, hwa)
    anchors = cells(10, size=64, per_row=10)[rng.integers(0, 10, hwa)]
    return make_case("post_above_survivors", logits, np.zeros((hwa, 4)), anchors, pre=300, post=64, marks={"P": [300], "fewer_survivors": [0], "counts": [10]})


def _outside():
    """Anchors fully outside the (100, 100) image clip to zero width or height and are dropped at min_box_size 0."""
    rng = np.random.default_rng(11)
    hwa = 150
    anchors = rand_anchors(rng, hwa, extent=96, max_side=32)
    out = rng.permutation(hwa)[:60]
    anchors[out[:30], 0::2] += 100                                # right of the image
    anchors[out[30:], 1::2] += 100                                # below it
    logits, _ = ranked_logits(rng, hwa, step=0.25)
    return make_case("outside_min0", logits, np.zeros((hwa, 4)), anchors, image_hw=[(100, 100)], pre=150, post=150,
                     marks={"P": [150], "filtered": [60]})


def _min_size():
    """min_box_size 4 on a (100, 100) image.  S = [0, 96, 80, 104) clips to height 4 and is dropped; K = [0, 93, 80, 101) clips to
    height 7 and survives although IoU(S, K) = 4/7 > 0.5 and S comes first; 8-pixel anchors hanging over the right edge by 4 or
    more are dropped too."""
    rng = np.random.default_rng(12)
    hwa = 70
    logits, perm = ranked_logits(rng, hwa)
    anchors = cells(hwa, size=8, per_row=10)
    anchors[:, 0::2] += 20                                        # columns 20 .. 100: the last column is inside
    over = perm[10:20]
    anchors[over, 0] = 96 + np.arange(10) % 5                     # x1 96 .. 100: clipped width 4 .. 0
    anchors[over, 2] = anchors[over, 0] + 8
    anchors[over, 1] = 8 * np.arange(10)
    anchors[over, 3] = anchors[over, 1] + 8
    anchors[perm[3]] = [0, 96, 80, 104]
    anchors[perm[5]] = [0, 93, 80, 101]
    return make_case("min_size_4", logits, np.zeros((hwa, 4)), anchors, image_hw=[(100, 100)], pre=70, post=70, min_box_size=4,
                     marks={"P": [70], "filtered": [11], "dropped_suppressor": [(0, 3, 5)]})


def _clamp(clamped: bool):
    """dw = dh = 100 on anchors in the middle of a (240, 232) image: with the clamp every box is the whole image; without it
    exp(100) overflows fp32 and the flag is raised."""
    rng = np.random.default_rng(13)
    hwa = 40
    anchors = rand_anchors(rng, hwa, extent=200, max_side=32)
    logits, _ = ranked_logits(rng, hwa)
    deltas = np.tile(np.array([0.25, -0.25, 100, 100], dtype=np.float32), (hwa, 1))
    if clamped:
        return make_case("clamp", logits, deltas, anchors, image_hw=[(240, 232)], pre=40, post=10, marks={"P": [40], "counts": [1], "whole_image": [0]})
    return make_case("no_clamp_overflow", logits, deltas, anchors, image_hw=[(240, 232)], pre=40, post=10, scale_clamp=float("inf"),
                     marks={"nonfinite": [0]})


def _big():
    """HWA 70 000 (indices cross 2^16), pre 12 000, post 2 000, two images.  Logits are multiples of 1/4 in [-12, 12]: the cut falls
    inside a group of equal logits whose indices lie on both sides of 2^16.  Image 0: (1 600, 2 000), thousands of survivors, the
    sweep stops at 2 000.  Image 1: (240, 232), half of its deltas are the clamp case (copies of the whole image), most other boxes
    clip to nothing: fewer survivors than post_nms_topk, the sweep visits every chunk."""
    rng = np.random.default_rng(70000)
    hwa = 70000
    anchors = rand_anchors(rng, hwa, extent=2048, max_side=128)
    logits = rng.integers(-48, 49, (2, hwa)) / 4.0
    deltas = rand_deltas(rng, (2, hwa))
    near = (anchors[:, 2] <= 232) & (anchors[:, 3] <= 232)      # (the clamp case needs the anchor inside the small image)
    pick = near & (rng.integers(0, 2, hwa) > 0)
    deltas[1, pick] = [0, 0, 100, 100]
    return make_case("big_70000", logits, deltas, anchors, image_hw=[(1600, 2000), (240, 232)], pre=12000, post=2000,
                     marks={"P": [12000, 12000], "tie_cut": [0, 1], "more_survivors": [0], "fewer_survivors": [1], "cut_spans_2_16": [0, 1],
                            "filtered": [0, 1000]})


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [_small(1), _small(63), _small(64), _small(65), _tie_cut(), _all_equal(), _batch(), _chain(), _early_stop(),
             _post_above_survivors(), _outside(), _min_size(), _clamp(True), _clamp(False), _big()]
    return {c["name"]: c for c in cases}


NAMES = ("hwa1", "hwa63", "hwa64", "hwa65", "tie_cut", "all_equal", "batch_2000", "chain_129", "early_stop_64", "post_above_survivors",
         "outside_min0", "min_size_4", "clamp", "no_clamp_overflow", "big_70000")
EXACT = tuple(n for n in NAMES if n != "no_clamp_overflow")          # the cases with a result (the other raises the flag)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference's records of a case: computed once, shared by the tests, never modified."""
    c = all_cases()[name]
    return ref.proposals(c["logits"], c["deltas"], c["anchors"], c["image_hw"], c["weights"], c["scale_clamp"], c["pre"], c["post"],
                         c["min_box_size"], c["nms_thresh"])


def check_exactness(c):
    a, d = c["anchors"].astype(np.float64), c["deltas"].astype(np.float64)
    assert np.all(a == np.round(a)) and a.min() >= 0 and a.max() < 2048
    assert np.all((a[:, 2:] - a[:, :2]) % 8 == 0) and np.all(a[:, 2:] - a[:, :2] > 0) and (a[:, 2:] - a[:, :2]).max() <= 1024
    assert np.all((d[..., :2] * 8) == np.round(d[..., :2] * 8))
    assert np.all((d[..., 2:] == 0) | (d[..., 2:] == 100))
    for n, (h, w) in enumerate(c["image_hw"]):
        big = d[n, :, 2] == 100
        assert np.all(d[n, big, 3] == 100)
        for k, dim in ((0, w), (1, h)):                           # the decoded box covers the image whatever exp's last bits:
            side = a[big, k + 2] - a[big, k]                      # exp(clamp) / 2 = 31.25; 31 leaves a margin of 2 pixels and more
            ctr = a[big, k] + 0.5 * side + d[n, big, k] * side
            assert np.all(ctr - 31 * side <= -1) and np.all(ctr + 31 * side >= dim + 1)
    assert c["nms_thresh"] in (0.5, 0.75) and c["min_box_size"] in (0.0, 4.0) and c["weights"] == WEIGHTS


def check_conditions(c, recs):
    """Every mark of the case, from the reference's records alone."""
    m = c["marks"]
    hwa = c["logits"].shape[1]
    for n, P in enumerate(m.get("P", [])):
        assert len(recs[n]["selected"]) == P == min(hwa, c["pre"])
    for n in m.get("tie_cut", []):
        assert recs[n]["next_logit"] is not None and recs[n]["cut_logit"] == recs[n]["next_logit"]
    for n in m.get("zeros", []):
        bits = {int(c["logits"][n, i:i + 1].view(np.int32)[0]) for i in recs[n]["selected"]}
        assert 0 in bits and -2 ** 31 in bits
    for n in m.get("selected_is_index_order", []):
        assert recs[n]["selected"] == list(range(len(recs[n]["selected"])))
    for n, want in enumerate(m.get("counts", [])):
        assert want is None or recs[n]["count"] == want
    for n, want in enumerate(m.get("index", [])):
        assert recs[n]["index"].tolist() == want
    for n, a, b, cc in m.get("chain", []):
        sup = recs[n]["suppressor"]
        assert sup[a] == -1 and sup[b] == a and sup[cc] == -1
        box = lambda p: ref.apply_deltas(c["deltas"][n, recs[n]["selected"][p]].astype(np.float64),
                                         c["anchors"][recs[n]["selected"][p]].astype(np.float64), c["weights"], c["scale_clamp"])
        assert ref.first_overlap(box(b)[None], box(cc), c["nms_thresh"]) == 0          # b would have suppressed c
    for n in m.get("more_survivors", []):
        assert len(recs[n]["survivors"]) > c["post"] == recs[n]["count"]
    for n in m.get("fewer_survivors", []):
        assert len(recs[n]["survivors"]) == recs[n]["count"] < c["post"]
    for n, least in enumerate(m.get("filtered", [])):
        assert len(recs[n]["filtered"]) >= least
    for n, s, k in m.get("dropped_suppressor", []):
        h, w = c["image_hw"][n]
        clip = lambda p: np.clip(c["anchors"][recs[n]["selected"][p]].astype(np.float64), 0, [w, h, w, h])
        assert recs[n]["suppressor"][s] == -2 and recs[n]["suppressor"][k] == -1 and s < k
        assert ref.first_overlap(clip(s)[None], clip(k), c["nms_thresh"]) == 0
    for n in m.get("whole_image", []):
        h, w = c["image_hw"][n]
        assert recs[n]["count"] >= 1 and np.all(recs[n]["boxes"] == np.array([0, 0, w, h], dtype=np.float32))
    for n in m.get("cut_spans_2_16", []):
        tied = np.flatnonzero(c["logits"][n] == np.float32(recs[n]["cut_logit"]))
        assert tied.min() < 2 ** 16 < tied.max() and recs[n]["selected"][-1] in tied
    if m.get("distinct_counts_or_sizes"):
        assert len({hw for hw in c["image_hw"]}) == len(c["image_hw"]) and len({r["count"] for r in recs}) > 1
    for n in m.get("nonfinite", []):
        assert recs[n]["nonfinite"]
    if "nonfinite" not in m:
        assert not any(r["nonfinite"] for r in recs)
