"""The inputs of the exact detection post-processing tests (tests/test_gpu_detect_exact.py runs the kernels on them,
tests/test_detect_ref.py checks the conditions and compares the reference with the CPU torch chain, without a GPU).  numpy only.

Every input is one on which fp32 arithmetic makes no rounding error, so the float64 reference (tests/detect_ref.py) has to be met bit
for bit, by both of batched_nms's branches:
  - proposal coordinates are integers in [-64, 2047]; the weights are (1, 1, 1, 1) and dw = dh = 0; dx, dy are 0 or m / width with
    integer m and width, height powers of two -- every step of the decoding is exact and every decoded, clipped coordinate an integer;
  - K * (max + 1) + max < 2^24 (max: the largest coordinate of an image's candidate boxes), so the class shift, the areas, the
    intersections and the unions are integers below 2^24 and the IoU is ONE correctly rounded division, which compares with a dyadic
    threshold as the true ratio does;
  - the NMS thresholds are 0.5, 0.25, 0.75; the score thresholds are dyadic; the probabilities are fed as they are (no softmax).

A case is a dict of the inputs (tests/detect_ref.py lists them) plus `group`, `marks` -- what the case is meant to reach -- and, for
batches, `mid`: a per_class_above between two images' candidate counts.  check_conditions asserts the exactness conditions and every
mark from the reference and select_passes alone, never from a kernel's output.  Images are (800, 1333) unless the case says otherwise.

Marks: candidates / survivors (per image), passes / winners (what select_passes gives for each image: the radix select's passes to
completion, 0 = no select), nq4 (an image above 4 096 rows: the NQ = 4 sweep), overflow (an image above 8 192 candidates: the LDS
pipeline flags it), and the semantic ones named after what they assert (threshold_edge, iou_edge, zero_area, alternate, tie_cut,
kept_span, far_suppressor, cs_sweep, cs_differs).

The select cases end after passes 1 to 5.  A sixth pass cannot be reached: a fifth-pass bin holds the keys that share the score,
the row and the upper 9 class bits -- at most 64 keys -- so the fifth pass always ends the select; no case is contorted to reach it.
"""
import functools

import numpy as np

import detect_ref as ref

IMAGE = (800, 1333)
LDS_CAP = 8192                      # LOCOV_DETECT_MAX_CANDIDATES: candidates per image of the LDS pipeline (and the largest top-k)
SWEEP_ROWS = 4096                   # rows above which dw_sweep_kernel runs its NQ = 4 instance
CPU_NMS_LIMIT = 6000                # the CPU chain builds an n x n matrix: NMS calls above this are not run on the CPU
PCA_MAX = 2 ** 31 - 1


def cells(n, size=16, first=0):
    """n pairwise disjoint size x size boxes of the (800, 1333) image (touching at most), row-major from cell `first`."""
    per_row = IMAGE[1] // size
    i = np.arange(first, first + n)
    assert (i // per_row + 1).max(initial=0) * size <= IMAGE[0]
    x, y = (i % per_row) * size, (i // per_row) * size
    return np.stack([x, y, x + size, y + size], axis=1).astype(np.float32)


def grid_boxes(rng, n, lo=-64, hi=2047, crowd=0):
    """n integer boxes in [lo, hi]; crowd > 0: jittered copies of that many boxes (long suppression chains)."""
    if crowd:
        c = grid_boxes(rng, crowd, 0, 1200)
        b = c[np.arange(n) % crowd] + rng.integers(-6, 7, (n, 4))
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 2)
        return np.clip(b, lo, hi).astype(np.float32)
    xy = rng.integers(lo, hi - 8, (n, 2))
    wh = rng.integers(4, 400, (n, 2))
    return np.concatenate([xy, np.minimum(xy + wh, hi)], axis=1).astype(np.float32)


def make_case(name, group, sizes, K, props, scores, deltas=None, image_shapes=None, score_thresh=0.0625, nms_thresh=0.5, topk=100,
              marks=None, mid=None):
    """scores [R, K]: the foreground probabilities (the background column is added as zeros)."""
    R = int(sum(sizes))
    props = np.ascontiguousarray(props, np.float32).reshape(R, 4)
    probs = np.zeros((R, K + 1), np.float32)
    probs[:, :K] = scores
    deltas = np.zeros((R, 4), np.float32) if deltas is None else np.ascontiguousarray(deltas, np.float32)
    if mid is None and len(sizes) > 1:                               # a switch that puts the fullest image alone on the per-class branch
        ends = np.cumsum(sizes)
        cand = [int((probs[e - n:e, :K] > np.float32(score_thresh)).sum()) for n, e in zip(sizes, ends)]
        mid = max(cand) if min(cand) < max(cand) else None
    return dict(name=name, group=group, sizes=list(sizes), K=K, props=props, probs=probs, deltas=deltas,
                image_shapes=list(image_shapes or [IMAGE] * len(sizes)), weights=(1.0, 1.0, 1.0, 1.0), score_thresh=score_thresh,
                nms_thresh=nms_thresh, topk=topk, marks=dict(marks or {}), mid=mid)


def variant(case, tag, **changes):
    c = dict(case)
    c["marks"] = dict(case["marks"])
    marks = changes.pop("marks", {})
    c.update(changes)
    c["marks"].update(marks)
    c["name"] = f"{case['name']}-{tag}"
    return c


def ulp(v, up):
    return np.nextafter(np.float32(v), np.float32(2.0 if up else 0.0))


# ---- semantics -----------------------------------------------------------------------------------------------------------------------

def _threshold_edge():
    rng = np.random.default_rng(1)
    R, K, thr = 70, 5, 0.0625
    pick = np.array([thr, ulp(thr, True), ulp(thr, False), 0.5, 0.25], np.float32)
    scores = pick[(np.arange(R)[:, None] * 3 + np.arange(K)[None, :]) % 5]
    return [make_case("threshold_edge", "semantics", [R], K, grid_boxes(rng, R, crowd=9), scores, score_thresh=thr, topk=300,
                      marks={"threshold_edge": True, "candidates": [int(3 * R * K / 5)]})]


def _iou_edge():
    """Pairs (a, b) in bands of their own, b inside a with the same height 1: the IoU is width(b) / width(a).  Per threshold t the
    ratios t exactly, the nearest grid ratios on either side of it, and (at 1/2) the issue's (0,0,10,10) / (0,0,10,5) pair.  Class 0
    has a first in score order, class 1 has b first."""
    out = []
    for num, thr in ((2, 0.5), (1, 0.25), (3, 0.75)):
        widths = [(1332, 333 * num), (1332, 333 * num + 1), (1332, 333 * num - 1), (1333, (1333 * num) // 4 + 1), (1333, (1333 * num) // 4)]
        props = []
        for i, (wa, wb) in enumerate(widths):
            props += [(0, 20 * i, wa, 20 * i + 1), (0, 20 * i, wb, 20 * i + 1)]
        if num == 2:
            props += [(0, 200, 10, 210), (0, 200, 10, 205)]
        props = np.array(props, np.float32)
        R = len(props)
        scores = np.zeros((R, 2), np.float32)
        scores[:, 0] = 0.5 + (R - np.arange(R)) * 2.0 ** -10          # class 0: a before b
        scores[:, 1] = 0.5 + (R - (np.arange(R) ^ 1)) * 2.0 ** -10    # class 1: b before a
        out.append(make_case(f"iou_edge_{num}_4", "semantics", [R], 2, props, scores, nms_thresh=thr, marks={"iou_edge": num}))
    return out


def _zero_area():
    props = np.array([
        [1400, 100, 1500, 200], [1400, 100, 1500, 200],               # right of the image: both clip to the line x = 1333 (0/0)
        [1350, 120, 1600, 180],                                       # ... and a third, different zero-area box on that line
        [100, 900, 300, 1000], [100, 900, 300, 1000],                 # below the image: y = 800
        [-64, -64, -10, -5], [-60, -50, -1, -1],                      # above and left: both clip to the point (0, 0)
        [1000, 50, 1333, 400],                                        # a large box that touches the right edge
        [1333, 100, 1333, 300],                                       # a degenerate proposal on that edge, inside the large box's side
        [1100, 100, 1100, 300], [1100, 200, 1200, 200],               # zero width / zero height inside the large box
        [1100, 100, 1100, 300],                                       # ... and a duplicate of the first (0/0 again)
        [1050, 60, 1300, 390],                                        # an ordinary box the large one suppresses
    ], np.float32)
    R = len(props)
    scores = np.stack([0.75 - np.arange(R) * 2.0 ** -8, np.full(R, 0.5)], axis=1).astype(np.float32)
    return [make_case("zero_area", "semantics", [R], 2, props, scores, marks={"zero_area": True, "survivors": [2 * (R - 1)]})]


def _chain():
    """200 boxes of 14 x 14 sliding by 4: neighbours have IoU 10/18, next-but-one 6/22.  In score order = sliding order every
    second one survives: positions 62, 64, ..., 126, 128 are kept across the 64-candidate words, 63, 65, 127 go.  Rows are a seeded
    permutation, so a row index is never a position."""
    n = 200
    i = np.arange(n)
    boxes = np.stack([4 * i, np.full(n, 30), 4 * i + 14, np.full(n, 44)], axis=1).astype(np.float32)
    perm = np.random.default_rng(2).permutation(n)
    props = np.zeros((n, 4), np.float32)
    scores = np.zeros((n, 1), np.float32)
    props[perm] = boxes
    scores[perm, 0] = 1.0 - i * 2.0 ** -12
    return [make_case("chain", "semantics", [n], 1, props, scores, topk=200, marks={"alternate": perm[0::2].tolist()})]


def _ties_topk():
    rng = np.random.default_rng(3)
    R, K = 60, 7
    base = make_case("ties", "semantics", [R], K, grid_boxes(rng, R, crowd=25), np.full((R, K), 0.5, np.float32), topk=100)
    s = len(ref.reference(variant(base, "count", topk=LDS_CAP))[0]["rows"])
    assert 40 < s < R * K
    return [variant(base, f"topk{k}", topk=k, marks={"tie_cut": min(k, s)}) for k in (1, s // 2, s, s + 1, LDS_CAP)]


def _ragged():
    out = []
    shapes = [(800, 1333), (640, 960), (480, 640), (1067, 800), (600, 600), (333, 500)]
    for tag, order in (("ragged", [0, 1, 2, 3, 4, 5]), ("ragged_front_empty", [1, 5, 0, 2, 3, 4])):
        sizes = [[65, 0, 1, 64, 63, 0][i] for i in order]
        rng = np.random.default_rng(4)
        R, K = sum(sizes), 6
        scores = rng.integers(0, 64, (R, K)).astype(np.float32) / 64
        out.append(make_case(tag, "semantics", sizes, K, grid_boxes(rng, R), scores, image_shapes=[shapes[i] for i in order],
                             score_thresh=0.5, topk=300))
    rng = np.random.default_rng(5)
    sizes = [(i * 7) % 12 for i in range(64)]
    R, K = sum(sizes), 3
    scores = rng.integers(0, 32, (R, K)).astype(np.float32) / 32
    out.append(make_case("ragged_64_images", "semantics", sizes, K, grid_boxes(rng, R, crowd=40), scores, score_thresh=0.25,
                         image_shapes=[(400 + 8 * i, 1333 - 16 * i) for i in range(64)]))
    return out


def _limits():
    out = []
    # the last class index: K = 32 767 (the shift unit must stay below 512: small boxes)
    K = 32767
    scores = np.zeros((2, K), np.float32)
    for r, c, v in ((0, 0, 0.5), (1, 0, 0.75), (0, K - 1, 0.5), (1, K - 1, 0.25), (1, 1024, 0.5), (0, 16383, 0.125)):
        scores[r, c] = v
    out.append(make_case("limit_classes", "limits", [2], K, [[0, 0, 16, 16], [4, 0, 20, 16]], scores,
                         marks={"candidates": [6], "last_class": K - 1}))
    # the last row index: R = 16 383, 8 192 passing rows (the LDS pipeline's capacity, in ONE class), row 16 382 among them.
    # 8 x 8 cells; every eighth passing row repeats its predecessor's cell (and is suppressed by it)
    R = 16383
    passing = np.r_[np.arange(0, 2 * 8191, 2), R - 1]
    props = cells(R, size=8)
    props[passing[3::8]] = props[passing[2::8]]
    scores = np.zeros((R, 1), np.float32)
    scores[passing, 0] = 1.0 - ((np.arange(8192) + 1) * 5 % 8192) * 2.0 ** -14         # (distinct; row 16 382 has the best)
    out.append(make_case("limit_rows", "limits", [R], 1, props, scores, topk=LDS_CAP,
                         marks={"candidates": [8192], "survivors": [7168], "last_row": R - 1, "nq4": True}))
    # K + 1 around the 256-column tile of the count / emit kernels and K around the 1 024-class step of the scan; rows around the
    # 64-row chunk
    for K in (255, 256, 257, 1023, 1024, 1025):
        rng = np.random.default_rng(K)
        sizes = [65, 63, 64]
        R = sum(sizes)
        scores = np.where(rng.random((R, K)) < 0.08, rng.integers(9, 64, (R, K)) / 64.0, 0.0).astype(np.float32)
        scores[:, K - 1] = np.where(np.arange(R) % 3 == 0, 1.0, scores[:, K - 1])       # (the last class leads the output)
        scores[64, :] = np.maximum(scores[64, :], 0.25)                  # row 64 of image 0: a candidate of every class
        out.append(make_case(f"limit_K{K}", "limits", sizes, K, grid_boxes(rng, R, 0, 1300, crowd=30), scores, score_thresh=0.125,
                             topk=LDS_CAP, marks={"last_class": K - 1}))
    return out


# ---- the LDS pipeline's capacity -----------------------------------------------------------------------------------------------------

def _capacity():
    out = []
    for n in (LDS_CAP - 1, LDS_CAP, LDS_CAP + 1):
        rng = np.random.default_rng(6)
        sizes, K = [10, 130], 64
        R = sum(sizes)
        scores = np.zeros((R, K), np.float32)
        scores[:10] = rng.integers(0, 64, (10, K)) / 64.0
        flat = rng.permutation(130 * K)[:n]
        scores[10:].reshape(-1)[flat] = rng.integers(5, 64, n) / 64.0
        out.append(make_case(f"capacity_{n}", "capacity", sizes, K, grid_boxes(rng, R, 0, 1300, crowd=50), scores, score_thresh=0.0625,
                             topk=LDS_CAP, marks={"candidates": [None, n], "overflow": n > LDS_CAP}, mid=4000))
    return out


# ---- the wide pipeline's radix select: pairwise disjoint boxes, every candidate survives ------------------------------------------

def _select_case(name, R, K, topk, scores, passes, winners, size=16):
    marks = {"survivors": [R * K], "passes": [passes], "winners": [winners], "overflow": True}
    return make_case(name, "select", [R], K, cells(R, size), scores, topk=topk, marks=marks)


def _select():
    tie = lambda R, K: np.full((R, K), 0.5, np.float32)
    out = [
        _select_case("select_300x80", 300, 80, 100, tie(300, 80), 4, 320),
        _select_case("select_8x5000", 8, 5000, 300, tie(8, 5000), 5, 320),
        _select_case("select_5x4000", 5, 4000, 300, tie(5, 4000), 4, 16000),
        _select_case("select_129x128", 129, 128, 300, tie(129, 128), 4, 512),
        _select_case("select_128x128_full_sort", 128, 128, 300, tie(128, 128), 0, 16384),
        _select_case("select_4x4097", 4, 4097, LDS_CAP, tie(4, 4097), 5, 8193),
    ]
    # 250 distinct high scores (the first 250 (row, class) pairs), then ties
    s = tie(250, 121)
    s.reshape(-1)[:250] = 0.75 + ((np.arange(250) * 37) % 250) * 2.0 ** -10
    out.append(_select_case("select_250x121_distinct_then_ties", 250, 121, 300, s, 4, 484))
    # distinct scores: 24 000 values 1 - j 2^-18 share their upper 11 key bits and split on the next 11 (16 to a bin); spread over
    # [1/16, 1) the first pass ends the select
    j = (np.arange(300 * 80) * 7919 % 24000).reshape(300, 80)
    out.append(_select_case("select_distinct_pass2", 300, 80, 100, (1.0 - (j + 1) * 2.0 ** -18).astype(np.float32), 2, 112))
    out.append(_select_case("select_distinct_pass1", 300, 80, 100, (1.0 - (j + 1) * 2.0 ** -15).astype(np.float32), 1, 4096))
    # scores that differ in their low 10 bits only (a score per row): the third pass splits them
    s = np.repeat((0.5 + (np.arange(300) * 7 % 300) * 2.0 ** -24).astype(np.float32)[:, None], 80, axis=1)
    out.append(_select_case("select_low_score_bits_pass3", 300, 80, 100, s, 3, 160))
    # a batch where only image 1 needs the select
    sizes, K = [100, 300], 80
    batch = make_case("select_one_image_of_two", "select", sizes, K, np.concatenate([cells(100), cells(300)]), tie(400, K), topk=100,
                      marks={"survivors": [8000, 24000], "passes": [0, 4], "winners": [8000, 320], "overflow": True}, mid=10000)
    out.append(batch)
    return out


# ---- the sweep beyond 4 096 rows ------------------------------------------------------------------------------------------------------

def sweep_case(name, n_a, n_b1, n_third, n_b2, nq4):
    """K = 2, R = 2 (n_a + n_b1 + n_b2) + 1 + n_third rows on disjoint 16 x 16 cells, in row order: n_a cells with two rows each
    (rows 2c, 2c + 1), ONE row with a cell of its own, n_b1 cells with two rows each, n_third rows that repeat the cells
    0 .. n_third - 1 a third time, n_b2 cells with two rows each.  Scores 1 - j 2^-14 with j the row in class 0 and the reversed row
    in class 1.  Class 0: a cell's two rows are neighbours in score order and the first is kept -- the even positions up to the
    single row, the odd ones behind it, so the kept set does not repeat with the period of the 4 096 positions one sweep register
    spans --, and a third copy sits far behind its suppressor.  Class 1: the third copies come first and suppress two rows that far
    behind them, and the kept set by row differs from the one by position."""
    pairs = lambda first, n: first + np.arange(2 * n) // 2
    cell = np.r_[pairs(0, n_a), n_a, pairs(n_a + 1, n_b1), np.arange(n_third), pairs(n_a + 1 + n_b1, n_b2)]
    R, n_cells = len(cell), n_a + 1 + n_b1 + n_b2
    props = cells(n_cells)[cell]
    j = np.arange(R)
    scores = np.stack([1.0 - j * 2.0 ** -14, 1.0 - (R - 1 - j) * 2.0 ** -14], axis=1).astype(np.float32)
    marks = {"candidates": [2 * R], "survivors": [2 * n_cells], "kept_span": R - 2, "far_suppressor": 2 * (n_a + n_b1) + 1 - (n_third - 1),
             "overflow": 2 * R > LDS_CAP}
    if nq4:
        marks["nq4"] = True
    return make_case(name, "sweep", [R], 2, props, scores, topk=LDS_CAP, marks=marks)      # (every survivor is output)


def _sweep():
    """R = 8 200: 2 048 cells twice (rows 0 .. 4 095), the single row 4 096, 950 cells twice, 51 third copies (rows 5 997 .. 6 047),
    1 076 cells twice: 4 075 of the image's 4 150 cells.  The sibling of the same generator with R = 520 is the one the CPU chain is
    compared on; the second R = 8 200 case has the image in a batch behind a small one, so the sweep's segment and matrix bases are
    not zero."""
    big = sweep_case("sweep_8200", 2048, 950, 51, 1076, True)
    small = sweep_case("sweep_520_sibling", 128, 60, 11, 66, False)
    assert big["sizes"] == [8200] and small["sizes"] == [520]
    rng = np.random.default_rng(8)
    head = make_case("head", "sweep", [40], 2, grid_boxes(rng, 40, crowd=7), rng.integers(0, 16, (40, 2)) / 16.0)
    both = []
    for tag, c in (("sweep_8200_second_image", big), ("sweep_520_sibling_second_image", small)):
        m = dict(c["marks"])
        for key in ("candidates", "survivors"):
            m[key] = [None] + m[key]
        both.append(make_case(tag, "sweep", [40] + c["sizes"], 2, np.concatenate([head["props"], c["props"]]),
                              np.concatenate([head["probs"][:, :2], c["probs"][:, :2]]), topk=LDS_CAP, marks=m, mid=1000))
    return [big, small] + both


# ---- class-specific regression ---------------------------------------------------------------------------------------------------------

def _cs_deltas(props, targets):
    """deltas [R, 4K] that move proposal r (width and height a power of two) to targets[r, k] (top-left corners, integers)."""
    R, K = targets.shape[:2]
    w, h = props[:, 2] - props[:, 0], props[:, 3] - props[:, 1]
    d = np.zeros((R, K, 4), np.float32)
    d[:, :, 0] = (targets[:, :, 0] - props[:, None, 0]) / w[:, None]
    d[:, :, 1] = (targets[:, :, 1] - props[:, None, 1]) / h[:, None]
    return d.reshape(R, 4 * K)


def _cs():
    out = []
    # rows that overlap in class 0 (all moved onto two spots) and are disjoint in class 1 (left where they are), nudged in class 2
    R, K = 12, 3
    props = cells(R, size=64)
    t = np.zeros((R, K, 2), np.float32)
    t[:, 0] = np.stack([100 + 8 * (np.arange(R) % 2) + 600 * (np.arange(R) % 3 == 0), np.full(R, 200)], axis=1)
    t[:, 1] = props[:, :2]
    t[:, 2] = props[:, :2] + np.stack([24 * (np.arange(R) % 2), -np.arange(R)], axis=1)       # (some leave the image at the top)
    scores = (0.25 + ((np.arange(R)[:, None] * 5 + np.arange(K)[None, :] * 3) % 11) * 2.0 ** -6).astype(np.float32)
    out.append(make_case("cs_small", "class_specific", [R], K, props, scores, deltas=_cs_deltas(props, t), score_thresh=0.25,
                         marks={"cs_differs": True}))
    # class 0: 400 boxes of 32 x 32 sliding by 8 along four lines (neighbours: IoU 0.6, next-but-one 1/3), in a seeded score order;
    # class 1: the proposals where they are, disjoint.  An image of its own in a batch behind cs_small's rows.
    R2, K2 = 400, 2
    props2 = cells(R2, size=32)
    i = np.arange(R2)
    t2 = np.zeros((R2, K2, 2), np.float32)
    t2[:, 0] = np.stack([8 * (i % 100), 100 * (i // 100)], axis=1)
    t2[:, 1] = props2[:, :2]
    order = np.random.default_rng(9).permutation(R2)
    scores2 = np.zeros((R2, K2), np.float32)
    scores2[order, 0] = 1.0 - i * 2.0 ** -12
    scores2[::7, 1] = 0.5
    out.append(make_case("cs_sweep", "class_specific", [R2], K2, props2, scores2, deltas=_cs_deltas(props2, t2), topk=300,
                         marks={"cs_sweep": 0}))
    return out


@functools.lru_cache(maxsize=None)
def _all():
    cases = (_threshold_edge() + _iou_edge() + _zero_area() + _chain() + _ties_topk() + _ragged() + _limits() + _capacity() + _select()
             + _sweep() + _cs())
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return {c["name"]: c for c in cases}


def names():
    return list(_all())


def get(name):
    return _all()[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference of a case, computed once and shared (read-only) by the tests that need it."""
    return ref.reference(get(name))


def candidate_counts(name):
    return [r["n_candidates"] for r in reference(name)]


def class_specific(case):
    return case["deltas"].shape[1] > 4


def largest_nms_call(case, per_class):
    """The boxes of the largest single NMS call the torch chain makes on the case with every image on the given branch (from the
    inputs alone: the candidates of an image, or of one class of an image)."""
    hit = case["probs"][:, :case["K"]] > np.float32(case["score_thresh"])
    ends = np.cumsum(case["sizes"])
    per_image = [hit[e - n:e] for n, e in zip(case["sizes"], ends)]
    if per_class:
        return max(int(h.sum(axis=0).max(initial=0)) for h in per_image)
    return max(int(h.sum()) for h in per_image)


def nonempty_classes(case):
    """The most classes with a candidate in one image: the per-class branch of the torch chain makes that many NMS calls."""
    hit = case["probs"][:, :case["K"]] > np.float32(case["score_thresh"])
    ends = np.cumsum(case["sizes"])
    return max(int(hit[e - n:e].any(axis=0).sum()) for n, e in zip(case["sizes"], ends))


# ---- the conditions ---------------------------------------------------------------------------------------------------------------------

def _is_dyadic(v, bits=24):
    return float(v) * 2 ** bits == int(float(v) * 2 ** bits) and float(np.float32(v)) == float(v)


def _f32_exact(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


def check_conditions(case):
    """The exactness conditions of the module docstring and every mark of the case; raises AssertionError."""
    name, K, marks = case["name"], case["K"], case["marks"]
    # integer proposals in range, unit weights, dw = dh = 0, dyadic thresholds
    props = case["props"].astype(np.float64)
    assert np.array_equal(props, np.round(props)) and props.min() >= -64 and props.max() <= 2047, name
    assert tuple(case["weights"]) == (1.0, 1.0, 1.0, 1.0), name
    d = case["deltas"].reshape(len(props), -1, 4)
    assert not d[:, :, 2:].any(), name
    assert case["nms_thresh"] in (0.5, 0.25, 0.75) and _is_dyadic(case["score_thresh"]) and case["score_thresh"] >= 0, name
    moved = d[:, :, :2].any(axis=(1, 2))
    for side in (props[moved, 2] - props[moved, 0], props[moved, 3] - props[moved, 1]):
        assert np.all(side > 0) and np.all(np.log2(side) == np.round(np.log2(side))), f"{name}: a moved proposal's side is no power of two"
    # every step of the decoding is exact in fp32 and every decoded, clipped coordinate an integer
    steps = ref.decode_steps(case)
    for key, v in steps.items():
        assert _f32_exact(v), f"{name}: {key} is not exact in fp32"
    boxes = steps["boxes"]
    assert np.array_equal(boxes, np.round(boxes)) and np.array_equal(steps["raw"], np.round(steps["raw"])), name
    assert np.array_equal(steps["mx"], np.round(steps["mx"])) and np.array_equal(steps["my"], np.round(steps["my"])), name
    assert np.all(np.isfinite(case["probs"])) and case["probs"].min() >= 0 and case["probs"].max() <= 1, name
    # the shift of batched_nms stays exact: K * (max + 1) + max < 2^24 per image, max over the candidates' boxes
    res = reference(name) if name in _all() and _all()[name] is case else ref.reference(case)
    r0 = 0
    for n_rows, out in zip(case["sizes"], res):
        p = case["probs"][r0:r0 + n_rows, :K]
        rows, cls = np.nonzero(p > np.float32(case["score_thresh"]))
        if len(rows):
            cb = boxes[r0 + rows, cls if boxes.shape[1] > 1 else 0]
            assert K * (cb.max() + 1) + cb.max() < 2 ** 24, f"{name}: the class shift leaves the exact integers"
        assert len(rows) == out["n_candidates"]
        r0 += n_rows
    assert len(case["sizes"]) <= 64 and max(case["sizes"]) < 1 << ref.ROW_BITS and K < 1 << ref.CLS_BITS and 1 <= case["topk"] <= LDS_CAP
    if case["mid"] is not None:
        cand = [x["n_candidates"] for x in res]
        assert min(cand) < case["mid"] <= max(cand), f"{name}: mid {case['mid']} is not between two images' candidate counts {cand}"

    # outside the select and the top-k cases every NMS survivor is output, so that no decision of the sweep hides behind the top-k
    if case["group"] != "select" and "tie_cut" not in marks:
        assert all(len(x["survivor_keys"]) <= case["topk"] for x in res), f"{name}: the top-k cuts survivors"

    # ---- marks
    for key in ("candidates", "survivors"):
        for want, out in zip(marks.get(key, []), res):
            got = out["n_candidates"] if key == "candidates" else len(out["survivor_keys"])
            assert want is None or got == want, f"{name}: {key} {got}, meant {want}"
    if "passes" in marks:
        got = [ref.select_passes(out["survivor_keys"], case["topk"]) for out in res]
        assert [g[0] for g in got] == marks["passes"] and [g[1] for g in got] == marks["winners"], f"{name}: select {got}"
    over = any(x["n_candidates"] > LDS_CAP for x in res)
    assert over == bool(marks.get("overflow", False)), f"{name}: overflow {over}"
    assert (max(case["sizes"]) > SWEEP_ROWS) == bool(marks.get("nq4", False)), name
    if "last_class" in marks:
        assert any(marks["last_class"] in x["per_class"] for x in res) and marks["last_class"] == K - 1, name
        assert any(marks["last_class"] in x["classes"] for x in res), name
    if "last_row" in marks:
        assert marks["last_row"] == case["sizes"][0] - 1 and marks["last_row"] in res[0]["rows"], name
    if marks.get("threshold_edge"):
        thr = np.float32(case["score_thresh"])
        p = case["probs"][:, :K]
        for v, passes in ((thr, False), (ulp(thr, True), True), (ulp(thr, False), False)):
            assert (p == v).sum() >= 10, name
            assert passes or v not in res[0]["scores"], name
        assert ulp(thr, True) in np.concatenate([x["scores"] for x in res]), f"{name}: no detection one ulp above the threshold"
        assert min(x["scores"].min() for x in res) > thr
    if "iou_edge" in marks:
        num = marks["iou_edge"]                                                  # threshold num / 4: sign of 4 inter - num union
        signs, b = set(), boxes[:, 0]
        for a in range(0, len(b), 2):
            inter, union = ref.iou_parts(b[a], b[a + 1:a + 2])
            margin = int(4 * inter[0] - num * union[0])
            signs.add((margin > 0) - (margin < 0))
            assert abs(margin) <= 4, f"{name}: pair {a} is not next to the threshold ({margin})"
            for c in (0, 1):                                                     # the pair's later box goes iff the ratio is above
                first, second = (a, a + 1) if c == 0 else (a + 1, a)
                kept = set(res[0]["rows"][res[0]["classes"] == c].tolist())
                assert first in kept and (second in kept) == (margin <= 0), name
        assert signs == {-1, 0, 1}, name
    if marks.get("zero_area"):
        b = boxes[:, 0]
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        zero = np.flatnonzero(area == 0)
        dup = sum(1 for i in zero for j in zero if i < j and np.array_equal(b[i], b[j]))
        assert len(zero) >= 8 and dup >= 4 and (props[zero, 2] - props[zero, 0] > 0).sum() >= 5, name
        big = np.flatnonzero(area == area.max())[0]
        inside = [i for i in zero if b[i, 0] >= b[big, 0] and b[i, 2] <= b[big, 2] and b[i, 1] >= b[big, 1] and b[i, 3] <= b[big, 3]]
        assert len(inside) >= 3 and set(zero.tolist()) <= set(res[0]["rows"].tolist()), name
    if "alternate" in marks:
        assert sorted(res[0]["rows"].tolist()) == sorted(marks["alternate"]) and len(res[0]["rows"]) == 100, name
        sup = res[0]["suppressors"][0]
        assert np.array_equal(np.flatnonzero(sup < 0), np.arange(0, 200, 2)) and sup[63] == 62 and sup[65] == 64 and sup[127] == 126, name
    if "tie_cut" in marks:
        s, k = len(res[0]["survivor_keys"]), marks["tie_cut"]
        assert len(res[0]["rows"]) == k == min(case["topk"], s) and len(np.unique(res[0]["scores"])) <= 1, name
        order = list(zip(res[0]["rows"].tolist(), res[0]["classes"].tolist()))
        assert order == sorted(order), name
    if "kept_span" in marks:
        out = res[-1]
        kept0 = np.flatnonzero(out["suppressors"][0] < 0)
        assert kept0.max() == marks["kept_span"] and kept0.min() == 0, name
        far = marks["far_suppressor"]
        for c in (0, 1):
            sup = out["suppressors"][c]
            pos = np.arange(len(sup))
            gap = np.where(sup >= 0, pos - sup, 0)
            assert gap.max() >= far, f"{name}: class {c}: the farthest suppressor is {gap.max()} positions away, meant {far}"
            if marks.get("nq4"):
                # a suppressor past 4 096 positions away, and the kept set (by position: the shifted branch; by row: the per-class
                # one) must not repeat 4 096 lower, or a sweep that folds its kept words onto one register would still be right
                assert gap.max() > SWEEP_ROWS, name
                kept_pos = sup < 0
                high = (sup >= SWEEP_ROWS) & (gap == 1)
                assert (high & ~kept_pos[np.maximum(sup - SWEEP_ROWS, 0)]).sum() >= 100, f"{name}: class {c}: the kept positions repeat"
                row_of = pos if c == 0 else len(sup) - 1 - pos
                kept_row = np.zeros(len(sup), bool)
                kept_row[row_of[kept_pos]] = True
                sup_row = row_of[np.maximum(sup, 0)]
                high = (sup >= 0) & (sup_row >= SWEEP_ROWS) & (gap == 1)
                assert (high & ~kept_row[np.maximum(sup_row - SWEEP_ROWS, 0)]).sum() >= 100, f"{name}: class {c}: the kept rows repeat"
        R = case["sizes"][-1]
        keys = out["survivor_keys"]
        keys1 = keys[(keys & np.uint64(1)) == 1]
        rows1 = np.sort(((keys1 >> np.uint64(ref.CLS_BITS)) & np.uint64((1 << ref.ROW_BITS) - 1)).astype(np.int64))
        pos1 = np.flatnonzero(out["suppressors"][1] < 0)
        assert np.array_equal(np.sort(R - 1 - rows1), pos1) and not np.array_equal(rows1, pos1), f"{name}: class 1 by row = by position"
    if "cs_sweep" in marks:
        c = marks["cs_sweep"]
        n, s = res[0]["per_class"][c]
        sup = res[0]["suppressors"][c]
        pos = np.arange(n)
        assert n == 400 and s > 128, f"{name}: {n} candidates, {s} survivors"
        assert ((sup >= 0) & (sup // 64 < pos // 64)).sum() >= 20, f"{name}: no suppression by an earlier step's survivor"
        assert ((sup >= 0) & (sup // 64 == pos // 64)).sum() >= 20, f"{name}: no suppression inside a step"
    if marks.get("cs_differs"):
        assert class_specific(case) and boxes.shape[1] == K
        n0, s0 = res[0]["per_class"][0]
        n1, s1 = res[0]["per_class"][1]
        assert s0 < n0 and s1 == n1 > 4, f"{name}: class 0 {n0}->{s0}, class 1 {n1}->{s1}"
        assert (steps["raw"] != boxes).any(), f"{name}: no decoded box is clipped"
