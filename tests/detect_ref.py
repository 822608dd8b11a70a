"""A float64 reference of the detection post-processing (locov_amd/csrc/detect.hip, detect_wide.hip; the torch chain of
locov_amd/roi_heads/box_emb_head.py: apply_deltas, Boxes.clip, `prob > thr` over the K foreground columns, class-wise greedy NMS,
merge by (descending score, row, class), top-k) and a host mirror of the wide pipeline's radix select.  numpy only.

The reference is the operation itself, not a restatement of a kernel: per class one greedy sweep in (descending score, row) order
on the UNSHIFTED boxes, an IoU of 0/0 suppressing nothing.  On the inputs of tests/detect_cases.py (integer boxes, dyadic
thresholds: see that file) fp32 arithmetic makes no rounding error, so both of batched_nms's branches -- the class-shifted boxes
and the per-class loop -- have to agree with it bit for bit.

A case is a dict (tests/detect_cases.py builds them): sizes (rows per image), K, props [R,4] float32, deltas [R,4] or [R,4K] float32,
probs [R,K+1] float32 (the last column is the background's), image_shapes [(height, width)], weights, score_thresh, nms_thresh, topk.
"""
import numpy as np

SCALE_CLAMP = float(np.log(1000.0 / 16))

# csrc/detect_wide.hip: merge keys  ~score << 29 | row << 15 | class, 61 bits; the radix select takes 11 bits a pass, the last pass 6
ROW_BITS, CLS_BITS, KEY_BITS = 14, 15, 61
DIGIT, PASSES, SELECT_CAP = 11, 6, 16384


def decode_steps(case):
    """Box2BoxTransform.apply_deltas + Boxes.clip in float64, every intermediate kept: a dict of arrays.  `boxes` is [R, bk, 4]
    (bk = 1 for class-agnostic deltas, K for [R, 4K]), clipped to the image of each row."""
    props = np.asarray(case["props"], np.float64)
    R, K = len(props), case["K"]
    d = np.asarray(case["deltas"], np.float64).reshape(R, -1, 4)
    wx, wy, ww, wh = (float(np.float32(1.0) / np.float32(w)) for w in case["weights"])       # (the chain multiplies by 1 / w)
    widths, heights = props[:, 2] - props[:, 0], props[:, 3] - props[:, 1]
    ctr_x, ctr_y = props[:, 0] + 0.5 * widths, props[:, 1] + 0.5 * heights
    dx, dy = d[:, :, 0] * wx, d[:, :, 1] * wy
    dw, dh = np.minimum(d[:, :, 2] * ww, SCALE_CLAMP), np.minimum(d[:, :, 3] * wh, SCALE_CLAMP)
    mx, my = dx * widths[:, None], dy * heights[:, None]
    pcx, pcy = mx + ctr_x[:, None], my + ctr_y[:, None]
    pw, ph = np.exp(dw) * widths[:, None], np.exp(dh) * heights[:, None]
    raw = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], axis=-1)
    lim = np.zeros((R, 2))
    r0 = 0
    for n, (h, w) in zip(case["sizes"], case["image_shapes"]):
        lim[r0:r0 + n] = (w, h)
        r0 += n
    boxes = raw.copy()
    for a in range(4):
        boxes[:, :, a] = np.minimum(np.maximum(raw[:, :, a], 0.0), lim[:, None, a & 1])
    assert boxes.shape[1] in (1, K)
    return dict(widths=widths, heights=heights, ctr_x=ctr_x, ctr_y=ctr_y, dx=dx, dy=dy, dw=dw, dh=dh, mx=mx, my=my, pcx=pcx, pcy=pcy,
                pw=pw, ph=ph, raw=raw, boxes=boxes)


def iou_parts(a, b):
    """(intersection, union) of box a [4] with the boxes b [m, 4], float64."""
    w = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), 0.0)
    h = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), 0.0)
    inter = w * h
    return inter, (a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter


def greedy_nms(boxes, thr):
    """The greedy sweep over boxes [m, 4] that are already in their order.  Returns (kept positions, suppressor [m]: the position of
    the kept box that suppressed a position, -1 for a kept one).  IoU > thr suppresses; 0/0 is NaN and suppresses nothing."""
    m = len(boxes)
    sup = np.full(m, -1, np.int64)
    kept = []
    for i in range(m):
        if sup[i] >= 0:
            continue
        kept.append(i)
        if i + 1 < m:
            inter, union = iou_parts(boxes[i], boxes[i + 1:])
            with np.errstate(divide="ignore", invalid="ignore"):
                hit = (inter / union > thr) & (sup[i + 1:] < 0)
            sup[i + 1:][hit] = i
    return np.asarray(kept, np.int64), sup


def merge_keys(scores, rows, classes):
    """The wide pipeline's merge keys of (float32 score, row, class): ascending key = (descending score, row, class) for scores > 0."""
    bits = (~np.ascontiguousarray(scores, np.float32).view(np.uint32)).astype(np.uint64)
    return (bits << np.uint64(ROW_BITS + CLS_BITS)) | (np.asarray(rows, np.uint64) << np.uint64(CLS_BITS)) | np.asarray(classes, np.uint64)


def reference(case):
    """Per image a dict: rows, classes (int64), scores (float32), boxes (float32 [n, 4]) of the detections in output order, and what
    the conditions of a case are checked from: n_candidates, per_class ({class: (candidates, survivors)}), survivor_keys (the merge
    keys of every NMS survivor, before the top-k), suppressors ({class: the suppressor array of greedy_nms})."""
    boxes_all = decode_steps(case)["boxes"]
    K, thr, nms_thr, topk = case["K"], float(np.float32(case["score_thresh"])), float(np.float32(case["nms_thresh"])), case["topk"]
    probs = np.asarray(case["probs"], np.float32)
    out, r0 = [], 0
    for n_rows in case["sizes"]:
        p = probs[r0:r0 + n_rows, :K]
        boxes = boxes_all[r0:r0 + n_rows]
        r0 += n_rows
        rows, cls = np.nonzero(p.astype(np.float64) > thr)
        sc = p[rows, cls]
        order = np.lexsort((rows, -sc.astype(np.float64), cls))               # class-major; descending score, ties by row
        rows, cls, sc = rows[order], cls[order], sc[order]
        cand_box = boxes[rows, cls if boxes.shape[1] > 1 else 0]
        starts = np.flatnonzero(np.r_[True, cls[1:] != cls[:-1]]) if len(cls) else np.zeros(0, np.int64)
        ends = np.r_[starts[1:], len(cls)]
        keep, per_class, suppressors = [], {}, {}
        for s, e in zip(starts, ends):
            if e - s == 1:
                k, sup = np.zeros(1, np.int64), np.full(1, -1, np.int64)
            else:
                k, sup = greedy_nms(cand_box[s:e], nms_thr)
            keep.append(s + k)
            per_class[int(cls[s])] = (int(e - s), len(k))
            suppressors[int(cls[s])] = sup
        keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
        rows_k, cls_k, sc_k, box_k = rows[keep], cls[keep], sc[keep], cand_box[keep]
        merge = np.lexsort((cls_k, rows_k, -sc_k.astype(np.float64)))[:topk]
        out.append(dict(rows=rows_k[merge].astype(np.int64), classes=cls_k[merge].astype(np.int64), scores=sc_k[merge].astype(np.float32),
                        boxes=box_k[merge].astype(np.float32).reshape(-1, 4), n_candidates=len(rows), per_class=per_class,
                        survivor_keys=merge_keys(sc_k, rows_k, cls_k), suppressors=suppressors))
    return out


def select_passes(keys, topk):
    """Host mirror of dw_select_kernel over the merge keys of one image's survivors.  Returns (passes run, winners): (0, len(keys))
    when the select does not run (at most SELECT_CAP survivors: the last launch sorts them all).  A pass takes the next digit of the
    keys under the prefix, finds the bin of the min(topk, n)-th key, and stops as soon as the keys below the prefix plus that bin's
    number at most SELECT_CAP; the winners are the keys below (prefix, bin + 1)."""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    if n <= SELECT_CAP:
        return 0, n
    assert int(keys.max()) < 1 << KEY_BITS and topk >= 1
    pre, below, k = 0, 0, min(topk, n)
    for p in range(PASSES):
        lo = KEY_BITS - DIGIT * (p + 1) if p < PASSES - 1 else 0
        nd = DIGIT if p < PASSES - 1 else KEY_BITS - DIGIT * (PASSES - 1)
        under = keys[(keys >> np.uint64(lo + nd)) == np.uint64(pre)]
        hist = np.bincount(((under >> np.uint64(lo)) & np.uint64((1 << nd) - 1)).astype(np.int64), minlength=1 << nd)
        cum = np.cumsum(hist)
        need = k - below
        b = int(np.searchsorted(cum, need))                                   # the first bin with cum >= need
        before = int(cum[b] - hist[b])
        new_pre = (pre << nd) | b
        if below + before + int(hist[b]) <= SELECT_CAP:
            thresh = (new_pre + 1) << lo
            return p + 1, int((keys < np.uint64(thresh)).sum()) if thresh < 1 << 64 else n
        pre, below = new_pre, below + before
    raise AssertionError("the select did not end: a last-pass bin holds one key")
