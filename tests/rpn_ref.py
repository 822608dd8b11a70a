"""The RPN's proposal generation of one feature level (include/locov_hip.h, a-10d) in float64, numpy only: the operation itself, one
box at a time, not a restatement of the kernels.  On the inputs of tests/rpn_cases.py fp32 arithmetic makes no rounding error, so
the kernels and the torch chain must equal this bit for bit.

proposals(...) returns one record per image with the outputs (boxes, logits, index, count: the first post_nms_topk survivors) and
the facts a case's conditions are checked from:
  selected     the anchor indices in selection order (descending logit, -0 == +0, then ascending index), P = min(HWA, pre) of them
  cut_logit    the logit at position P - 1            next_logit   the logit the cut left out (None when P == HWA)
  nonfinite    a selected logit or decoded box is inf / NaN as an fp32 value (before the clip)
  filtered     selection positions dropped by the size filter
  suppressor   per selection position: the position of the kept box that suppressed it, -1 for a kept box, -2 for a filtered one
  survivors    selection positions kept by the NMS, before the slice
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def selection_order(logits):
    """Every index in descending logit order, ties (-0.0 == +0.0 among them) by ascending index."""
    v = np.asarray(logits, dtype=np.float64) + 0.0        # (-0.0 + 0.0 = +0.0)
    return sorted(range(len(v)), key=lambda i: (-v[i], i))


def apply_deltas(d, a, weights, scale_clamp):
    wx, wy, ww, wh = (float(w) for w in weights)
    w, h = a[2] - a[0], a[3] - a[1]
    cx, cy = a[0] + 0.5 * w, a[1] + 0.5 * h
    dx, dy, dw, dh = d[0] / wx, d[1] / wy, min(d[2] / ww, scale_clamp), min(d[3] / wh, scale_clamp)
    pcx, pcy = dx * w + cx, dy * h + cy
    with np.errstate(over="ignore"):
        pw, ph = np.exp(dw) * w, np.exp(dh) * h
    return np.array([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], dtype=np.float64)


def first_overlap(kept, b, thr):
    """The first row of kept [k, 4] whose IoU with box b is > thr, -1 when there is none (0 / 0 is NaN: not greater)."""
    if len(kept) == 0:
        return -1
    w = np.maximum(np.minimum(kept[:, 2], b[2]) - np.maximum(kept[:, 0], b[0]), 0.0)
    h = np.maximum(np.minimum(kept[:, 3], b[3]) - np.maximum(kept[:, 1], b[1]), 0.0)
    inter = w * h
    union = (kept[:, 2] - kept[:, 0]) * (kept[:, 3] - kept[:, 1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        over = inter / union > thr
    return int(np.argmax(over)) if over.any() else -1


def proposals_one(logits, deltas, anchors, hw, weights, scale_clamp, pre, post, min_box_size, nms_thresh):
    logits = np.asarray(logits, dtype=np.float32)
    deltas64, anchors64 = np.asarray(deltas, dtype=np.float64), np.asarray(anchors, dtype=np.float64)
    order = selection_order(logits)
    P, h, w = min(len(order), int(pre)), float(hw[0]), float(hw[1])
    sel = order[:P]
    rec = {"selected": sel, "cut_logit": float(logits[sel[-1]]) if P else None,
           "next_logit": float(logits[order[P]]) if P < len(order) else None, "nonfinite": False}
    boxes, filtered, suppressor, kept = [], [], [], []
    kept_boxes = np.zeros((P, 4), dtype=np.float64)
    for p, i in enumerate(sel):
        raw = apply_deltas(deltas64[i], anchors64[i], weights, scale_clamp)
        if not (np.isfinite(logits[i]) and np.all(np.abs(raw) <= FLT_MAX)):       # (NaN compares false)
            rec["nonfinite"] = True
        b = np.array([min(max(raw[0], 0.0), w), min(max(raw[1], 0.0), h), min(max(raw[2], 0.0), w), min(max(raw[3], 0.0), h)])
        boxes.append(b)
        if not (b[2] - b[0] > min_box_size and b[3] - b[1] > min_box_size):
            filtered.append(p)
            suppressor.append(-2)
            continue
        by = first_overlap(kept_boxes[:len(kept)], b, nms_thresh)
        suppressor.append(kept[by] if by >= 0 else -1)
        if by < 0:
            kept_boxes[len(kept)] = b
            kept.append(p)
    out = kept[:int(post)]
    rec.update(filtered=filtered, suppressor=suppressor, survivors=kept, count=len(out),
               boxes=np.array([boxes[p] for p in out], dtype=np.float32).reshape(-1, 4),
               logits=np.array([logits[sel[p]] for p in out], dtype=np.float32),
               index=np.array([sel[p] for p in out], dtype=np.int64))
    return rec


def proposals(logits, deltas, anchors, image_hw, weights, scale_clamp, pre, post, min_box_size, nms_thresh):
    """logits [N, HWA], deltas [N, HWA, 4], anchors [HWA, 4], image_hw: N (h, w) pairs -> a record per image."""
    return [proposals_one(logits[n], deltas[n], anchors, image_hw[n], weights, scale_clamp, pre, post, min_box_size, nms_thresh)
            for n in range(len(logits))]
