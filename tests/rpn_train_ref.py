"""numpy reference of the RPN's training half ([D2-upstream] RPN.label_and_sample_anchors and RPN.losses), stated as the operation,
one anchor at a time -- not as the kernels of csrc/rpn_train.hip and not as the torch chain of locov_amd/proposal_generator.py.

  * IoU: single IEEE fp32 operations on fp32 inputs in torch's pairwise_iou order (np.float32 arithmetic): area products, min / max,
    the differences, clamp at 0, the product, one division by (area_a + area_b) - inter.
  * the Matcher (first maximum; every interval that holds overwrites; the low-quality promotion of every anchor whose IoU with a box
    EQUALS that box's maximum over all anchors), the image without ground truth, the boundary test, the draw from given keys.
  * the two losses and their gradients in float64.

Besides the results, every function records the facts the cases of tests/rpn_train_cases.py assert their conditions from.
"""
import numpy as np

F = np.float32


def iou_column(gt, b):
    """IoU of every ground-truth box gt [G, 4] with ONE anchor b [4], fp32 step by step."""
    gt = gt.astype(F, copy=False)
    b = b.astype(F, copy=False)
    area_a = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    w = np.minimum(gt[:, 2], b[2]) - np.maximum(gt[:, 0], b[0])
    h = np.minimum(gt[:, 3], b[3]) - np.maximum(gt[:, 1], b[1])
    w = np.where(w < 0, F(0), w)
    h = np.where(h < 0, F(0), h)
    inter = w * h
    union = (area_a + area_b) - inter
    assert inter.dtype == F and union.dtype == F
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inter > 0, inter / union, F(0)).astype(F)


def label_image(anchors, gt, image_hw, thresholds, labels_of, allow_low_quality=True, boundary_thresh=-1.0):
    """One image.  thresholds: [-inf, t1, ..., inf]; labels_of: the interval labels.  Returns a record with `labels` (int8, before
    the draw), `matched` (index into gt, 0 without ground truth), `matched_boxes` [HWA, 4] and the case facts."""
    hwa, G = anchors.shape[0], gt.shape[0]
    rec = {"n_gt": G, "promoted": 0, "promoted_other_box": 0, "tie_for_max": 0, "zero_max_boxes": 0, "outside": 0, "outside_labelled": 0}
    labels = np.zeros(hwa, dtype=np.int8)
    matched = np.zeros(hwa, dtype=np.int64)
    if G:
        iou = np.stack([iou_column(gt, anchors[i]) for i in range(hwa)], axis=1)          # [G, HWA]
        highest = iou.max(axis=1)                                                          # per box, over ALL anchors
        rec["zero_max_boxes"] = int((highest == 0).sum())
        for i in range(hwa):
            col = iou[:, i]
            j = int(np.argmax(col))                                                        # the FIRST maximum
            best = col[j]
            ml = 1
            for lab, lo, hi in zip(labels_of, thresholds[:-1], thresholds[1:]):
                if best >= F(lo) and best < F(hi):
                    ml = lab
            hits = np.nonzero(col == highest)[0]
            if allow_low_quality and hits.size:
                if ml != 1:
                    rec["promoted"] += 1
                    if j not in hits.tolist():
                        rec["promoted_other_box"] += 1
                ml = 1
            if best > 0 and int((col == best).sum()) > 1:
                rec["tie_for_max"] += 1
            labels[i], matched[i] = ml, j
    if boundary_thresh >= 0:
        h, w = image_hw
        t = boundary_thresh
        for i in range(hwa):
            b = anchors[i]
            if not (b[0] >= F(-t) and b[1] >= F(-t) and b[2] < F(w + t) and b[3] < F(h + t)):
                rec["outside"] += 1
                rec["outside_labelled"] += int(labels[i] >= 0)
                labels[i] = -1
    rec["labels"], rec["matched"] = labels, matched
    rec["matched_boxes"] = gt[matched].astype(F) if G else np.zeros((hwa, 4), dtype=F)
    rec["pop_pos"], rec["pop_neg"] = int((labels == 1).sum()), int((labels == 0).sum())
    return rec


def draw(labels, rnd_pos, rnd_neg, budget, positive_fraction):
    """subsample_labels with background label 0 from given keys: the num_pos positives of smallest rnd_pos, then the num_neg negatives
    of smallest rnd_neg; equal keys in anchor order.  Returns (final labels, record)."""
    out = np.full(labels.shape, -1, dtype=np.int8)
    max_pos = int(budget * positive_fraction)
    rec = {"max_pos": max_pos, "tie_at_cut": False}
    pos = [i for i in range(labels.size) if labels[i] == 1]
    neg = [i for i in range(labels.size) if labels[i] == 0]
    num_pos = min(len(pos), max_pos)
    num_neg = min(len(neg), budget - num_pos)
    for members, keys, k, value in ((pos, rnd_pos, num_pos, 1), (neg, rnd_neg, num_neg, 0)):
        order = sorted(members, key=lambda i: (float(keys[i]), i))
        for i in order[:k]:
            out[i] = value
        if 0 < k < len(order) and keys[order[k - 1]] == keys[order[k]]:
            rec["tie_at_cut"] = True
    rec.update(num_pos=num_pos, num_neg=num_neg, pop_pos=len(pos), pop_neg=len(neg))
    return out, rec


def label_and_sample(anchors, gt_per_image, image_hws, thresholds, labels_of, allow_low_quality, boundary_thresh, rnd, budget,
                     positive_fraction):
    """The batch: per image (final labels, matched boxes, record).  rnd [2, N, HWA] float64."""
    out = []
    for n, (gt, hw) in enumerate(zip(gt_per_image, image_hws)):
        rec = label_image(anchors, gt, hw, thresholds, labels_of, allow_low_quality, boundary_thresh)
        final, drec = draw(rec["labels"], rnd[0, n], rnd[1, n], budget, positive_fraction)
        rec.update(drec)
        rec["final"] = final
        out.append(rec)
    return out


def get_deltas64(src, tgt, weights):
    src, tgt = src.astype(np.float64), tgt.astype(np.float64)
    sw, sh = src[..., 2] - src[..., 0], src[..., 3] - src[..., 1]
    scx, scy = src[..., 0] + 0.5 * sw, src[..., 1] + 0.5 * sh
    tw, th = tgt[..., 2] - tgt[..., 0], tgt[..., 3] - tgt[..., 1]
    tcx, tcy = tgt[..., 0] + 0.5 * tw, tgt[..., 1] + 0.5 * th
    wx, wy, ww, wh = weights
    return np.stack([wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * np.log(tw / sw), wh * np.log(th / sh)], axis=-1)


def losses(logits, deltas, labels, anchors, matched_boxes, weights, beta, budget, w_cls=1.0, w_loc=1.0):
    """float64: (loss_rpn_cls, loss_rpn_loc, d loss_rpn_cls / d logits, d loss_rpn_loc / d deltas).  logits [N, HWA], deltas
    [N, HWA, 4], labels [N, HWA] (after the draw), matched_boxes [N, HWA, 4]."""
    N, hwa = labels.shape
    norm = float(budget * N)
    x = logits.astype(np.float64)
    dl, dd = np.zeros_like(x), np.zeros(deltas.shape, dtype=np.float64)
    cls = loc = 0.0
    for n in range(N):
        for i in range(hwa):
            lab = labels[n, i]
            if lab >= 0:
                v, y = x[n, i], float(lab == 1)
                cls += max(v, 0.0) - v * y + np.log1p(np.exp(-abs(v)))
                sig = 1.0 / (1.0 + np.exp(-v)) if v >= 0 else np.exp(v) / (1.0 + np.exp(v))
                dl[n, i] = (sig - y) * w_cls / norm
            if lab == 1:
                e = deltas[n, i].astype(np.float64) - get_deltas64(anchors[i], matched_boxes[n, i], weights)
                a = np.abs(e)
                if beta < 1e-5:
                    loc += a.sum()
                    dd[n, i] = np.sign(e) * w_loc / norm
                else:
                    loc += np.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta).sum()
                    dd[n, i] = np.where(a < beta, e / beta, np.sign(e)) * w_loc / norm
    return cls / norm * w_cls, loc / norm * w_loc, dl, dd
