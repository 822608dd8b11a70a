"""A literal loop restatement of the LVIS box-AP protocol, shaped like the public lvis-api's LVISResults.limit_dets_per_image and
LVISEval._prepare / _compute_iou / evaluate_img / accumulate / _summarize, and written independently of locov_amd/evaluation.py:
dicts and Python loops, no CSR, no cells, no two-pass matching.  (One stated difference from lvis-api: a match is recorded as a
flag, not as the gt's id, so a gt with id 0 counts as a match.)

evaluate(gt, dets, max_dets_per_image): gt is an LVIS-format dict; dets a list of (image_id, contiguous class, score,
[x1, y1, x2, y2]) with fp32 boxes.  -> {"precision" [T,R,K,A], "recall" [T,K,A], "stats" [13]} in float64."""
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0., 1., 101)
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]


def limit_dets_per_image(anns, max_dets):
    """LVISResults.limit_dets_per_image: per image, the first max_dets of sorted(..., key=score, reverse=True) (which is stable)."""
    img_ann = defaultdict(list)
    for ann in anns:
        img_ann[ann["image_id"]].append(ann)
    for img_id, _anns in img_ann.items():
        if len(_anns) <= max_dets:
            continue
        _anns = sorted(_anns, key=lambda ann: ann["score"], reverse=True)
        img_ann[img_id] = _anns[:max_dets]
    return [ann for anns in img_ann.values() for ann in anns]


def _iou(d, g):
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    return i / (d[2] * d[3] + g[2] * g[3] - i)


def _evaluate_img(gt, dt, area_rng, nel):
    """One (image, category) in one area range.  nel: the category is in the image's not_exhaustive_category_ids."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    g_ignore = [1 if (g["ignore"] or g["area"] < area_rng[0] or g["area"] > area_rng[1]) else 0 for g in gt]
    gt_idx = sorted(range(len(gt)), key=lambda i: g_ignore[i])                 # (sorted() is stable, like the mergesort argsort)
    gt = [gt[i] for i in gt_idx]
    gt_ig = [g_ignore[i] for i in gt_idx]
    dt_idx = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dt_idx]
    ious = [[_iou(d["bbox"], g["bbox"]) for g in gt] for d in dt]
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gt_m = np.zeros((T, G), dtype=bool)
    dt_m = np.zeros((T, D), dtype=bool)
    dt_ig = np.zeros((T, D), dtype=bool)
    for tind, t in enumerate(IOU_THRS):
        if len(ious) == 0:
            break
        for dind in range(D):
            iou = min(t, 1 - 1e-10)
            m = -1
            for gind in range(G):
                if gt_m[tind, gind]:                                           # matched already: no crowd exception
                    continue
                if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                    break
                if ious[dind][gind] < iou:
                    continue
                iou = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = gt_ig[m]
            dt_m[tind, dind] = True
            gt_m[tind, m] = True
    dt_ig_mask = np.array([d["area"] < area_rng[0] or d["area"] > area_rng[1] or nel for d in dt], dtype=bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(~dt_m, np.repeat(dt_ig_mask, T, 0)))
    return dict(dt_m=dt_m, dt_ig=dt_ig, gt_ig=np.array(gt_ig), scores=[d["score"] for d in dt])


def evaluate(gt, dets, max_dets_per_image=300):
    img_ids = sorted({im["id"] for im in gt["images"]})
    cat_ids = sorted(c["id"] for c in gt["categories"])
    K = len(cat_ids)
    anns = []
    for image_id, c, score, box in dets:
        if not 0 <= c < K:
            continue                                                           # a class outside the bank: left out first
        b = np.asarray(box, dtype=np.float32)
        xywh = [float(b[0]), float(b[1]), float(np.float32(b[2] - b[0])), float(np.float32(b[3] - b[1]))]
        anns.append(dict(image_id=image_id, category_id=cat_ids[c], bbox=xywh, area=xywh[2] * xywh[3], score=float(score)))
    anns = limit_dets_per_image(anns, max_dets_per_image)

    # _prepare
    img_nl = {im["id"]: set(im.get("neg_category_ids", ())) for im in gt["images"]}
    img_nel = {im["id"]: set(im.get("not_exhaustive_category_ids", ())) for im in gt["images"]}
    img_pl = defaultdict(set)
    gts, dts = defaultdict(list), defaultdict(list)
    for a in gt["annotations"]:
        g = dict(bbox=[float(v) for v in a["bbox"]], area=float(a["area"]), ignore=int(a.get("ignore", 0)))
        gts[a["image_id"], a["category_id"]].append(g)
        img_pl[a["image_id"]].add(a["category_id"])
    for d in anns:
        img_id, cat_id = d["image_id"], d["category_id"]
        if cat_id not in img_nl[img_id] and cat_id not in img_pl[img_id]:
            continue                                                           # neither positive nor negative for the image
        dts[img_id, cat_id].append(d)

    eval_imgs = {}
    for cat in cat_ids:
        for a_ind, a_rng in enumerate(AREA_RNG):
            for img in img_ids:
                eval_imgs[cat, a_ind, img] = _evaluate_img(gts.get((img, cat), []), dts.get((img, cat), []), a_rng, cat in img_nel[img])

    # accumulate
    T, R, A = len(IOU_THRS), len(REC_THRS), len(AREA_RNG)
    precision = -np.ones((T, R, K, A))
    recall = -np.ones((T, K, A))
    for k, cat in enumerate(cat_ids):
        for a in range(A):
            E = [eval_imgs[cat, a, img] for img in img_ids]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            dt_scores = np.concatenate([e["scores"] for e in E], axis=0)
            dt_idx = np.argsort(-dt_scores, kind="mergesort")
            dt_m = np.concatenate([e["dt_m"] for e in E], axis=1)[:, dt_idx]
            dt_ig = np.concatenate([e["dt_ig"] for e in E], axis=1)[:, dt_idx]
            gt_ig = np.concatenate([e["gt_ig"] for e in E])
            num_gt = np.count_nonzero(gt_ig == 0)
            if num_gt == 0:
                continue
            tps = np.logical_and(dt_m, np.logical_not(dt_ig))
            fps = np.logical_and(np.logical_not(dt_m), np.logical_not(dt_ig))
            tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
            fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
            for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                tp, fp = np.array(tp), np.array(fp)
                num_tp = len(tp)
                rc = tp / num_gt
                recall[t, k, a] = rc[-1] if num_tp else 0
                pr = (tp / (fp + tp + np.spacing(1))).tolist()
                for i in range(num_tp - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                rec_thrs_insert_idx = np.searchsorted(rc, REC_THRS, side="left")
                pr_at_recall = [0.0] * R
                try:
                    for _idx, pr_idx in enumerate(rec_thrs_insert_idx):
                        pr_at_recall[_idx] = pr[pr_idx]
                except IndexError:
                    pass
                precision[t, :, k, a] = np.array(pr_at_recall)

    # _summarize
    freq = {c["id"]: c.get("frequency") for c in gt["categories"]}
    freq_groups = [[k for k, cat in enumerate(cat_ids) if freq[cat] == name] for name in ("r", "c", "f")]

    def summarize(ap, iou_thr=None, a=0, freq_group_idx=None):
        if ap:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, freq_groups[freq_group_idx], a] if freq_group_idx is not None else s[:, :, :, a]
        else:
            s = recall[:, :, a]
        s = s[s > -1]
        return -1.0 if len(s) == 0 else float(np.mean(s))

    stats = np.array([summarize(1), summarize(1, iou_thr=0.5), summarize(1, iou_thr=0.75), summarize(1, a=1), summarize(1, a=2),
                      summarize(1, a=3), summarize(1, freq_group_idx=0), summarize(1, freq_group_idx=1), summarize(1, freq_group_idx=2),
                      summarize(0), summarize(0, a=1), summarize(0, a=2), summarize(0, a=3)])
    return dict(precision=precision, recall=recall, stats=stats)
