"""A literal loop restatement of the COCO box-AP protocol (COCOeval with iouType="bbox", useCats=1), shaped like its evaluateImg /
accumulate / summarize and written independently of locov_amd/evaluation.py: dicts and Python loops, no CSR, no two-pass form.

evaluate(gt, dets, max_dets): gt is a COCO-format dict; dets a list of (image_id, contiguous class, score, [x1, y1, x2, y2]) with
fp32 boxes.  -> {"precision" [T,R,K,A,M], "recall" [T,K,A,M], "scores" [T,R,K,A,M], "stats" [12]} in float64."""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0., 1., 101)
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]


def _iou(d, g, crowd):
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


def _evaluate_img(gts, dts, a_rng, max_det):
    """One (image, category) cell in one area range; dts already sorted by descending score and cut to maxDets[-1]."""
    if len(gts) == 0 and len(dts) == 0:
        return None
    g_ignore = [1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gts]
    gtind = sorted(range(len(gts)), key=lambda i: g_ignore[i])                 # (sorted() is stable)
    gts = [gts[i] for i in gtind]
    gt_ig = [g_ignore[i] for i in gtind]
    dts = dts[:max_det]
    T, G, D = len(IOU_THRS), len(gts), len(dts)
    ious = [[_iou(d["bbox"], g["bbox"], g["iscrowd"]) for g in gts] for d in dts]
    gtm = np.zeros((T, G), dtype=bool)
    dtm = np.zeros((T, D), dtype=bool)
    dt_ig = np.zeros((T, D), dtype=bool)
    for tind, t in enumerate(IOU_THRS):
        for dind in range(D):
            iou = min(t, 1 - 1e-10)
            m = -1
            for gind in range(G):
                if gtm[tind, gind] and not gts[gind]["iscrowd"]:
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
            dtm[tind, dind] = True
            gtm[tind, m] = True
    out = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dts], dtype=bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(~dtm, np.repeat(out, T, 0)))
    return dict(dtm=dtm, dt_ig=dt_ig, gt_ig=np.array(gt_ig), scores=[d["score"] for d in dts])


def evaluate(gt, dets, max_dets=(1, 10, 100)):
    img_ids = sorted({im["id"] for im in gt["images"]})
    cat_ids = sorted(c["id"] for c in gt["categories"])
    gts, dts = {}, {}
    for a in gt["annotations"]:
        g = dict(bbox=[float(v) for v in a["bbox"]], area=float(a["area"]), iscrowd=int(a.get("iscrowd", 0)))
        g["ignore"] = g["iscrowd"]
        gts.setdefault((a["image_id"], a["category_id"]), []).append(g)
    for image_id, c, score, box in dets:
        b = np.asarray(box, dtype=np.float32)
        xywh = [float(b[0]), float(b[1]), float(np.float32(b[2] - b[0])), float(np.float32(b[3] - b[1]))]
        dts.setdefault((image_id, cat_ids[c]), []).append(dict(bbox=xywh, area=xywh[2] * xywh[3], score=float(score)))
    max_det = max_dets[-1]
    eval_imgs = {}
    for cat in cat_ids:
        for a_ind, a_rng in enumerate(AREA_RNG):
            for img in img_ids:
                d = dts.get((img, cat), [])
                d = [d[i] for i in np.argsort([-x["score"] for x in d], kind="mergesort")][:max_det]
                eval_imgs[cat, a_ind, img] = _evaluate_img(gts.get((img, cat), []), d, a_rng, max_det)

    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNG), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k, cat in enumerate(cat_ids):
        for a in range(A):
            for m, cap in enumerate(max_dets):
                E = [eval_imgs[cat, a, img] for img in img_ids]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["scores"][0:cap] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dt_sorted = dt_scores[inds]
                dtm = np.concatenate([e["dtm"][:, 0:cap] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ig"][:, 0:cap] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gt_ig"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q, ss = np.zeros((R,)), np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds2 = np.searchsorted(rc, REC_THRS, side="left")
                    try:
                        for ri, pi in enumerate(inds2):
                            q[ri] = pr[pi]
                            ss[ri] = dt_sorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)

    def summarize(ap, t=None, a=0, m=M - 1):
        if m >= M:
            return -1.0
        s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
        if t is not None:
            s = s[t:t + 1]
        s = s[s > -1]
        return -1.0 if len(s) == 0 else float(np.mean(s))

    stats = np.array([summarize(1), summarize(1, t=0), summarize(1, t=5), summarize(1, a=1), summarize(1, a=2), summarize(1, a=3),
                      summarize(0, m=0), summarize(0, m=1), summarize(0, m=2), summarize(0, a=1), summarize(0, a=2), summarize(0, a=3)])
    return dict(precision=precision, recall=recall, scores=scores, stats=stats)
