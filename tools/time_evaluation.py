"""COCOEvaluator.evaluate() / LVISEvaluator.evaluate() on the device (csrc/coco_eval.hip) against the package's host path, on
synthetic sets of COCO-val / LVIS-val size.

    timeout -k 10 900 python tools/time_evaluation.py [--protocol coco|lvis] [--images 5000] [--categories 80 1203] [--repeats 7]
                                                      [--warmup 2] [--host-repeats 2] [--proposals P] [--out records.json]

A set: `images` images, `categories` categories, 7 gts and 100 dets per image from a seed (60 dets are jittered copies of the
image's gts with their class, 40 are random boxes of random classes; 5 % of the gts are crowd; fp32 scores).  The dets are fed as
one Instances per image, on the device for the device path and on the CPU for the host path; only evaluate() is timed.

Per set: the wall time of evaluate() on the device (it ends in its one device-to-host copy, which synchronises) over `repeats`
runs after `warmup`, median and 10th / 90th percentile; the evaluator's own device function once more with a `mark` callback
that synchronises the device after each of its steps, to state the share of the gathering of the per-image tensors, the orderings
(four stable sorts and two searches), the match launch, the accumulate launch, and the copy with the host's means; the host
path's evaluate() `host-repeats` times; and whether the two paths' arrays are equal bit for bit.  Needs a ROCm GPU.

--protocol lvis (categories default to 1203): a federated set from a seed -- per image 11 gts over 4 of its categories (3 % with
ignore = 1), 6 neg_category_ids and 1 not_exhaustive_category_id (drawn from all categories, so now and then a positive one), and
300 dets (120 jittered copies of the image's gts with their class, 60 random boxes of its negative categories, 120 random boxes of
random classes, nearly all of them unlisted); 320 dets are fed for every tenth image, so the cap of 300 acts; the categories are
rare / common / frequent 337 : 461 : 405, as in LVIS v1.  The steps then start with the cap (ops.lvis_limit).

--proposals P: the proposal recall ("box_proposals") instead of the AP: the same gts (7 per image under coco, 11 under lvis) and P
proposals per image -- three jittered copies of every gt, the rest random boxes, normal logits -- fed as {"proposals": Instances}.
evaluate() on the device and the host definition beside it, the marks gather / orderings / launch / sum / copy, and whether the
totals, recalls and ARs of the two paths are equal bit for bit (asserted)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def spread(v, unit="ms"):
    return {f"median_{unit}": float(np.median(v)), f"p10_{unit}": float(np.percentile(v, 10)), f"p90_{unit}": float(np.percentile(v, 90)),
            "n": len(v)}


def synthetic(n_images, n_categories, seed=0, gts_per_image=7, dets_per_image=100, matched=60):
    """-> the COCO-format gt dict and per image (image_id, boxes fp32 [100, 4] XYXY, scores fp32, classes int64)."""
    rng = np.random.default_rng(seed)
    anns, per_image = [], []
    for img in range(1, n_images + 1):
        wh = rng.choice([12.0, 24.0, 48.0, 80.0, 140.0, 260.0], size=(gts_per_image, 2)) * rng.uniform(0.7, 1.3, size=(gts_per_image, 2))
        xy = rng.uniform(0, 400, size=(gts_per_image, 2))
        cat = rng.integers(0, n_categories, size=gts_per_image)
        for g in range(gts_per_image):
            anns.append(dict(id=len(anns) + 1, image_id=img, category_id=int(cat[g]) + 1, iscrowd=int(rng.random() < 0.05),
                             bbox=[float(xy[g, 0]), float(xy[g, 1]), float(wh[g, 0]), float(wh[g, 1])], area=float(wh[g, 0] * wh[g, 1])))
        pick = rng.integers(0, gts_per_image, size=matched)
        bxy = xy[pick] + rng.normal(0, 4, size=(matched, 2))
        bwh = wh[pick] * rng.uniform(0.8, 1.25, size=(matched, 2))
        rxy, rwh = rng.uniform(0, 400, size=(dets_per_image - matched, 2)), rng.uniform(8, 200, size=(dets_per_image - matched, 2))
        x1y1 = np.concatenate([bxy, rxy])
        boxes = np.concatenate([x1y1, x1y1 + np.concatenate([bwh, rwh])], axis=1).astype(np.float32)
        classes = np.concatenate([cat[pick], rng.integers(0, n_categories, size=dets_per_image - matched)]).astype(np.int64)
        per_image.append((img, boxes, rng.random(dets_per_image).astype(np.float32), classes))
    gt = dict(images=[dict(id=i) for i in range(1, n_images + 1)], annotations=anns,
              categories=[dict(id=c + 1, name=f"c{c}") for c in range(n_categories)])
    return gt, per_image


def synthetic_lvis(n_images, n_categories, seed=0, gts_per_image=11, pos_cats=4, n_neg=6, n_nel=1, dets_per_image=300, matched=120,
                   on_neg=60):
    """-> the LVIS-format gt dict and per image (image_id, boxes fp32 [300 or 320, 4] XYXY, scores fp32, classes int64)."""
    rng = np.random.default_rng(seed)
    K = n_categories
    freq = np.array(["r"] * (337 * K // 1203) + ["c"] * (461 * K // 1203) + ["f"] * K)[:K][rng.permutation(K)]
    anns, images, per_image = [], [], []
    for img in range(1, n_images + 1):
        wh = rng.choice([12.0, 24.0, 48.0, 80.0, 140.0, 260.0], size=(gts_per_image, 2)) * rng.uniform(0.7, 1.3, size=(gts_per_image, 2))
        xy = rng.uniform(0, 400, size=(gts_per_image, 2))
        pos = rng.choice(K, size=min(pos_cats, K), replace=False)
        cat = pos[rng.integers(0, len(pos), size=gts_per_image)]
        for g in range(gts_per_image):
            anns.append(dict(id=len(anns) + 1, image_id=img, category_id=int(cat[g]) + 1, ignore=int(rng.random() < 0.03),
                             bbox=[float(xy[g, 0]), float(xy[g, 1]), float(wh[g, 0]), float(wh[g, 1])], area=float(wh[g, 0] * wh[g, 1])))
        neg = np.setdiff1d(rng.choice(K, size=min(n_neg, K), replace=False), cat)
        nel = rng.choice(K, size=min(n_nel, K), replace=False)
        images.append(dict(id=img, neg_category_ids=[int(c) + 1 for c in neg], not_exhaustive_category_ids=[int(c) + 1 for c in nel]))
        n = dets_per_image + (20 if img % 10 == 0 else 0)
        pick = rng.integers(0, gts_per_image, size=matched)
        bxy = xy[pick] + rng.normal(0, 4, size=(matched, 2))
        bwh = wh[pick] * rng.uniform(0.8, 1.25, size=(matched, 2))
        rxy, rwh = rng.uniform(0, 400, size=(n - matched, 2)), rng.uniform(8, 200, size=(n - matched, 2))
        x1y1 = np.concatenate([bxy, rxy])
        boxes = np.concatenate([x1y1, x1y1 + np.concatenate([bwh, rwh])], axis=1).astype(np.float32)
        neg_cls = neg[rng.integers(0, len(neg), size=on_neg)] if len(neg) else rng.integers(0, K, size=on_neg)
        classes = np.concatenate([cat[pick], neg_cls, rng.integers(0, K, size=n - matched - on_neg)]).astype(np.int64)
        per_image.append((img, boxes, rng.random(n).astype(np.float32), classes))
    gt = dict(images=images, annotations=anns, categories=[dict(id=c + 1, name=f"c{c}", frequency=str(freq[c])) for c in range(K)])
    return gt, per_image


def feed(evaluator, per_image, device):
    from locov_amd.structures import Boxes, Instances
    evaluator.reset()
    for img, boxes, scores, classes in per_image:
        inst = Instances((480, 640))
        inst.pred_boxes = Boxes(torch.from_numpy(boxes).to(device))
        inst.scores = torch.from_numpy(scores).to(device)
        inst.pred_classes = torch.from_numpy(classes).to(device)
        evaluator.process([dict(image_id=img)], [dict(instances=inst)])


def step_times(ev, dev):
    """The evaluator's own device function with a synchronisation after each of its steps -> milliseconds per step."""
    t, marks = {}, [time.perf_counter()]

    def mark(name):
        torch.cuda.synchronize(dev)
        marks.append(time.perf_counter())
        t[name] = (marks[-1] - marks[-2]) * 1e3

    tensors = ev._gathered(dev)
    mark("gather")
    ev._evaluate_device(*tensors, mark=mark)
    return t


def measure(n_images, n_categories, args, dev):
    from locov_amd.evaluation import COCOEvaluator, LVISEvaluator
    t0 = time.perf_counter()
    if args.protocol == "lvis":
        gt, per_image = synthetic_lvis(n_images, n_categories)
        on_dev, on_host = LVISEvaluator(gt), LVISEvaluator(gt)
        keys = ("precision", "recall", "stats")
    else:
        gt, per_image = synthetic(n_images, n_categories)
        on_dev, on_host = COCOEvaluator(gt), COCOEvaluator(gt)
        keys = ("precision", "recall", "scores", "stats")
    rec = {"images": n_images, "categories": n_categories, "dets": sum(len(p[2]) for p in per_image), "gts": len(gt["annotations"]),
           "build_s": time.perf_counter() - t0}
    feed(on_dev, per_image, dev)
    wall = []
    for it in range(args.warmup + args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = on_dev.evaluate()
        torch.cuda.synchronize(dev)
        if it >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    rec["device_evaluate"] = spread(wall)
    stages = [step_times(on_dev, dev) for _ in range(args.warmup + args.repeats)][args.warmup:]
    rec["device_stages_ms"] = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
    total = sum(rec["device_stages_ms"].values())
    rec["device_stage_share"] = {k: v / total for k, v in rec["device_stages_ms"].items()}
    print(json.dumps({f"{n_categories} categories, device": rec}), flush=True)
    feed(on_host, per_image, "cpu")
    host = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        res_host = on_host.evaluate()
        host.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({f"{n_categories} categories, host evaluate ms": host[-1]}), flush=True)
    rec["host_evaluate"] = spread(host)
    rec["equal_bits"] = all(on_dev.eval[k].tobytes() == on_host.eval[k].tobytes() for k in keys)
    rec["AP"], rec["AP50"] = res["bbox"]["AP"], res_host["bbox"]["AP50"]
    if args.protocol == "lvis":
        rec["protocol"] = "lvis"
        rec["APr"], rec["APc"], rec["APf"] = (res["bbox"][k] for k in ("APr", "APc", "APf"))
        assert rec["equal_bits"], "the device path and the host path differ"
    rec["speedup_median"] = rec["host_evaluate"]["median_ms"] / rec["device_evaluate"]["median_ms"]
    return rec


def synthetic_proposals(gt, n_proposals, seed=1, copies=3):
    """-> per image (image_id, boxes fp32 [P, 4] XYXY, logits fp32 [P]): `copies` jittered copies of each of the image's gts (as many
    as fit), the rest random boxes; normal logits, the copies' a little higher."""
    rng = np.random.default_rng(seed)
    by_image = {}
    for a in gt["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a["bbox"])
    per_image = []
    for im in gt["images"]:
        g = np.array(by_image.get(im["id"], []), dtype=np.float64).reshape(-1, 4)
        near = np.repeat(g, copies, axis=0)[:n_proposals]
        bxy = near[:, :2] + rng.normal(0, 4, size=(len(near), 2))
        bwh = near[:, 2:] * rng.uniform(0.8, 1.25, size=(len(near), 2))
        m = n_proposals - len(near)
        x1y1, wh = np.concatenate([bxy, rng.uniform(0, 400, size=(m, 2))]), np.concatenate([bwh, rng.uniform(8, 200, size=(m, 2))])
        logits = rng.normal(0, 2, size=n_proposals) + np.concatenate([np.full(len(near), 1.0), np.zeros(m)])
        per_image.append((im["id"], np.concatenate([x1y1, x1y1 + wh], axis=1).astype(np.float32), logits.astype(np.float32)))
    return per_image


def feed_proposals(evaluator, per_image, device):
    from locov_amd.structures import Boxes, Instances
    evaluator.reset()
    for img, boxes, logits in per_image:
        inst = Instances((480, 640))
        inst.proposal_boxes = Boxes(torch.from_numpy(boxes).to(device))
        inst.objectness_logits = torch.from_numpy(logits).to(device)
        evaluator.process([dict(image_id=img)], [dict(proposals=inst)])


def measure_proposals(n_images, args, dev):
    """--proposals P: the "box_proposals" part of evaluate() (nothing else is fed, so "bbox" costs nothing), with the marks of
    COCOEvaluator._evaluate_proposals: gather (the concatenation), orderings (two stable sorts and a search), launch, sum, copy."""
    from locov_amd.evaluation import COCOEvaluator, LVISEvaluator
    t0 = time.perf_counter()
    if args.protocol == "lvis":
        gt, _ = synthetic_lvis(n_images, 1203, dets_per_image=180)
        on_dev, on_host = LVISEvaluator(gt), LVISEvaluator(gt)
    else:
        gt, _ = synthetic(n_images, 80, dets_per_image=60)
        on_dev, on_host = COCOEvaluator(gt), COCOEvaluator(gt)
    per_image = synthetic_proposals(gt, args.proposals)
    rec = {"protocol": args.protocol, "images": n_images, "proposals": sum(len(p[2]) for p in per_image), "gts": len(gt["annotations"]),
           "build_s": time.perf_counter() - t0}
    feed_proposals(on_dev, per_image, dev)
    wall = []
    for it in range(args.warmup + args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = on_dev.evaluate()
        torch.cuda.synchronize(dev)
        if it >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    rec["device_evaluate"] = spread(wall)
    stages = []
    for _ in range(args.warmup + args.repeats):
        t, marks = {}, [time.perf_counter()]

        def mark(name):
            torch.cuda.synchronize(dev)
            marks.append(time.perf_counter())
            t[name] = (marks[-1] - marks[-2]) * 1e3

        on_dev._evaluate_proposals(mark=mark)
        stages.append(t)
    stages = stages[args.warmup:]
    rec["device_stages_ms"] = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
    total = sum(rec["device_stages_ms"].values())
    rec["device_stage_share"] = {k: v / total for k, v in rec["device_stages_ms"].items()}
    print(json.dumps({"proposals, device": rec}), flush=True)
    feed_proposals(on_host, per_image, "cpu")
    host = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        res_host = on_host.evaluate()
        host.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"proposals, host evaluate ms": host[-1]}), flush=True)
    rec["host_evaluate"] = spread(host)
    rec["equal_bits"] = all(np.asarray(on_dev.proposal_eval[k]).tobytes() == np.asarray(on_host.proposal_eval[k]).tobytes()
                            for k in ("counts", "num_pos", "recalls", "ar"))
    assert rec["equal_bits"] and repr(res) == repr(res_host), "the device path and the host path differ"
    rec["box_proposals"] = dict(res["box_proposals"])
    rec["speedup_median"] = rec["host_evaluate"]["median_ms"] / rec["device_evaluate"]["median_ms"]
    rec["launch_over_host"] = rec["device_stages_ms"]["launch"] / rec["host_evaluate"]["median_ms"]
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--proposals", type=int, default=0, help="time the proposal recall of this many proposals per image instead of the AP")
    ap.add_argument("--protocol", choices=("coco", "lvis"), default="coco")
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--categories", type=int, nargs="+", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.categories is None:
        args.categories = [1203] if args.protocol == "lvis" else [80, 1203]
    if not torch.cuda.is_available():
        raise SystemExit("time_evaluation: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rec = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "sets": []}
    if args.proposals > 0:
        rec["sets"].append(measure_proposals(args.images, args, dev))
        print(json.dumps(rec["sets"][-1]), flush=True)
        args.categories = []
    for k in args.categories:
        rec["sets"].append(measure(args.images, k, args, dev))
        print(json.dumps(rec["sets"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
