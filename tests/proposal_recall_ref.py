"""A literal restatement of the public Detectron2 _evaluate_box_proposals (detectron2/evaluation/coco_evaluation.py), in torch on
the CPU, written independently of locov_amd/evaluation.py: the overlaps.max(dim=0) / max_overlaps.max(dim=0) loop with the -1
marking, per image, area range and limit.  Two stated differences from upstream, both the issue's: the sort by objectness is
stable (upstream's is not), and the per-image overlaps are laid out in the ground truth's by-image order so that the matching
itself can be compared, not only its totals.

A case is (gt, props): gt a COCO-format dict, props a list of (image_id, fp32 logits [n], fp32 boxes [n, 4] XYXY) in feed order."""
import numpy as np
import torch

AREAS = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))      # all, small, medium, large
NAMES = ("", "s", "m", "l")


def _pairwise_iou(boxes1, boxes2):
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    wh = torch.min(boxes1[:, None, 2:], boxes2[:, 2:]) - torch.max(boxes1[:, None, :2], boxes2[:, :2])
    wh.clamp_(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


def evaluate(gt, props, lvis=False, limits=(100, 1000)):
    """-> dict(gt_overlaps fp32 [A * L, G], counts int64 [A, L, T], num_pos int64 [A, L], recalls fp32 [A, L, T], ar fp32 [A, L],
    results: the "box_proposals" dict)."""
    thresholds = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)
    image_ids = sorted({im["id"] for im in gt["images"]})
    by_image = {i: [] for i in image_ids}
    for a in gt["annotations"]:
        if a["image_id"] in by_image:
            by_image[a["image_id"]].append(a)
    start, n = {}, 0
    for i in image_ids:
        start[i] = n
        n += len(by_image[i])
    A, L, T = len(AREAS), len(limits), len(thresholds)
    out = torch.zeros((A * L, n), dtype=torch.float32)
    counts, num_pos = np.zeros((A, L, T), dtype=np.int64), np.zeros((A, L), dtype=np.int64)
    recalls, ar = np.zeros((A, L, T), dtype=np.float32), np.zeros((A, L), dtype=np.float32)
    results = {}
    for l, limit in enumerate(limits):
        for a, area_range in enumerate(AREAS):
            gt_overlaps = []
            for image_id, logits, boxes in props:
                logits, boxes = torch.from_numpy(np.asarray(logits, dtype=np.float32)), torch.from_numpy(np.asarray(boxes, dtype=np.float32))
                inds = logits.sort(descending=True, stable=True)[1]
                boxes = boxes[inds]
                anno = [o for o in by_image[image_id] if lvis or o["iscrowd"] == 0]
                gt_boxes = torch.as_tensor([[o["bbox"][0], o["bbox"][1], o["bbox"][0] + o["bbox"][2], o["bbox"][1] + o["bbox"][3]] for o in anno],
                                           dtype=torch.float32).reshape(-1, 4)
                gt_areas = torch.as_tensor([o["area"] for o in anno], dtype=torch.float32)
                if len(gt_boxes) == 0 or len(boxes) == 0:
                    continue
                valid = (gt_areas >= area_range[0]) & (gt_areas <= area_range[1])
                gt_boxes = gt_boxes[valid]
                num_pos[a, l] += len(gt_boxes)
                if len(gt_boxes) == 0:
                    continue
                boxes = boxes[:limit]
                overlaps = _pairwise_iou(boxes, gt_boxes)
                _gt_overlaps = torch.zeros(len(gt_boxes))
                for j in range(min(len(boxes), len(gt_boxes))):
                    max_overlaps, argmax_overlaps = overlaps.max(dim=0)
                    gt_ovr, gt_ind = max_overlaps.max(dim=0)
                    assert gt_ovr >= 0
                    box_ind = argmax_overlaps[gt_ind]
                    _gt_overlaps[j] = overlaps[box_ind, gt_ind]
                    assert _gt_overlaps[j] == gt_ovr
                    overlaps[box_ind, :] = -1
                    overlaps[:, gt_ind] = -1
                gt_overlaps.append(_gt_overlaps)
                out[a * L + l, start[image_id]:start[image_id] + len(_gt_overlaps)] = _gt_overlaps
            gt_overlaps = torch.cat(gt_overlaps, dim=0) if len(gt_overlaps) else torch.zeros(0, dtype=torch.float32)
            rec = torch.zeros_like(thresholds)
            for i, t in enumerate(thresholds):
                counts[a, l, i] = int((gt_overlaps >= t).sum())
                rec[i] = (gt_overlaps >= t).float().sum() / float(num_pos[a, l]) if num_pos[a, l] else float("nan")
            recalls[a, l], ar[a, l] = rec.numpy(), rec.mean().item()
            results[f"AR{NAMES[a]}@{limit}"] = float(rec.mean().item() * 100)
    ordered = {f"AR{name}@{limit}": results[f"AR{name}@{limit}"] for limit in limits for name in NAMES}
    return dict(gt_overlaps=out.numpy(), counts=counts, num_pos=num_pos, recalls=recalls, ar=ar, results=ordered)
