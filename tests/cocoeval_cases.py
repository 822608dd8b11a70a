"""Small synthetic ground truth and detections for the COCO box-AP tests, built from a seed (no fixture files).

A case is (gt, dets): gt a COCO-format dict, dets a list of (image_id, contiguous class, fp32 score, fp32 [x1, y1, x2, y2]) in
the order the evaluator is fed.  Box coordinates are halves and scores multiples of 1/64, so every value is exact in fp32."""
import numpy as np
import torch


def _gt(image_ids, cat_ids, anns):
    """anns: (image_id, category_id, [x, y, w, h], area or None, iscrowd)"""
    return dict(images=[dict(id=i, height=480, width=640) for i in image_ids],
                categories=[dict(id=c, name=f"cat{c}") for c in cat_ids],
                annotations=[dict(id=n + 1, image_id=i, category_id=c, bbox=[float(v) for v in b],
                                  area=float(b[2] * b[3] if ar is None else ar), iscrowd=int(crowd))
                             for n, (i, c, b, ar, crowd) in enumerate(anns)])


def _det(image_id, c, score, xywh):
    x, y, w, h = xywh
    return image_id, c, np.float32(score), np.array([x, y, x + w, y + h], dtype=np.float32)


def handworked():
    """The issue's hand-worked case: one image, one category, two gts, three dets; the third det's IoU is exactly 0.5."""
    gt = _gt([1], [1], [(1, 1, [0, 0, 10, 10], 100, 0), (1, 1, [50, 50, 10, 10], 100, 0)])
    dets = [_det(1, 0, 0.9, [0, 0, 10, 10]), _det(1, 0, 0.8, [100, 100, 10, 10]), _det(1, 0, 0.7, [50, 50, 10, 5])]
    return gt, dets


def perfect(seed=5):
    """Dets equal to the gts, with distinct scores: one gt per cell, two per (category, area range)."""
    rng = np.random.default_rng(seed)
    anns, dets = [], []
    sizes = [8, 20, 50, 80, 120, 200]
    n = 0
    for img, s in enumerate(sizes, start=1):
        for c, cat in enumerate((10, 20)):
            box = [float(rng.integers(0, 200)), float(rng.integers(0, 200)), s, s + 2 * c]
            anns.append((img, cat, box, None, 0))
            dets.append(_det(img, c, 1 - (n + 1) / 64, box))
            n += 1
    return _gt(list(range(1, len(sizes) + 1)), [10, 20], anns), dets


def edge_cases():
    """For max_dets = (1, 2, 5): every situation of the issue's list (named in the comments)."""
    images = [9, 4, 17, 2, 30]                                 # image ids out of order, here and in the det list
    cats = [3, 7, 11, 20, 42, 50]
    anns = [
        (9, 3, [10, 10, 30, 30], None, 0),                     # a cell with gts and no dets (image 9, category 3)
        (17, 3, [0, 0, 20, 20], None, 0),                      # a small gt: ignored in the medium range, where it still takes a det
        (17, 3, [100, 100, 60, 60], None, 0),
        (17, 3, [300, 100, 120, 120], None, 0),
        (2, 3, [0, 0, 200, 200], None, 1),                     # a crowd gt matched by several dets
        (2, 3, [50, 50, 10, 10], 100, 0),                      # an IoU exactly on a threshold (0.5)
        (30, 3, [0, 0, 10, 5], 50, 0),                         # equal IoU with the det [0,0,10,10]: the later gt takes it
        (30, 3, [0, 5, 10, 5], 50, 0),
        (4, 7, [20, 20, 50, 50], None, 1),                     # a category whose only gts are crowd: stays -1
        (4, 11, [5, 5, 40, 40], None, 0),                      # a category with gts and no dets at all: precision 0, recall 0
        (9, 11, [60, 60, 100, 100], None, 0),
        (9, 42, [10, 10, 40, 40], 900, 0),                     # (the annotation's own area field, not w * h)
        (4, 42, [10, 10, 100, 100], None, 0),
    ]                                                          # category 20: no cell at all (-1); category 50: dets only
    dets = [
        _det(17, 0, 0.5, [0, 0, 20, 20]), _det(17, 0, 0.5, [100, 100, 60, 50]),        # equal scores inside a cell
        _det(17, 0, 0.75, [300, 100, 120, 100]), _det(17, 0, 0.25, [1, 1, 20, 20]),
        _det(17, 0, 0.5, [400, 400, 8, 8]),                                          # an unmatched det outside the medium range
        _det(17, 0, 0.125, [100, 100, 60, 60]), _det(17, 0, 0.0625, [300, 100, 120, 120]),    # more than maxDets[-1] dets: these two drop
        _det(4, 0, 0.5, [30, 30, 40, 40]), _det(4, 0, 0.875, [200, 200, 150, 150]),    # a cell with dets and no gts; 0.5 again
        _det(2, 0, 0.625, [10, 10, 50, 50]), _det(2, 0, 0.5, [100, 100, 40, 40]), _det(2, 0, 0.375, [20, 120, 60, 60]),
        _det(2, 0, 0.6875, [50, 50, 10, 5]),
        _det(30, 0, 0.9375, [0, 0, 10, 10]), _det(30, 0, 0.5, [0, 0, 10, 5.5]),
        _det(4, 1, 0.5, [20, 20, 50, 50]), _det(4, 1, 0.25, [25, 25, 20, 20]), _det(9, 1, 0.75, [0, 0, 30, 30]),
        _det(9, 4, 0.5, [10, 10, 40, 40]), _det(4, 4, 0.5, [12, 8, 100, 100]), _det(2, 4, 0.5, [0, 0, 50, 50]),
        _det(9, 5, 0.5, [0, 0, 10, 10]),
    ]
    return _gt(images, cats, anns), dets


def random_case(seed, n_images=6, n_cats=4, dets_per_image=12):
    rng = np.random.default_rng(seed)
    image_ids = [int(v) for v in rng.permutation(np.arange(1, 4 * n_images))[:n_images]]
    cat_ids = [int(v) for v in np.sort(rng.permutation(np.arange(1, 3 * n_cats))[:n_cats])]
    half = lambda lo, hi: float(rng.integers(2 * lo, 2 * hi)) / 2
    anns, dets = [], []
    for img in image_ids:
        boxes = []
        for _ in range(int(rng.integers(0, 6))):
            s = float(rng.choice([6, 14, 28, 40, 70, 110, 180]))
            b = [half(0, 300), half(0, 300), s + half(0, 8), s + half(0, 8)]
            c = int(rng.integers(0, n_cats))
            area = b[2] * b[3] * float(rng.choice([1.0, 0.75, 0.5]))
            anns.append((img, cat_ids[c], b, area, rng.random() < 0.15))
            boxes.append((c, b))
        if rng.random() < 0.15:
            continue                                           # an image with no det
        for _ in range(int(rng.integers(1, dets_per_image + 1))):
            score = float(rng.integers(1, 17)) / 16
            if boxes and rng.random() < 0.7:
                c, b = boxes[int(rng.integers(0, len(boxes)))]
                j = [b[0] + half(-3, 4), b[1] + half(-3, 4), max(b[2] + half(-4, 5), 1), max(b[3] + half(-4, 5), 1)]
                if rng.random() < 0.2:
                    j = list(b)
                if rng.random() < 0.1:
                    c = int(rng.integers(0, n_cats))
                dets.append(_det(img, c, score, j))
            else:
                dets.append(_det(img, int(rng.integers(0, n_cats)), score, [half(0, 300), half(0, 300), half(2, 150), half(2, 150)]))
    return _gt(image_ids, cat_ids, anns), dets


def carry_case(seed=11, n_images=40, per_image=75):
    """One category, about 3 000 dets with scores quantised to 1/64: more than one chunk of the accumulation, ties across its borders."""
    rng = np.random.default_rng(seed)
    anns, dets = [], []
    for img in range(1, n_images + 1):
        gts = []
        for _ in range(6):
            s = float(rng.choice([10, 30, 60, 120]))
            b = [float(rng.integers(0, 400)), float(rng.integers(0, 400)), s, s]
            gts.append(b)
            anns.append((img, 1, b, None, rng.random() < 0.1))
        for n in range(per_image):
            score = float(rng.integers(1, 65)) / 64
            if n < 12:
                b = gts[n % 6]
                box = [b[0] + float(rng.integers(-2, 3)), b[1] + float(rng.integers(-2, 3)), b[2], b[3]]
            else:
                box = [float(rng.integers(0, 400)), float(rng.integers(0, 400)), float(rng.integers(4, 100)), float(rng.integers(4, 100))]
            dets.append(_det(img, 0, score, box))
    return _gt(list(range(1, n_images + 1)), [1], anns), dets


def many_gts_case(seed=13, n_gts=150):
    """One cell whose IoU matrix does not fit the cell's LDS (150 gts, 6 dets under max_dets = (1, 2, 5)), next to a small one."""
    rng = np.random.default_rng(seed)
    anns, dets = [], []
    for n in range(n_gts):
        b = [float(rng.integers(0, 300)), float(rng.integers(0, 300)), float(rng.integers(8, 60)), float(rng.integers(8, 60))]
        anns.append((1, 1, b, None, n % 17 == 0))
    for n in range(6):
        b = anns[int(rng.integers(0, n_gts))][2]
        dets.append(_det(1, 0, (60 - n) / 64, [b[0] + (n % 2), b[1], b[2], b[3]]))
    anns.append((2, 1, [10, 10, 40, 40], None, 0))
    dets.append(_det(2, 0, 0.5, [10, 10, 40, 36]))
    return _gt([1, 2], [1], anns), dets


def feed(evaluator, dets, device="cpu"):
    """process() the dets as one single-image batch per run of equal image ids, in the list's order, as Instances on `device`."""
    from locov_amd.structures import Boxes, Instances
    runs = []
    for d in dets:
        if not runs or runs[-1][0] != d[0]:
            runs.append((d[0], []))
        runs[-1][1].append(d)
    for image_id, ds in runs:
        inst = Instances((480, 640))
        inst.pred_boxes = Boxes(torch.from_numpy(np.stack([d[3] for d in ds])).to(device))
        inst.scores = torch.tensor([float(d[2]) for d in ds], dtype=torch.float32, device=device)
        inst.pred_classes = torch.tensor([d[1] for d in ds], dtype=torch.int64, device=device)
        evaluator.process([dict(image_id=image_id)], [dict(instances=inst)])
