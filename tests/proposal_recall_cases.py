"""Small synthetic ground truth and proposals for the proposal-recall tests, built by hand or from a seed (no fixture files).

A case is (gt, props): gt a COCO-format dict, props a list of (image_id, fp32 logits [n], fp32 boxes [n, 4] XYXY) in the order
the evaluator is fed, one entry per processed image.  Coordinates are halves and logits multiples of 1/64, so every value is
exact in fp32."""
import numpy as np
import torch


def _gt(image_ids, anns):
    """anns: (image_id, [x, y, w, h], area or None, iscrowd[, category_id])"""
    return dict(images=[dict(id=i, height=480, width=640) for i in image_ids],
                categories=[dict(id=1, name="cat1"), dict(id=2, name="cat2")],
                annotations=[dict(id=n + 1, image_id=a[0], category_id=a[4] if len(a) > 4 else 1, bbox=[float(v) for v in a[1]],
                                  area=float(a[1][2] * a[1][3] if a[2] is None else a[2]), iscrowd=int(a[3]))
                             for n, a in enumerate(anns)])


def _props(image_id, rows):
    """rows: (logit, [x, y, w, h])"""
    logits = np.array([r[0] for r in rows], dtype=np.float32)
    boxes = np.array([[r[1][0], r[1][1], r[1][0] + r[1][2], r[1][1] + r[1][3]] for r in rows], dtype=np.float32).reshape(-1, 4)
    return image_id, logits, boxes


def handworked():
    """Two images.  Image 1: gts A = [0,0,10,10] (area 100, small) and B = [100,100,40,40] (area 1600, medium); proposals
    [0,0,10,5] (IoU 0.5 with A), [100,100,40,33] (IoU 0.825 with B), one far away.  Image 2: gt C = [0,0,100,100] (large) and one
    proposal [0,0,100,72] (IoU 0.72).  Overlaps 0.5, 0.825, 0.72 -> thresholds reached: 1 (0.5 itself), 7 (0.5 .. 0.8) and 5
    (0.5 .. 0.7) of 10.  Per threshold the counts are 3, 2, 2, 2, 2, 1, 1, 0, 0, 0 of 3 gts; ARs = 1 / 10, ARm = 7 / 10,
    ARl = 5 / 10; the same at both limits."""
    gt = _gt([1, 2], [(1, [0, 0, 10, 10], None, 0), (1, [100, 100, 40, 40], None, 0), (2, [0, 0, 100, 100], None, 0)])
    props = [_props(1, [(0.5, [100, 100, 40, 33]), (2.0, [300, 300, 20, 20]), (1.0, [0, 0, 10, 5])]),
             _props(2, [(0.25, [0, 0, 100, 72])])]
    return gt, props


def edge_cases():
    """Every small situation of the issue's list, one image each (named in the comments); image ids out of order, here and in the
    feed order."""
    images = [9, 4, 17, 2, 30, 12, 7, 21, 5, 6, 8]
    anns = [
        # image 9: P < G (two proposals, three gts)
        (9, [10, 10, 30, 30], None, 0), (9, [100, 100, 50, 50], None, 0, 2), (9, [300, 200, 120, 120], None, 0),
        # image 4: P == G
        (4, [20, 20, 40, 40], None, 0), (4, [200, 100, 20, 20], None, 0, 2),
        # image 17: P > G
        (17, [0, 0, 20, 20], None, 0), (17, [100, 100, 60, 60], None, 0),
        # image 2: gts and no proposal: adds nothing to num_pos
        (2, [50, 50, 10, 10], None, 0), (2, [150, 50, 100, 100], None, 0),
        # image 30: proposals and only crowd gts: skipped under COCO, counted under LVIS
        (30, [0, 0, 200, 200], None, 1), (30, [50, 50, 20, 20], None, 1),
        # image 12: never processed
        (12, [5, 5, 40, 40], None, 0),
        # image 7: areas of exactly 1024 (small and medium) and 9216 (medium and large), and the annotation's own area field
        (7, [0, 0, 32, 32], None, 0), (7, [100, 0, 96, 96], None, 0), (7, [300, 0, 50, 50], 900, 0), (7, [300, 100, 20, 20], None, 1),
        # image 21: IoUs exactly 0.5 (50 / 100) and fp32(0.55) (110 / 200)
        (21, [0, 0, 10, 10], None, 0), (21, [100, 0, 20, 10], None, 0),
        # image 5: one proposal with IoU 0.5 to two gts: the lower gt takes it, the other is left with nothing
        (5, [0, 0, 10, 12], None, 0), (5, [0, 8, 10, 12], None, 0),
        # image 6: two proposals of equal logit and equal IoU 0.6 to the first gt: the one fed first is taken, which leaves the
        # second gt the other one (IoU 1 / 3); had the later one been taken, the second gt would be left with nothing
        (6, [0, 0, 10, 10], None, 0), (6, [0, 6, 10, 10], None, 0),
        # image 8: both gts have their best IoU with the same proposal (20 / 21 and 19 / 22); the second must look again once the
        # first has taken it, and finds 0.7
        (8, [0, 0, 20, 20], None, 0), (8, [0, 2, 20, 20], None, 0),
    ]
    props = [
        _props(17, [(1.0, [0, 0, 20, 18]), (0.5, [100, 100, 60, 50]), (2.0, [400, 400, 10, 10]), (0.5, [2, 0, 20, 20]), (0.25, [100, 104, 60, 60])]),
        _props(9, [(0.5, [10, 10, 30, 24]), (0.75, [300, 200, 120, 100])]),
        _props(4, [(0.25, [20, 20, 40, 30]), (0.25, [200, 100, 20, 16])]),
        _props(2, []),
        _props(30, [(1.0, [0, 0, 200, 180]), (0.5, [50, 50, 20, 20])]),
        _props(7, [(1.0, [0, 0, 32, 32]), (0.75, [100, 0, 96, 96]), (0.5, [300, 0, 50, 40]), (0.25, [300, 100, 20, 20])]),
        _props(21, [(1.0, [0, 0, 10, 5]), (0.5, [100, 0, 11, 10])]),
        _props(5, [(1.0, [0, 4, 10, 12]), (0.5, [0, 0, 10, 5])]),
        _props(6, [(0.5, [0, 0, 10, 6]), (0.5, [0, 4, 10, 6]), (2.0, [400, 400, 10, 10])]),
        _props(8, [(1.0, [0, 0, 20, 21]), (0.5, [0, 2, 20, 14])]),
    ]
    return _gt(images, anns), props


def limit_case():
    """One image with 101 proposals.  The gt B is reached only by the proposal fed last, whose logit equals that of the one fed
    just before it: the stable order puts it at rank 101, so AR@100 drops it and AR@1000 keeps it."""
    gt = _gt([3], [(3, [0, 0, 40, 40], None, 0), (3, [200, 200, 100, 100], None, 0)])
    rows = [(4.0, [0, 0, 40, 36])]
    rows += [(3.0 - n / 64, [300 + (n % 10) * 8, 10 + (n // 10) * 8, 6, 6]) for n in range(99)]
    rows += [(rows[-1][0], [200, 200, 100, 90])]
    assert len(rows) == 101
    return gt, [_props(3, rows)]


def wide_case(seed=3, n_gts=65, n_props=300):
    """One image with 65 gts and 300 proposals: more than one wave of columns, more than one stride of rows, many equal IoUs."""
    rng = np.random.default_rng(seed)
    anns, rows = [], []
    for n in range(n_gts):
        s = float(rng.choice([12, 24, 40, 64, 100]))
        anns.append((1, [float(rng.integers(0, 60)) * 8, float(rng.integers(0, 40)) * 8, s, s], None, rng.random() < 0.1))
    for n in range(n_props):
        b = anns[int(rng.integers(0, n_gts))][1]
        j = [b[0] + float(rng.integers(-4, 5)) / 2 * 4, b[1] + float(rng.integers(-1, 2)) * 4, b[2], b[3]] if rng.random() < 0.8 else \
            [float(rng.integers(0, 500)), float(rng.integers(0, 400)), float(rng.integers(8, 120)), float(rng.integers(8, 120))]
        rows.append((float(rng.integers(0, 33)) / 64, j))
    return _gt([1], anns), [_props(1, rows)]


def long_case(n_props=2100, edge=2048):
    """One image with 2 100 proposals of distinct logits in descending feed order: gt 0 is reached only by rank edge - 1 (the last
    one a limit of `edge` keeps), gt 1 only by rank edge (the first one it drops), gt 2 by rank 0."""
    gt = _gt([1], [(1, [0, 0, 40, 40], None, 0), (1, [100, 0, 40, 40], None, 0), (1, [200, 0, 100, 100], None, 0)])
    rows = [(64.0 - n / 64, [300 + (n % 40) * 8, 200 + (n // 40) * 4, 6, 3]) for n in range(n_props)]
    rows[0] = (rows[0][0], [200, 0, 100, 80])
    rows[edge - 1] = (rows[edge - 1][0], [0, 0, 40, 30])
    rows[edge] = (rows[edge][0], [100, 0, 40, 36])
    return gt, [_props(1, rows)]


def many_gts_case(n_gts=1025):
    """One image with more gts than the kernel's declared cap and six proposals, next to a small image."""
    anns = [(1, [(n % 40) * 16, (n // 40) * 16, 12, 12], None, 0) for n in range(n_gts)]
    anns.append((2, [10, 10, 40, 40], None, 0))
    rows = [(1.0 - n / 64, [(7 * n % 40) * 16, (n * 5) * 16, 12, 9 + n % 3]) for n in range(6)]
    return _gt([1, 2], anns), [_props(1, rows), _props(2, [(0.5, [10, 10, 40, 36])])]


def random_case(seed, n_images=12, n_props=40):
    """About 12 images x 40 proposals x 0-9 gts, tie-heavy: coarse logits, proposals that copy or slightly shift a gt."""
    rng = np.random.default_rng(seed)
    image_ids = [int(v) for v in rng.permutation(np.arange(1, 4 * n_images))[:n_images]]
    half = lambda lo, hi: float(rng.integers(2 * lo, 2 * hi)) / 2
    anns, props = [], []
    for img in image_ids:
        boxes = []
        for _ in range(int(rng.integers(0, 10))):
            s = float(rng.choice([6, 14, 28, 32, 40, 70, 96, 110, 180]))
            b = [half(0, 300), half(0, 300), s + float(rng.choice([0, 0, 2.5])), s]
            anns.append((img, b, b[2] * b[3] * float(rng.choice([1.0, 1.0, 0.5])), rng.random() < 0.15, int(rng.integers(1, 3))))
            boxes.append(b)
        if rng.random() < 0.1:
            continue                                           # an image that is never processed
        rows = []
        for _ in range(int(rng.integers(0, n_props + 1)) if rng.random() < 0.9 else 0):
            logit = float(rng.integers(-8, 9)) / 4
            if boxes and rng.random() < 0.75:
                b = boxes[int(rng.integers(0, len(boxes)))]
                d = float(rng.choice([0, 0, 2, -2, 4]))
                rows.append((logit, [b[0] + d, b[1], b[2], b[3]] if rng.random() < 0.5 else [b[0], b[1] + d, b[2], b[3]]))
            else:
                rows.append((logit, [half(0, 300), half(0, 300), half(2, 150), half(2, 150)]))
        props.append(_props(img, rows))
    order = rng.permutation(len(props))
    return _gt(image_ids, anns), [props[i] for i in order]


def feed(evaluator, props, device="cpu"):
    """process() one single-image batch per entry, in the list's order, as {"proposals": Instances} on `device`."""
    from locov_amd.structures import Boxes, Instances
    for image_id, logits, boxes in props:
        inst = Instances((480, 640))
        inst.proposal_boxes = Boxes(torch.from_numpy(boxes).to(device))
        inst.objectness_logits = torch.from_numpy(logits).to(device)
        evaluator.process([dict(image_id=image_id)], [dict(proposals=inst)])
