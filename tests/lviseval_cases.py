"""Small synthetic federated ground truth and detections for the LVIS box-AP tests, built from a seed (no fixture files).

A case is (gt, dets): gt an LVIS-format dict (images with neg_category_ids / not_exhaustive_category_ids, categories with
frequency, annotations with an optional ignore), dets a list of (image_id, contiguous class, fp32 score, fp32 [x1, y1, x2, y2]) in
the order the evaluator is fed.  Box coordinates are halves and scores multiples of 1/64, so every value is exact in fp32."""
import numpy as np

from cocoeval_cases import _det, feed  # noqa: F401  (the same det tuples, fed the same way)

# the match kernel's rule for a cell of D dets and G gts (csrc/coco_eval.hip: kCellLds, kGtmStride): the IoU matrix and the
# matched flags stay in the wave's LDS slice while D * G * 8 + G * 64 <= 8192, else they live in the workspace
CELL_LDS, GTM_STRIDE = 8192, 64


def fits_lds(D, G):
    return D * G * 8 + G * GTM_STRIDE <= CELL_LDS


def _gt(images, cats, anns):
    """images: (id, neg_category_ids, not_exhaustive_category_ids); cats: (id, frequency or None);
    anns: (image_id, category_id, [x, y, w, h], area or None, ignore or None)"""
    categories = []
    for c, f in cats:
        categories.append(dict(id=c, name=f"cat{c}"))
        if f is not None:
            categories[-1]["frequency"] = f
    annotations = []
    for n, (i, c, b, ar, ig) in enumerate(anns):
        annotations.append(dict(id=n + 1, image_id=i, category_id=c, bbox=[float(v) for v in b],
                                area=float(b[2] * b[3] if ar is None else ar)))
        if ig is not None:
            annotations[-1]["ignore"] = int(ig)
    return dict(images=[dict(id=i, height=480, width=640, neg_category_ids=list(neg), not_exhaustive_category_ids=list(nel))
                        for i, neg, nel in images], categories=categories, annotations=annotations)


def handworked():
    """The issue's hand-worked case: A and F unlisted, B a false positive, C ignored (not exhaustive), D a true positive, E a false
    positive of a category with no gt."""
    gt = _gt([(1, [2], [1]), (2, [1], []), (3, [], [])], [(1, "f"), (2, "c"), (3, "r")], [(1, 1, [0, 0, 10, 10], 100, None)])
    dets = [_det(3, 0, 0.99, [0, 0, 10, 10]),          # A
            _det(2, 0, 0.95, [0, 0, 10, 10]),          # B
            _det(1, 0, 0.92, [100, 100, 10, 10]),      # C
            _det(1, 0, 0.90, [0, 0, 10, 10]),          # D
            _det(1, 1, 0.70, [0, 0, 10, 10]),          # E
            _det(1, 2, 0.60, [0, 0, 10, 10])]          # F
    return gt, dets


def cap_example():
    """The issue's cap example (max_dets_per_image = 2): scores .9 (class 0), .5 (class 1), .5 (class 0) keep the first two."""
    gt = _gt([(1, [], [])], [(1, "f"), (2, "c")], [(1, 1, [0, 0, 10, 10], None, None), (1, 2, [20, 20, 10, 10], None, None)])
    dets = [_det(1, 0, 0.9, [30, 30, 10, 10]), _det(1, 1, 0.5, [20, 20, 10, 10]), _det(1, 0, 0.5, [0, 0, 10, 10])]
    return gt, dets


def edge_cases():
    """Every situation of the issue's list (named in the comments); meant for the caps 300 and 3."""
    # image ids out of order, here and in the det list; image 12 has no det
    images = [(9, [], []),
              (4, [7, 20], []),                        # categories 7 and 20 are negatives of image 4
              (17, [], [3]),                           # category 3 is not exhaustively annotated in image 17
              (2, [], [7]),                            # a not-exhaustive cell with neither gt nor neg entry: unlisted all the same
              (30, [], []),
              (12, [], [])]
    # no category is rare: an empty frequency group; categories 20 and 42 have no frequency and belong to no group
    cats = [(3, "f"), (7, "c"), (11, "f"), (20, None), (42, None), (50, "f")]
    anns = [
        (17, 3, [0, 0, 20, 20], None, None),                   # the not-exhaustive cell with gts (image 17, category 3)
        (17, 3, [100, 100, 60, 60], None, 0),
        (17, 3, [300, 100, 120, 120], None, 1),                # a gt with ignore = 1
        (2, 3, [50, 50, 10, 10], 100, None),                   # an IoU exactly 0.5 with the det [50, 50, 10, 5]
        (30, 3, [0, 0, 10, 5], 50, None),                      # equal IoU with the det [0, 0, 10, 10]: the later gt takes it
        (30, 3, [0, 5, 10, 5], 50, None),
        (9, 7, [20, 20, 50, 50], None, None),
        (4, 11, [5, 5, 40, 40], None, None),                   # a category with gts and no dets (11)
        (12, 11, [60, 60, 100, 100], None, None),
        (9, 42, [10, 10, 40, 40], 900, None),                  # area field 900: small, while the box and its two dets are medium
        (4, 42, [10, 10, 60, 60], None, None),
        (2, 50, [0, 0, 30, 30], None, None),
    ]                                                          # category 20: no gts at all, dets in a negative cell
    dets = [
        # image 17: the not-exhaustive cell: one det matched, one (far away) unmatched and so ignored; one on the ignore = 1 gt.
        # Scores 0.75, then 0.5 four times: equal scores at the boundary of the cap 3.  The classes outside [0, K) come first in
        # score and must not use up the cap.
        _det(17, 6, 0.984375, [0, 0, 20, 20]), _det(17, -1, 0.984375, [0, 0, 20, 20]),
        _det(17, 0, 0.5, [0, 0, 20, 20]), _det(17, 0, 0.5, [400, 400, 50, 50]), _det(17, 0, 0.75, [300, 100, 120, 100]),
        _det(17, 0, 0.5, [100, 100, 60, 50]), _det(17, 5, 0.5, [0, 0, 30, 30]),
        # image 4: the neg-only cell of category 7: all false positives, those outside an area range ignored in it; category 20
        _det(4, 1, 0.5, [20, 20, 10, 10]), _det(4, 1, 0.625, [20, 20, 50, 50]), _det(4, 1, 0.25, [200, 200, 150, 150]),
        _det(4, 3, 0.5, [0, 0, 50, 50]), _det(4, 4, 0.25, [10, 10, 60, 60]),
        # image 9: an unlisted cell with dets (category 50: no gt here, not a negative); the two identical 40 x 40 dets
        _det(9, 5, 0.9375, [0, 0, 30, 30]), _det(9, 5, 0.5, [100, 100, 30, 30]),
        _det(9, 4, 0.5, [10, 10, 40, 40]), _det(9, 4, 0.375, [10, 10, 40, 40]), _det(9, 1, 0.75, [22, 20, 50, 50]),
        # image 2: the not-exhaustive cell without gt or neg entry (category 7): unlisted; the IoU of exactly 0.5; equal scores
        # across images (0.5 again)
        _det(2, 1, 0.875, [20, 20, 50, 50]), _det(2, 0, 0.6875, [50, 50, 10, 5]), _det(2, 5, 0.5, [0, 0, 30, 28]),
        _det(2, 5, 0.5, [200, 200, 30, 30]),
        # image 30: the equal IoU
        _det(30, 0, 0.9375, [0, 0, 10, 10]), _det(30, 0, 0.5, [0, 0, 10, 5.5]),
    ]
    return _gt(images, cats, anns), dets


def random_case(seed, n_images=6, n_cats=5, dets_per_image=14):
    rng = np.random.default_rng(seed)
    image_ids = [int(v) for v in rng.permutation(np.arange(1, 4 * n_images))[:n_images]]
    cat_ids = [int(v) for v in np.sort(rng.permutation(np.arange(1, 3 * n_cats))[:n_cats])]
    cats = [(c, [None, "r", "c", "f"][int(rng.integers(0, 4))]) for c in cat_ids]
    half = lambda lo, hi: float(rng.integers(2 * lo, 2 * hi)) / 2
    images, anns, dets = [], [], []
    for img in image_ids:
        boxes = []
        for _ in range(int(rng.integers(0, 6))):
            s = float(rng.choice([6, 14, 28, 40, 70, 110, 180]))
            b = [half(0, 300), half(0, 300), s + half(0, 8), s + half(0, 8)]
            c = int(rng.integers(0, n_cats))
            area = b[2] * b[3] * float(rng.choice([1.0, 0.75, 0.5]))
            anns.append((img, cat_ids[c], b, area, [None, 0, 1][int(rng.choice(3, p=[0.5, 0.35, 0.15]))]))
            boxes.append((c, b))
        positive = {cat_ids[c] for c, _ in boxes}
        neg = [c for c in cat_ids if c not in positive and rng.random() < 0.4]
        nel = [c for c in cat_ids if rng.random() < 0.25]
        images.append((img, neg, nel))
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
                    c = int(rng.integers(-1, n_cats + 1))      # (sometimes outside the bank)
                dets.append(_det(img, c, score, j))
            else:
                dets.append(_det(img, int(rng.integers(0, n_cats)), score, [half(0, 300), half(0, 300), half(2, 150), half(2, 150)]))
    return _gt(images, cats, anns), dets


def straddle_case(cap=5, seed=17):
    """For max_dets_per_image = cap: two cells of `cap` dets, one with the most gts whose IoU matrix and flags still fit the cell's
    LDS and one with one gt more (78 and 79 at cap 5); each image is fed cap + 1 dets, so the cap acts too.  Category 2 is a
    negative of image 1 and unlisted in image 2."""
    g_in = max(g for g in range(1, 1024) if fits_lds(cap, g))
    assert fits_lds(cap, g_in) and not fits_lds(cap, g_in + 1)
    rng = np.random.default_rng(seed)
    anns, dets = [], []
    for img, n_gts in ((1, g_in), (2, g_in + 1)):
        mine = []
        for n in range(n_gts):
            b = [float(rng.integers(0, 300)), float(rng.integers(0, 300)), float(rng.integers(8, 60)), float(rng.integers(8, 60))]
            mine.append(b)
            anns.append((img, 1, b, None, 1 if n % 17 == 0 else None))
        for n in range(cap):
            b = mine[int(rng.integers(0, n_gts))]
            dets.append(_det(img, 0, (60 - n) / 64, [b[0] + (n % 2), b[1], b[2], b[3]]))
        dets.append(_det(img, 1, 0.5, [10, 10, 40, 36]))       # the image's lowest score: past the cap
    anns.append((1, 3, [0, 0, 10, 10], None, None))
    return _gt([(1, [2], []), (2, [], [1])], [(1, "f"), (2, "r"), (3, "c")], anns), dets


def large_case(seed=23, n_listed_images=4, per_image=320):
    """For the default cap of 300: category 1 is listed in four images that are fed 320 dets each, about 300 of them of class 0,
    so the category has more than 1 024 listed dets (more than one chunk of the accumulation) after the cap has cut each image
    to 300.  Image 2 marks the category not exhaustive (its unmatched dets are ignored) and image 5 neither holds it nor lists
    it (its 150 class-0 dets are unlisted); with scores in 1/64 steps both kinds are spread over the whole walk, across the
    chunk boundary.  Category 2 is a negative of some images and unlisted in the others."""
    rng = np.random.default_rng(seed)
    images, anns, dets = [], [], []
    for img in range(1, n_listed_images + 2):
        listed = img <= n_listed_images
        gts = []
        if listed:
            for _ in range(6):
                s = float(rng.choice([10, 30, 60, 120]))
                b = [float(rng.integers(0, 400)), float(rng.integers(0, 400)), s, s]
                gts.append(b)
                anns.append((img, 1, b, None, 1 if rng.random() < 0.1 else None))
        images.append((img, [2] if img % 2 else [], [1] if img == 2 else []))
        for n in range(per_image if listed else 170):
            score = float(rng.integers(1, 65)) / 64
            if listed and n < 14:
                b = gts[n % 6]
                box = [b[0] + float(rng.integers(-2, 3)), b[1] + float(rng.integers(-2, 3)), b[2], b[3]]
            else:
                box = [float(rng.integers(0, 400)), float(rng.integers(0, 400)), float(rng.integers(4, 100)), float(rng.integers(4, 100))]
            dets.append(_det(img, 0 if n < 14 or rng.random() < 0.93 else 1, score, box))
    anns.append((1, 2, [0, 0, 50, 50], None, None))
    return _gt(images, [(1, "r"), (2, "f")], anns), dets
