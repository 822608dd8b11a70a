"""The wide detection post-processing (csrc/detect_wide.hip, ops.detect_postprocess_wide) against the torch chain it replaces at
LVIS-style thresholds (SCORE_THRESH_TEST 1e-4, DETECTIONS_PER_IMAGE 300 over the 1 203-class bank: up to 1.2e6 candidates per image,
where the LDS pipeline of csrc/detect.hip flags OVERFLOW).  The detections must be BIT-IDENTICAL to fast_rcnn_inference with the fused
path off, for every candidate count: batched_nms's shifted branch below _PER_CLASS_NMS_ABOVE candidates, its per-class branch from
there on, the merge order (descending score, row, class) and the top-k."""
import importlib.util
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_postprocess_cases", os.path.join(HERE, "test_gpu_postprocess.py"))
pp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pp)                     # (its helpers: _predictor, _inputs, _run, _same)

WEIGHTS, CLAMP = (10.0, 10.0, 5.0, 5.0), 4.135166556742356


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _candidates(predictions, thresh):
    probs = torch.softmax(predictions[0], dim=-1)[:, :-1]
    return probs, int((probs > thresh).sum())


@pytest.mark.parametrize("sizes,classes,sigma,thresh,topk,kw", [
    ([1000], 1203, 3.0, 1e-4, 300, {}),                                       # the LVIS evaluation call: per-class branch
    ([1000] * 8, 1203, 3.0, 1e-4, 300, {}),
    ([1000], 1203, 1.0, 1e-4, 300, {}),                                       # nearly every one of the 1.2e6 pairs a candidate
    ([1000] * 8, 1203, 1.0, 1e-4, 300, {}),
    ([300], 80, 2.0, 0.0, 100, {}),                                           # 24 000 candidates: the shifted branch above 8 192
    ([1000, 100], 1203, 3.0, 1e-4, 300, {}),                                  # one image above 40 000 candidates, one below
    ([400, 400], 1203, 3.0, 1e-4, 300, {"dup_rows": 50}),                     # exact score ties
    ([1000], 1203, 3.0, 1e-4, 300, {"crowd": 12}),                            # long same-class suppression chains
    ([50] * 64, 400, 1.0, 1e-4, 300, {}),                                     # the most images one call takes
], ids=["lvis_1img", "lvis_8img", "dense_1img", "dense_8img", "shifted_24k", "mixed_branches", "ties", "crowd", "64_images"])
def test_wide_postprocess_is_bit_identical_to_the_torch_chain(pkg, monkeypatch, sizes, classes, sigma, thresh, topk, kw):
    pred = pp._predictor(pkg, classes, topk=topk, thresh=thresh)
    predictions, props = pp._inputs(pkg, sizes, classes, sigma, seed=len(sizes) * 11 + classes, **kw)
    probs, total = _candidates(predictions, thresh)
    per_image = [int((p > thresh).sum()) for p in probs.split(sizes)]
    assert max(per_image) > pkg.ops._lib.DETECT_MAX_CANDIDATES                    # (the LDS pipeline overflows: the wide one runs)
    want = pp._run(pkg, pred, predictions, props, False, monkeypatch)
    got = pp._run(pkg, pred, predictions, props, True, monkeypatch)
    pp._same(got, want)
    assert min(len(r) for r, n in zip(got[0], per_image) if n) > 0
    if sizes == [1000, 100]:
        beh = pkg.roi_heads.box_emb_head
        assert per_image[0] >= beh._PER_CLASS_NMS_ABOVE > per_image[1] > pkg.ops._lib.DETECT_MAX_CANDIDATES
    got2 = pp._run(pkg, pred, predictions, props, True, monkeypatch)         # (the remembered setting: straight to the wide path)
    pp._same(got2, want)


@pytest.mark.parametrize("per_class_above", [1, 9000, 24000, 24001, 10 ** 6])
def test_wide_postprocess_follows_a_patched_branch_switch(pkg, monkeypatch, per_class_above):
    """_PER_CLASS_NMS_ABOVE is read at call time: 24 000 candidates on either side of it, exactly at it, and far from it."""
    beh = pkg.roi_heads.box_emb_head
    monkeypatch.setattr(beh, "_PER_CLASS_NMS_ABOVE", per_class_above)
    pred = pp._predictor(pkg, 80, topk=100, thresh=0.0)
    predictions, props = pp._inputs(pkg, [300], 80, 2.0, seed=5, crowd=30)
    assert _candidates(predictions, 0.0)[1] == 24000
    want = pp._run(pkg, pred, predictions, props, False, monkeypatch)
    got = pp._run(pkg, pred, predictions, props, True, monkeypatch)
    pp._same(got, want)


def _borderline_pair(pkg):
    """Two proposals whose decoded boxes (large coordinates) have an IoU that rounds to opposite sides of 0.5 with and without the
    class-1 shift of batched_nms -- found by a seeded search over box pairs, decoded and clipped as the chain does."""
    beh = pkg.roi_heads.box_emb_head
    g = torch.Generator().manual_seed(7)
    n = 1 << 16
    x = torch.rand(n, 1, generator=g) * 20000 + 20000
    w = torch.rand(n, 1, generator=g) * 3000 + 1000
    a = torch.cat([x, x, x + w, x + w], dim=1)
    dx = w * (torch.rand(n, 1, generator=g) * 2e-6 + 1.0 / 3.0 - 1e-6)    # IoU within ~1e-6 of 0.5
    b = a + torch.cat([dx, torch.zeros_like(dx), dx, torch.zeros_like(dx)], dim=1)
    t = beh.Box2BoxTransform(WEIGHTS)
    zero = torch.zeros(n, 4, device="cuda")
    da = t.apply_deltas(zero, a.cuda()).clamp(0, 60000)
    db = t.apply_deltas(zero, b.cuda()).clamp(0, 60000)

    def iou_gt(p, q):
        left, right = torch.maximum(p[:, 0], q[:, 0]), torch.minimum(p[:, 2], q[:, 2])
        top, bottom = torch.maximum(p[:, 1], q[:, 1]), torch.minimum(p[:, 3], q[:, 3])
        inter = (right - left).clamp(min=0) * (bottom - top).clamp(min=0)
        sa, sb = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]), (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
        return inter / (sa + sb - inter) > 0.5

    unit = torch.maximum(da.amax(dim=1), db.amax(dim=1)) + 1
    differ = iou_gt(da, db) != iou_gt(da + unit[:, None], db + unit[:, None])
    i = int(differ.nonzero()[0, 0])
    return a[i], b[i]


def test_the_two_branches_really_differ_and_both_match_the_chain(pkg, monkeypatch):
    beh = pkg.roi_heads.box_emb_head
    from locov_amd.structures import Boxes, Instances
    a, b = _borderline_pair(pkg)
    props = Instances((60000, 60000))
    props.proposal_boxes = Boxes(torch.stack([a, b]).float().cuda())
    logits = torch.tensor([[-20.0, 12.0, 0.0], [-20.0, 11.0, 0.0]], device="cuda")     # class 1 only, row 0 first
    deltas = torch.zeros(2, 4, device="cuda")
    pred = pp._predictor(pkg, 2, topk=10, thresh=1e-4)
    with torch.no_grad():
        boxes = pred.predict_boxes((logits, deltas), [props])[0].clamp(0, 60000)
    scores = torch.softmax(logits, dim=-1)[:, 1]
    cls = torch.ones(2, dtype=torch.int64, device="cuda")
    kept = {}
    for pca in (1, 3):                                                   # per-class (2 >= 1) / shifted (2 < 3)
        monkeypatch.setattr(beh, "_PER_CLASS_NMS_ABOVE", pca)
        kept[pca] = len(beh.batched_nms(boxes, scores, cls, 0.5))
    assert sorted(kept.values()) == [1, 2], kept                         # the two NMS forms disagree on this input
    probs = torch.softmax(logits, dim=-1)
    for pca in (1, 3):
        monkeypatch.setattr(beh, "_PER_CLASS_NMS_ABOVE", pca)
        want = pp._run(pkg, pred, (logits, deltas), [props], False, monkeypatch)
        assert len(want[0][0]) == kept[pca]
        out = pkg.ops.detect_postprocess_wide(probs, deltas, props.proposal_boxes.tensor, [2], [(60000, 60000)], WEIGHTS,
                                              pred.box2box_transform.scale_clamp, 1e-4, 0.5, 10, pca)
        got_boxes, got_scores, got_classes, got_rows, counts = out
        assert counts == [kept[pca]]
        n = counts[0]
        r = want[0][0]
        assert torch.equal(got_boxes[0, :n], r.pred_boxes.tensor) and torch.equal(got_scores[0, :n], r.scores)
        assert torch.equal(got_classes[0, :n], r.pred_classes) and torch.equal(got_rows[0, :n], want[1][0])


def test_direct_calls(pkg):
    ops = pkg.ops
    # at <= 8 192 candidates: the same outputs as the LDS pipeline
    predictions, props = pp._inputs(pkg, [1000, 600], 1203, 3.0, seed=21)
    probs = torch.softmax(predictions[0], dim=-1)
    boxes = torch.cat([p.proposal_boxes.tensor for p in props])
    args = (probs, predictions[1], boxes, [1000, 600], [(800, 1333)] * 2, WEIGHTS, CLAMP, 0.05, 0.5, 100)
    lds = ops.detect_postprocess(*args)
    assert lds is not None and min(lds[4]) > 0
    for pca in (40000, 1):
        wide = ops.detect_postprocess_wide(*args, per_class_above=pca)
        assert wide[4] == lds[4]
        for b, (x, y) in enumerate(zip(wide[:4], lds[:4])):
            for i, n in enumerate(lds[4]):
                assert torch.equal(x[i, :n], y[i, :n])
    # 1.2e6 candidates: a result, not None
    predictions, props = pp._inputs(pkg, [1000], 1203, 0.3, seed=22)
    probs = torch.softmax(predictions[0], dim=-1)
    assert int((probs[:, :-1] > 1e-4).sum()) > 1_190_000
    out = ops.detect_postprocess_wide(probs, predictions[1], props[0].proposal_boxes.tensor, [1000], [(800, 1333)], WEIGHTS, CLAMP,
                                      1e-4, 0.5, 300, 40000)
    assert out is not None and out[4] == [300]
    assert bool((out[1][0, :-1] >= out[1][0, 1:]).all())
    # non-finite input: None (the caller runs the torch chain)
    deltas = predictions[1].clone()
    deltas[3, 0] = float("inf")
    assert ops.detect_postprocess_wide(probs, deltas, props[0].proposal_boxes.tensor, [1000], [(800, 1333)], WEIGHTS, CLAMP, 1e-4,
                                       0.5, 300, 40000) is None
    bad = probs.clone()
    bad[5, 7] = float("nan")
    assert ops.detect_postprocess_wide(bad, predictions[1], props[0].proposal_boxes.tensor, [1000], [(800, 1333)], WEIGHTS, CLAMP, 1e-4,
                                       0.5, 300, 40000) is None


def test_an_lvis_threshold_call_reads_the_host_once(pkg, monkeypatch):
    """After one warm-up call (which finds the overflow and remembers it), pred.inference at 1e-4 / top-300 on 8 images makes ONE
    host read: implicit synchronisations (torch's sync-debug mode) plus event waits."""
    pred = pp._predictor(pkg, 1203, topk=300, thresh=1e-4)
    predictions, props = pp._inputs(pkg, [1000] * 8, 1203, 3.0, seed=31)
    beh = pkg.roi_heads.box_emb_head
    monkeypatch.setattr(beh, "_FUSED_POSTPROCESS", True)
    with torch.no_grad():
        pred.inference(predictions, props)
    torch.cuda.synchronize()
    waits = []
    orig = torch.cuda.Event.synchronize

    def counted(self):
        waits.append(1)
        return orig(self)

    monkeypatch.setattr(torch.cuda.Event, "synchronize", counted)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            with torch.no_grad():
                res, _ = pred.inference(predictions, props)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [x for x in w if "synchroniz" in str(x.message)]
    assert len(syncs) + len(waits) == 1, ([str(x.message) for x in syncs], len(waits))
    assert len(res) == 8 and all(len(r) == 300 for r in res)


def test_evaluation_call_through_the_heads_at_lvis_thresholds(pkg, monkeypatch):
    sys.path.insert(0, os.path.dirname(HERE))
    import bench
    args = bench.parse(["--images", "2", "--proposals", "1000", "--classes", "1203", "--no-cpu-baseline"])
    wl = bench.Workload(args, torch.device("cuda", 0))
    pred = wl.eval_heads().box_predictor
    pred.test_score_thresh, pred.test_topk_per_image = 1e-4, 300
    beh = pkg.roi_heads.box_emb_head
    outs = {}
    for fused in (False, True):
        monkeypatch.setattr(beh, "_FUSED_POSTPROCESS", fused)
        inst, _ = wl.step_eval(2)
        torch.cuda.synchronize()
        outs[fused] = inst
    assert ("_detect_overflow" in pred.__dict__) and len(pred._detect_overflow) == 1
    assert all(len(x) == 300 for x in outs[True])
    for a, b in zip(outs[True], outs[False]):
        assert len(a) == len(b) and torch.equal(a.scores, b.scores) and torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)
        assert torch.equal(a.pred_classes, b.pred_classes)
