"""Class-specific box regression (deltas [R, 4K]: MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG False, the plain FastRCNNOutputLayers) in the
two device post-processing pipelines (csrc/detect.hip: locov_detect_postprocess_cs, csrc/detect_wide.hip: locov_detect_postprocess_wide_cs)
against the torch chain (fast_rcnn_inference on boxes [R, 4K]).  The detections must be BIT-IDENTICAL: every candidate (r, c) has its OWN
decoded box -- in batched_nms's shift unit, in both of its branches, and in the output."""
import importlib.util
import os
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_postprocess_cases", os.path.join(HERE, "test_gpu_postprocess.py"))
pp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pp)                     # (its helpers: _inputs, _run, _same)

WEIGHTS, CLAMP = (10.0, 10.0, 5.0, 5.0), 4.135166556742356
SHAPES4 = [(800, 1333), (640, 960), (480, 640), (1067, 800)]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _predictor(pkg, classes, topk=100, thresh=0.05):
    cfg = pkg.config.get_cfg()
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = classes
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = thresh
    cfg.MODEL.ROI_BOX_HEAD.NAME = "FastRCNNOutputLayers"
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = False
    cfg.TEST.DETECTIONS_PER_IMAGE = topk
    pred = pkg.roi_heads.box_emb_head.build_box_predictor(cfg, 256).cuda().eval()
    assert type(pred).__name__ == "FastRCNNOutputLayers" and pred.bbox_pred.out_features == 4 * classes
    return pred


def _inputs(pkg, sizes, classes, sigma, seed, dup_rows=0, **kw):
    """test_gpu_postprocess._inputs with deltas [R, 4K] (per-coordinate spread 1, 1, 0.5, 0.5); duplicated rows copy their 4K deltas."""
    (logits, _), props = pp._inputs(pkg, sizes, classes, sigma, seed, dup_rows=dup_rows, **kw)
    R = sum(sizes)
    g = torch.Generator().manual_seed(seed + 1000)
    deltas = (torch.randn(R, classes, 4, generator=g) * torch.tensor([1.0, 1.0, 0.5, 0.5])).reshape(R, 4 * classes)
    if dup_rows and R > 2 * dup_rows:
        deltas[dup_rows:2 * dup_rows] = deltas[:dup_rows]
    return (logits, deltas.cuda()), props


def _per_image(predictions, sizes, thresh):
    probs = torch.softmax(predictions[0], dim=-1)[:, :-1]
    return [int((p > thresh).sum()) for p in probs.split(sizes)]


def _differ(a, b):
    return any(len(x) != len(y) or not torch.equal(x.pred_boxes.tensor, y.pred_boxes.tensor) for x, y in zip(a[0], b[0]))


def _check(pkg, pred, predictions, props, monkeypatch, per_image, agnostic_differs=False):
    want = pp._run(pkg, pred, predictions, props, False, monkeypatch)
    got = pp._run(pkg, pred, predictions, props, True, monkeypatch)
    pp._same(got, want)
    if any(per_image):
        assert min(len(r) for r, n in zip(got[0], per_image) if n) > 0
    else:
        assert all(len(r) == 0 for r in got[0])
    if agnostic_differs:                       # (a class-agnostic pipeline on the class-0 deltas finds other boxes)
        first = (predictions[0], predictions[1][:, :4].contiguous())
        agn = pp._run(pkg, pred, first, props, True, monkeypatch)
        pp._same(agn, pp._run(pkg, pred, first, props, False, monkeypatch))
        assert _differ(agn, got)
    return got, want


@pytest.mark.parametrize("sizes,classes,sigma,kw", [
    ([300, 0, 1, 517], 80, 2.0, {"image_shapes": SHAPES4}),                    # ragged, an empty image
    ([1500], 3, 0.2, {"crowd": 40}),                                           # every proposal a candidate of every class
    ([2700], 3, 0.2, {}),                                                      # 8 100 candidates: the 8 192-slot sort, full
    ([400, 400], 65, 2.5, {"dup_rows": 50}),                                   # exact score ties (rows with identical 4K deltas)
    ([37] * 64, 20, 1.0, {}),                                                  # the most images one call takes
    ([200], 1203, 0.01, {}),                                                   # nothing passes the threshold
    ([64], 1, 0.1, {}),                                                        # K = 1: 4K = 4
], ids=["ragged", "crowd", "full_sort", "ties", "64_images", "nothing_passes", "one_class"])
def test_lds_pipeline_is_bit_identical_to_the_torch_chain(pkg, monkeypatch, sizes, classes, sigma, kw):
    pred = _predictor(pkg, classes)
    predictions, props = _inputs(pkg, sizes, classes, sigma, seed=len(sizes) * 7 + classes, **kw)
    assert predictions[1].shape[1] == 4 * classes
    per_image = _per_image(predictions, sizes, 0.05)
    assert max(per_image) <= pkg.ops._lib.DETECT_MAX_CANDIDATES
    assert (max(per_image) == 0) == (sigma == 0.01)
    _check(pkg, pred, predictions, props, monkeypatch, per_image, agnostic_differs=(len(sizes) == 4))
    assert not getattr(pred, "_detect_overflow", None)


@pytest.mark.parametrize("sizes,classes,sigma,kw", [
    ([400, 400], 1203, 3.0, {"dup_rows": 50}),                                 # exact score ties
    ([1000], 1203, 3.0, {"crowd": 12}),                                        # 16-word sets, R x K > 2^20, long suppression chains
    ([50] * 64, 400, 1.0, {}),                                                 # the most images one call takes
], ids=["ties", "crowd_1000x1203", "64_images"])
def test_wide_pipeline_is_bit_identical_to_the_torch_chain(pkg, monkeypatch, sizes, classes, sigma, kw):
    pred = _predictor(pkg, classes, topk=300, thresh=1e-4)
    predictions, props = _inputs(pkg, sizes, classes, sigma, seed=len(sizes) * 11 + classes, **kw)
    per_image = _per_image(predictions, sizes, 1e-4)
    assert max(per_image) > pkg.ops._lib.DETECT_MAX_CANDIDATES                   # (the LDS pipeline overflows: the wide one runs)
    _, want = _check(pkg, pred, predictions, props, monkeypatch, per_image)
    assert len(pred._detect_overflow) == 1
    pp._same(pp._run(pkg, pred, predictions, props, True, monkeypatch), want)  # (the remembered setting: straight to the wide path)


@pytest.mark.parametrize("per_class_above", [1, 9000, 24000, 24001, 10 ** 6])
def test_wide_pipeline_follows_a_patched_branch_switch(pkg, monkeypatch, per_class_above):
    """24 000 candidates on either side of _PER_CLASS_NMS_ABOVE, exactly at it, and far from it."""
    beh = pkg.roi_heads.box_emb_head
    monkeypatch.setattr(beh, "_PER_CLASS_NMS_ABOVE", per_class_above)
    pred = _predictor(pkg, 80, topk=100, thresh=0.0)
    predictions, props = _inputs(pkg, [300], 80, 2.0, seed=5, crowd=30)
    per_image = _per_image(predictions, [300], 0.0)
    assert per_image == [24000] and per_image[0] > pkg.ops._lib.DETECT_MAX_CANDIDATES
    _check(pkg, pred, predictions, props, monkeypatch, per_image, agnostic_differs=(per_class_above in (1, 10 ** 6)))


def test_one_wide_call_takes_both_branches(pkg, monkeypatch):
    beh = pkg.roi_heads.box_emb_head
    sizes = [300, 150]
    pred = _predictor(pkg, 80, topk=100, thresh=0.0)
    predictions, props = _inputs(pkg, sizes, 80, 2.0, seed=9, crowd=25)
    per_image = _per_image(predictions, sizes, 0.0)
    switch = (per_image[0] + per_image[1]) // 2
    assert per_image[0] >= switch > per_image[1] > pkg.ops._lib.DETECT_MAX_CANDIDATES
    monkeypatch.setattr(beh, "_PER_CLASS_NMS_ABOVE", switch)
    _check(pkg, pred, predictions, props, monkeypatch, per_image)


def _iou_gt(p, q, thr=0.5):
    left, right = torch.maximum(p[:, 0], q[:, 0]), torch.minimum(p[:, 2], q[:, 2])
    top, bottom = torch.maximum(p[:, 1], q[:, 1]), torch.minimum(p[:, 3], q[:, 3])
    inter = (right - left).clamp(min=0) * (bottom - top).clamp(min=0)
    sa, sb = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]), (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
    return inter / (sa + sb - inter) > thr


def test_the_shift_unit_is_the_maximum_over_the_candidates_own_boxes(pkg, monkeypatch):
    """A 60 000 x 60 000 image (nothing is clipped), two classes, class 1 the only one with candidates.  Row 2's class-1 box lies far
    out (x2 ~ 55 000: the largest candidate coordinate) while its class-0 box is small, and rows 0 / 1 are a pair whose class-1 IoU
    rounds to opposite sides of 0.5 under the true shift unit and under the one a class-agnostic pipeline would form from the rows'
    class-0 boxes.  Fused and chain agree under both branches, in both pipelines."""
    beh = pkg.roi_heads.box_emb_head
    from locov_amd.structures import Boxes, Instances
    t = beh.Box2BoxTransform(WEIGHTS)
    far_prop = torch.tensor([[10.0, 10.0, 50.0, 50.0]])
    far_delta = torch.tensor([[13750.0, 0.0, 0.0, 0.0]])                   # dx = 1375 widths of 40
    far = t.apply_deltas(far_delta.cuda(), far_prop.cuda())
    unit = float(far.max()) + 1.0
    assert 55000 < unit < 56000
    g = torch.Generator().manual_seed(7)
    n = 1 << 16
    x = torch.rand(n, 1, generator=g) * 20000 + 20000
    w = torch.rand(n, 1, generator=g) * 3000 + 1000
    a = torch.cat([x, x, x + w, x + w], dim=1)
    dx = w * (torch.rand(n, 1, generator=g) * 2e-6 + 1.0 / 3.0 - 1e-6)    # IoU within ~1e-6 of 0.5
    b = a + torch.cat([dx, torch.zeros_like(dx), dx, torch.zeros_like(dx)], dim=1)
    zero = torch.zeros(n, 4, device="cuda")
    da, db = t.apply_deltas(zero, a.cuda()), t.apply_deltas(zero, b.cuda())
    assert float(torch.maximum(da.max(), db.max())) < unit - 1
    small_unit = 51.0                                                       # (max coordinate of the rows' class-0 boxes + 1)
    differ = _iou_gt(da + unit, db + unit) != _iou_gt(da + small_unit, db + small_unit)
    assert bool(differ.any())
    i = int(differ.nonzero()[0, 0])
    props = Instances((60000, 60000))
    props.proposal_boxes = Boxes(torch.cat([a[i:i + 1], b[i:i + 1], far_prop]).float().cuda())
    logits = torch.tensor([[-20.0, 12.0, 0.0], [-20.0, 11.0, 0.0], [-20.0, 10.0, 0.0]], device="cuda")     # class 1 only, in row order
    deltas = torch.zeros(3, 8, device="cuda")
    deltas[:2, 0:2] = -1e6                                                  # class 0 of the pair: clipped to the origin
    deltas[:2, 2:4] = -100.0
    deltas[2, 4:8] = far_delta[0].cuda()
    pred = _predictor(pkg, 2, topk=10, thresh=1e-4)
    with torch.no_grad():
        decoded = pred.predict_boxes((logits, deltas), [props])[0].clamp(0, 60000).view(3, 2, 4)
    assert float(decoded[:, 0].max()) + 1.0 <= small_unit and float(decoded[:, 1].max()) + 1.0 == unit
    assert float(decoded.max()) < 60000                                    # (nothing is clipped at the far side)
    probs = torch.softmax(logits, dim=-1)
    kept = {}
    for pca in (1, 4):                                                      # per-class (3 >= 1) / shifted (3 < 4)
        monkeypatch.setattr(beh, "_PER_CLASS_NMS_ABOVE", pca)
        want = pp._run(pkg, pred, (logits, deltas), [props], False, monkeypatch)
        if pca == 4:                          # (pred.inference tries the LDS pipeline first, which is the shifted branch: it is only
            pp._same(pp._run(pkg, pred, (logits, deltas), [props], True, monkeypatch), want)      # the chain's while 8 192 < the switch)
        kept[pca] = len(want[0][0])
        assert torch.equal(want[0][0].pred_boxes.tensor[-1], decoded[2, 1])
        outs = [pkg.ops.detect_postprocess_wide(probs, deltas, props.proposal_boxes.tensor, [3], [(60000, 60000)], WEIGHTS, CLAMP, 1e-4,
                                                0.5, 10, pca)]
        if pca == 4:                                                        # (the LDS pipeline is the shifted branch)
            outs.append(pkg.ops.detect_postprocess(probs, deltas, props.proposal_boxes.tensor, [3], [(60000, 60000)], WEIGHTS, CLAMP,
                                                   1e-4, 0.5, 10))
        for out in outs:
            assert out is not None and out[4] == [kept[pca]]
            m, r = out[4][0], want[0][0]
            assert torch.equal(out[0][0, :m], r.pred_boxes.tensor) and torch.equal(out[1][0, :m], r.scores)
            assert torch.equal(out[2][0, :m], r.pred_classes) and torch.equal(out[3][0, :m], want[1][0])
    want_shifted = 2 if bool(_iou_gt(da[i:i + 1] + unit, db[i:i + 1] + unit)) else 3
    assert kept[4] == want_shifted and {kept[4], 2 if bool(_iou_gt(da[i:i + 1] + small_unit, db[i:i + 1] + small_unit)) else 3} == {2, 3}


def _chain_tensors(pkg, pred, predictions, props, monkeypatch):
    return pp._run(pkg, pred, predictions, props, False, monkeypatch)


def test_direct_calls(pkg, monkeypatch):
    ops = pkg.ops
    sizes, K = [300, 200], 80
    shapes = [(800, 1333)] * 2
    for wide, thresh, topk in ((False, 0.05, 100), (True, 0.0, 100)):
        pred = _predictor(pkg, K, topk=topk, thresh=thresh)
        predictions, props = _inputs(pkg, sizes, K, 2.0, seed=21)
        probs = torch.softmax(predictions[0], dim=-1)
        boxes = torch.cat([p.proposal_boxes.tensor for p in props])
        args = (probs, predictions[1], boxes, sizes, shapes, WEIGHTS, pred.box2box_transform.scale_clamp, thresh, 0.5, topk)
        out = ops.detect_postprocess_wide(*args, per_class_above=20000) if wide else ops.detect_postprocess(*args)   # (on the parent: ValueError)
        monkeypatch.setattr(pkg.roi_heads.box_emb_head, "_PER_CLASS_NMS_ABOVE", 20000)       # (the wide call: one image on either side)
        want = _chain_tensors(pkg, pred, predictions, props, monkeypatch)
        assert out is not None and min(out[4]) > 0
        for i, m in enumerate(out[4]):
            r = want[0][i]
            assert m == len(r)
            assert torch.equal(out[0][i, :m], r.pred_boxes.tensor) and torch.equal(out[1][i, :m], r.scores)
            assert torch.equal(out[2][i, :m], r.pred_classes) and torch.equal(out[3][i, :m], want[1][i])
        for width in (8, 4 * K - 4, 4 * K + 4):
            with pytest.raises(ValueError):
                ops.detect_postprocess(probs, predictions[1].new_zeros(sum(sizes), width), boxes, sizes, shapes, WEIGHTS, CLAMP, thresh, 0.5, topk)
            with pytest.raises(ValueError):
                ops.detect_postprocess_wide(probs, predictions[1].new_zeros(sum(sizes), width), boxes, sizes, shapes, WEIGHTS, CLAMP, thresh,
                                            0.5, topk, 40000)


def test_a_nan_delta_of_a_non_candidate_hands_the_call_to_the_chain(pkg, monkeypatch):
    ops = pkg.ops
    sizes, K = [300], 80
    pred = _predictor(pkg, K)
    predictions, props = _inputs(pkg, sizes, K, 2.0, seed=3)
    probs = torch.softmax(predictions[0], dim=-1)
    r, c = 7, int(probs[7, :K].argmin())
    assert float(probs[r, c]) < 0.05                                        # (r, c) is no candidate
    predictions[1][r, 4 * c] = float("nan")
    args = (probs, predictions[1], props[0].proposal_boxes.tensor, sizes, [(800, 1333)], WEIGHTS, CLAMP, 0.05, 0.5, 100)
    assert ops.detect_postprocess(*args) is None
    assert ops.detect_postprocess_wide(*args, per_class_above=40000) is None
    with pytest.warns(RuntimeWarning, match="non-finite"):
        want = pp._run(pkg, pred, predictions, props, False, monkeypatch)
    with pytest.warns(RuntimeWarning, match="non-finite"):
        got = pp._run(pkg, pred, predictions, props, True, monkeypatch)
    pp._same(got, want)
    assert len(got[0][0]) > 0


def test_a_class_specific_lvis_threshold_call_reads_the_host_once(pkg, monkeypatch):
    """After one warm-up call (which finds the overflow and remembers it), a class-specific pred.inference at 1e-4 / top-300 makes ONE
    host read: implicit synchronisations (torch's sync-debug mode) plus event waits."""
    pred = _predictor(pkg, 1203, topk=300, thresh=1e-4)
    predictions, props = _inputs(pkg, [400, 400], 1203, 3.0, seed=31)
    beh = pkg.roi_heads.box_emb_head
    monkeypatch.setattr(beh, "_FUSED_POSTPROCESS", True)
    with torch.no_grad():
        pred.inference(predictions, props)
    torch.cuda.synchronize()
    assert len(pred._detect_overflow) == 1
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
    assert len(res) == 2 and all(len(r) == 300 for r in res)


def test_evaluation_call_through_the_heads_with_the_plain_predictor(pkg, monkeypatch):
    """EmbeddingRes5ROIHeads with MODEL.ROI_BOX_HEAD.NAME "FastRCNNOutputLayers" and class-specific regression, on a small head: the
    evaluation call's Instances are bit-identical with the fused post-processing on and off."""
    from locov_amd.structures import Boxes, Instances, ShapeSpec
    beh = pkg.roi_heads.box_emb_head
    K = 20
    cfg = pkg.config.get_cfg()
    cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = 32
    cfg.MODEL.RESNETS.WIDTH_PER_GROUP = 8
    cfg.MODEL.ROI_HEADS.NAME = "EmbeddingRes5ROIHeads"
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = K
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.05
    cfg.MODEL.ROI_BOX_HEAD.NAME = "FastRCNNOutputLayers"
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = False
    cfg.MODEL.ROI_BOX_HEAD.RES5_BACKEND = "hip"
    cfg.MODEL.ROI_BOX_HEAD.RES5_DTYPE = "fp32"
    torch.manual_seed(3)
    heads = pkg.build_roi_heads(cfg, {"res4": ShapeSpec(channels=128, stride=16)}).cuda().eval()
    pred = heads.box_predictor
    assert type(pred).__name__ == "FastRCNNOutputLayers" and pred.bbox_pred.out_features == 4 * K
    g = torch.Generator().manual_seed(5)
    feats = {"res4": torch.randn(2, 128, 25, 38, generator=g).cuda()}
    props = []
    for _ in range(2):
        xy = torch.rand(120, 2, generator=g) * torch.tensor([400.0, 250.0])
        p = Instances((400, 608))
        p.proposal_boxes = Boxes(torch.cat([xy, xy + torch.rand(120, 2, generator=g) * 150 + 16], dim=1).cuda())
        props.append(p)
    with torch.no_grad():                      # (random-init logits are ~0: scale the two layers until scores and deltas spread)
        x = heads._shared_roi_transform([feats["res4"]], [p.proposal_boxes for p in props], pooled=True)
        scores, deltas = pred(x)
        pred.cls_score.weight.mul_(2.0 / float(scores.std()))
        pred.bbox_pred.weight.mul_(0.5 / float(deltas.std()))
    outs = {}
    for fused in (False, True):
        monkeypatch.setattr(beh, "_FUSED_POSTPROCESS", fused)
        with torch.no_grad():
            inst, _ = heads(None, feats, props, None)
        torch.cuda.synchronize()
        outs[fused] = inst
    assert sum(len(x) for x in outs[True]) > 0
    for a, b in zip(outs[True], outs[False]):
        assert len(a) == len(b) and torch.equal(a.scores, b.scores) and torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)
        assert torch.equal(a.pred_classes, b.pred_classes)
