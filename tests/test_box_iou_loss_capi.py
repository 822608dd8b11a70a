"""CPU-side checks of the IoU box-regression losses (csrc/box_iou_loss.hip: locov_box_iou_loss; BBOX_REG_LOSS_TYPE "giou" / "diou" /
"ciou"): the export, argument errors before anything touches a device, the config key on every predictor class and the torch chain of
FastRCNNOutputLayers.box_reg_loss -- the path a CPU run, unvalidated boxes and LOCOV_FUSED_LOSSES=0 take -- against the float64
restatement of upstream (tests/box_iou_ref.py).  No compute on a device: there is no GPU here."""
import ctypes
import os
import re

import pytest
import torch

import box_iou_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "locov_box_iou_loss"


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_export_and_binding(lib):
    from locov_amd import _lib
    with open(os.path.join(ROOT, "include", "locov_hip.h")) as f:
        header = f.read()
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    decl = re.search(r"\bint %s\(([^;]*)\);" % NAME, header)
    assert decl, "not declared in include/locov_hip.h"
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[NAME][1]) == 16
    assert lib.locov_abi_version() == _lib.ABI_VERSION == 8
    assert "#define LOCOV_ABI_VERSION 8" in header
    for k, name in enumerate(("GIOU", "DIOU", "CIOU")):
        assert "#define LOCOV_BOX_IOU_%s %d" % (name, k) in header and getattr(_lib, "BOX_IOU_" + name) == k


def _call(lib, boxes=256, gt=512, pred=1024, ld=4, cls=2048, R=1536, K=80, kind=0, loss=4096, dpred=8192):
    p = ctypes.c_void_p
    return lib.locov_box_iou_loss(p(boxes), p(gt), p(pred), ld, p(cls), R, K, 10.0, 10.0, 5.0, 5.0, ref.SCALE_CLAMP, kind, p(loss),
                                  p(dpred), None)


@pytest.mark.parametrize("kw,msg", [
    ({"loss": 0}, b"null pointer"),
    ({"pred": 0}, b"null pointer"),
    ({"R": -1}, b"[R, 4] or [R, 4 * num_classes]"),
    ({"ld": 6}, b"[R, 4] or [R, 4 * num_classes]"),
    ({"kind": 7}, b"unknown kind 7"),
    ({"boxes": 260}, b"16-byte aligned"),
    ({"gt": 520}, b"16-byte aligned"),
])
def test_argument_errors_are_reported_before_any_launch(lib, kw, msg):
    """(the pointers are small fake addresses: a call that got as far as a launch would not return an argument error)"""
    rc = _call(lib, **kw)
    assert rc < 0
    err = lib.locov_last_error()
    assert err.startswith(NAME.encode()) and msg in err, err


def test_ops_box_iou_loss_rejects_host_tensors_and_unknown_kinds():
    from locov_amd import ops
    from locov_amd._lib import LocovError
    pred, boxes, cls = torch.zeros(3, 4), torch.tensor([[0., 0., 4., 4.]] * 3), torch.zeros(3, dtype=torch.int64)
    args = (pred, boxes, boxes, cls, 5, ref.WEIGHTS, ref.SCALE_CLAMP)
    with pytest.raises(LocovError, match="no CPU fallback"):
        ops.box_iou_loss(*args, "giou")
    with pytest.raises(ValueError, match="ciou.*diou.*giou"):
        ops.box_iou_loss(*args, "iou")
    with pytest.raises(ValueError, match=r"pred_deltas \[R, 4 \| 4K\]"):
        ops.box_iou_loss(torch.zeros(3, 8), boxes, boxes, cls, 5, ref.WEIGHTS, ref.SCALE_CLAMP, "giou")
    with pytest.raises(ValueError, match=r"pred_deltas \[R, 4 \| 4K\]"):
        ops.box_iou_loss(pred, boxes, boxes, cls.int(), 5, ref.WEIGHTS, ref.SCALE_CLAMP, "diou")


@pytest.mark.parametrize("name", ["FastRCNNOutputLayers", "EmbeddingFastRCNNOutputLayers", "EmbeddingGroundingFastRCNNOutputLayers"])
@pytest.mark.parametrize("loss_type", ["smooth_l1", "giou", "diou", "ciou"])
def test_from_config_carries_the_loss_type(name, loss_type):
    import locov_amd
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.ROI_BOX_HEAD.NAME = name
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = 16
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = 7
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = loss_type
    bp = locov_amd.build_box_predictor(cfg, 32)
    assert type(bp).__name__ == name and bp.box_reg_loss_type == loss_type


# ------------------------------------------------------------------ the torch chain of box_reg_loss

K = 5


def _predictor(loss_type, agnostic):
    from locov_amd.roi_heads import box_emb_head as beh
    return beh.FastRCNNOutputLayers(8, box2box_transform=beh.Box2BoxTransform(ref.WEIGHTS), num_classes=K, cls_agnostic_bbox_reg=agnostic,
                                    box_reg_loss_type=loss_type)


def _inputs(agnostic):
    """40 rows: about half background, two ignored, inf / NaN predictions in two background rows, one foreground row whose dw is above
    the clamp."""
    g = torch.Generator().manual_seed(11)
    n = 40
    boxes = torch.rand(n, 4, generator=g) * 200
    boxes[:, 2:] = boxes[:, :2] + 4 + torch.rand(n, 2, generator=g) * 100
    gt = boxes + torch.randn(n, 4, generator=g) * 5
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    cls = torch.randint(0, K, (n,), generator=g)
    cls[torch.rand(n, generator=g) < 0.5] = K
    cls[[7, 23]] = -1
    pred = torch.randn(n, 4 if agnostic else 4 * K, generator=g) * 0.3
    bg = (cls == K).nonzero()[:, 0]
    pred[bg[0]] = float("inf")
    pred[bg[1], 1::4] = float("nan")
    fg = ((cls >= 0) & (cls < K)).nonzero()[:, 0]
    clamped = int(fg[2])
    pred[clamped, (0 if agnostic else 4 * int(cls[clamped])) + 2] = 30.0           # dw = 30 / 5 = 6 > log(1000 / 16) = 4.135...
    assert 12 <= len(bg) <= 28 and len(fg) >= 8
    return boxes, gt, cls, pred, clamped


def _expected_nonzero(cls, pred, clamped):
    fg = (cls >= 0) & (cls < K)
    want = torch.zeros_like(pred, dtype=torch.bool)
    for r in fg.nonzero()[:, 0].tolist():
        c0 = 0 if pred.shape[1] == 4 else 4 * int(cls[r])
        want[r, c0:c0 + 4] = True
    want[clamped, (0 if pred.shape[1] == 4 else 4 * int(cls[clamped])) + 2] = False
    return want


@pytest.mark.parametrize("agnostic", [True, False])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_cpu_chain_equals_the_float64_restatement(kind, agnostic):
    boxes, gt, cls, pred, clamped = _inputs(agnostic)
    want, g64, _ = ref.box_reg_loss(kind, boxes, gt, pred, cls, K)            # (by index: the dirty rows are never touched)
    bp = _predictor(kind, agnostic)
    for validated in (False, True):                                   # (validated on the CPU: still the chain, without fvcore's assert)
        p = pred.clone().requires_grad_(True)
        got = bp.box_reg_loss(boxes, gt, p, cls, boxes_validated=validated)
        got.backward()
        assert got.dtype == torch.float32 and torch.isfinite(got)
        assert abs(float(got.detach()) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
        assert torch.isfinite(p.grad).all()
        # non-zero only in the foreground rows' (class) columns, never in the clamped column, somewhere in every foreground row, and
        # exactly where the float64 gradient is: inside those columns a zero is legitimate (a predicted box whose x extent lies within
        # the ground truth's, or contains it, has no derivative in dx for "giou")
        allowed = _expected_nonzero(cls, pred, clamped)
        assert not (p.grad != 0)[~allowed].any() and not (g64 != 0)[~allowed].any()
        assert torch.equal((p.grad != 0).any(dim=1), allowed.any(dim=1))
        assert torch.equal(p.grad != 0, g64 != 0)
        # (not a gate the issue sets, a sanity bound on the fp32 chain: its gradient is the float64 one to fp32 accuracy)
        assert float((p.grad.double() - g64).abs().max()) <= 1e-4 * float(g64.abs().max())


@pytest.mark.parametrize("agnostic", [True, False])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_cpu_chain_all_background(kind, agnostic):
    boxes, gt, cls, pred, _ = _inputs(agnostic)
    cls = torch.where(cls < 0, cls, torch.full_like(cls, K))
    p = pred.clone().requires_grad_(True)
    got = _predictor(kind, agnostic).box_reg_loss(boxes, gt, p, cls)
    got.backward()
    assert float(got.detach()) == 0.0 and not p.grad.any()
    assert float(ref.box_reg_loss(kind, boxes, gt, torch.zeros_like(pred), cls, K)[0]) == 0.0


@pytest.mark.parametrize("kind", ref.KINDS)
def test_losses_apply_the_loss_weight_and_ignore_the_beta(kind):
    from locov_amd.structures import Boxes, Instances
    boxes, gt, cls, pred, _ = _inputs(True)
    p = Instances((400, 400))
    p.proposal_boxes, p.gt_boxes = Boxes(boxes), Boxes(gt)
    p.gt_classes = cls = torch.where(cls < 0, torch.full_like(cls, -100), cls)          # (cross_entropy's ignore_index)
    scores = torch.zeros(len(cls), K + 1)
    pred = torch.nan_to_num(pred, 0.0, 0.0, 0.0)
    bp = _predictor(kind, True)
    one = bp.losses((scores, pred), [p])["loss_box_reg"]
    bp.smooth_l1_beta = 0.7
    bp.loss_weight["loss_box_reg"] = 2.0
    assert torch.equal(bp.losses((scores, pred), [p])["loss_box_reg"], one * 2.0)


def test_an_unknown_loss_type_still_raises():
    boxes, gt, cls, pred, _ = _inputs(True)
    with pytest.raises(ValueError, match="Invalid bbox reg loss type 'l2'"):
        _predictor("l2", True).box_reg_loss(boxes, gt, pred, cls)


def test_unvalidated_boxes_keep_the_box_assert():
    """fvcore's `assert (x2 >= x1).all()` stays on the unvalidated path: a foreground proposal of negative width decodes to x2 < x1."""
    boxes = torch.tensor([[10., 10., 5., 30.]])
    gt = torch.tensor([[4., 8., 12., 28.]])
    bp = _predictor("giou", True)
    with pytest.raises(AssertionError, match="bad box"):
        bp.box_reg_loss(boxes, gt, torch.zeros(1, 4), torch.zeros(1, dtype=torch.int64))
    bp.box_reg_loss(boxes, gt, torch.zeros(1, 4), torch.zeros(1, dtype=torch.int64), boxes_validated=True)
