"""Host surface of the RPN's training half (locov_amd/proposal_generator.py, locov_amd/config.py), without a GPU: the new config
keys, from_config's wiring, the constructor's defaults, the loss weights, the unsupported loss types, the logged counters of the
torch chain, and training without targets."""
import numpy as np
import pytest
import torch

import rpn_train_cases as tc
from locov_amd.config import get_cfg
from locov_amd.roi_heads.labelling import Matcher, get_event_storage
from locov_amd.structures import ImageList, ShapeSpec


def test_config_defaults_are_upstreams():
    r = get_cfg().MODEL.RPN
    assert r.IOU_THRESHOLDS == [0.3, 0.7] and r.IOU_LABELS == [0, -1, 1]
    assert r.BATCH_SIZE_PER_IMAGE == 256 and r.POSITIVE_FRACTION == 0.5 and r.BOUNDARY_THRESH == -1
    assert r.LOSS_WEIGHT == 1.0 and r.BBOX_REG_LOSS_WEIGHT == 1.0 and r.BBOX_REG_LOSS_TYPE == "smooth_l1" and r.SMOOTH_L1_BETA == 0.0


def test_from_config_wires_every_key():
    from locov_amd.proposal_generator import build_proposal_generator
    cfg = get_cfg()
    r = cfg.MODEL.RPN
    r.IOU_THRESHOLDS, r.IOU_LABELS = [0.25, 0.5, 0.75], [0, -1, 0, 1]
    r.BATCH_SIZE_PER_IMAGE, r.POSITIVE_FRACTION, r.BOUNDARY_THRESH = 64, 0.25, 0
    r.LOSS_WEIGHT, r.BBOX_REG_LOSS_WEIGHT, r.SMOOTH_L1_BETA = 2.0, 0.25, 0.125
    rpn = build_proposal_generator(cfg, {"res4": ShapeSpec(channels=32, stride=16)})
    m = rpn.anchor_matcher
    assert type(m) is Matcher and m.allow_low_quality_matches and m.labels == [0, -1, 0, 1]
    assert m.thresholds == [-float("inf"), 0.25, 0.5, 0.75, float("inf")]
    assert rpn.batch_size_per_image == 64 and rpn.positive_fraction == 0.25 and rpn.anchor_boundary_thresh == 0
    assert rpn.loss_weight == {"loss_rpn_cls": 2.0, "loss_rpn_loc": 0.5}
    assert rpn.box_reg_loss_type == "smooth_l1" and rpn.smooth_l1_beta == 0.125


def test_the_old_constructor_call_still_works():
    from torch import nn
    from locov_amd.proposal_generator import RPN
    from locov_amd.roi_heads.box_emb_head import Box2BoxTransform
    rpn = RPN(in_features=["res4"], head=nn.Identity(), anchor_generator=nn.Identity(), box2box_transform=Box2BoxTransform((1, 1, 1, 1)),
              pre_nms_topk=(20, 10), post_nms_topk=(8, 5), nms_thresh=0.5, min_box_size=1.0)
    m = rpn.anchor_matcher
    assert m.thresholds[1:-1] == [0.3, 0.7] and m.labels == [0, -1, 1] and m.allow_low_quality_matches
    assert rpn.batch_size_per_image == 256 and rpn.positive_fraction == 0.5 and rpn.anchor_boundary_thresh == -1.0
    assert rpn.loss_weight == {"loss_rpn_cls": 1.0, "loss_rpn_loc": 1.0}
    assert rpn.box_reg_loss_type == "smooth_l1" and rpn.smooth_l1_beta == 0.0


def _chain_losses(c, **kw):
    rpn = tc.make_rpn(c, **kw)
    anchors, gt, rnd = tc.inputs(c)
    labels, boxes = rpn.label_and_sample_anchors(anchors, gt, rnd)
    return rpn.losses(anchors, [torch.from_numpy(c["logits"])], labels, [torch.from_numpy(c["deltas"])], boxes), labels


def test_a_float_loss_weight_is_both_weights():
    c = tc.case("tie_max")
    one, _ = _chain_losses(c)
    flt, _ = _chain_losses(c, loss_weight=3.0)
    dct, _ = _chain_losses(c, loss_weight={"loss_rpn_cls": 3.0, "loss_rpn_loc": 3.0})
    only, _ = _chain_losses(c, loss_weight={"loss_rpn_loc": 3.0})
    for k in ("loss_rpn_cls", "loss_rpn_loc"):
        assert torch.equal(flt[k], dct[k]) and torch.equal(flt[k], one[k] * 3.0)
    assert torch.equal(only["loss_rpn_cls"], one["loss_rpn_cls"]) and torch.equal(only["loss_rpn_loc"], flt["loss_rpn_loc"])


def test_iou_loss_types_are_not_implemented():
    c = tc.case("tie_max")
    with pytest.raises(NotImplementedError, match="BBOX_REG_LOSS_TYPE 'giou'"):
        _chain_losses(c, box_reg_loss_type="giou")


def test_the_chain_logs_the_sampled_counts():
    c = tc.case("b7_with_empty")
    storage = get_event_storage()
    scalars = getattr(storage, "scalars", None)
    assert scalars is not None                                  # (no Detectron2 trainer here: the module's own sink)
    scalars.pop("rpn/num_pos_anchors", None)
    _, labels = _chain_losses(c)
    recs = tc.reference("b7_with_empty")
    assert scalars["rpn/num_pos_anchors"] == np.mean([r["num_pos"] for r in recs])
    assert scalars["rpn/num_neg_anchors"] == np.mean([r["num_neg"] for r in recs])


def test_training_without_targets_still_returns_no_losses(monkeypatch):
    from locov_amd.proposal_generator import build_proposal_generator
    rpn = build_proposal_generator(get_cfg(), {"res4": ShapeSpec(channels=32, stride=16)}).train()
    A = rpn.rpn_head.num_anchors
    monkeypatch.setattr(rpn.rpn_head, "flat_predictions",
                        lambda feats: ([torch.zeros(1, 6 * A)], [torch.zeros(1, 6 * A, 4)]))           # (the head itself needs a device)
    images = ImageList(torch.zeros(1, 3, 32, 48), [(32, 48)])
    proposals, losses = rpn(images, {"res4": torch.zeros(1, 32, 2, 3)})
    assert losses == {} and len(proposals) == 1


def test_rnd_of_the_wrong_shape_is_rejected():
    c = tc.case("tie_max")
    rpn = tc.make_rpn(c)
    anchors, gt, rnd = tc.inputs(c)
    with pytest.raises(ValueError, match="rnd"):
        rpn.label_and_sample_anchors(anchors, gt, rnd[:, :1])
    with pytest.raises(ValueError, match="rnd"):
        rpn.label_and_sample_anchors(anchors, gt, rnd.float())
