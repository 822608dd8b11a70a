"""Host surface of the proposal generator (locov_amd/proposal_generator.py), without a GPU: the anchors against their closed form,
Detectron2's state-dict keys, the config defaults, the registry's two names and the training-with-targets error."""
import math

import pytest
import torch

from locov_amd.config import get_cfg
from locov_amd.structures import ImageList, Instances, ShapeSpec


def test_exported_from_the_package():
    import locov_amd
    for name in ("RPN", "StandardRPNHead", "DefaultAnchorGenerator", "build_proposal_generator"):
        assert getattr(locov_amd, name) is getattr(locov_amd.proposal_generator, name)


def test_anchor_values_and_ordering_on_a_2x3_map():
    from locov_amd.proposal_generator import DefaultAnchorGenerator
    sizes, ratios, stride = [32, 64], [0.5, 1.0, 2.0], 16
    for offset in (0.0, 0.5):
        gen = DefaultAnchorGenerator([sizes], [ratios], [stride], offset=offset)
        assert gen.num_cell_anchors == [6] and gen.box_dim == 4
        got = gen([torch.zeros(1, 8, 2, 3)])[0].tensor
        want = []
        for y in range(2):                                                # ordered (y, x, a); sizes the outer loop of a
            for x in range(3):
                for s in sizes:
                    for r in ratios:
                        w = math.sqrt(s * s / r)
                        h = r * w
                        cx, cy = (x + offset) * stride, (y + offset) * stride
                        want.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
        want = torch.tensor(want, dtype=torch.float64)
        assert got.shape == (36, 4) and got.dtype == torch.float32
        assert (got.double() - want).abs().max().item() <= 2 ** -23 * 64   # fp32 sums of fp32 halves of sides up to 91
        assert gen([torch.zeros(1, 8, 2, 3)])[0].tensor is got            # cached per map shape
    assert DefaultAnchorGenerator([sizes], [ratios], [stride]).state_dict() == {}


def test_state_dict_keys_are_detectron2s():
    from locov_amd.proposal_generator import build_proposal_generator
    rpn = build_proposal_generator(get_cfg(), {"res4": ShapeSpec(channels=32, stride=16)})
    want = {f"rpn_head.{layer}.{p}" for layer in ("conv", "objectness_logits", "anchor_deltas") for p in ("weight", "bias")}
    assert set(rpn.state_dict()) == want
    head = rpn.rpn_head
    assert tuple(head.conv.weight.shape) == (32, 32, 3, 3) and tuple(head.objectness_logits.weight.shape) == (15, 32, 1, 1)
    assert tuple(head.anchor_deltas.weight.shape) == (60, 32, 1, 1)
    assert all(float(l.bias.detach().abs().max()) == 0.0 for l in (head.conv, head.objectness_logits, head.anchor_deltas))
    assert 0.005 < float(head.conv.weight.detach().std()) < 0.02


def test_from_config_defaults():
    from locov_amd.proposal_generator import RPN, DefaultAnchorGenerator, StandardRPNHead, build_proposal_generator
    cfg = get_cfg()
    assert cfg.MODEL.PROPOSAL_GENERATOR.NAME == "RPN" and cfg.MODEL.PROPOSAL_GENERATOR.MIN_SIZE == 0
    assert cfg.MODEL.ANCHOR_GENERATOR.SIZES == [[32, 64, 128, 256, 512]] and cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS == [[0.5, 1.0, 2.0]]
    assert cfg.MODEL.ANCHOR_GENERATOR.OFFSET == 0.0 and cfg.MODEL.RPN.HEAD_NAME == "StandardRPNHead"
    assert cfg.MODEL.RPN.IN_FEATURES == ["res4"] and tuple(cfg.MODEL.RPN.BBOX_REG_WEIGHTS) == (1.0, 1.0, 1.0, 1.0)
    assert cfg.MODEL.RPN.CONV_DIMS == [-1]
    rpn = build_proposal_generator(cfg, {"res4": ShapeSpec(channels=64, stride=16)})
    assert isinstance(rpn, RPN) and isinstance(rpn.rpn_head, StandardRPNHead) and isinstance(rpn.anchor_generator, DefaultAnchorGenerator)
    assert rpn.in_features == ["res4"] and rpn.nms_thresh == 0.7 and rpn.min_box_size == 0.0
    assert rpn.pre_nms_topk == {True: 12000, False: 6000} and rpn.post_nms_topk == {True: 2000, False: 1000}
    assert rpn.box2box_transform.weights == (1.0, 1.0, 1.0, 1.0)
    assert rpn.anchor_generator.strides == [16] and rpn.anchor_generator.num_cell_anchors == [15] and rpn.rpn_head.num_anchors == 15


def test_both_proposal_generator_names():
    from locov_amd.proposal_generator import RPN, build_proposal_generator
    cfg = get_cfg()
    shape = {"res4": ShapeSpec(channels=32, stride=16)}
    assert isinstance(build_proposal_generator(cfg, shape), RPN)
    cfg.MODEL.PROPOSAL_GENERATOR.NAME = "PrecomputedProposals"
    assert build_proposal_generator(cfg, shape) is None
    cfg.MODEL.PROPOSAL_GENERATOR.NAME = "NoSuchGenerator"
    with pytest.raises(KeyError):
        build_proposal_generator(cfg, shape)


def test_training_with_targets_is_not_implemented():
    from locov_amd.proposal_generator import build_proposal_generator
    rpn = build_proposal_generator(get_cfg(), {"res4": ShapeSpec(channels=32, stride=16)}).train()
    images = ImageList(torch.zeros(1, 3, 32, 48), [(32, 48)])
    with pytest.raises(NotImplementedError, match="training losses"):
        rpn(images, {"res4": torch.zeros(1, 32, 2, 3)}, [Instances((32, 48))])


def test_multi_level_inputs_take_the_chain_on_the_cpu():
    """Two levels, CPU tensors: predict_proposals answers with the torch chain (the per-level top-k, NMS per level)."""
    from locov_amd.proposal_generator import RPN, DefaultAnchorGenerator, StandardRPNHead
    from locov_amd.roi_heads.box_emb_head import Box2BoxTransform
    gen = DefaultAnchorGenerator([[32], [64]], [[1.0]], [8, 16])
    rpn = RPN(in_features=["p3", "p4"], head=StandardRPNHead(32, 1), anchor_generator=gen, box2box_transform=Box2BoxTransform((1, 1, 1, 1)),
              pre_nms_topk=(20, 10), post_nms_topk=(8, 5), nms_thresh=0.5).eval()
    feats = [torch.zeros(2, 32, 4, 6), torch.zeros(2, 32, 2, 3)]
    anchors = gen(feats)
    g = torch.Generator().manual_seed(0)
    logits = [torch.randn(2, 24, generator=g), torch.randn(2, 6, generator=g)]
    deltas = [torch.zeros(2, 24, 4), torch.zeros(2, 6, 4)]
    out = rpn.predict_proposals(anchors, logits, deltas, [(32, 48), (32, 48)])
    assert len(out) == 2
    for inst in out:
        assert 1 <= len(inst) <= 5 and inst.image_size == (32, 48)
        s = inst.objectness_logits
        assert bool((s[:-1] >= s[1:]).all()) and tuple(inst.proposal_boxes.tensor.shape) == (len(inst), 4)
