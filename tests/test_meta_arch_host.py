"""The meta-architecture's host side (locov_amd/meta_arch.py, structures.ImageList.from_tensors), without a GPU: the padding rule
against hand-written expectations, the single-image detector_postprocess against the Detectron2 stub's, the order and arguments
of the calls with recording stand-ins for the three sub-modules, and build_model from a yaml."""
import os
import sys

import pytest
import torch
from torch import nn

STUBS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stubs")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------ ImageList.from_tensors

def _img(c, h, w, base):
    return torch.arange(c * h * w, dtype=torch.float32).reshape(c, h, w) + base


def test_from_tensors_one_image_is_only_wrapped():
    from locov_amd.structures import ImageList
    a = _img(3, 5, 7, 1.0)
    il = ImageList.from_tensors([a])
    assert tuple(il.tensor.shape) == (1, 3, 5, 7) and il.image_sizes == [(5, 7)] and len(il) == 1
    assert torch.equal(il.tensor[0], a) and torch.equal(il[0], a)


def test_from_tensors_three_sizes_divisibility_and_pad_value():
    from locov_amd.structures import ImageList
    ims = [_img(3, 37, 53, 1.0), _img(3, 40, 41, 2.0), _img(3, 5, 64, 3.0)]
    il = ImageList.from_tensors(ims)                                      # divisibility 0: the largest height and width
    assert tuple(il.tensor.shape) == (3, 3, 40, 64) and il.image_sizes == [(37, 53), (40, 41), (5, 64)]
    for i, (im, (h, w)) in enumerate(zip(ims, il.image_sizes)):
        assert torch.equal(il.tensor[i, :, :h, :w], im) and torch.equal(il[i], im)
        assert il.tensor[i, :, h:, :].abs().sum() == 0 and il.tensor[i, :, :, w:].abs().sum() == 0
    il = ImageList.from_tensors(ims, 32, pad_value=-7.5)                  # rounded up to 32, another pad value
    assert tuple(il.tensor.shape) == (3, 3, 64, 64)
    want = torch.full((3, 3, 64, 64), -7.5)
    for i, im in enumerate(ims):
        want[i, :, :im.shape[1], :im.shape[2]] = im
    assert torch.equal(il.tensor, want)
    assert tuple(ImageList.from_tensors(ims, 1).tensor.shape) == (3, 3, 40, 64)            # 1 rounds nothing
    assert tuple(ImageList.from_tensors([ims[0]], 32).tensor.shape) == (1, 3, 64, 64)


def test_from_tensors_square_size_and_constraint_divisibility():
    from locov_amd.structures import ImageList, padded_batch_size
    ims = [_img(1, 9, 20, 0.0), _img(1, 12, 3, 0.0)]
    il = ImageList.from_tensors(ims, 0, padding_constraints={"square_size": 48})
    assert tuple(il.tensor.shape) == (2, 1, 48, 48)
    il = ImageList.from_tensors(ims, 0, padding_constraints={"square_size": 40, "size_divisibility": 16})
    assert tuple(il.tensor.shape) == (2, 1, 48, 48)                      # the constraint's own divisibility wins over the argument
    assert padded_batch_size([(9, 20), (12, 3)], 8, {"square_size": 0}) == (16, 24)
    assert padded_batch_size([(9, 20), (12, 3)], 0, {}) == (12, 20)
    il = ImageList.from_tensors([torch.ones(3, 4, dtype=torch.uint8), torch.ones(2, 6, dtype=torch.uint8)], pad_value=9)   # no channel dim
    assert il.tensor.dtype == torch.uint8 and il.tensor.tolist() == [[[1, 1, 1, 1, 9, 9]] * 3, [[1] * 6] * 2 + [[9] * 6]]


# ------------------------------------------------------------------------------------------------------ detector_postprocess

@pytest.fixture()
def d2():
    """The Detectron2 stub as `detectron2` for one test (tests/test_d2_seam.py's arrangement)."""
    assert not any(m == "detectron2" or m.startswith("detectron2.") for m in sys.modules), "a real detectron2 is loaded"
    sys.path.insert(0, STUBS)
    import detectron2
    import detectron2.modeling.postprocessing
    import detectron2.structures
    yield detectron2
    sys.path.remove(STUBS)
    for m in [m for m in sys.modules if m == "detectron2" or m.startswith("detectron2.")]:
        del sys.modules[m]


def _raw_results(seed, n=60, size=(800, 1333)):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([size[1] * 1.1, size[0] * 1.1]) - 40.0
    wh = torch.rand(n, 2, generator=g) * 300.0
    boxes = torch.cat([xy, xy + wh], dim=1)
    boxes[3, 2] = boxes[3, 0]                                            # zero width
    boxes[7] = torch.tensor([1400.0, 10.0, 1500.0, 30.0])                # empty once clipped
    boxes[11] = torch.tensor([-50.0, -60.0, -1.0, -2.0])
    return boxes, torch.rand(n, generator=g), torch.randint(0, 80, (n,), generator=g)


@pytest.mark.parametrize("out_size", [(480, 640), (800, 1333), (1213, 2017)])
def test_detector_postprocess_equals_the_detectron2_stub(d2, out_size):
    from detectron2.modeling.postprocessing import detector_postprocess as d2_postprocess
    from detectron2.structures import Boxes as D2Boxes, Instances as D2Instances
    from locov_amd.meta_arch import detector_postprocess
    from locov_amd.structures import Boxes, Instances
    boxes, scores, classes = _raw_results(5)
    ours = Instances((800, 1333), pred_boxes=Boxes(boxes.clone()), scores=scores, pred_classes=classes)
    theirs = D2Instances((800, 1333), pred_boxes=D2Boxes(boxes.clone()), scores=scores, pred_classes=classes)
    got, want = detector_postprocess(ours, *out_size), d2_postprocess(theirs, *out_size)
    assert type(got) is Instances and type(got.pred_boxes) is Boxes and got.image_size == want.image_size == out_size
    assert 0 < len(want) < len(boxes) and len(got) == len(want)
    assert torch.equal(_bits(got.pred_boxes.tensor), _bits(want.pred_boxes.tensor))
    assert torch.equal(_bits(got.scores), _bits(want.scores)) and torch.equal(got.pred_classes, want.pred_classes)
    assert torch.equal(ours.pred_boxes.tensor, boxes)                    # the input's boxes are not scaled in place
    # on Detectron2's own classes it answers with them
    again = detector_postprocess(D2Instances((800, 1333), pred_boxes=D2Boxes(boxes.clone()), scores=scores, pred_classes=classes), *out_size)
    assert type(again) is D2Instances and type(again.pred_boxes) is D2Boxes
    assert torch.equal(_bits(again.pred_boxes.tensor), _bits(want.pred_boxes.tensor))


def test_detector_postprocess_falls_back_to_proposal_boxes():
    from locov_amd.meta_arch import detector_postprocess
    from locov_amd.structures import Boxes, Instances
    r = Instances((100, 200), proposal_boxes=Boxes(torch.tensor([[10.0, 10.0, 50.0, 50.0], [150.0, 20.0, 150.0, 40.0]])),
                  objectness_logits=torch.tensor([1.0, 2.0]))
    out = detector_postprocess(r, 50, 100)
    assert out.proposal_boxes.tensor.tolist() == [[5.0, 5.0, 25.0, 25.0]] and out.objectness_logits.tolist() == [1.0]
    with pytest.raises(AssertionError, match="must contain boxes"):
        detector_postprocess(Instances((100, 200), scores=torch.zeros(2)), 50, 100)


# ------------------------------------------------------------------------------------------------------ orchestration

class _Backbone(nn.Module):
    size_divisibility = 16
    padding_constraints = {}

    def __init__(self, log):
        super().__init__()
        self.log = log
        self.w = nn.Parameter(torch.ones(1))

    def forward(self, x):
        self.log.append(("backbone", x))
        return {"res4": x[:, :1, ::16, ::16] * self.w}


class _Rpn(nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, images, features, gt_instances=None):
        from locov_amd.structures import Boxes, Instances
        self.log.append(("rpn", images, features, gt_instances))
        props = [Instances(s, proposal_boxes=Boxes(torch.tensor([[0.0, 0.0, 8.0, 8.0]])), objectness_logits=torch.zeros(1)) for s in images.image_sizes]
        return props, ({"loss_rpn_cls": features["res4"].sum() * 0 + 3.0, "loss_rpn_loc": torch.tensor(4.0)} if gt_instances is not None else {})


class _Heads(nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log = log

    def _results(self, image_sizes):
        from locov_amd.structures import Boxes, Instances
        out = []
        for h, w in image_sizes:
            b = torch.tensor([[1.0, 2.0, w - 1.0, h - 2.0], [w + 5.0, 0.0, w + 9.0, 4.0], [3.0, 3.0, 10.0, 12.0]])    # the middle one clips away
            out.append(Instances((h, w), pred_boxes=Boxes(b), scores=torch.tensor([0.9, 0.8, 0.7]), pred_classes=torch.tensor([1, 2, 3])))
        return out

    def forward(self, images, features, proposals, targets=None):
        self.log.append(("heads", images, features, proposals, targets))
        if self.training:
            return proposals, {"loss_cls": features["res4"].sum() * 0 + 1.0, "loss_box_reg": torch.tensor(2.0)}
        return self._results(images.image_sizes), {}

    def forward_with_given_boxes(self, features, instances):
        self.log.append(("given", features, instances))
        return instances


def _model(cls_name, log, rpn=True):
    from locov_amd import meta_arch
    cls = getattr(meta_arch, cls_name)
    return cls(backbone=_Backbone(log), proposal_generator=_Rpn(log) if rpn else None, roi_heads=_Heads(log),
               pixel_mean=[10.0, 20.0, 30.0], pixel_std=[2.0, 4.0, 8.0], input_format="BGR")


def _inputs(with_gt=False, with_size=True):
    from locov_amd.structures import Boxes, Instances
    g = torch.Generator().manual_seed(0)
    out = []
    for (h, w), (oh, ow) in (((40, 50), (80, 100)), ((33, 64), (66, 32))):
        d = {"image": torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g)}
        if with_size:
            d.update(height=oh, width=ow)
        if with_gt:
            d["instances"] = Instances((h, w), gt_boxes=Boxes(torch.tensor([[2.0, 2.0, 20.0, 20.0]])), gt_classes=torch.tensor([1]))
        out.append(d)
    return out


def _expected_batch(inputs, div=16):
    mean, std = torch.tensor([10.0, 20.0, 30.0]).view(3, 1, 1), torch.tensor([2.0, 4.0, 8.0]).view(3, 1, 1)
    hb = max(d["image"].shape[1] for d in inputs)
    wb = max(d["image"].shape[2] for d in inputs)
    hb, wb = (hb + div - 1) // div * div, (wb + div - 1) // div * div
    want = torch.zeros(len(inputs), 3, hb, wb)
    for i, d in enumerate(inputs):
        _, h, w = d["image"].shape
        want[i, :, :h, :w] = (d["image"].float() - mean) / std
    return want


@pytest.mark.parametrize("cls_name", ["GeneralizedRCNN", "OvrRCNN"])
def test_training_call_order_arguments_and_the_shape_of_the_answer(cls_name):
    log = []
    model = _model(cls_name, log).train()
    inputs = _inputs(with_gt=True)
    out = model(inputs)
    assert [e[0] for e in log] == ["backbone", "rpn", "heads"]
    batch = log[0][1]
    assert torch.equal(_bits(batch), _bits(_expected_batch(inputs)))
    _, images, features, gt = log[1]
    assert images.tensor is batch and images.image_sizes == [(40, 50), (33, 64)] and set(features) == {"res4"}
    assert [len(t) for t in gt] == [1, 1] and torch.equal(gt[0].gt_boxes.tensor, inputs[0]["instances"].gt_boxes.tensor)
    _, images2, features2, proposals, targets = log[2]
    assert images2 is images and features2 is features and targets is gt and len(proposals) == 2 and proposals[0].has("proposal_boxes")
    if cls_name == "OvrRCNN":
        first, losses = out
        assert first == {}
    else:
        losses = out
    assert list(losses) == ["loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"]         # detector losses first
    assert [float(v.detach()) for v in losses.values()] == [1.0, 2.0, 3.0, 4.0]
    sum(losses.values()).backward()
    assert model.backbone.w.grad is not None
    # without "instances" the sub-modules get None
    log.clear()
    model(_inputs(with_gt=False))
    assert log[1][3] is None and log[2][4] is None


@pytest.mark.parametrize("cls_name", ["GeneralizedRCNN", "OvrRCNN"])
def test_inference_postprocesses_to_the_requested_size(cls_name):
    from locov_amd.meta_arch import detector_postprocess
    from locov_amd.structures import Boxes, Instances
    log = []
    model = _model(cls_name, log).eval()
    inputs = _inputs()
    out = model(inputs)                                                   # eval mode: forward is inference
    assert [e[0] for e in log] == ["backbone", "rpn", "heads"] and log[1][3] is None and log[2][4] is None
    assert isinstance(out, list) and len(out) == 2 and all(set(o) == {"instances"} for o in out)
    raw = model.roi_heads._results([(40, 50), (33, 64)])
    for o, r, d in zip(out, raw, inputs):
        want = detector_postprocess(r, d["height"], d["width"])
        got = o["instances"]
        assert type(got) is Instances and type(got.pred_boxes) is Boxes
        assert got.image_size == (d["height"], d["width"]) and len(got) == len(want) == 2
        assert torch.equal(_bits(got.pred_boxes.tensor), _bits(want.pred_boxes.tensor))
        assert torch.equal(got.pred_classes, torch.tensor([1, 3])) and torch.equal(got.scores, want.scores)
    assert out[0]["instances"].pred_boxes.tensor[0].tolist() == [2.0, 4.0, 98.0, 76.0]          # x2 in both directions
    # without height / width the image's own size is the output size
    plain = model.inference(_inputs(with_size=False))
    assert [p["instances"].image_size for p in plain] == [(40, 50), (33, 64)]
    assert plain[1]["instances"].pred_boxes.tensor[0].tolist() == [1.0, 2.0, 63.0, 31.0]
    # do_postprocess=False: the ROI heads' results as they are
    raw_out = model.inference(inputs, do_postprocess=False)
    assert [len(r) for r in raw_out] == [3, 3] and raw_out[0].image_size == (40, 50)
    with pytest.raises(AssertionError):
        model.train().inference(inputs)


def test_detected_instances_skip_the_proposals_and_the_box_head():
    from locov_amd.structures import Boxes, Instances
    log = []
    model = _model("OvrRCNN", log).eval()
    inputs = _inputs()
    given = [Instances((40, 50), pred_boxes=Boxes(torch.tensor([[5.0, 5.0, 25.0, 30.0]])), pred_classes=torch.tensor([7])),
             Instances((33, 64), pred_boxes=Boxes(torch.tensor([[0.0, 0.0, 64.0, 33.0]])), pred_classes=torch.tensor([2]))]
    out = model.inference(inputs, detected_instances=given)
    assert [e[0] for e in log] == ["backbone", "given"]
    assert log[1][1].keys() == {"res4"} and [len(i) for i in log[1][2]] == [1, 1]
    assert out[0]["instances"].pred_boxes.tensor.tolist() == [[10.0, 10.0, 50.0, 60.0]] and out[0]["instances"].pred_classes.tolist() == [7]
    assert out[1]["instances"].pred_boxes.tensor.tolist() == [[0.0, 0.0, 32.0, 66.0]]
    assert given[0].pred_boxes.tensor.tolist() == [[5.0, 5.0, 25.0, 30.0]]


def test_precomputed_proposals_come_from_the_inputs():
    from locov_amd.structures import Boxes, Instances
    log = []
    model = _model("OvrRCNN", log, rpn=False)
    assert model.proposal_generator is None
    inputs = _inputs(with_gt=True)
    for d in inputs:
        h, w = d["image"].shape[1:]
        d["proposals"] = Instances((h, w), proposal_boxes=Boxes(torch.tensor([[1.0, 1.0, 9.0, 9.0], [2.0, 2.0, 12.0, 12.0]])),
                                   objectness_logits=torch.zeros(2))
    first, losses = model.train()(inputs)
    assert first == {} and list(losses) == ["loss_cls", "loss_box_reg"]
    assert [e[0] for e in log] == ["backbone", "heads"] and [len(p) for p in log[1][3]] == [2, 2]
    log.clear()
    model.eval().inference(inputs)
    assert [e[0] for e in log] == ["backbone", "heads"] and log[1][3][1].proposal_boxes.tensor.shape == (2, 4)
    with pytest.raises(AssertionError, match="proposals"):
        model.inference(_inputs())


# ------------------------------------------------------------------------------------------------------ build_model

YAML = """
MODEL:
  META_ARCHITECTURE: "OvrRCNN"
  DEVICE: "cpu"
  PIXEL_STD: [57.375, 57.12, 58.395]
  BACKBONE:
    FREEZE_AT: 2
  RESNETS:
    RES2_OUT_CHANNELS: 32
    WIDTH_PER_GROUP: 8
    STEM_OUT_CHANNELS: 16
  ROI_HEADS:
    NAME: "EmbeddingRes5ROIHeads"
    NUM_CLASSES: 5
  ROI_BOX_HEAD:
    CLS_AGNOSTIC_BBOX_REG: True
    EMBEDDING_BASED: True
    EMB_DIM: 32
"""


def _cfg(tmp_path, extra=""):
    from locov_amd.config import get_cfg
    path = tmp_path / "model.yaml"
    path.write_text(YAML + extra)
    cfg = get_cfg()
    cfg.merge_from_file(str(path))
    return cfg


def test_config_defaults_are_detectron2s():
    from locov_amd.config import get_cfg
    cfg = get_cfg()
    assert cfg.MODEL.META_ARCHITECTURE == "GeneralizedRCNN" and cfg.MODEL.PIXEL_MEAN == [103.530, 116.280, 123.675]
    assert cfg.MODEL.PIXEL_STD == [1.0, 1.0, 1.0] and cfg.INPUT.FORMAT == "BGR" and cfg.VIS_PERIOD == 0


def test_build_model_from_yaml_and_its_state_dict(tmp_path):
    import locov_amd
    from locov_amd.meta_arch import META_ARCH_REGISTRY, GeneralizedRCNN, OvrRCNN
    cfg = _cfg(tmp_path)
    model = locov_amd.build_model(cfg)
    assert type(model) is OvrRCNN and isinstance(model, GeneralizedRCNN) and model.device == torch.device("cpu")
    assert isinstance(model.proposal_generator, locov_amd.RPN) and model.input_format == "BGR" and model.vis_period == 0
    keys = list(model.state_dict())
    prefixes = ("backbone.", "proposal_generator.", "roi_heads.")
    assert keys and all(k.startswith(prefixes) for k in keys)
    assert all(any(k.startswith(p) for k in keys) for p in prefixes)
    assert not any("pixel_" in k for k in keys)
    assert tuple(model.pixel_mean.shape) == (3, 1, 1) and model.pixel_std.flatten().tolist() == pytest.approx([57.375, 57.12, 58.395])
    assert "pixel_mean" in dict(model.named_buffers())
    # its own state_dict loads strictly: nothing is expected for the pixel buffers
    model.load_state_dict(model.state_dict(), strict=True)
    assert "OvrRCNN" in META_ARCH_REGISTRY and "GeneralizedRCNN" in META_ARCH_REGISTRY

    cfg2 = cfg.clone()
    cfg2.MODEL.META_ARCHITECTURE = "GeneralizedRCNN"
    cfg2.MODEL.PROPOSAL_GENERATOR.NAME = "PrecomputedProposals"
    plain = locov_amd.build_model(cfg2)
    assert type(plain) is GeneralizedRCNN and plain.proposal_generator is None
    assert not any(k.startswith("proposal_generator.") for k in plain.state_dict())


def test_build_model_refuses_visualisation_and_unknown_names(tmp_path):
    import locov_amd
    cfg = _cfg(tmp_path)
    cfg.VIS_PERIOD = 20
    with pytest.raises(NotImplementedError, match="vis_period"):
        locov_amd.build_model(cfg)
    cfg.VIS_PERIOD = 0
    cfg.MODEL.META_ARCHITECTURE = "PanopticFPN"
    with pytest.raises(KeyError, match="PanopticFPN"):
        locov_amd.build_model(cfg)


def test_wrappers_reject_cpu_tensors():
    from locov_amd import ops
    from locov_amd._lib import LocovError
    with pytest.raises(LocovError):
        ops.preprocess_images([torch.zeros(3, 4, 4, dtype=torch.uint8)], [0.0] * 3, [1.0] * 3)
    with pytest.raises(LocovError):
        ops.detector_rescale(torch.zeros(2, 4), [2], [(10, 10)], [(20, 20)])
