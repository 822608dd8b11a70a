"""The detector end to end on the device (locov_amd/meta_arch.py): a small real OvrRCNN -- R50-C4, random weights, FrozenBN, five
classes -- on two uint8 images of different sizes whose "height" / "width" differ from the image sizes.

model.inference and the training forward must equal, bit for bit, the composition done by hand: the normalised, padded batch
computed on the CPU and uploaded, then model.backbone, model.proposal_generator, model.roi_heads, then the single-image torch
detector_postprocess.  Equality is what the design implies: the preprocessing kernel gives the CPU expression's bits, everything
after it is the same code on the same bits, and the batched rescale gives the torch chain's bits."""
import pytest
import torch

import backbone_ref as br

pytestmark = pytest.mark.gpu

STD = [57.375, 57.12, 58.395]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _build_model(pkg, **backbone_keys):
    torch.manual_seed(11)
    cfg = pkg.config.get_cfg()
    for k, v in backbone_keys.items():
        cfg.MODEL.BACKBONE[k] = v
    cfg.MODEL.META_ARCHITECTURE = "OvrRCNN"
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.PIXEL_STD = STD
    cfg.MODEL.RPN.PRE_NMS_TOPK_TEST, cfg.MODEL.RPN.POST_NMS_TOPK_TEST = 200, 50
    cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = 200, 50
    cfg.MODEL.ROI_HEADS.NAME = "EmbeddingRes5ROIHeads"
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = 5
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = 64
    m = pkg.build_model(cfg)
    assert type(m) is pkg.OvrRCNN and m.device.type == "cuda"
    br.randomize_frozen_bn(m.backbone, 3)
    m.roi_heads.box_predictor.set_class_embeddings(torch.randn(6, 64) * 0.05)        # five classes and the background
    m.roi_heads.num_classes = m.roi_heads.box_predictor.num_classes
    return m


@pytest.fixture(scope="module")
def model(pkg):
    # the backbone's trainable stages (FREEZE_AT 2: res3, res4) on the device training path: its forward repeats its bits, which
    # the torch (MIOpen) path under autograd does not on an MI355X (res4 differed between two calls on the same batch)
    return _build_model(pkg, TRAIN_ON_DEVICE=True)


def _inputs(pkg, with_gt=False):
    g = torch.Generator().manual_seed(5)
    out = []
    for (h, w), (oh, ow) in (((96, 128), (240, 427)), ((80, 112), (61, 75))):
        d = {"image": torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g), "height": oh, "width": ow}
        if with_gt:
            boxes = torch.tensor([[8.0, 10.0, 60.0, 70.0], [50.0, 20.0, w - 6.0, h - 9.0], [30.0, 30.0, 62.0, 58.0]])
            d["instances"] = pkg.structures.Instances((h, w), gt_boxes=pkg.structures.Boxes(boxes), gt_classes=torch.tensor([0, 3, 4]))
        out.append(d)
    return out


def _hand_batch(pkg, model, inputs):
    """The normalised, padded batch by the CPU torch expression, uploaded."""
    mean, std = model.pixel_mean.cpu(), model.pixel_std.cpu()
    cpu = pkg.structures.ImageList.from_tensors([(d["image"] - mean) / std for d in inputs], model.backbone.size_divisibility,
                                                padding_constraints=model.backbone.padding_constraints)
    return pkg.structures.ImageList(cpu.tensor.cuda(), cpu.image_sizes)


def _hand_inference(pkg, model, inputs):
    images = _hand_batch(pkg, model, inputs)
    features = model.backbone(images.tensor)
    proposals, _ = model.proposal_generator(images, features, None)
    results, _ = model.roi_heads(images, features, proposals, None)
    return [pkg.detector_postprocess(r, d["height"], d["width"]) for r, d in zip(results, inputs)]


def _same_instances(a, b):
    assert type(a) is type(b) and a.image_size == b.image_size and len(a) == len(b)
    assert set(a.get_fields()) == set(b.get_fields()) == {"pred_boxes", "scores", "pred_classes"}
    assert torch.equal(a.pred_boxes.tensor.view(torch.int32), b.pred_boxes.tensor.view(torch.int32))
    assert torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)) and torch.equal(a.pred_classes, b.pred_classes)


def test_inference_equals_the_composition_by_hand(pkg, model):
    model.eval()
    inputs = _inputs(pkg)
    with torch.no_grad():
        want, again = _hand_inference(pkg, model, inputs), _hand_inference(pkg, model, inputs)
        for a, b in zip(want, again):                                     # the stages themselves repeat their bits
            _same_instances(a, b)
        got = model.inference(inputs)
        raw = model.inference(inputs, do_postprocess=False)
        via_forward = model(inputs)
    assert isinstance(got, list) and len(got) == 2 and all(set(g) == {"instances"} for g in got)
    for g, f, w, r, d in zip(got, via_forward, want, raw, inputs):
        assert len(w) >= 1                                                # an empty comparison would show nothing
        assert g["instances"].image_size == (d["height"], d["width"]) and r.image_size == tuple(d["image"].shape[1:])
        assert len(r) >= len(w)
        _same_instances(g["instances"], w)
        _same_instances(f["instances"], w)
        assert type(g["instances"]) is pkg.structures.Instances and type(g["instances"].pred_boxes) is pkg.structures.Boxes


def test_preprocess_image_equals_the_uploaded_cpu_batch(pkg, model):
    inputs = _inputs(pkg)
    got, want = model.preprocess_image(inputs), _hand_batch(pkg, model, inputs)
    assert got.image_sizes == want.image_sizes == [(96, 128), (80, 112)] and tuple(got.tensor.shape) == (2, 3, 96, 128)
    assert torch.equal(got.tensor.view(torch.int32), want.tensor.view(torch.int32))
    assert torch.equal(got[1], got.tensor[1, :, :80, :112])


def test_training_losses_equal_the_composition_by_hand(pkg, model):
    model.train()
    inputs = _inputs(pkg, with_gt=True)

    def by_hand():
        torch.manual_seed(21)
        images = _hand_batch(pkg, model, inputs)
        gt = [d["instances"].to(model.device) for d in inputs]
        features = model.backbone(images.tensor)
        assert features["res4"].requires_grad
        proposals, proposal_losses = model.proposal_generator(images, features, gt)
        _, detector_losses = model.roi_heads(images, features, proposals, gt)
        return {k: v.detach().clone() for k, v in {**detector_losses, **proposal_losses}.items()}

    try:
        want, again = by_hand(), by_hand()
        for k, v in want.items():                                         # the stages themselves repeat their bits
            assert torch.equal(v.view(torch.int32), again[k].view(torch.int32)), k

        model.zero_grad(set_to_none=True)
        torch.manual_seed(21)
        first, losses = model(inputs)
        assert first == {} and list(losses) == ["loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"]
        for k, v in losses.items():
            assert torch.isfinite(v).all() and torch.equal(v.detach().view(torch.int32), want[k].view(torch.int32)), k
        sum(losses.values()).backward()
        trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        with_grad = [(n, p) for n, p in trainable if p.grad is not None]
        assert trainable and with_grad
        for n, p in with_grad:
            assert torch.isfinite(p.grad).all(), n
        assert any(float(p.grad.abs().max()) > 0 for n, p in with_grad if n.startswith("roi_heads."))
        assert any(float(p.grad.abs().max()) > 0 for n, p in with_grad if n.startswith("proposal_generator."))
        assert any(float(p.grad.abs().max()) > 0 for n, p in with_grad if n.startswith("backbone."))      # FREEZE_AT 2: res3, res4 train
    finally:
        model.zero_grad(set_to_none=True)
        model.eval()
