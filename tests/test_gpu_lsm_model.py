"""The LSM training model end to end on the device (locov_amd/meta_arch.py: DistillProposalMMSSRCNN, DistillOnlyProposalMMSSRCNN),
in the pattern of tests/test_gpu_meta_arch.py: a small real model -- R50-C4, random weights, five classes, GroundingHead and a
one-layer TransformerHead, KD distillation, SPATIAL_DROPOUT 16, FREEZE False -- on two uint8 images of different sizes with ground
truth and captions given as token lists, with an explicit `sample`.

The training forward must equal, bit for bit, the composition done by hand from the same modules and the same sample: the model
adds no arithmetic of its own, only the order of the calls, the prefixes and one stacked NaN test."""
import warnings

import numpy as np
import pytest
import torch

import backbone_ref as br
import lsm_model_cases as mc

pytestmark = pytest.mark.gpu

DETECTOR = ["loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"]
GROUNDING = ["CE_loss (Align Words, Choose Caption)", "CE_loss (Align Words, Choose Image)", "CE_loss (Align Regions, Choose Caption)",
             "CE_loss (Align Regions, Choose Image)"]
TRANSFORMER = ["Masked Language Modeling Loss", "Image Caption Matching Loss"]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _build(pkg, arch):
    torch.manual_seed(11)
    m = pkg.build_model(mc.toy_cfg(pkg, "cuda", arch=arch, **{"MODEL.LANGUAGE_BACKBONE.FREEZE": False}), tokenizer=mc.ToyTokenizer())
    br.randomize_frozen_bn(m.backbone, 3)
    m.roi_heads.box_predictor.set_class_embeddings(torch.randn(6, mc.HIDDEN) * 0.05)       # five classes and the background
    m.roi_heads.num_classes = m.roi_heads.box_predictor.num_classes
    return m


@pytest.fixture(scope="module")
def model(pkg):
    m = _build(pkg, "DistillProposalMMSSRCNN")
    assert type(m) is pkg.DistillProposalMMSSRCNN and m.device.type == "cuda"
    return m


def _tokens(inputs):
    return {k: [d["tokens"][k] for d in inputs] for k in ("input_ids", "token_type_ids", "attention_mask", "special_tokens_mask")}


def _by_hand(pkg, model, inputs, sample, grid=True):
    """distill_prop_mmss_gcnn.py:229-442 from the model's own modules; returns (outputs, losses, number of sampled proposals)."""
    torch.manual_seed(21)
    caption = model.language_backbone.body.forward_tokenized(_tokens(inputs), sample.get("mlm_draws"))
    images = model.preprocess_image(inputs)
    gt = [d["instances"].to(model.device) for d in inputs]
    features = model.backbone(images.tensor)
    proposals, proposal_losses = model.proposal_generator(images, features, gt)
    grid_features, box_features, sampled, detector_losses = model.roi_heads(images, features, proposals, gt)
    outputs, losses, dist = {}, {**detector_losses, **proposal_losses}, {}
    branches = []
    if grid:
        branches.append(("", "", pkg.grid_regions(grid_features, images.image_sizes, images.tensor.shape[-2:], 16, True, keys=sample.get("grid_keys"))))
    branches.append(("Box ", "box_", pkg.box_regions(box_features, sampled, 16, True, keys=sample.get("box_keys"))[0]))
    mmss = {}
    for tag, dtag, regions in branches:
        for name in ("GroundingHead", "TransformerHead"):
            o, l, d = model.mmss_heads[name](regions, caption)
            outputs.update({tag + k: v for k, v in o.items()})
            mmss.update({tag + k: v for k, v in l.items()})
            dist.update({dtag + k: v for k, v in d.items()})
    if grid:
        mmss["kd_loss"] = model.distill_loss(dist["trans"], dist["w2r"], dist["r2w"])
    mmss["box_kd_loss"] = model.distill_loss(dist["box_trans"], dist["box_w2r"], dist["box_r2w"])
    if grid:
        mmss["mixbox_kd_loss"] = model.distill_loss(dist["trans"], dist["box_w2r"], dist["box_r2w"])
    losses.update(mmss)
    return outputs, losses, sum(len(p) for p in sampled), tuple(grid_features.shape)


def _sample(pkg, model, inputs, grid=True):
    """An explicit sample: the stored MLM draws (which mask a word of every caption), grid keys and box keys of the sizes a dry
    pass of the composition reports."""
    rng = np.random.default_rng(17)
    sample = {"mlm_draws": torch.from_numpy(mc.mlm_draws()).cuda()}
    _, _, n_boxes, gshape = _by_hand(pkg, model, inputs, sample, grid)
    assert gshape[2] * gshape[3] >= 16 and n_boxes >= 4                   # (random weights: few proposals survive the RPN's NMS)
    sample["grid_keys"] = torch.from_numpy(rng.random((gshape[0], gshape[2] * gshape[3]))).cuda()
    sample["box_keys"] = torch.from_numpy(rng.random(n_boxes)).cuda()
    return sample


def _bits_equal(a, b, k):
    assert a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), k


def _waits(fn):
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, sum("synchroniz" in str(m.message) for m in w)


def _check_training(pkg, model, grid):
    model.train()
    inputs = mc.inputs(pkg, tokens=True)
    try:
        sample = _sample(pkg, model, inputs, grid)
        (want_out, want, _, _), hand_waits = _waits(lambda: _by_hand(pkg, model, inputs, sample, grid))
        again = _by_hand(pkg, model, inputs, sample, grid)[1]
        for k in want:                                                    # the stages themselves repeat their bits
            _bits_equal(want[k], again[k], k)

        model.zero_grad(set_to_none=True)
        torch.manual_seed(21)
        (outputs, losses), model_waits = _waits(lambda: model(inputs, sample=sample))
        tags = ([""] if grid else []) + ["Box "]
        kd = ["kd_loss", "box_kd_loss", "mixbox_kd_loss"] if grid else ["box_kd_loss"]
        assert list(losses) == DETECTOR + [t + k for t in tags for k in GROUNDING + TRANSFORMER] + kd
        assert list(losses) == list(want) and list(outputs) == list(want_out)
        assert any(k.startswith("Box Batch Accuracy") for k in outputs) and "Box Masked Language Modeling Accuracy" in outputs
        for k, v in losses.items():
            assert v.dim() == 0 and torch.isfinite(v).all(), k
            _bits_equal(v, want[k], k)
        for k, v in outputs.items():
            _bits_equal(v, want_out[k], k)
        print(f"host waits: the composition by hand {hand_waits}, the model's forward {model_waits}")
        assert model_waits == hand_waits + 1                              # the one stacked NaN test

        sum(losses.values()).backward()
        emb_pred = model.roi_heads.box_predictor.emb_pred.weight
        word = model.language_backbone.body.bert_model.word_embeddings.weight
        assert emb_pred is model.mmss_heads["GroundingHead"].v2l_projection.weight
        assert word is model.mmss_heads["TransformerHead"].heads.predictions.decoder.weight
        for name, p in (("emb_pred.weight", emb_pred), ("word_embeddings.weight", word)):
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name
        for n, p in model.named_parameters():
            assert p.grad is None or torch.isfinite(p.grad).all(), n
    finally:
        model.zero_grad(set_to_none=True)
        model.eval()


def test_training_forward_equals_the_composition_by_hand(pkg, model):
    _check_training(pkg, model, grid=True)


def test_distill_only_model_skips_the_grid_branch(pkg):
    m = _build(pkg, "DistillOnlyProposalMMSSRCNN")
    assert type(m) is pkg.DistillOnlyProposalMMSSRCNN
    _check_training(pkg, m, grid=False)


def test_a_sample_that_masks_nothing_raises_as_the_reference_does(pkg, model):
    model.train()
    try:
        draws = torch.ones((2, 2, mc.T), dtype=torch.float64, device="cuda")           # u = 1 selects no token: the MLM loss is NaN
        torch.manual_seed(21)
        with pytest.raises(ValueError):
            model(mc.inputs(pkg, tokens=True), sample={"mlm_draws": draws})
    finally:
        model.zero_grad(set_to_none=True)
        model.eval()


def test_inference_equals_generalized_rcnn_from_the_same_weights(pkg, model):
    model.eval()
    cfg = mc.toy_cfg(pkg, "cuda", arch="GeneralizedRCNN")
    plain = pkg.build_model(cfg)
    assert type(plain) is pkg.GeneralizedRCNN
    plain.roi_heads.box_predictor.set_class_embeddings(model.roi_heads.box_predictor.cls_score.weight.detach().clone())
    plain.roi_heads.num_classes = plain.roi_heads.box_predictor.num_classes
    sd = {k: v for k, v in model.state_dict().items() if k.startswith(("backbone.", "proposal_generator.", "roi_heads."))}
    plain.load_state_dict(sd, strict=True)
    plain.eval()
    inputs = mc.inputs(pkg, with_gt=False, tokens=True)
    with torch.no_grad():
        got, want, via_forward = model.inference(inputs), plain.inference(inputs), model(inputs)
    assert len(got) == len(want) == 2
    for g, f, w, d in zip(got, via_forward, want, inputs):
        a, b = g["instances"], w["instances"]
        assert len(b) >= 1 and a.image_size == b.image_size == (d["height"], d["width"]) and len(a) == len(b) == len(f["instances"])
        _bits_equal(a.pred_boxes.tensor, b.pred_boxes.tensor, "pred_boxes")
        _bits_equal(a.scores, b.scores, "scores")
        assert torch.equal(a.pred_classes, b.pred_classes) and torch.equal(f["instances"].scores, a.scores)


def test_caption_path_is_one_launch_and_no_host_wait(pkg, model):
    from torch.profiler import ProfilerActivity, profile
    body = model.language_backbone.body
    model.train()
    try:
        tokens = _tokens(mc.inputs(pkg, tokens=True))
        draws = torch.from_numpy(mc.mlm_draws()).cuda()
        body.forward_tokenized(tokens, draws)                                          # warm-up: the pinned staging block
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            torch.cuda.set_sync_debug_mode("error")                                    # the call itself enqueues without a host read
            try:
                out = body.forward_tokenized(tokens, draws)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()]
        print("caption path launches:", kernels)
        assert len(kernels) == 1 and "caption_embed_kernel" in kernels[0], kernels
        assert out["mlm_mask"].sum(dim=1).min() >= 1 and out["encoded_tokens"] is out["input_embeddings"]
    finally:
        model.eval()
