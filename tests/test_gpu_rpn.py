"""The RPN proposal generation on the device (csrc/rpn.hip through ops.rpn_proposals, locov_amd/proposal_generator.py) against the
float64 reference of the operation itself (tests/rpn_ref.py) on the exact cases of tests/rpn_cases.py -- no tolerance: counts and
indices equal the reference's, boxes and logits equal it as int32 bit patterns, rows at or beyond an image's count are zero (index
-1), a second call gives the same bits, the flag word is 0 -- and, on one realistic case, against the module's torch chain on the
device, bit for bit as well.  tests/test_rpn_ref.py checks without a GPU that every case reaches what it is meant to and that the
reference equals the CPU torch chain."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_cases as rc
import rpn_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_fused(pkg, c):
    return pkg.ops._rpn_proposals_flags(dev(c["logits"]), dev(c["deltas"]), dev(c["anchors"]), c["image_hw"], c["weights"], c["scale_clamp"],
                                        c["pre"], c["post"], c["min_box_size"], c["nms_thresh"])


def bits(t):
    return t.cpu().numpy().view(np.int32)


def assert_equals_reference(out, recs, post):
    boxes, logits, index, counts = out
    assert tuple(boxes.shape) == (len(recs), post, 4) and tuple(logits.shape) == (len(recs), post) and index.dtype == torch.int64
    assert counts == [r["count"] for r in recs]
    for n, r in enumerate(recs):
        k = r["count"]
        assert index[n, :k].cpu().tolist() == r["index"].tolist()
        assert np.array_equal(bits(boxes[n, :k]), r["boxes"].view(np.int32))
        assert np.array_equal(bits(logits[n, :k]), r["logits"].view(np.int32))
        assert not bits(boxes[n, k:]).any() and not bits(logits[n, k:]).any() and bool((index[n, k:] == -1).all())


@pytest.mark.parametrize("name", rc.EXACT)
def test_fused_equals_reference_bit_for_bit(pkg, name):
    c = rc.all_cases()[name]
    out, flags = run_fused(pkg, c)
    assert flags == 0
    assert_equals_reference(out, rc.reference(name), c["post"])
    again, flags = run_fused(pkg, c)
    assert flags == 0 and all(torch.equal(a, b) for a, b in zip(out[:3], again[:3])) and out[3] == again[3]


def _module(pkg, pre, post, nms_thresh=0.7, min_box_size=0.0, scale_clamp=None):
    from locov_amd.proposal_generator import RPN, DefaultAnchorGenerator, StandardRPNHead
    from locov_amd.roi_heads.box_emb_head import Box2BoxTransform
    b2b = Box2BoxTransform((1.0, 1.0, 1.0, 1.0)) if scale_clamp is None else Box2BoxTransform((1.0, 1.0, 1.0, 1.0), scale_clamp)
    return RPN(in_features=["res4"], head=StandardRPNHead(32, 15), anchor_generator=DefaultAnchorGenerator([[32]], [[1.0]], [16]),
               box2box_transform=b2b, pre_nms_topk=(pre, pre), post_nms_topk=(post, post), nms_thresh=nms_thresh, min_box_size=min_box_size)


def _predict(rpn, c, logits=None, deltas=None):
    from locov_amd.structures import Boxes
    return rpn.predict_proposals([Boxes(dev(c["anchors"]))], [dev(c["logits"]) if logits is None else logits],
                                 [dev(c["deltas"]) if deltas is None else deltas], c["image_hw"])


def test_non_finite_values_raise_the_flag_and_the_module_answers_with_the_chain(pkg, monkeypatch):
    """exp(100) without the clamp; a NaN delta and an inf logit inside the selection: the flag is set; the module in evaluation mode
    returns the chain's result (the non-finite proposals dropped), in training mode it raises FloatingPointError."""
    c = rc.all_cases()["no_clamp_overflow"]
    assert rc.reference(c["name"])[0]["nonfinite"] and run_fused(pkg, c)[1] == pkg._lib.RPN_FLAG_NONFINITE

    c = rc.all_cases()["hwa65"]
    sel = rc.reference("hwa65")[0]["selected"]
    nan_delta, inf_logit = c["deltas"].copy(), c["logits"].copy()
    nan_delta[0, sel[3], 1] = np.nan
    inf_logit[0, sel[0]] = np.inf                                 # (stays the first selected)
    for logits, deltas in ((c["logits"], nan_delta), (inf_logit, c["deltas"])):
        bad = dict(c, logits=logits, deltas=deltas)
        assert run_fused(pkg, bad)[1] == pkg._lib.RPN_FLAG_NONFINITE
        assert pkg.ops.rpn_proposals(dev(logits), dev(deltas), dev(c["anchors"]), c["image_hw"], c["weights"], c["scale_clamp"], c["pre"],
                                     c["post"], c["min_box_size"], c["nms_thresh"]) is None
        rpn = _module(pkg, c["pre"], c["post"], c["nms_thresh"]).cuda().eval()
        got = _predict(rpn, bad)
        monkeypatch.setenv("LOCOV_FUSED_RPN", "0")
        want = _predict(rpn, bad)
        monkeypatch.delenv("LOCOV_FUSED_RPN")
        assert len(got) == len(want) == 1 and 0 < len(got[0]) < len(_predict(rpn, c)[0]) + 1
        assert torch.equal(got[0].proposal_boxes.tensor, want[0].proposal_boxes.tensor)
        assert torch.equal(got[0].objectness_logits, want[0].objectness_logits)
        assert bool(torch.isfinite(got[0].proposal_boxes.tensor).all()) and bool(torch.isfinite(got[0].objectness_logits).all())
        with pytest.raises(FloatingPointError):
            _predict(rpn.train(), bad)


def test_realistic_case_equals_the_torch_chain_on_the_device(pkg, monkeypatch):
    """50 x 84 x 15 anchors of the default generator, randn logits, 0.2 randn deltas, images 800 x 1333 and 600 x 1000,
    6 000 / 1 000 / 0.7: the fused path against find_top_rpn_proposals on the same device tensors, every output bit for bit."""
    from locov_amd.proposal_generator import DefaultAnchorGenerator, find_top_rpn_proposals
    from locov_amd.roi_heads.box_emb_head import Box2BoxTransform
    gen = DefaultAnchorGenerator([[32, 64, 128, 256, 512]], [[0.5, 1.0, 2.0]], [16]).cuda()
    anchors = gen([torch.zeros(2, 1, 50, 84, device="cuda")])[0].tensor
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2, 63000, generator=g).cuda()
    deltas = (0.2 * torch.randn(2, 63000, 4, generator=g)).cuda()
    sizes = [(800, 1333), (600, 1000)]
    b2b = Box2BoxTransform((1.0, 1.0, 1.0, 1.0))
    out, flags = pkg.ops._rpn_proposals_flags(logits, deltas, anchors, sizes, b2b.weights, b2b.scale_clamp, 6000, 1000, 0.0, 0.7)
    assert flags == 0
    boxes, scores, index, counts = out
    want = find_top_rpn_proposals([logits], [deltas], [anchors], sizes, b2b, 0.7, 6000, 1000, 0.0, False)
    assert counts == [len(w[2]) for w in want] and min(counts) > 500
    for n, (wb, ws, wi, _) in enumerate(want):
        k = counts[n]
        assert torch.equal(index[n, :k], wi)
        assert np.array_equal(bits(boxes[n, :k]), bits(wb)) and np.array_equal(bits(scores[n, :k]), bits(ws))
        assert bool((index[n, k:] == -1).all()) and not bits(boxes[n, k:]).any()


# ------------------------------------------------------------------------------------------------ module level
C, H, W, A, N = 32, 6, 8, 3, 2


@pytest.fixture(scope="module")
def small_rpn(pkg):
    from locov_amd.proposal_generator import build_proposal_generator
    from locov_amd.structures import ShapeSpec
    cfg = pkg.config.get_cfg()
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[32]]
    cfg.MODEL.RPN.POST_NMS_TOPK_TEST = 40
    torch.manual_seed(11)
    rpn = build_proposal_generator(cfg, {"res4": ShapeSpec(channels=C, stride=16)})
    with torch.no_grad():                                         # (std 0.01 would leave every logit next to 0)
        for layer in (rpn.rpn_head.conv, rpn.rpn_head.objectness_logits, rpn.rpn_head.anchor_deltas):
            layer.weight.mul_(10.0)
            layer.bias.normal_(std=0.1)
    g = torch.Generator().manual_seed(12)
    return rpn.cuda().eval(), torch.randn(N, C, H, W, generator=g).cuda()


def rel_err(got, want):
    want = want.double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30))


def test_head_against_conv2d_in_float64(pkg, small_rpn):
    """The tolerance is the one tests/test_gpu_res5_train.py applies to ops.conv3x3_nhwc_ex (rel_err < 2e-6 against float64)."""
    rpn, x = small_rpn
    head = rpn.rpn_head
    assert head.num_anchors == A
    d = lambda t: t.detach().double().cpu()
    t = F.relu(F.conv2d(d(x), d(head.conv.weight), d(head.conv.bias), padding=1))
    want_l = F.conv2d(t, d(head.objectness_logits.weight), d(head.objectness_logits.bias))
    want_d = F.conv2d(t, d(head.anchor_deltas.weight), d(head.anchor_deltas.bias))
    got_l, got_d = head([x])
    assert tuple(got_l[0].shape) == (N, A, H, W) and tuple(got_d[0].shape) == (N, 4 * A, H, W)
    assert rel_err(got_l[0], want_l) < 2e-6 and rel_err(got_d[0], want_d) < 2e-6
    flat_l, flat_d = head.flat_predictions([x])                   # the same numbers in the (y, x, a) flattening
    assert torch.equal(flat_l[0], got_l[0].permute(0, 2, 3, 1).reshape(N, -1))
    assert torch.equal(flat_d[0], got_d[0].reshape(N, A, 4, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, 4))
    assert flat_l[0].is_contiguous() and flat_d[0].is_contiguous()


def test_module_proposals_equal_the_reference_on_its_own_predictions(pkg, small_rpn):
    from locov_amd.structures import ImageList
    rpn, x = small_rpn
    sizes = [(96, 128), (80, 120)]
    props, losses = rpn(ImageList(torch.zeros(N, 3, 96, 128), sizes), {"res4": x})
    assert losses == {} and len(props) == N
    logits, deltas = rpn.rpn_head.flat_predictions([x])
    anchors = rpn.anchor_generator([x])[0].tensor
    chain = rpn.box2box_transform
    recs = ref.proposals(logits[0].cpu().numpy(), deltas[0].cpu().numpy(), anchors.cpu().numpy(), sizes, chain.weights, chain.scale_clamp,
                         6000, 40, 0.0, 0.7)
    # the reference decodes in float64, the kernel in fp32: the selection, the survivors and the logits are compared exactly, the
    # boxes to fp32 rounding of coordinates up to 128 (a few ulp of 2^-17)
    (fb, fl, fi, counts), flags = pkg.ops._rpn_proposals_flags(logits[0], deltas[0], anchors, sizes, chain.weights, chain.scale_clamp,
                                                               6000, 40, 0.0, 0.7)
    assert flags == 0 and counts == [r["count"] for r in recs]
    for n, (inst, r, size) in enumerate(zip(props, recs, sizes)):
        assert inst.image_size == size and len(inst) == r["count"] > 5
        assert fi[n, :r["count"]].cpu().tolist() == r["index"].tolist()           # the same anchors, in the same order
        assert np.array_equal(bits(inst.objectness_logits), r["logits"].view(np.int32))
        assert np.abs(inst.proposal_boxes.tensor.cpu().numpy().astype(np.float64) - r["boxes"]).max() < 1e-4
        assert torch.equal(inst.proposal_boxes.tensor, fb[n, :r["count"]]) and torch.equal(inst.objectness_logits, fl[n, :r["count"]])


def test_roi_heads_accept_the_proposals(pkg, small_rpn):
    from locov_amd.structures import ImageList, ShapeSpec
    rpn, x = small_rpn
    sizes = [(96, 128), (80, 120)]
    props, _ = rpn(ImageList(torch.zeros(N, 3, 96, 128), sizes), {"res4": x})
    cfg = pkg.config.get_cfg()
    cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = 32
    cfg.MODEL.RESNETS.WIDTH_PER_GROUP = 8
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = 96
    cfg.MODEL.ROI_HEADS.NAME = "EmbeddingRes5ROIHeads"
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0
    torch.manual_seed(3)
    heads = pkg.build_roi_heads(cfg, {"res4": ShapeSpec(channels=128, stride=16)}).cuda().eval()
    heads.box_predictor.set_class_embeddings(torch.randn(81, 96) * 0.05)
    heads.num_classes = heads.box_predictor.num_classes
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        inst, losses = heads(None, {"res4": torch.randn(N, 128, H, W, generator=g).cuda()}, props, None)
    assert losses == {} and len(inst) == N
    for i, size in zip(inst, sizes):
        assert i.image_size == size and len(i) > 0 and bool(torch.isfinite(i.pred_boxes.tensor).all())
