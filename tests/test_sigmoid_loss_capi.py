"""CPU-side checks of the sigmoid / federated classification loss (csrc/sigmoid_loss.hip: locov_fed_loss_classes,
locov_sigmoid_cls_loss, locov_sigmoid_cls_loss_workspace_bytes): the exports, argument errors before anything touches a device, the
predictor's constructor checks and configuration keys, and the torch chain of FastRCNNOutputLayers.losses against a literal float64
restatement of [D2-upstream, unverified] sigmoid_cross_entropy_loss / get_fed_loss_classes.  No compute on a device: there is no GPU
here."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locov_fed_loss_classes", "locov_sigmoid_cls_loss_workspace_bytes", "locov_sigmoid_cls_loss")


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_exports(lib):
    from locov_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "locov_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        m = re.search(r"^int(?:64_t)? %s\(([^;)]*)\);" % name, header, re.M)        # (the declaration, not its comment)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name       # header and binding agree
    assert lib.locov_abi_version() == _lib.ABI_VERSION == 8
    assert "#define LOCOV_ABI_VERSION 8" in header
    limit = int(re.search(r"#define LOCOV_FED_LOSS_MAX_CLASSES (\d+)", header).group(1))
    assert limit == _lib.FED_LOSS_MAX_CLASSES == ops.FED_LOSS_MAX_CLASSES >= ops.DETECT_MAX_CLASSES


def test_workspace_bytes(lib):
    f = lib.locov_sigmoid_cls_loss_workspace_bytes
    assert f(0) == 0 and f(-3) == 0
    assert 0 < f(1) <= f(5) <= f(1536) <= f(10 ** 7)
    assert f(10 ** 7) == f(10 ** 9)                                   # (a bounded number of blocks: grid-stride over the rows)
    assert f(1536) % 8 == 0


def _loss(lib, R=1536, C=1204, ld=None, scores=256, labels=512, mask=768, ws=1024, ws_bytes=None, loss=2048, dscores=4096, stats=8192):
    p = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = lib.locov_sigmoid_cls_loss_workspace_bytes(R)
    return lib.locov_sigmoid_cls_loss(p(scores), C if ld is None else ld, p(labels), p(mask), R, C, p(ws), ws_bytes, p(loss), p(dscores),
                                      p(stats), None)


@pytest.mark.parametrize("kw,msg", [
    ({"C": 1, "ld": 4}, b"K = C - 1 >= 1"),
    ({"C": 0, "ld": 4}, b"K = C - 1 >= 1"),
    ({"ld": 1203}, b"row stride"),
    ({"loss": 0}, b"null pointer"),
    ({"scores": 0}, b"null pointer"),
    ({"labels": 0}, b"null pointer"),
    ({"ws_bytes": 8}, b"workspace too small"),
    ({"ws": 0}, b"workspace too small"),
    ({"R": -1}, b"R >= 0"),
])
def test_loss_argument_errors_are_reported_before_any_launch(lib, kw, msg):
    """(the pointers are small fake addresses: a call that got as far as a launch would not return an argument error)"""
    rc = _loss(lib, **kw)
    assert rc < 0
    err = lib.locov_last_error()
    assert err.startswith(b"locov_sigmoid_cls_loss") and msg in err, err


def _fed(lib, labels=256, R=512, weights=512, rnd=768, K=1203, num_fed=50, mask=1024, counts=2048):
    p = ctypes.c_void_p
    return lib.locov_fed_loss_classes(p(labels), R, p(weights), p(rnd), K, num_fed, p(mask), p(counts), None)


@pytest.mark.parametrize("kw,msg", [
    ({"K": 0}, b"1 <= K <="),
    ({"K": -4}, b"1 <= K <="),
    ({"K": 32768}, b"1 <= K <="),
    ({"num_fed": -1}, b"num_fed >= 0"),
    ({"R": -1}, b"R >= 0"),
    ({"labels": 0}, b"null pointer"),
    ({"weights": 0}, b"null pointer"),
    ({"rnd": 0}, b"null pointer"),
    ({"mask": 0}, b"null pointer"),
    ({"counts": 0}, b"null pointer"),
])
def test_fed_argument_errors_are_reported_before_any_launch(lib, kw, msg):
    rc = _fed(lib, **kw)
    assert rc < 0
    err = lib.locov_last_error()
    assert err.startswith(b"locov_fed_loss_classes") and msg in err, err


def test_ops_reject_host_tensors_and_bad_arguments():
    from locov_amd import ops
    from locov_amd._lib import LocovError
    y = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(LocovError):
        ops.sigmoid_cls_loss(torch.zeros(3, 4), y)
    with pytest.raises(TypeError):
        ops.sigmoid_cls_loss([[0.0, 0.0]], y[:1])
    with pytest.raises(LocovError):
        ops.fed_loss_classes(y, torch.ones(4), 2)
    with pytest.raises(TypeError):
        ops.fed_loss_classes(y, [1.0, 1.0], 2)


# ------------------------------------------------------------------ the predictor: constructor, configuration, torch chain

def _predictor(num_classes, **kw):
    from locov_amd.roi_heads import box_emb_head as beh
    return beh.FastRCNNOutputLayers(8, box2box_transform=beh.Box2BoxTransform((10.0, 10.0, 5.0, 5.0)), num_classes=num_classes,
                                    cls_agnostic_bbox_reg=True, **kw)


def _proposals(gt_classes):
    from locov_amd.structures import Boxes, Instances
    p = Instances((100, 100))
    n = len(gt_classes)
    p.proposal_boxes = Boxes(torch.tensor([[10., 10., 50., 50.]] * n).reshape(n, 4))
    p.gt_boxes = Boxes(torch.tensor([[12., 8., 48., 55.]] * n).reshape(n, 4))
    p.gt_classes = torch.as_tensor(gt_classes, dtype=torch.int64)
    return p


def test_constructor_checks():
    bp = _predictor(3)
    assert bp.use_sigmoid_ce is False and bp.use_fed_loss is False and bp.fed_loss_num_classes == 50
    with pytest.raises(AssertionError, match="sigmoid"):
        _predictor(3, use_fed_loss=True, get_fed_loss_cls_weights=lambda: torch.ones(3))
    with pytest.raises(AssertionError, match="num_classes"):
        _predictor(3, use_fed_loss=True, use_sigmoid_ce=True, get_fed_loss_cls_weights=lambda: torch.ones(4))
    bp = _predictor(3, use_fed_loss=True, use_sigmoid_ce=True, get_fed_loss_cls_weights=lambda: [1.0, 4.0, 9.0], fed_loss_num_classes=2)
    assert bp.fed_loss_cls_weights.tolist() == [1.0, 4.0, 9.0] and bp.fed_loss_cls_weights.dtype == torch.float32
    assert "fed_loss_cls_weights" in dict(bp.named_buffers()) and "fed_loss_cls_weights" not in bp.state_dict()
    assert sorted(bp.state_dict()) == sorted(_predictor(3).state_dict())              # checkpoint keys do not change


@pytest.mark.parametrize("name", ["FastRCNNOutputLayers", "EmbeddingFastRCNNOutputLayers", "EmbeddingGroundingFastRCNNOutputLayers"])
def test_from_config_reads_the_four_keys(monkeypatch, name):
    import locov_amd
    from locov_amd.roi_heads import box_emb_head as beh
    cfg = locov_amd.config.get_cfg()
    box_head = cfg.MODEL.ROI_BOX_HEAD
    assert (box_head.USE_SIGMOID_CE, box_head.USE_FED_LOSS, box_head.FED_LOSS_FREQ_WEIGHT_POWER, box_head.FED_LOSS_NUM_CLASSES) == \
        (False, False, 0.5, 50)
    box_head.NAME = name
    box_head.CLS_AGNOSTIC_BBOX_REG = True
    box_head.EMBEDDING_BASED = name != "FastRCNNOutputLayers"
    box_head.EMB_DIM = 16
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = 5
    bp = locov_amd.build_box_predictor(cfg, 8)
    assert bp.use_sigmoid_ce is False and bp.use_fed_loss is False and not hasattr(bp, "fed_loss_cls_weights")

    box_head.USE_SIGMOID_CE = True
    box_head.USE_FED_LOSS = True
    box_head.FED_LOSS_FREQ_WEIGHT_POWER = 0.25
    box_head.FED_LOSS_NUM_CLASSES = 3
    cfg.DATASETS.TRAIN = ("lvis_v1_train",)
    monkeypatch.setitem(sys.modules, "detectron2.data", None)                   # (Detectron2 absent, wherever this runs)
    with pytest.raises(RuntimeError, match="Detectron2 is not importable"):     # (the message names what is missing)
        locov_amd.build_box_predictor(cfg, 8)
    seen = []

    def weights(dataset_names, freq_weight_power):
        seen.append((tuple(dataset_names), freq_weight_power))
        return torch.tensor([1.0, 16.0, 81.0, 256.0, 625.0]) ** freq_weight_power
    monkeypatch.setattr(beh, "get_fed_loss_cls_weights", weights)
    bp = locov_amd.build_box_predictor(cfg, 8)
    assert seen == [(("lvis_v1_train",), 0.25)]
    assert bp.use_sigmoid_ce is True and bp.use_fed_loss is True and bp.fed_loss_num_classes == 3
    assert torch.allclose(bp.fed_loss_cls_weights, torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]))
    box_head.USE_FED_LOSS = False
    bp = locov_amd.build_box_predictor(cfg, 8)
    assert bp.use_sigmoid_ce is True and bp.use_fed_loss is False


def upstream_sigmoid_loss(scores, gt_classes, fed_classes=None):
    """[D2-upstream, unverified] sigmoid_cross_entropy_loss, literally, in the dtype of the scores; fed_classes: the class indices
    get_fed_loss_classes returned (the background index K may be among them)."""
    N, K = scores.shape[0], scores.shape[1] - 1
    target = scores.new_zeros(N, K + 1)
    target[range(len(gt_classes)), gt_classes] = 1
    target = target[:, :K]
    cls_loss = F.binary_cross_entropy_with_logits(scores[:, :-1], target, reduction="none")
    if fed_classes is not None:
        fed_loss_classes_mask = fed_classes.new_zeros(K + 1)
        fed_loss_classes_mask[fed_classes] = 1
        fed_loss_classes_mask = fed_loss_classes_mask[:K]
        weight = fed_loss_classes_mask.view(1, K).expand(N, K).to(scores.dtype)
    else:
        weight = 1
    return torch.sum(cls_loss * weight) / N


def test_cpu_torch_chain_equals_the_upstream_restatement_in_float64():
    g = torch.Generator().manual_seed(3)
    K = 6
    scores = (torch.randn(9, K + 1, generator=g) * 3.0).requires_grad_(True)
    labels = torch.tensor([0, 2, 2, K, K, 5, K, 0, K])
    s64 = scores.detach().double().requires_grad_(True)

    bp = _predictor(K, use_sigmoid_ce=True)
    out = bp.losses((scores, torch.zeros(9, 4)), [_proposals(labels)])
    want = upstream_sigmoid_loss(s64, labels)
    assert abs(float(out["loss_cls"].detach()) - float(want.detach())) <= 1e-5 * max(1.0, abs(float(want)))
    out["loss_cls"].backward()
    want.backward()
    assert float((scores.grad.double() - s64.grad).abs().max()) * 9 <= 5e-7
    assert float(scores.grad[:, -1].abs().max()) == 0.0              # the background column never enters the loss
    assert bp._fed_loss_mask is None
    pred = scores.detach().argmax(1)
    assert bp.classification_stats()["cls_accuracy"] == float((pred == labels).sum()) / 9

    # federated: classes {0, 2, 5} and the background are present (4 of a budget of 5), so ONE class is sampled among {1, 3, 4}; class 3
    # has weight 0 and cannot be; the draw is the predictor's own (torch.manual_seed), restated here
    weights = torch.tensor([3.0, 1.0, 2.0, 0.0, 2.0, 1.0])
    bp = _predictor(K, use_sigmoid_ce=True, use_fed_loss=True, get_fed_loss_cls_weights=lambda: weights, fed_loss_num_classes=5)
    torch.manual_seed(11)
    rnd = torch.empty(K).exponential_()
    key = weights / rnd
    sampled = 1 if key[1] >= key[4] else 4
    torch.manual_seed(11)
    scores.grad = None
    out = bp.losses((scores, torch.zeros(9, 4)), [_proposals(labels)])
    assert bp._fed_loss_mask.tolist() == [1, int(sampled == 1), 1, 0, int(sampled == 4), 1]
    assert bp._fed_loss_counts.tolist() == [4, 1]
    s64.grad = None
    want = upstream_sigmoid_loss(s64, labels, torch.tensor([0, 2, 5, K, sampled]))
    assert abs(float(out["loss_cls"].detach()) - float(want.detach())) <= 1e-5 * max(1.0, abs(float(want)))
    out["loss_cls"].backward()
    want.backward()
    assert float((scores.grad.double() - s64.grad).abs().max()) * 9 <= 5e-7
    off = [c for c in range(K) if c not in (0, 2, 5, sampled)]
    assert float(scores.grad[:, off].abs().max()) == 0.0            # masked-out classes: exact zeros

    # a budget the labels already fill: nothing is sampled;  more asked for than can be sampled: every class with a weight > 0
    bp.fed_loss_num_classes = 4
    bp.losses((scores, torch.zeros(9, 4)), [_proposals(labels)])
    assert bp._fed_loss_mask.tolist() == [1, 0, 1, 0, 0, 1] and bp._fed_loss_counts.tolist() == [4, 0]
    bp.fed_loss_num_classes = 40
    bp.losses((scores, torch.zeros(9, 4)), [_proposals(labels)])
    assert bp._fed_loss_mask.tolist() == [1, 1, 1, 0, 1, 1] and bp._fed_loss_counts.tolist() == [4, 2]


def test_cpu_torch_chain_gives_invalid_labels_no_loss_and_counts_them():
    K = 3
    scores = torch.tensor([[1., -2., 0.5, 0.], [0.3, 0.2, -1., 2.], [4., 4., 4., 4.]], requires_grad=True)
    bp = _predictor(K, use_sigmoid_ce=True)
    out = bp.losses((scores, torch.zeros(3, 4)), [_proposals([1, K, -100])])
    want = upstream_sigmoid_loss(scores.detach().double()[:2], torch.tensor([1, K])) * 2 / 3       # the divisor stays R
    assert abs(float(out["loss_cls"].detach()) - float(want.detach())) <= 1e-5 * max(1.0, abs(float(want)))
    out["loss_cls"].backward()
    assert float(scores.grad[2].abs().max()) == 0.0
    with pytest.raises(ValueError, match="1 of 3"):
        bp.classification_stats()


def test_cpu_inference_probabilities_follow_the_loss_type():
    scores = torch.tensor([[1., -2., 0.5, 0.], [0.3, 0.2, -1., 2.]])
    p = _proposals([0, 0])
    assert torch.equal(_predictor(3, use_sigmoid_ce=True).predict_probs((scores, None), [p])[0], torch.sigmoid(scores))
    assert torch.equal(_predictor(3).predict_probs((scores, None), [p])[0], F.softmax(scores, dim=-1))
    assert torch.equal(_predictor(3, use_sigmoid_ce=True).losses((scores[:0], torch.zeros(0, 4)), [])["loss_cls"], scores[:0].sum() * 0)
