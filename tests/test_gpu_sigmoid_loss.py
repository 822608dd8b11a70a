"""The sigmoid / federated classification loss on the device (csrc/sigmoid_loss.hip: ops.sigmoid_cls_loss = locov_sigmoid_cls_loss,
ops.fed_loss_classes = locov_fed_loss_classes, and FastRCNNOutputLayers.losses / inference with use_sigmoid_ce / use_fed_loss through
them) against float64 torch on the CPU.

Inputs: logits of sigma 3, labels drawn from [0, K] (K: background), every 5th row background, every 7th label invalid (-100).
Gates:
  value     |loss - loss64| <= 1e-5 max(1, |loss64|)                      (the gate of tests/test_gpu_cls_loss.py for a sum formed the
            same way: fp32 terms, fp64 accumulation)
  gradient  e = R max|g - g64| <= 2 e_torch + 1.2e-7, e_torch the same quantity for torch's own fp32 chain (zeros target, index-put,
            binary_cross_entropy_with_logits, mask, sum / R) on the device on the same inputs; factor and floor are those of
            tests/test_gpu_cls_loss.py.  Both figures are printed per shape.
  stats     the six integers equal the upstream formulas ([D2-upstream, unverified] _log_classification_stats) evaluated with torch
            on the CPU from the same fp32 logits; a label outside [0, K] is invalid (the sigmoid loss has no ignore index).
  classes   the federated mask and counts equal a torch restatement ([D2-upstream, unverified] get_fed_loss_classes, the multinomial
            written as the top keys weights / rnd) exactly.
"""
import functools
import importlib.util
import os
import subprocess
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -100
SHAPES = [(1, 2), (3, 2), (5, 66), (257, 49), (257, 81), (1536, 1204), (4099, 3), (4099, 4)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import _lib, ops
    _lib.load()
    return ops


def _inputs(R, C):
    g = torch.Generator().manual_seed(1000 * R + C)
    scores = torch.randn(R, C, generator=g) * 3.0
    labels = torch.randint(0, C, (R,), generator=g)
    labels[4::5] = C - 1                                              # background rows
    labels[6::7] = INVALID
    mask = (torch.rand(C - 1, generator=g) < 0.5).to(torch.uint8)
    return scores, labels, mask


def upstream_stats(scores, labels):
    """[D2-upstream, unverified] _log_classification_stats, literally, + the labels the index-put of the sigmoid loss fails on."""
    num_instances = labels.numel()
    pred_classes = scores.argmax(dim=1)
    bg_class_ind = scores.shape[1] - 1
    fg_inds = (labels >= 0) & (labels < bg_class_ind)
    num_fg = fg_inds.nonzero().numel()
    fg_gt_classes = labels[fg_inds]
    fg_pred_classes = pred_classes[fg_inds]
    num_false_negative = (fg_pred_classes == bg_class_ind).nonzero().numel()
    num_accurate = (pred_classes == labels).nonzero().numel()
    fg_num_accurate = (fg_pred_classes == fg_gt_classes).nonzero().numel()
    num_invalid = ((labels < 0) | (labels > bg_class_ind)).nonzero().numel()
    return [num_instances, num_fg, num_accurate, fg_num_accurate, num_false_negative, num_invalid]


def upstream_chain(scores, labels, mask=None):
    """[D2-upstream, unverified] sigmoid_cross_entropy_loss as upstream writes it, in the dtype and on the device of the scores: the
    zeros target, the index-put, the slice, binary_cross_entropy_with_logits, the class-mask broadcast, sum / N.  Rows with an invalid
    label (upstream's index-put fails on them) contribute nothing; the divisor stays N."""
    N, K = scores.shape[0], scores.shape[1] - 1
    valid = (labels >= 0) & (labels <= K)
    rows = valid.nonzero().view(-1)
    target = scores.new_zeros(N, K + 1)
    target[rows, labels[rows]] = 1
    target = target[:, :K]
    cls_loss = F.binary_cross_entropy_with_logits(scores[:, :-1], target, reduction="none")
    weight = valid.view(N, 1).to(scores.dtype)
    if mask is not None:
        weight = weight * mask.view(1, K).expand(N, K).to(scores.dtype)
    return torch.sum(cls_loss * weight) / N


def _f64(scores, labels, mask=None):
    s = scores.double().requires_grad_(True)
    loss = upstream_chain(s, labels, mask)
    loss.backward()
    return loss.detach(), s.grad


@functools.lru_cache(maxsize=None)
def _case(R, C, masked):
    """One shape's inputs, float64 expectation and torch's own fp32 error on the device; computed once, never modified."""
    scores, labels, mask = _inputs(R, C)
    mask = mask if masked else None
    loss64, g64 = _f64(scores, labels, mask)
    s = scores.cuda().requires_grad_(True)
    upstream_chain(s, labels.cuda(), None if mask is None else mask.cuda()).backward()
    e_torch = R * float((s.grad.cpu().double() - g64).abs().max())
    return {"scores": scores, "labels": labels, "mask": mask, "loss64": loss64, "g64": g64, "e_torch": e_torch,
            "stats": upstream_stats(scores, labels)}


def _run(ops, c, grad=True, **kw):
    s = c["scores"].cuda().requires_grad_(grad)
    loss, stats = ops.sigmoid_cls_loss(s, c["labels"].cuda(), None if c["mask"] is None else c["mask"].cuda(), **kw)
    return s, loss, stats


@pytest.mark.parametrize("masked", [False, True], ids=["all_classes", "class_mask"])
@pytest.mark.parametrize("R,C", SHAPES)
def test_value_gradient_and_stats_against_float64(ops, R, C, masked):
    c = _case(R, C, masked)
    s, loss, stats = _run(ops, c)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and stats.dtype == torch.int64 and tuple(stats.shape) == (6,)
    loss.backward()
    got, want = float(loss.detach()), float(c["loss64"])
    g = s.grad.cpu()
    e = R * float((g.double() - c["g64"]).abs().max())
    print(f"sigmoid_cls_loss [{R}, {C}] masked={masked}: loss {got:.9g} (float64 {want:.9g}, diff {abs(got - want):.3g}); "
          f"R max|g - g64|: e = {e:.3e}, e_torch = {c['e_torch']:.3e}")
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
    assert e <= 2.0 * c["e_torch"] + 1.2e-7
    # exact zeros: the background column, masked-out classes, invalid rows
    assert float(g[:, -1].abs().sum()) == 0.0
    invalid = (c["labels"] < 0) | (c["labels"] > C - 1)
    assert float(g[invalid].abs().sum()) == 0.0
    if masked:
        assert float(g[:, :-1][:, c["mask"] == 0].abs().sum()) == 0.0
        on = g[~invalid][:, :-1][:, c["mask"] == 1]
        assert on.numel() == 0 or float(on.abs().min()) > 0.0
    assert stats.tolist() == c["stats"]


def test_hand_built_rows(ops):
    """Equal maxima (the lowest index wins), a background row, a false negative, labels below and above the range."""
    scores = torch.tensor([[2., 2., 0., 0.],       # gt 1: two equal maxima -> pred 0, wrong
                           [0., -1., -2., 0.],     # gt 0: ties the background's 0 -> pred 0, accurate
                           [-1., -1., -1., 0.],    # gt bg, pred bg
                           [-1., -1., -1., 0.],    # gt 2: pred bg -> false negative
                           [1., 0., 0., 0.],       # gt 7: out of range
                           [1., 0., 0., 0.]])      # gt -1: out of range
    labels = torch.tensor([1, 0, 3, 2, 7, -1])
    assert upstream_stats(scores, labels) == [6, 3, 2, 1, 1, 2]
    c = {"scores": scores, "labels": labels, "mask": None}
    s, loss, stats = _run(ops, c)
    assert stats.tolist() == [6, 3, 2, 1, 1, 2]
    loss.backward()
    want, g64 = _f64(scores, labels)
    assert abs(float(loss) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    assert float(s.grad[4:].abs().sum()) == 0.0 and float(s.grad[:, 3].abs().sum()) == 0.0
    bg = s.grad[2, :3].cpu().double()                                  # a background row is all-negative: sigmoid(x) / R
    assert float((bg - torch.sigmoid(scores[2, :3].double()) / 6).abs().max()) * 6 <= 1.2e-7


def test_backward_scales_by_the_incoming_gradient(ops):
    c = _case(257, 81, True)
    s, loss, _ = _run(ops, c)
    (loss * 0.25).backward()
    s2, loss2, _ = _run(ops, c)
    loss2.backward()
    assert torch.equal(s.grad, s2.grad * 0.25)                        # (a power of two: exact)


@pytest.mark.parametrize("R,C", [(5, 2), (257, 81), (1536, 1204), (4099, 4)])
def test_column_slice_of_a_wider_matrix_gives_the_bits_of_its_copy(ops, R, C):
    """ld > C and a base that is 4 bytes past a 16-byte boundary: scalar loads, against the contiguous copy (16-byte loads at C = 1204
    and C = 4; at R = 4099 there are more row groups than blocks, so a wave takes a second row)."""
    c = _case(R, C, True)
    wide = torch.randn(R, C + 7, generator=torch.Generator().manual_seed(5)).cuda()
    wide[:, 1:1 + C] = c["scores"].cuda()
    view = wide[:, 1:1 + C].requires_grad_(True)
    assert view.stride(0) == C + 7 and view.data_ptr() % 16 == 4
    loss_v, stats_v = ops.sigmoid_cls_loss(view, c["labels"].cuda(), c["mask"].cuda())
    loss_v.backward()
    s, loss, stats = _run(ops, c)
    loss.backward()
    assert torch.equal(loss_v, loss) and torch.equal(stats_v, stats)
    assert view.grad.is_contiguous() and torch.equal(view.grad, s.grad)


@pytest.mark.parametrize("R,C", [(257, 81), (1536, 1204), (4099, 4)])
def test_two_calls_give_the_same_bits(ops, R, C):
    c = _case(R, C, True)
    outs = []
    for _ in range(2):
        s, loss, stats = _run(ops, c)
        loss.backward()
        outs.append((loss.detach().clone(), s.grad.clone(), stats.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_no_gradient_buffer_without_requires_grad_and_null_stats(ops):
    R, C = 1536, 1204
    c = _case(R, C, False)
    s, y = c["scores"].cuda(), c["labels"].cuda()
    ops.sigmoid_cls_loss(s, y)                                        # (the cached workspace exists from here on)
    peaks = {}
    for grad in (False, True):
        x = s.clone().requires_grad_(grad)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, stats = ops.sigmoid_cls_loss(x, y)
        torch.cuda.synchronize()
        peaks[grad] = torch.cuda.max_memory_allocated() - base
        assert loss.requires_grad == grad
    assert peaks[False] < R * C * 4 // 8 and peaks[True] >= R * C * 4
    with torch.no_grad():                                             # (nor under no_grad)
        x = s.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ops.sigmoid_cls_loss(x, y)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base < R * C * 4 // 8
    ref, ref_stats = ops.sigmoid_cls_loss(s, y)
    loss, none = ops.sigmoid_cls_loss(s, y, want_stats=False)
    assert none is None and torch.equal(loss, ref)
    x = s.clone().requires_grad_(True)
    loss, none = ops.sigmoid_cls_loss(x, y, want_stats=False)
    loss.backward()
    assert none is None and torch.equal(loss, ref) and x.grad is not None


def test_argument_checks(ops):
    from locov_amd._lib import LocovError
    s, y, m = torch.zeros(4, 5).cuda(), torch.zeros(4, dtype=torch.int64).cuda(), torch.ones(4, dtype=torch.uint8).cuda()
    w = torch.ones(4).cuda()
    with pytest.raises(TypeError):
        ops.sigmoid_cls_loss(s.half(), y)
    with pytest.raises(TypeError):
        ops.sigmoid_cls_loss(s, y.int())
    with pytest.raises(TypeError):
        ops.sigmoid_cls_loss(s, y, m.bool())
    with pytest.raises(LocovError):
        ops.sigmoid_cls_loss(s, y.cpu())
    with pytest.raises(LocovError):
        ops.sigmoid_cls_loss(s, y, m.cpu())
    with pytest.raises(ValueError):
        ops.sigmoid_cls_loss(s, y[:3])
    with pytest.raises(ValueError):
        ops.sigmoid_cls_loss(s, y, m[:3])
    with pytest.raises(ValueError):
        ops.sigmoid_cls_loss(s[0], y)
    with pytest.raises(ValueError):
        ops.sigmoid_cls_loss(s[:, :1], y)
    with pytest.raises(ValueError):
        ops.sigmoid_cls_loss(s[:0], y[:0])
    with pytest.raises(TypeError):
        ops.fed_loss_classes(y.int(), w, 2)
    with pytest.raises(TypeError):
        ops.fed_loss_classes(y, w.double(), 2)
    with pytest.raises(LocovError):
        ops.fed_loss_classes(y.cpu(), w, 2)
    with pytest.raises(LocovError):
        ops.fed_loss_classes(y, w, 2, rnd=torch.ones(4))
    with pytest.raises(ValueError):
        ops.fed_loss_classes(y, w, -1)
    with pytest.raises(ValueError):
        ops.fed_loss_classes(y, w, 2, rnd=w[:3])
    with pytest.raises(ValueError):
        ops.fed_loss_classes(y, w[:0], 2)


# ------------------------------------------------------------------ the federated class set

def restated_fed_loss_classes(labels, weights, num_fed, rnd):
    """[D2-upstream, unverified] get_fed_loss_classes on the CPU, the multinomial written as the top keys weights / rnd (an IEEE fp32
    division), equal keys to the lower class index; too few candidates: all of them."""
    K = weights.numel()
    unique = torch.unique(labels[(labels >= 0) & (labels <= K)])
    n_present = len(unique)
    present = torch.zeros(K + 1, dtype=torch.bool)
    present[unique] = True
    ok = (~present[:K] & torch.isfinite(weights) & (weights > 0)).tolist()
    key = (weights / rnd).tolist()
    cand = sorted((c for c in range(K) if ok[c]), key=lambda c: (-key[c], c))
    n_take = min(max(0, num_fed - n_present), len(cand))
    mask = present[:K].clone()
    mask[cand[:n_take]] = True
    return mask.to(torch.uint8), [n_present, n_take]


def _label_sets(K, g):
    sets = {
        "fills_budget": torch.arange(0, min(K, 60)).repeat(3),                       # (>= num_fed = 50 at K >= 65: nothing is sampled)
        "all_background": torch.full((9,), K),
        "with_invalid": torch.cat([torch.randint(0, K + 1, (40,), generator=g), torch.tensor([-1, -100, K + 1, 2 ** 40])]),
        "many_rows": torch.randint(0, K + 1, (3000,), generator=g),                  # (grid-stride over the labels inside the block)
        "no_rows": torch.empty(0, dtype=torch.int64),
    }
    return sets


@pytest.mark.parametrize("K", [1, 5, 65, 1203])
def test_fed_loss_classes_equal_the_restatement(ops, K):
    g = torch.Generator().manual_seed(K)
    weights = torch.rand(K, generator=g) * 20 + 0.5
    sparse = weights.clone()                                           # weights with zeros (and one that is not finite): too few candidates
    sparse[torch.rand(K, generator=g) < 0.8] = 0.0
    if K > 2:
        sparse[1] = float("inf")
    rnd = torch.empty(K).exponential_(generator=g).clamp_min(1e-30)
    for name, labels in _label_sets(K, g).items():
        for w in (weights, sparse):
            for num_fed in sorted({0, 1, 50, K + 5}):
                want_mask, want_counts = restated_fed_loss_classes(labels, w, num_fed, rnd)
                mask, counts = ops.fed_loss_classes(labels.cuda(), w.cuda(), num_fed, rnd=rnd.cuda())
                assert mask.dtype == torch.uint8 and counts.dtype == torch.int32 and mask.is_cuda and counts.is_cuda
                assert counts.tolist() == want_counts, (name, num_fed)
                assert torch.equal(mask.cpu(), want_mask), (name, num_fed)
    # (the cases really are what they are named for)
    if K >= 65:
        assert restated_fed_loss_classes(_label_sets(K, g)["fills_budget"], weights, 50, rnd)[1] == [60, 0]
    assert restated_fed_loss_classes(torch.full((9,), K), weights, 50, rnd)[1] == [1, min(49, K)]
    n_sparse = int(((sparse > 0) & torch.isfinite(sparse)).sum())
    assert restated_fed_loss_classes(torch.full((9,), K), sparse, K + 5, rnd)[1] == [1, n_sparse] and n_sparse < K + 4


def test_fed_loss_classes_equal_keys_at_the_cut_go_to_the_lower_index(ops):
    # keys: class 0 -> 8, 1 -> 4, 2 -> 4, 3 -> 4, 4 -> 2, 5 -> present, 6 -> 4 (weight 2 / rnd 0.5)
    weights = torch.tensor([8.0, 4.0, 4.0, 4.0, 2.0, 9.0, 2.0])
    rnd = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5])
    labels = torch.tensor([5, 5, 7])                                   # class 5 and the background: 2 present
    for num_fed, want in [(3, [1, 0, 0, 0, 0, 1, 0]), (4, [1, 1, 0, 0, 0, 1, 0]), (5, [1, 1, 1, 0, 0, 1, 0]), (6, [1, 1, 1, 1, 0, 1, 0]),
                          (7, [1, 1, 1, 1, 0, 1, 1]), (8, [1, 1, 1, 1, 1, 1, 1])]:
        mask, counts = ops.fed_loss_classes(labels.cuda(), weights.cuda(), num_fed, rnd=rnd.cuda())
        assert mask.tolist() == want and counts.tolist() == [2, num_fed - 2], num_fed
        assert restated_fed_loss_classes(labels, weights, num_fed, rnd)[0].tolist() == want


def test_fed_loss_classes_draw_their_own_keys_reproducibly(ops):
    K = 1203
    g = torch.Generator().manual_seed(2)
    weights = (torch.rand(K, generator=g) * 100 + 1).sqrt().cuda()
    labels = torch.randint(0, 21, (512,), generator=g)                               # at most 21 classes present, the rest to sample
    n_present = len(torch.unique(labels))
    labels = labels.cuda()
    masks = []
    for seed in (9, 9, 10):
        torch.manual_seed(seed)
        mask, counts = ops.fed_loss_classes(labels, weights, 50)
        assert 0 < n_present <= 21 and counts.tolist() == [n_present, 50 - n_present] and int(mask.sum()) == 50
        masks.append(mask)
    assert torch.equal(masks[0], masks[1]) and not torch.equal(masks[0], masks[2])
    torch.manual_seed(9)                                                              # the draw is the documented one
    rnd = torch.empty(K, device="cuda").exponential_()
    assert torch.equal(ops.fed_loss_classes(labels, weights, 50, rnd=rnd)[0], masks[0])


# ------------------------------------------------------------------ through the predictor

FED_WEIGHTS = [float(1 + (7 * c) % 13) ** 0.5 for c in range(48)]


def _embedding_predictor(use_fed_loss=False, num_fed=20):
    import locov_amd
    from locov_amd.roi_heads import box_emb_head as beh
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = 64
    cfg.MODEL.ROI_BOX_HEAD.FREEZE_EMB_PRED = False
    cfg.MODEL.ROI_HEADS.DETACH_CLASS_PREDICTOR = False
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = 48
    cfg.MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE = True
    cfg.MODEL.ROI_BOX_HEAD.USE_FED_LOSS = use_fed_loss
    cfg.MODEL.ROI_BOX_HEAD.FED_LOSS_NUM_CLASSES = num_fed
    torch.manual_seed(4)
    real = beh.get_fed_loss_cls_weights
    beh.get_fed_loss_cls_weights = lambda names, power: torch.tensor(FED_WEIGHTS)    # (the seam tests replace)
    try:
        bp = locov_amd.build_box_predictor(cfg, 128).cuda().train()
    finally:
        beh.get_fed_loss_cls_weights = real
    g = torch.Generator().manual_seed(7)
    bank = torch.randn(49, 64, generator=g) * 2.0                     # 48 + 1 bank, background row exactly 0
    bank[-1] = 0
    bp.set_class_embeddings(bank)
    return bp, g


def _sampled_batch(g):
    """2 images x 16 sampled proposals with a 48 + 1 bank."""
    from locov_amd.structures import Boxes, Instances
    props = []
    for _ in range(2):
        p = Instances((800, 1333))
        xy = torch.rand(16, 2, generator=g) * 500
        p.proposal_boxes = Boxes(torch.cat([xy, xy + 20 + torch.rand(16, 2, generator=g) * 100], 1).cuda())
        p.gt_boxes = Boxes((p.proposal_boxes.tensor + 3.0))
        y = torch.randint(0, 48, (16,), generator=g)
        y[4:] = 48                                                    # a quarter foreground, the rest background
        p.gt_classes = y.cuda()
        props.append(p)
    x = torch.relu(torch.randn(32, 128, generator=g)).cuda().requires_grad_(True)
    return props, x


@pytest.mark.parametrize("use_fed_loss", [False, True], ids=["sigmoid_ce", "fed_loss"])
def test_embedding_predictor_losses_run_the_fused_calls(ops, monkeypatch, use_fed_loss):
    bp, g = _embedding_predictor(use_fed_loss)
    assert bp.use_sigmoid_ce and bp.use_fed_loss == use_fed_loss
    props, x = _sampled_batch(g)
    calls = []
    real_loss, real_fed = ops.sigmoid_cls_loss, ops.fed_loss_classes
    monkeypatch.setattr(ops, "sigmoid_cls_loss", lambda *a, **k: (calls.append("loss"), real_loss(*a, **k))[1])
    monkeypatch.setattr(ops, "fed_loss_classes", lambda *a, **k: (calls.append("fed"), real_fed(*a, **k))[1])
    monkeypatch.setattr(ops, "cls_loss", lambda *a, **k: pytest.fail("the softmax loss ran"))
    scores, deltas = bp(x)
    assert tuple(scores.shape) == (32, 49) and scores.requires_grad
    torch.manual_seed(21)
    losses = bp.losses((scores, deltas), props, boxes_validated=True)
    assert calls == (["fed", "loss"] if use_fed_loss else ["loss"]) and sorted(losses) == ["loss_box_reg", "loss_cls"]
    labels = torch.cat([p.gt_classes for p in props]).cpu()
    mask = None
    if use_fed_loss:
        torch.manual_seed(21)
        rnd = torch.empty(48, device="cuda").exponential_().cpu()
        mask, counts = restated_fed_loss_classes(labels, torch.tensor(FED_WEIGHTS), 20, rnd)
        assert torch.equal(bp._fed_loss_mask.cpu(), mask) and bp._fed_loss_counts.tolist() == counts
        assert counts[0] + counts[1] == 20 and 0 < counts[1]
    else:
        assert bp._fed_loss_mask is None
    want, _ = _f64(scores.detach().cpu(), labels, mask)
    assert abs(float(losses["loss_cls"]) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    losses["loss_cls"].backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.0
    assert bp.emb_pred.weight.grad is not None and float(bp.emb_pred.weight.grad.abs().max()) > 0.0
    stats = bp.classification_stats()
    up = upstream_stats(scores.detach().cpu(), labels)
    assert stats == {"cls_accuracy": up[2] / 32, "fg_cls_accuracy": up[3] / up[1], "false_negative": up[4] / up[1]}


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import torch
sys.path.insert(0, {tests!r})
import test_gpu_sigmoid_loss as T
from locov_amd import ops
from locov_amd.roi_heads import box_emb_head as beh
assert beh._FUSED_BOX_LOSS is False

def no_fused(*a, **k):
    raise AssertionError("a fused loss op called with LOCOV_FUSED_LOSSES=0")
ops.sigmoid_cls_loss = ops.fed_loss_classes = ops.cls_loss = no_fused
bp, g = T._embedding_predictor(True)
props, x = T._sampled_batch(g)
scores, deltas = bp(x)
torch.manual_seed(21)
losses = bp.losses((scores, deltas), props, boxes_validated=True)
stats = bp.classification_stats()
print("CHILD", float(losses["loss_cls"]).hex(), "".join(str(v) for v in bp._fed_loss_mask.tolist()), stats["cls_accuracy"])
"""


def test_switch_off_gives_the_torch_chain_with_the_same_class_set_in_a_fresh_process(ops):
    """LOCOV_FUSED_LOSSES is read at import: a child process with it at 0 and the same seed runs the torch chain; the fused value of this
    process meets the gate against it and the class set is the same."""
    env = dict(os.environ, LOCOV_FUSED_LOSSES="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("CHILD")][-1].split()
    torch_value, torch_mask, torch_acc = float.fromhex(line[1]), line[2], float(line[3])
    bp, g = _embedding_predictor(True)
    props, x = _sampled_batch(g)
    scores, deltas = bp(x)
    torch.manual_seed(21)
    losses = bp.losses((scores, deltas), props, boxes_validated=True)
    assert abs(float(losses["loss_cls"]) - torch_value) <= 1e-5 * max(1.0, abs(torch_value))
    assert "".join(str(v) for v in bp._fed_loss_mask.tolist()) == torch_mask and len(torch_mask) == 48
    assert bp.classification_stats()["cls_accuracy"] == torch_acc


def test_losses_add_no_host_wait(ops):
    """losses() with the federated sigmoid loss and the work queued after it make no device-to-host read
    (torch.cuda.set_sync_debug_mode, as tools/find_syncs.py); classification_stats() makes exactly one."""
    bp, g = _embedding_predictor(True)
    props, x = _sampled_batch(g)
    scores, deltas = bp(x)
    bp.losses((scores, deltas), props, boxes_validated=True)           # (warm-up: workspaces, the bias check of the bank)
    scores, deltas = bp(x)
    torch.cuda.synchronize()

    def waits(fn):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return out, sum("synchroniz" in str(m.message) for m in w)

    def step():
        losses = bp.losses((scores, deltas), props, boxes_validated=True)
        grads = torch.autograd.grad(sum(losses.values()), [scores, deltas])      # more work queued behind it
        return grads[0] @ grads[0].t()

    _, n = waits(step)
    assert n == 0
    stats, n = waits(bp.classification_stats)
    assert n == 1 and "cls_accuracy" in stats


# ------------------------------------------------------------------ inference

_spec = importlib.util.spec_from_file_location("_postprocess_cases", os.path.join(ROOT, "tests", "test_gpu_postprocess.py"))
pp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pp)                     # (its helpers: _inputs, _run, _same)


def _detector(pkg, classes, topk, thresh, use_sigmoid_ce):
    cfg = pkg.config.get_cfg()
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = classes
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = thresh
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE = use_sigmoid_ce
    cfg.TEST.DETECTIONS_PER_IMAGE = topk
    return pkg.roi_heads.box_emb_head.build_box_predictor(cfg, 256).cuda().eval()


@pytest.mark.parametrize("sizes,classes,thresh,topk,use_sigmoid_ce", [
    ([200, 200], 80, 0.05, 100, True),
    ([300], 1203, 1e-4, 300, True),                                    # LVIS thresholds: the wide pipeline
    ([200, 200], 80, 0.05, 100, False),                                # the softmax, as before
], ids=["sigmoid_80", "sigmoid_lvis_wide", "softmax_80"])
def test_inference_is_bit_identical_to_the_torch_chain_on_its_probabilities(ops, monkeypatch, sizes, classes, thresh, topk, use_sigmoid_ce):
    import locov_amd as pkg
    beh = pkg.roi_heads.box_emb_head
    pred = _detector(pkg, classes, topk, thresh, use_sigmoid_ce)
    assert pred.use_sigmoid_ce == use_sigmoid_ce
    predictions, props = pp._inputs(pkg, sizes, classes, 3.0, seed=len(sizes) * 13 + classes)
    # (logits around -4, as a sigmoid-trained head gives them: at 80 classes the candidates then fit the LDS pipeline; the softmax does
    # not see the shift)
    predictions = (predictions[0] - 4.0, predictions[1])
    scores = predictions[0]
    probs = torch.sigmoid(scores) if use_sigmoid_ce else F.softmax(scores, dim=-1)
    if use_sigmoid_ce:
        assert not torch.equal(probs, F.softmax(scores, dim=-1))
    per_image = [int((p[:, :-1] > thresh).sum()) for p in probs.split(sizes)]
    if classes == 1203:
        assert max(per_image) > pkg.ops._lib.DETECT_MAX_CANDIDATES     # (the LDS pipeline overflows: the wide one runs)
    else:
        assert 0 < max(per_image) <= pkg.ops._lib.DETECT_MAX_CANDIDATES
    # the torch chain on these probabilities, written out
    monkeypatch.setattr(beh, "_FUSED_POSTPROCESS", False)
    with torch.no_grad():
        want = beh.fast_rcnn_inference(pred.predict_boxes(predictions, props), probs.split(sizes), [p.image_size for p in props],
                                       thresh, pred.test_nms_thresh, topk)
    assert all(len(r) > 0 for r in want[0])
    pp._same(pp._run(pkg, pred, predictions, props, False, monkeypatch), want)       # predict_probs follows the loss type
    calls = []
    for name in ("_detect_postprocess_flags", "detect_postprocess_wide"):
        real = getattr(pkg.ops, name)
        monkeypatch.setattr(pkg.ops, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    got = pp._run(pkg, pred, predictions, props, True, monkeypatch)
    pp._same(got, want)
    # (the LDS pipeline is tried first; its overflow flag routes to the wide one, which only the LVIS case needs)
    assert calls[0] == "_detect_postprocess_flags" and ("detect_postprocess_wide" in calls) == (classes == 1203)
