"""The classification loss and its training statistics on the device (csrc/cls_loss.hip: ops.cls_loss = locov_cls_loss, and
FastRCNNOutputLayers.losses / classification_stats through it) against float64 torch on the CPU.

Inputs: logits of sigma 3 with the last (background) column exactly 0, labels drawn from [0, C), every 7th row ignore_index.
Gates:
  value     |loss - loss64| <= 1e-5 max(1, |loss64|)                      (the project's loss_cls gate, tests/test_label_and_losses.py)
  gradient  e = n_valid max|g - g64| <= 2 e_torch + 1.2e-7, e_torch the same quantity for torch's own fp32 cross_entropy backward on
            the device on the same inputs: the factor 2 allows another summation order and nothing sloppier (a missing max
            subtraction, an approximate exp); 1.2e-7 is one fp32 ulp at 1.  Both figures are printed per shape.
  stats     the six integers equal the upstream formulas ([D2-upstream, unverified] _log_classification_stats) evaluated with torch
            on the CPU from the same fp32 logits.
"""
import functools
import os
import subprocess
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = -100
SHAPES = [(1, 1), (3, 1), (5, 1), (1, 2), (3, 2), (5, 2), (3, 65), (257, 49), (257, 81), (1536, 1204), (4099, 3), (4099, 4)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import _lib, ops
    _lib.load()
    return ops


def _inputs(R, C, seed=0):
    g = torch.Generator().manual_seed(1000 * R + C + seed)
    scores = torch.randn(R, C, generator=g) * 3.0
    scores[:, -1] = 0.0
    labels = torch.randint(0, C, (R,), generator=g)
    labels[6::7] = IGNORE
    return scores, labels


def upstream_stats(scores, labels):
    """[D2-upstream, unverified] _log_classification_stats, literally, + the labels torch would assert on."""
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
    num_invalid = (((labels < 0) | (labels > bg_class_ind)) & (labels != IGNORE)).nonzero().numel()
    return [num_instances, num_fg, num_accurate, fg_num_accurate, num_false_negative, num_invalid]


def _f64(scores, labels):
    s = scores.double().requires_grad_(True)
    loss = F.cross_entropy(s, labels, reduction="mean", ignore_index=IGNORE)
    if bool((labels != IGNORE).any()):
        loss.backward()
        return loss.detach(), s.grad
    return loss.detach(), torch.zeros_like(s)


@functools.lru_cache(maxsize=None)
def _case(R, C):
    """One shape's inputs, float64 expectation and torch's own fp32 error on the device; computed once, never modified."""
    scores, labels = _inputs(R, C)
    loss64, g64 = _f64(scores, labels)
    n_valid = int((labels != IGNORE).sum())
    s = scores.cuda().requires_grad_(True)
    F.cross_entropy(s, labels.cuda(), reduction="mean").backward()
    e_torch = n_valid * float((s.grad.cpu().double() - g64).abs().max())
    return {"scores": scores, "labels": labels, "loss64": loss64, "g64": g64, "n_valid": n_valid, "e_torch": e_torch,
            "stats": upstream_stats(scores, labels)}


def _run(ops, scores, labels, grad=True, **kw):
    s = scores.cuda().requires_grad_(grad) if not scores.is_cuda else scores
    loss, stats = ops.cls_loss(s, labels.cuda(), **kw)
    return s, loss, stats


@pytest.mark.parametrize("R,C", SHAPES)
def test_value_gradient_and_stats_against_float64(ops, R, C):
    c = _case(R, C)
    s, loss, stats = _run(ops, c["scores"], c["labels"])
    assert loss.dim() == 0 and loss.dtype == torch.float32 and stats.dtype == torch.int64 and tuple(stats.shape) == (6,)
    loss.backward()
    got, want = float(loss), float(c["loss64"])
    g = s.grad.cpu()
    e = c["n_valid"] * float((g.double() - c["g64"]).abs().max())
    print(f"cls_loss [{R}, {C}]: loss {got:.9g} (float64 {want:.9g}, diff {abs(got - want):.3g}); n_valid max|g - g64|: "
          f"e = {e:.3e}, e_torch = {c['e_torch']:.3e}")
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
    assert e <= 2.0 * c["e_torch"] + 1.2e-7
    ignored = c["labels"] == IGNORE
    assert float(g[ignored].abs().sum()) == 0.0                       # exact zeros
    assert stats.tolist() == c["stats"]
    if C == 1:                                                        # background only
        assert got == 0.0 and float(g.abs().max()) == 0.0


def test_backward_scales_by_the_incoming_gradient(ops):
    c = _case(257, 81)
    s, loss, _ = _run(ops, c["scores"], c["labels"])
    (loss * 0.25).backward()
    s2, loss2, _ = _run(ops, c["scores"], c["labels"])
    loss2.backward()
    assert torch.equal(s.grad, s2.grad * 0.25)                        # (a power of two: exact)


def test_hand_built_ties_background_rows_and_an_out_of_range_label(ops):
    from locov_amd.roi_heads import box_emb_head as beh
    from locov_amd.structures import Boxes, Instances
    scores = torch.tensor([[2., 2., 0., 0.],       # gt 1: two equal maxima -> pred 0 (the lowest index), wrong
                           [0., -1., -2., 0.],     # gt 0: a foreground logit ties the background's 0 -> pred 0, accurate
                           [-1., -1., -1., 0.],    # gt bg
                           [-3., -2., -1., 0.],    # gt bg
                           [-1., -1., -1., 0.],    # gt 2: pred bg -> false negative
                           [1., 0., 0., 0.]])      # gt 7: out of range
    labels = torch.tensor([1, 0, 3, 3, 2, 7])
    assert upstream_stats(scores, labels) == [6, 3, 3, 1, 1, 1]
    s, loss, stats = _run(ops, scores, labels)
    assert stats.tolist() == [6, 3, 3, 1, 1, 1]
    loss.backward()
    # the out-of-range row is treated as ignored: the same bits as with ignore_index there, and the float64 value
    ign = labels.clone()
    ign[5] = IGNORE
    s2, loss2, stats2 = _run(ops, scores, ign)
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(s.grad, s2.grad) and float(s.grad[5].abs().sum()) == 0.0
    assert stats2.tolist() == [6, 3, 3, 1, 1, 0]
    want, g64 = _f64(scores, ign)
    assert abs(float(loss) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    st = scores.cuda().requires_grad_(True)
    F.cross_entropy(st, ign.cuda(), reduction="mean").backward()
    e_torch = 5 * float((st.grad.cpu().double() - g64).abs().max())
    assert 5 * float((s.grad.cpu().double() - g64).abs().max()) <= 2.0 * e_torch + 1.2e-7

    # through the predictor: the counts stay on the device, classification_stats() reads them and names the bad labels
    bp = beh.FastRCNNOutputLayers(8, box2box_transform=beh.Box2BoxTransform((10.0, 10.0, 5.0, 5.0)), num_classes=3,
                                  cls_agnostic_bbox_reg=True).cuda()

    def proposals(y):
        p = Instances((100, 100))
        p.proposal_boxes = Boxes(torch.tensor([[10., 10., 50., 50.]] * 6).cuda())
        p.gt_boxes = Boxes(torch.tensor([[12., 8., 48., 55.]] * 6).cuda())
        p.gt_classes = y.cuda()
        return p
    out = bp.losses((scores.cuda(), torch.zeros(6, 4).cuda()), [proposals(labels)])
    assert torch.equal(out["loss_cls"], loss.detach()) and bp._cls_stats.is_cuda
    with pytest.raises(ValueError, match="1 of 6"):
        bp.classification_stats()
    bp.losses((scores.cuda(), torch.zeros(6, 4).cuda()), [proposals(ign)])
    assert bp.classification_stats() == {"cls_accuracy": 3 / 6, "fg_cls_accuracy": 1 / 3, "false_negative": 1 / 3}


@pytest.mark.parametrize("R,C", [(5, 2), (257, 81), (1536, 1204), (4099, 4)])
def test_column_slice_of_a_wider_matrix_gives_the_bits_of_its_copy(ops, R, C):
    """ld > C and a base that is 4 bytes past a 16-byte boundary: scalar loads, against the contiguous copy (16-byte loads at C = 1204
    and C = 4; at R = 4099 there are more row groups than blocks, so a wave takes a second row)."""
    c = _case(R, C)
    wide = torch.randn(R, C + 7, generator=torch.Generator().manual_seed(5)).cuda()
    wide[:, 1:1 + C] = c["scores"].cuda()
    view = wide[:, 1:1 + C].requires_grad_(True)
    assert view.stride(0) == C + 7 and view.data_ptr() % 16 == 4
    loss_v, stats_v = ops.cls_loss(view, c["labels"].cuda())
    loss_v.backward()
    s, loss, stats = _run(ops, c["scores"], c["labels"])
    loss.backward()
    assert torch.equal(loss_v, loss) and torch.equal(stats_v, stats)
    assert view.grad.is_contiguous() and torch.equal(view.grad, s.grad)


def test_all_labels_ignored_gives_nan_and_a_zero_gradient(ops):
    scores, _ = _inputs(9, 49)
    labels = torch.full((9,), IGNORE, dtype=torch.int64)
    assert torch.isnan(F.cross_entropy(scores, labels))               # torch's value
    s, loss, stats = _run(ops, scores, labels)
    assert torch.isnan(loss)
    loss.backward()
    assert float(s.grad.abs().sum()) == 0.0 and not torch.isnan(s.grad).any()
    assert stats.tolist() == [9, 0, 0, 0, 0, 0]


def test_no_gradient_buffer_without_requires_grad_and_null_stats(ops):
    R, C = 1536, 1204
    c = _case(R, C)
    s, y = c["scores"].cuda(), c["labels"].cuda()
    ops.cls_loss(s, y)                                                # (the cached workspace exists from here on)
    peaks = {}
    for grad in (False, True):
        x = s.clone().requires_grad_(grad)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, stats = ops.cls_loss(x, y)
        torch.cuda.synchronize()
        peaks[grad] = torch.cuda.max_memory_allocated() - base
        assert loss.requires_grad == grad
    assert peaks[False] < R * C * 4 // 8 and peaks[True] >= R * C * 4
    with torch.no_grad():                                             # (nor under no_grad)
        x = s.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ops.cls_loss(x, y)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base < R * C * 4 // 8
    ref, ref_stats = ops.cls_loss(s, y)
    loss, none = ops.cls_loss(s, y, want_stats=False)
    assert none is None and torch.equal(loss, ref)
    x = s.clone().requires_grad_(True)
    loss, none = ops.cls_loss(x, y, want_stats=False)
    loss.backward()
    assert none is None and torch.equal(loss, ref) and x.grad is not None


@pytest.mark.parametrize("R,C", [(257, 81), (1536, 1204), (4099, 4)])
def test_two_calls_give_the_same_bits(ops, R, C):
    c = _case(R, C)
    outs = []
    for _ in range(2):
        s, loss, stats = _run(ops, c["scores"], c["labels"])
        loss.backward()
        outs.append((loss.detach().clone(), s.grad.clone(), stats.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_argument_checks(ops):
    from locov_amd._lib import LocovError
    s, y = torch.zeros(4, 5).cuda(), torch.zeros(4, dtype=torch.int64).cuda()
    with pytest.raises(TypeError):
        ops.cls_loss(s.half(), y)
    with pytest.raises(TypeError):
        ops.cls_loss(s, y.int())
    with pytest.raises(LocovError):
        ops.cls_loss(s, y.cpu())
    with pytest.raises(ValueError):
        ops.cls_loss(s, y[:3])
    with pytest.raises(ValueError):
        ops.cls_loss(s[0], y)
    with pytest.raises(ValueError):
        ops.cls_loss(s[:0], y[:0])


# ------------------------------------------------------------------ through the predictor

def _embedding_predictor():
    import locov_amd
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = 64
    cfg.MODEL.ROI_BOX_HEAD.FREEZE_EMB_PRED = False
    cfg.MODEL.ROI_HEADS.DETACH_CLASS_PREDICTOR = False
    torch.manual_seed(4)
    bp = locov_amd.build_box_predictor(cfg, 128).cuda().train()
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


def test_embedding_predictor_losses_run_the_fused_call(ops, monkeypatch):
    bp, g = _embedding_predictor()
    props, x = _sampled_batch(g)
    calls = []
    real = ops.cls_loss
    monkeypatch.setattr(ops, "cls_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    scores, deltas = bp(x)
    assert tuple(scores.shape) == (32, 49) and scores.requires_grad
    losses = bp.losses((scores, deltas), props, boxes_validated=True)
    assert calls == [1] and sorted(losses) == ["loss_box_reg", "loss_cls"]
    labels = torch.cat([p.gt_classes for p in props]).cpu()
    want, _ = _f64(scores.detach().cpu(), labels)
    assert abs(float(losses["loss_cls"]) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    losses["loss_cls"].backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.0
    assert bp.emb_pred.weight.grad is not None and float(bp.emb_pred.weight.grad.abs().max()) > 0.0
    stats = bp.classification_stats()
    assert stats["cls_accuracy"] == upstream_stats(scores.detach().cpu(), labels)[2] / 32 and "fg_cls_accuracy" in stats
    from locov_amd.roi_heads.labelling import get_event_storage
    bp.log_classification_stats()
    assert get_event_storage().scalars["fast_rcnn/cls_accuracy"] == stats["cls_accuracy"]


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import torch
import torch.nn.functional as F
sys.path.insert(0, {tests!r})
import test_gpu_cls_loss as T
from locov_amd import ops
from locov_amd.roi_heads import box_emb_head as beh
assert beh._FUSED_BOX_LOSS is False

def no_fused(*a, **k):
    raise AssertionError("ops.cls_loss called with LOCOV_FUSED_LOSSES=0")
ops.cls_loss = no_fused
bp, g = T._embedding_predictor()
props, x = T._sampled_batch(g)
scores, deltas = bp(x)
losses = bp.losses((scores, deltas), props, boxes_validated=True)
want = F.cross_entropy(scores, torch.cat([p.gt_classes for p in props]), reduction="mean")
assert torch.equal(losses["loss_cls"], want)
stats = bp.classification_stats()
print("CHILD", float(want).hex(), stats["cls_accuracy"])
"""


def test_switch_off_reproduces_the_torch_value_in_a_fresh_process(ops):
    """LOCOV_FUSED_LOSSES is read at import: a child process with it at 0 runs the torch line (bit-equal to F.cross_entropy there) and
    the torch form of the statistics; the fused value of this process meets the gate against it."""
    env = dict(os.environ, LOCOV_FUSED_LOSSES="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("CHILD")][-1].split()
    torch_value, torch_acc = float.fromhex(line[1]), float(line[2])
    bp, g = _embedding_predictor()
    props, x = _sampled_batch(g)
    losses = bp.losses(bp(x), props, boxes_validated=True)
    assert abs(float(losses["loss_cls"]) - torch_value) <= 1e-5 * max(1.0, abs(torch_value))
    assert bp.classification_stats()["cls_accuracy"] == torch_acc


def test_losses_add_no_host_wait(ops):
    """losses() and the work queued after it make no device-to-host read (torch.cuda.set_sync_debug_mode, as tools/find_syncs.py);
    classification_stats() makes exactly one."""
    bp, g = _embedding_predictor()
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
