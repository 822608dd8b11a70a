"""The IoU box-regression losses on the device (csrc/box_iou_loss.hip: ops.box_iou_loss = locov_box_iou_loss, and
FastRCNNOutputLayers.box_reg_loss / losses through it for BBOX_REG_LOSS_TYPE "giou" / "diou" / "ciou") against the float64 restatement
of upstream (tests/box_iou_ref.py) and the torch chain of box_reg_loss on the same inputs.

Gates.  The kernel does a row in fp64 and rounds the loss and each gradient entry to fp32 once; the torch chain rounds every step.  With
g64 / loss64 the float64 results and g_max = max|g64|:
  main gate   max|g - g64| <= e_chain + 2^-23 g_max, e_chain = max|g_chain - g64| of the fp32 torch chain on the device -- a kernel
              that rounds once cannot be further from the truth than a chain that rounds every step, plus one rounding of the result;
              |loss - loss64| <= |loss_chain - loss64| + 2^-23 |loss64| likewise.  Condition on the inputs: e_chain <= 1e-5 g_max.
  once gate   (the small hand-built cases, where no chain is run) max|g - g64| <= 2^-23 g_max and |loss - loss64| <= 2^-23 |loss64| +
              2^-52: one fp32 rounding of the result (2^-24 relative, doubled), and -- the losses are formed as 1 - iou + ..., which is
              ~1e-11 for identical boxes -- one fp64 rounding at 1 of either evaluation.
The three error figures of the main case are printed."""
import functools
import warnings

import pytest
import torch

import box_iou_ref as ref

pytestmark = pytest.mark.gpu

KINDS = ref.KINDS
K_MAIN = 16
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import _lib, ops
    _lib.load()
    return ops


def _predictor(kind, agnostic, K):
    from locov_amd.roi_heads import box_emb_head as beh
    return beh.FastRCNNOutputLayers(8, box2box_transform=beh.Box2BoxTransform(ref.WEIGHTS), num_classes=K, cls_agnostic_bbox_reg=agnostic,
                                    box_reg_loss_type=kind)


def _inputs(n, K, agnostic, seed, last_fg=False):
    """The recipe of test_one_launch_box_reg_loss_equals_the_torch_chain: boxes up to 900 px, ground truth = box + N(0, 6), about half
    background, 5 % ignored, deltas N(0, 0.3); CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    boxes = torch.rand(n, 4, generator=g) * 600
    boxes[:, 2:] = boxes[:, :2] + 4 + torch.rand(n, 2, generator=g) * 300
    gt = boxes + torch.randn(n, 4, generator=g) * 6
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    cls = torch.randint(0, K, (n,), generator=g)
    cls[torch.rand(n, generator=g) < 0.5] = K                       # background
    cls[torch.rand(n, generator=g) < 0.05] = -1                     # ignored
    if last_fg:
        cls[-1] = K - 1
    pred = torch.randn(n, 4 if agnostic else 4 * K, generator=g) * 0.3
    return boxes, gt, cls, pred


def _class_col(cls, r, agnostic):
    return 0 if agnostic else 4 * int(cls[r])


@functools.lru_cache(maxsize=None)
def _main_inputs(agnostic):
    """700 rows, seed 3, inf / NaN / -inf in three background rows, dw = 30 (above the clamp) in five foreground rows; computed once,
    never modified."""
    boxes, gt, cls, pred = _inputs(700, K_MAIN, agnostic, 3)
    bad = (cls == K_MAIN).nonzero()[:3, 0]
    pred[bad[0]] = float("inf")
    pred[bad[1]] = float("nan")
    pred[bad[2], 1] = -float("inf")
    clamped = ((cls >= 0) & (cls < K_MAIN)).nonzero()[:5, 0].tolist()
    for r in clamped:
        pred[r, _class_col(cls, r, agnostic) + 2] = 30.0
    return boxes, gt, cls, pred, clamped


@functools.lru_cache(maxsize=None)
def _main_ref(kind, agnostic):
    boxes, gt, cls, pred, _ = _main_inputs(agnostic)
    return ref.box_reg_loss(kind, boxes, gt, pred, cls, K_MAIN)[:2]


def _run(bp, boxes, gt, pred, cls, validated):
    """box_reg_loss on the device: validated = the fused launch, else the torch chain.  -> (loss, gradient) on the CPU, float64."""
    p = pred.cuda().requires_grad_(True)
    loss = bp.box_reg_loss(boxes.cuda(), gt.cuda(), p, cls.cuda(), boxes_validated=validated)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    return loss.detach().cpu().double(), p.grad.cpu().double()


def _main_gate(what, got, chain, want, condition=True):
    (loss, g), (loss_c, g_c), (loss64, g64) = got, chain, want
    g_max = float(g64.abs().max())
    e_chain, e_fused = float((g_c - g64).abs().max()), float((g - g64).abs().max())
    v_chain, v_fused = abs(float(loss_c - loss64)), abs(float(loss - loss64))
    print(f"box_iou_loss {what}: gradient max|g - g64| fused {e_fused:.3e}, chain {e_chain:.3e}, g_max {g_max:.3e}; "
          f"value fused {v_fused:.3e}, chain {v_chain:.3e}, loss64 {float(loss64):.9g}")
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    if condition:
        assert e_chain <= 1e-5 * g_max                                # (a condition on the inputs, not on the kernel)
    assert e_fused <= e_chain + ULP * g_max
    assert v_fused <= v_chain + ULP * abs(float(loss64))


def _once_gate(got, want):
    (loss, g), (loss64, g64) = got, want
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    assert float((g - g64).abs().max()) <= ULP * float(g64.abs().max())
    assert abs(float(loss - loss64)) <= ULP * abs(float(loss64)) + 2.0 ** -52


@pytest.mark.parametrize("agnostic", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_value_and_gradient_against_float64_and_the_torch_chain(ops, kind, agnostic):
    boxes, gt, cls, pred, clamped = _main_inputs(agnostic)
    want = _main_ref(kind, agnostic)
    bp = _predictor(kind, agnostic, K_MAIN)
    chain = _run(bp, boxes, gt, pred, cls, validated=False)
    got = _run(bp, boxes, gt, pred, cls, validated=True)
    _main_gate(f"{kind} [700, {pred.shape[1]}]", got, chain, want)
    g, g64 = got[1], want[1]
    assert torch.equal(g != 0, g64 != 0)                              # the float64 gradient's non-zero pattern, exactly
    for r in clamped:
        assert float(g[r, _class_col(cls, r, agnostic) + 2]) == 0.0
    fg = (cls >= 0) & (cls < K_MAIN)
    assert not g[~fg].any() and bool((g[fg] != 0).any(dim=1).all())


@pytest.mark.parametrize("agnostic", [True, False])
@pytest.mark.parametrize("R", [1, 257, 2048])
def test_shapes_around_the_block(ops, R, agnostic):
    """One row; one row past a 256-thread stride with the last row foreground; 2048 rows (eight strides)."""
    K = 3
    boxes, gt, cls, pred = _inputs(R, K, agnostic, 100 + R, last_fg=True)
    for kind in KINDS:
        want = ref.box_reg_loss(kind, boxes, gt, pred, cls, K)[:2]
        got = _run(_predictor(kind, agnostic, K), boxes, gt, pred, cls, validated=True)
        _once_gate(got, want)
        assert torch.equal(got[1] != 0, want[1] != 0)
        assert bool((got[1][-1] != 0).any())


@pytest.mark.parametrize("agnostic", [True, False])
def test_all_background_gives_zero_loss_and_no_gradient(ops, agnostic):
    boxes, gt, cls, pred, _ = _main_inputs(agnostic)
    cls = torch.where(cls < 0, cls, torch.full_like(cls, K_MAIN))
    for kind in KINDS:
        loss, g = _run(_predictor(kind, agnostic, K_MAIN), boxes, gt, pred, cls, validated=True)
        assert float(loss) == 0.0 and not g.any()


@pytest.mark.parametrize("agnostic", [True, False])
def test_non_contiguous_predictions(ops, agnostic):
    """A column block of a wider matrix, as ops.box_reg_loss takes it: the bits of the contiguous copy, the gradient in the view's shape."""
    boxes, gt, cls, pred, _ = _main_inputs(agnostic)
    n, ld = pred.shape
    wide = torch.randn(n, ld + 3, generator=torch.Generator().manual_seed(5)).cuda()
    wide[:, 1:1 + ld] = pred.cuda()
    for kind in KINDS:
        view = wide[:, 1:1 + ld].detach().requires_grad_(True)
        assert not view.is_contiguous()
        lv = ops.box_iou_loss(view, boxes.cuda(), gt.cuda(), cls.cuda(), K_MAIN, ref.WEIGHTS, ref.SCALE_CLAMP, kind)
        lv.backward()
        p = pred.cuda().requires_grad_(True)
        lc = ops.box_iou_loss(p, boxes.cuda(), gt.cuda(), cls.cuda(), K_MAIN, ref.WEIGHTS, ref.SCALE_CLAMP, kind)
        lc.backward()
        assert torch.equal(lv, lc) and tuple(view.grad.shape) == (n, ld) and torch.equal(view.grad, p.grad)


# ------------------------------------------------------------------ ties and the strict mask

def _hand_case(boxes, gt):
    n = len(boxes)
    return (torch.tensor(boxes, dtype=torch.float32), torch.tensor(gt, dtype=torch.float32), torch.zeros(n, dtype=torch.int64),
            torch.zeros(n, 4))


@pytest.mark.parametrize("kind", KINDS)
def test_identical_boxes_share_the_gradient_at_every_max_and_min(ops, kind):
    """Integer proposals of even width and height, zero deltas, ground truth = proposal: the decoding reproduces the box exactly, so
    every max / min of the loss sees two equal arguments -- torch sends half the gradient to each."""
    boxes, gt, cls, pred = _hand_case([[10, 20, 50, 80], [0, 0, 2, 2], [300, 100, 812, 356]], [[10, 20, 50, 80], [0, 0, 2, 2], [300, 100, 812, 356]])
    loss64, g64, decoded = ref.box_reg_loss(kind, boxes, gt, pred, cls, 1)
    assert torch.equal(decoded, boxes.double())                        # exact
    assert bool((g64 != 0).any())
    got = _run(_predictor(kind, True, 1), boxes, gt, pred, cls, validated=True)
    _once_gate(got, (loss64, g64))


@pytest.mark.parametrize("kind", KINDS)
def test_disjoint_and_touching_pairs_have_no_intersection(ops, kind):
    """Row 0: disjoint boxes; row 1: boxes that touch along an edge (min x2 == max x1: the strict mask is false); row 2: touching at
    a corner.  The intersection is exactly zero, nothing flows through it; giou is above 1 for the disjoint pair."""
    boxes, gt, cls, pred = _hand_case([[10, 10, 30, 40], [0, 0, 10, 10], [0, 0, 10, 10]], [[50, 60, 90, 100], [10, 0, 20, 10], [10, 10, 30, 20]])
    loss64, g64, decoded = ref.box_reg_loss(kind, boxes, gt, pred, cls, 1)
    lt, rb = torch.max(decoded[:, :2], gt[:, :2].double()), torch.min(decoded[:, 2:], gt[:, 2:].double())
    assert bool((rb[0] < lt[0]).all()) and float(rb[1, 0]) == float(lt[1, 0]) and bool((rb[2] == lt[2]).all())
    bp = _predictor(kind, True, 1)
    chain = _run(bp, boxes, gt, pred, cls, validated=False)
    got = _run(bp, boxes, gt, pred, cls, validated=True)
    _main_gate(f"{kind} disjoint / touching", got, chain, (loss64, g64), condition=False)
    assert torch.equal(got[1] != 0, g64 != 0)
    if kind == "giou":
        assert float(_run(bp, boxes[:1], gt[:1], pred[:1], cls[:1], validated=True)[0]) > 1.0


@pytest.mark.parametrize("agnostic", [True, False])
def test_two_calls_give_the_same_bits(ops, agnostic):
    boxes, gt, cls, pred, _ = _main_inputs(agnostic)
    for kind in KINDS:
        bp = _predictor(kind, agnostic, K_MAIN)
        a = _run(bp, boxes, gt, pred, cls, validated=True)
        b = _run(bp, boxes, gt, pred, cls, validated=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ through the predictor

def _cfg_predictor(kind="giou", weight=1.0):
    import locov_amd
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.ROI_BOX_HEAD.NAME = "FastRCNNOutputLayers"
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = K_MAIN
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = kind
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT = weight
    return locov_amd.build_box_predictor(cfg, 32).cuda().train()


def _proposals(boxes, gt, cls):
    """Two images' sampled proposals on the device (ignored rows carry cross_entropy's ignore_index)."""
    from locov_amd.structures import Boxes, Instances
    cls = torch.where(cls < 0, torch.full_like(cls, -100), cls)
    props, half = [], len(cls) // 2
    for sl in (slice(0, half), slice(half, None)):
        p = Instances((1000, 1000))
        p.proposal_boxes, p.gt_boxes, p.gt_classes = Boxes(boxes[sl].cuda()), Boxes(gt[sl].cuda()), cls[sl].cuda()
        props.append(p)
    return props


def _surface_inputs():
    boxes, gt, cls, pred, _ = _main_inputs(True)
    pred = torch.nan_to_num(pred, nan=0.0, posinf=0.0, neginf=0.0)
    scores = torch.randn(len(cls), K_MAIN + 1, generator=torch.Generator().manual_seed(9))
    return boxes, gt, cls, pred, scores


def test_losses_of_a_configured_predictor_run_the_fused_entry(ops, monkeypatch):
    from locov_amd import _lib
    lib = _lib.load()
    boxes, gt, cls, pred, scores = _surface_inputs()
    props = _proposals(boxes, gt, cls)
    launches = []
    real = ops.box_iou_loss

    def counted(*a, **k):
        before = lib.locov_launch_count()
        out = real(*a, **k)
        launches.append(lib.locov_launch_count() - before)
        return out
    monkeypatch.setattr(ops, "box_iou_loss", counted)

    outs = {}
    for weight in (1.0, 2.0):
        bp = _cfg_predictor("giou", weight)
        assert bp.box_reg_loss_type == "giou" and bp.loss_weight["loss_box_reg"] == weight
        p, s = pred.cuda().requires_grad_(True), scores.cuda().requires_grad_(True)
        losses = bp.losses((s, p), props, boxes_validated=True)
        assert sorted(losses) == ["loss_box_reg", "loss_cls"]
        losses["loss_box_reg"].backward()
        outs[weight] = (losses["loss_box_reg"].detach().cpu().double(), p.grad.cpu().double())
    assert launches == [1, 1]                                         # forward and gradient: ONE library launch per losses()
    # against the torch chain (unvalidated boxes) and float64, under the main gate
    p = pred.cuda().requires_grad_(True)
    chain_loss = _cfg_predictor("giou").losses((scores.cuda(), p), props, boxes_validated=False)["loss_box_reg"]
    chain_loss.backward()
    assert launches == [1, 1]
    cls100 = torch.where(cls < 0, torch.full_like(cls, -100), cls)
    want = ref.box_reg_loss("giou", boxes, gt, pred, cls100, K_MAIN)[:2]
    _main_gate("giou through losses()", outs[1.0], (chain_loss.detach().cpu().double(), p.grad.cpu().double()), want)
    # loss_weight 2: exactly twice the value and the gradient
    assert torch.equal(outs[2.0][0], outs[1.0][0] * 2.0) and torch.equal(outs[2.0][1], outs[1.0][1] * 2.0)


def test_losses_add_no_host_wait(ops):
    """losses() of a giou predictor and the work queued after it make no device-to-host read (torch.cuda.set_sync_debug_mode, as
    tests/test_gpu_cls_loss.py::test_losses_add_no_host_wait)."""
    boxes, gt, cls, pred, scores = _surface_inputs()
    props = _proposals(boxes, gt, cls)
    bp = _cfg_predictor("giou")
    s, p = scores.cuda().requires_grad_(True), pred.cuda().requires_grad_(True)
    bp.losses((s, p), props, boxes_validated=True)                     # (warm-up: workspaces)
    torch.cuda.synchronize()

    def step():
        losses = bp.losses((s, p), props, boxes_validated=True)
        grads = torch.autograd.grad(sum(losses.values()), [s, p])      # more work queued behind it
        return grads[1] @ grads[1].t()

    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sum("synchroniz" in str(m.message) for m in w) == 0
