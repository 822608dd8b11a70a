"""The RPN's training half on the device (csrc/rpn_train.hip through ops.rpn_label_anchors / rpn_sample_anchors / rpn_loss, and
locov_amd/proposal_generator.py) against the reference of the operation itself (tests/rpn_train_ref.py) on the cases of
tests/rpn_train_cases.py: labels, matched boxes and counters bit for bit; the losses and gradients against float64 within a margin
measured from the torch fp32 chain on the same case; the head's autograd against a float64 conv2d; RPN.forward in training.
tests/test_rpn_train_ref.py checks without a GPU that every case reaches what it is meant to and that the reference equals the chain.

The margin of every float comparison here: the torch fp32 path's own error against the same float64 on the same case (max norm per
tensor), twice, plus 2^-22 of the largest reference entry -- the device's expf / log1pf / logf are not correctly rounded, and its
GEMMs sum in another order; the factor covers both."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_train_cases as tc
import rpn_train_ref as ref

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


def margin(path32, want):
    """(allowed, measured fp32-path error): 2 x the fp32 path's error + 2^-22 of the largest reference entry."""
    want = np.asarray(want, dtype=np.float64)
    err = float(np.abs(np.asarray(path32, dtype=np.float64) - want).max())
    return 2 * err + 2.0 ** -22 * float(np.abs(want).max()), err


def close(got, path32, want, what):
    allowed, err32 = margin(path32, want)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())
    print(f"{what}: device error {err:.3e}, fp32 path error {err32:.3e}, allowed {allowed:.3e}")
    assert err <= allowed, what


def final_labels(name):
    recs = tc.reference(name)
    return np.stack([r["final"] for r in recs]), np.stack([r["matched_boxes"] for r in recs])


@pytest.mark.parametrize("name", tc.NAMES)
def test_kernels_equal_reference_bit_for_bit(pkg, name, monkeypatch):
    c = tc.case(name)
    rpn = tc.make_rpn(c)
    anchors, gt, rnd = tc.inputs(c, "cuda")
    labels, boxes = rpn.label_and_sample_anchors(anchors, gt, rnd)
    assert rpn._fused_batch is not None
    recs = tc.reference(name)
    counts = rpn._fused_batch[4].cpu().tolist()
    for lab, box, r, cnt in zip(labels, boxes, recs, counts):
        assert lab.dtype == torch.int8
        assert np.array_equal(lab.cpu().numpy(), r["final"])
        assert np.array_equal(box.cpu().numpy().view(np.int32), r["matched_boxes"].view(np.int32))
        assert cnt == [r["pop_pos"], r["pop_neg"], r["num_pos"], r["num_neg"]]
    # the pre-sampling labels of the first kernel pair, and the torch chain on the device: the same labels and boxes
    n_gt = [g.gt_boxes.tensor.shape[0] for g in gt]
    pre = pkg.ops.rpn_label_anchors(anchors[0].tensor, torch.cat([g.gt_boxes.tensor for g in gt]) if sum(n_gt) else None, n_gt, c["image_hw"],
                                    rpn.anchor_matcher.thresholds, rpn.anchor_matcher.labels, True, c["boundary"])[0]
    assert np.array_equal(pre.cpu().numpy(), np.stack([r["labels"] for r in recs]))
    if name in tc.SMALL:
        monkeypatch.setenv("LOCOV_FUSED_RPN", "0")
        chain_labels, chain_boxes = rpn.label_and_sample_anchors(anchors, gt, rnd)
        assert rpn._fused_batch is None
        assert all(torch.equal(a, b) for a, b in zip(labels, chain_labels)) and all(torch.equal(a, b) for a, b in zip(boxes, chain_boxes))


def run_loss(pkg, c, lab, mb, deltas, beta, w_cls, w_loc):
    norm = c["budget"] * lab.shape[0]
    logits, d = dev(c["logits"]).requires_grad_(), dev(deltas).requires_grad_()
    loss, flags = pkg.ops.rpn_loss(logits, d, dev(lab), dev(c["anchors"]), dev(mb), c["weights"], beta, w_cls / norm, w_loc / norm)
    loss.sum().backward()
    return loss.detach().cpu(), logits.grad.cpu(), d.grad.cpu(), int(flags.cpu()[0])


@pytest.mark.parametrize("name", tc.SMALL + ["big_over_and_fill"])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_loss_kernel_against_float64(pkg, name, beta, monkeypatch):
    c = dict(tc.case(name), beta=beta)
    lab, mb = final_labels(name)
    w_cls, w_loc = 2.0, 0.5
    loss, dl, dd, flags = run_loss(pkg, c, lab, mb, c["deltas"], beta, w_cls, w_loc)
    loss2, dl2, dd2, _ = run_loss(pkg, c, lab, mb, c["deltas"], beta, w_cls, w_loc)
    assert flags == 0
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(dl, dl2) and torch.equal(dd, dd2)     # the same bits
    want = ref.losses(c["logits"], c["deltas"], lab, c["anchors"], mb, c["weights"], beta, c["budget"], w_cls, w_loc)
    # the torch fp32 chain on the same case, on the device
    monkeypatch.setenv("LOCOV_FUSED_RPN", "0")
    rpn = tc.make_rpn(c, loss_weight={"loss_rpn_cls": w_cls, "loss_rpn_loc": w_loc})
    anchors, _, _ = tc.inputs(c, "cuda")
    lg, dt = dev(c["logits"]).requires_grad_(), dev(c["deltas"]).requires_grad_()
    out = rpn.losses(anchors, [lg], list(dev(lab)), [dt], list(dev(mb)))
    (out["loss_rpn_cls"] + out["loss_rpn_loc"]).backward()
    close(float(loss[0]), float(out["loss_rpn_cls"]), want[0], f"{name} beta {beta} loss_rpn_cls")
    close(float(loss[1]), float(out["loss_rpn_loc"]), want[1], f"{name} beta {beta} loss_rpn_loc")
    close(dl.numpy(), lg.grad.cpu().numpy(), want[2], f"{name} beta {beta} d logits")
    close(dd.numpy(), dt.grad.cpu().numpy(), want[3], f"{name} beta {beta} d deltas")
    # untouched entries are exactly 0
    assert not dl.numpy()[lab < 0].any() and not dd.numpy()[lab != 1].any()


@pytest.mark.parametrize("name", ["b7_with_empty", "outside_gt", "big_over_and_fill"])
def test_l1_gradient_entries_are_exact(pkg, name):
    """Predictions far from every target (|pred - target| >= 900): each entry of a positive anchor is exactly +- weight / normalizer,
    the sign that of pred - target; everything else is exactly 0."""
    c = tc.case(name)
    lab, mb = final_labels(name)
    w_loc = 0.5
    _, _, dd, _ = run_loss(pkg, c, lab, mb, c["deltas_far"], 0.0, 1.0, w_loc)
    step = np.float32(w_loc / (c["budget"] * lab.shape[0]))
    dd = dd.numpy()
    pos = lab == 1
    assert pos.any()
    assert np.array_equal(dd[pos], np.sign(c["deltas_far"][pos]).astype(np.float32) * step)
    assert not dd[~pos].any()


def test_degenerate_positive_anchor_raises_the_flag(pkg):
    c = tc.case("tie_max")
    lab, mb = final_labels("tie_max")
    i = int(np.nonzero(lab[0] == 1)[0][0])
    assert run_loss(pkg, c, lab, mb, c["deltas"], 0.0, 1.0, 1.0)[3] == 0
    j = int(np.nonzero(lab[0] != 1)[0][0])
    bad = dict(c, anchors=c["anchors"].copy())
    bad["anchors"][j, 2] = bad["anchors"][j, 0]                    # a zero-width anchor that is NOT positive: no flag
    assert run_loss(pkg, bad, lab, mb, c["deltas"], 0.0, 1.0, 1.0)[3] == 0
    bad["anchors"][i, 2] = bad["anchors"][i, 0]                    # a zero-width positive anchor
    assert run_loss(pkg, bad, lab, mb, c["deltas"], 0.0, 1.0, 1.0)[3] == pkg.ops.RPN_LOSS_FLAG_DEGENERATE


# ------------------------------------------------------------------------------------------------ the head's autograd

def head_reference(head, x, gl, gd, dtype):
    """conv2d autograd on the CPU in `dtype`: gradients of sum(logits * gl) + sum(deltas * gd) to x, the two 1x1 layers, the 3x3."""
    p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in head.named_parameters()}
    xx = x.detach().cpu().to(dtype).requires_grad_()
    t = F.relu(F.conv2d(xx, p["conv.weight"], p["conv.bias"], padding=1))
    N = x.shape[0]
    lo = F.conv2d(t, p["objectness_logits.weight"], p["objectness_logits.bias"]).permute(0, 2, 3, 1).reshape(N, -1)
    de = F.conv2d(t, p["anchor_deltas.weight"], p["anchor_deltas.bias"]).permute(0, 2, 3, 1).reshape(N, -1, 4)
    ((lo * gl.cpu().to(dtype)).sum() + (de * gd.cpu().to(dtype)).sum()).backward()
    out = {k: v.grad.numpy() for k, v in p.items()}
    out["x"] = xx.grad.numpy()
    return out


def test_head_autograd_against_float64_conv2d(pkg, monkeypatch):
    from locov_amd.proposal_generator import StandardRPNHead
    torch.manual_seed(7)
    head = StandardRPNHead(32, 3).cuda()
    for p in head.parameters():
        torch.nn.init.normal_(p, std=0.1)
    x = torch.randn(2, 32, 6, 10, device="cuda")
    gl, gd = torch.randn(2, 6 * 10 * 3, device="cuda"), torch.randn(2, 6 * 10 * 3, 4, device="cuda")
    with torch.no_grad():
        plain = head.flat_predictions([x])

    def run(x_in):
        head.zero_grad(set_to_none=True)
        logits, deltas = head.flat_predictions([x_in])
        assert torch.equal(logits[0], plain[0][0]) and torch.equal(deltas[0], plain[1][0])           # the no_grad path's bits
        ((logits[0] * gl).sum() + (deltas[0] * gd).sum()).backward()
        return {k: v.grad.detach().cpu().numpy().copy() for k, v in head.named_parameters()}

    calls = []
    real = pkg.ops.conv3x3_nhwc_ex
    monkeypatch.setattr(pkg.ops, "conv3x3_nhwc_ex", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    xg = x.clone().requires_grad_()
    got = run(xg)
    assert len(calls) == 2                                          # the forward and the data gradient
    got["x"] = xg.grad.cpu().numpy()
    want, path32 = head_reference(head, x, gl, gd, torch.float64), head_reference(head, x, gl, gd, torch.float32)
    for k in want:
        close(got[k], path32[k], want[k], f"head gradient {k}")
    # the input does not require grad: no data gradient is computed, the parameters' gradients are the same bits
    del calls[:]
    again = run(x)
    assert len(calls) == 1
    assert all(np.array_equal(again[k], got[k]) for k in again)


# ------------------------------------------------------------------------------------------------ RPN.forward in training

def small_rpn(pkg):
    from locov_amd.config import get_cfg
    from locov_amd.proposal_generator import build_proposal_generator
    from locov_amd.structures import Boxes, ImageList, Instances, ShapeSpec
    torch.manual_seed(3)
    cfg = get_cfg()
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[16, 32, 64]]
    cfg.MODEL.RPN.BATCH_SIZE_PER_IMAGE = 64
    rpn = build_proposal_generator(cfg, {"res4": ShapeSpec(channels=32, stride=16)}).cuda().train()
    size = (96, 160)
    images = ImageList(torch.zeros(2, 3, *size), [size, size])
    feats = {"res4": torch.randn(2, 32, 6, 10, device="cuda")}
    gt = [Instances(size, gt_boxes=Boxes(torch.tensor([[8.0, 8.0, 40.0, 36.0], [70.0, 20.0, 130.0, 80.0]], device="cuda"))),
          Instances(size, gt_boxes=Boxes(torch.tensor([[30.0, 30.0, 62.0, 62.0]], device="cuda")))]
    rnd = torch.rand(2, 2, 6 * 10 * 9, dtype=torch.float64, device="cuda")
    real = rpn.label_and_sample_anchors
    rpn.label_and_sample_anchors = lambda a, g, r=None: real(a, g, rnd)          # the same draw in every forward
    return rpn, images, feats, gt


def test_forward_in_training(pkg, monkeypatch):
    rpn, images, feats, gt = small_rpn(pkg)
    proposals, losses = rpn(images, feats, gt)
    assert set(losses) == {"loss_rpn_cls", "loss_rpn_loc"} and rpn._fused_batch is not None and rpn._pending_log is None
    labels = rpn._fused_batch[2]
    n_cls, n_loc = int((labels >= 0).sum()), 4 * int((labels == 1).sum())
    assert n_loc > 0 and n_cls == 2 * 64
    from locov_amd.roi_heads.labelling import get_event_storage
    sc = get_event_storage().scalars
    assert sc["rpn/num_pos_anchors"] == n_loc / 4 / 2 and sc["rpn/num_neg_anchors"] == (n_cls - n_loc / 4) / 2
    # proposals: the no_grad path's
    with torch.no_grad():
        anchors = rpn.anchor_generator([feats["res4"]])
        logits, deltas = rpn.rpn_head.flat_predictions([feats["res4"]])
        plain = rpn.predict_proposals(anchors, logits, deltas, images.image_sizes)
    for a, b in zip(proposals, plain):
        assert torch.equal(a.proposal_boxes.tensor, b.proposal_boxes.tensor) and torch.equal(a.objectness_logits, b.objectness_logits)
    # the chain's losses under the same draw.  Both are within their own error of the exact value: the chain within the fp32 bound
    # of tests/test_rpn_train_ref.py ((n + 8) 2^-24 for a sum of n terms), the kernel within twice that plus 2^-22 (the margin of
    # this file) -- so they differ by at most 3 (n + 8) 2^-24 + 2^-22, relative
    monkeypatch.setenv("LOCOV_FUSED_RPN", "0")
    _, chain = rpn(images, feats, gt)
    monkeypatch.delenv("LOCOV_FUSED_RPN")
    assert rpn._fused_batch is None
    for k, n in (("loss_rpn_cls", n_cls), ("loss_rpn_loc", n_loc)):
        a, b = float(losses[k]), float(chain[k])
        print(f"{k}: fused {a!r} chain {b!r}")
        assert abs(a - b) <= (3 * (n + 8) * 2.0 ** -24 + 2.0 ** -22) * abs(b)
    # one SGD step moves the head and invalidates its packed operands
    head = rpn.rpn_head
    before = {k: v.detach().clone() for k, v in head.named_parameters()}
    key, packed = head._operands_key, head._operands()[0].clone()
    opt = torch.optim.SGD(rpn.parameters(), lr=0.1)
    (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
    opt.step()
    assert all(not torch.equal(v.detach(), before[k]) for k, v in head.named_parameters())
    assert head._operands()[0].shape == packed.shape and head._operands_key != key and not torch.equal(head._operands()[0], packed)


def test_training_enqueue_makes_no_host_synchronisation(pkg):
    """Labelling, sampling and the losses read nothing back: torch's synchronisation debug mode in "error" around the enqueue part
    (everything between the head and predict_proposals, whose one read the counters then ride behind)."""
    rpn, images, feats, gt = small_rpn(pkg)
    rpn(images, feats, gt)                                          # (warm-up: workspaces, pinned buffers)
    anchors = rpn.anchor_generator([feats["res4"]])
    logits, deltas = rpn.rpn_head.flat_predictions([feats["res4"]])
    torch.cuda.synchronize()
    waits = [0]
    plain = torch.cuda.Event.synchronize

    def counted(self):
        waits[0] += 1
        return plain(self)

    torch.cuda.Event.synchronize = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        labels, boxes = rpn.label_and_sample_anchors(anchors, gt)
        rpn._defer_log = True
        losses = rpn.losses(anchors, logits, labels, deltas, boxes)
        (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
    finally:
        rpn._defer_log = False
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.Event.synchronize = plain
    assert waits[0] == 0 and rpn._pending_log is not None
    rpn._flush_log()
    assert rpn._pending_log is None


def test_limits_route_to_the_chain(pkg):
    c = tc.case("tie_max")
    rpn = tc.make_rpn(c)
    anchors, gt, rnd = tc.inputs(c, "cuda")
    fused = rpn.label_and_sample_anchors(anchors, gt, rnd)
    assert rpn._fused_batch is not None
    # two levels: the same anchors split in two
    from locov_amd.structures import Boxes
    a = anchors[0].tensor
    two = [Boxes(a[:100]), Boxes(a[100:])]
    got = rpn.label_and_sample_anchors(two, gt, rnd)
    assert rpn._fused_batch is None
    assert all(torch.equal(x, y) for x, y in zip(fused[0] + fused[1], got[0] + got[1]))
    # more images than a call takes
    n = pkg.ops.RPN_MAX_IMAGES + 1
    many = [gt[i % 2] for i in range(n)]
    rnd_many = rnd[:, [i % 2 for i in range(n)]].contiguous()
    got = rpn.label_and_sample_anchors(anchors, many, rnd_many)
    assert rpn._fused_batch is None and len(got[0]) == n
    assert torch.equal(got[0][0], fused[0][0]) and torch.equal(got[0][n - 1], fused[0][(n - 1) % 2]) and torch.equal(got[1][1], fused[1][1])
