"""Without a GPU: every case of tests/rpn_train_cases.py is exact in fp32 and reaches what it is meant to under the reference alone
(tests/rpn_train_ref.py), and the torch chain of RPN.label_and_sample_anchors / RPN.losses equals the reference on the CPU -- labels and
matched boxes exactly, losses and autograd gradients within fp32 rounding -- so that the GPU tests hold the kernels against a
reference the chain agrees with."""
import numpy as np
import pytest
import torch

import rpn_train_cases as tc
import rpn_train_ref as ref


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_is_exact_and_reaches_its_marks(name):
    c = tc.case(name)
    tc.check_exactness(c)
    tc.check_conditions(c, tc.reference(name))


def test_shapes_cover_the_listed_ground():
    cases = [tc.case(n) for n in tc.NAMES]
    assert {c["anchors"].shape[0] for c in cases} == {189, 12765}
    assert {len(c["gt"]) for c in cases} == {1, 2, 3}
    assert {0, 1, 5, 70} <= {g.shape[0] for c in cases for g in c["gt"]}


def chain(c):
    rpn = tc.make_rpn(c)
    anchors, gt, rnd = tc.inputs(c)
    labels, boxes = rpn.label_and_sample_anchors(anchors, gt, rnd)
    return rpn, anchors, labels, boxes


@pytest.mark.parametrize("name", tc.NAMES)
def test_cpu_chain_labels_equal_reference(name):
    c = tc.case(name)
    _, _, labels, boxes = chain(c)
    B, max_pos = c["budget"], int(c["budget"] * c["fraction"])
    for lab, box, r in zip(labels, boxes, tc.reference(name)):
        assert lab.dtype == torch.int8 and tuple(box.shape) == (c["anchors"].shape[0], 4)
        got = lab.numpy()
        assert np.array_equal(got, r["final"])
        assert np.array_equal(box.numpy().view(np.int32), r["matched_boxes"].view(np.int32))
        # the draw never exceeds the budget and never picks outside the populations
        assert (got == 1).sum() <= max_pos and (got >= 0).sum() <= B
        assert not (got[r["labels"] != 1] == 1).any() and not (got[r["labels"] != 0] == 0).any()


@pytest.mark.parametrize("name", tc.SMALL + ["big_over_and_fill"])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_cpu_chain_losses_against_float64(name, beta):
    """Bounds.  A loss is an fp32 sum of n non-negative terms, each a few roundings: relative error at most (n + 8) 2^-24.  A gradient
    entry is one sigmoid (or a sign, or e / beta) times weight / normalizer -- a few roundings: 8 x 2^-24 of the largest entry."""
    c = dict(tc.case(name), beta=beta)
    rpn = tc.make_rpn(c, loss_weight={"loss_rpn_cls": 2.0, "loss_rpn_loc": 0.5})
    anchors, gt, rnd = tc.inputs(c)
    labels, boxes = rpn.label_and_sample_anchors(anchors, gt, rnd)
    logits = torch.from_numpy(c["logits"]).requires_grad_()
    deltas = torch.from_numpy(c["deltas"]).requires_grad_()
    out = rpn.losses(anchors, [logits], labels, [deltas], boxes)
    assert set(out) == {"loss_rpn_cls", "loss_rpn_loc"}
    (out["loss_rpn_cls"] + out["loss_rpn_loc"]).backward()
    lab = np.stack([r["final"] for r in tc.reference(name)])
    mb = np.stack([r["matched_boxes"] for r in tc.reference(name)])
    cls, loc, dl, dd = ref.losses(c["logits"], c["deltas"], lab, c["anchors"], mb, c["weights"], beta, c["budget"], 2.0, 0.5)
    n_cls, n_loc = int((lab >= 0).sum()), 4 * int((lab == 1).sum())
    assert abs(float(out["loss_rpn_cls"]) - cls) <= (n_cls + 8) * 2.0 ** -24 * abs(cls)
    assert abs(float(out["loss_rpn_loc"]) - loc) <= (n_loc + 8) * 2.0 ** -24 * abs(loc)
    assert np.abs(logits.grad.numpy() - dl).max() <= 8 * 2.0 ** -24 * max(np.abs(dl).max(), 1e-30)
    assert np.abs(deltas.grad.numpy() - dd).max() <= 8 * 2.0 ** -24 * max(np.abs(dd).max(), 1e-30)
    assert not logits.grad.numpy()[lab < 0].any() and not deltas.grad.numpy()[lab != 1].any()


def test_drawn_keys_pick_every_positive_uniformly():
    """rnd=None, 200 draws: every positive anchor of an image with more positives than max_pos is picked num_pos / population of the
    time, within 5 standard deviations of the binomial count.  This checks the wiring of the drawn keys, it is no statistical claim."""
    c = tc.case("b7_with_empty")
    rpn = tc.make_rpn(c)
    anchors, gt, _ = tc.inputs(c)
    r = tc.reference("b7_with_empty")[0]
    pos = np.nonzero(r["labels"] == 1)[0]
    assert pos.size > r["num_pos"] == 3
    torch.manual_seed(1234)
    draws, hits = 200, np.zeros(pos.size)
    for _ in range(draws):
        got = rpn.label_and_sample_anchors(anchors, gt)[0][0].numpy()
        assert (got == 1).sum() == 3 and not (got[r["labels"] != 1] == 1).any()
        hits += got[pos] == 1
    p = 3.0 / pos.size
    assert np.abs(hits - draws * p).max() <= 5 * np.sqrt(draws * p * (1 - p))
