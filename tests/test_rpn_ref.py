"""Without a GPU: every case of tests/rpn_cases.py reaches what it is meant to under the float64 reference alone (tests/rpn_ref.py),
and the torch chain of locov_amd/proposal_generator.py (find_top_rpn_proposals: stable sort, gather, apply_deltas, finite test, clip,
nonempty, batched_nms, slice) equals the reference on the CPU on every exact case -- boxes and logits as bit patterns, indices and
counts -- so that the GPU tests hold the kernels against a reference the chain agrees with."""
import numpy as np
import pytest
import torch

import rpn_cases as rc


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_is_exact_and_reaches_its_marks(name):
    c = rc.all_cases()[name]
    rc.check_exactness(c)
    rc.check_conditions(c, rc.reference(name))


def test_every_listed_shape_is_present():
    cases = rc.all_cases()
    assert set(cases) == set(rc.NAMES)
    assert [cases[f"hwa{n}"]["logits"].shape[1] for n in (1, 63, 64, 65)] == [1, 63, 64, 65]
    assert all(cases[f"hwa{n}"]["pre"] > n for n in (1, 63, 64, 65))
    big = cases["big_70000"]
    assert big["logits"].shape == (2, 70000) and (big["pre"], big["post"]) == (12000, 2000)
    assert cases["batch_2000"]["logits"].shape == (3, 2000) and cases["tie_cut"]["logits"].shape == (1, 60)


def chain_on_cpu(c, training=False):
    from locov_amd.proposal_generator import find_top_rpn_proposals
    from locov_amd.roi_heads.box_emb_head import Box2BoxTransform
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return find_top_rpn_proposals([t(c["logits"])], [t(c["deltas"])], [t(c["anchors"])], c["image_hw"],
                                  Box2BoxTransform(c["weights"], c["scale_clamp"]), c["nms_thresh"], c["pre"], c["post"], c["min_box_size"],
                                  training)


@pytest.mark.parametrize("name", rc.EXACT)
def test_cpu_chain_equals_reference(name):
    c = rc.all_cases()[name]
    for rec, (boxes, logits, index, level) in zip(rc.reference(name), chain_on_cpu(c)):
        assert len(index) == rec["count"]
        assert index.tolist() == rec["index"].tolist()
        assert np.array_equal(boxes.numpy().view(np.int32), rec["boxes"].view(np.int32))
        assert np.array_equal(logits.numpy().view(np.int32), rec["logits"].view(np.int32))
        assert not level.any()


def test_cpu_chain_on_non_finite_boxes():
    """exp(100) without the clamp: evaluation drops the proposals (all of them here), training raises as Detectron2 does."""
    c = rc.all_cases()["no_clamp_overflow"]
    assert [len(r[2]) for r in chain_on_cpu(c)] == [0]
    with pytest.raises(FloatingPointError):
        chain_on_cpu(c, training=True)
