"""The COCO box-AP evaluator's host path (numpy, float64: the definition) against a hand-worked case and against the loop
restatement of the protocol in tests/cocoeval_ref.py; the derived results and inference_on_dataset.  No GPU needed."""
import json
import math

import numpy as np
import pytest
import torch

import cocoeval_cases as cases
import cocoeval_ref


def _run(gt, dets, max_dets=(1, 10, 100), **kw):
    from locov_amd.evaluation import COCOEvaluator
    ev = COCOEvaluator(gt, max_dets=max_dets, **kw)
    cases.feed(ev, dets)
    return ev, ev.evaluate()


def _same(got, want):
    for key in ("precision", "recall", "scores", "stats"):
        assert got[key].dtype == np.float64 and np.array_equal(got[key], want[key]), key


def test_the_hand_worked_case():
    ev, res = _run(*cases.handworked())
    p, r = ev.eval["precision"], ev.eval["recall"]
    assert p.shape == (10, 101, 1, 4, 3) and r.shape == (10, 1, 4, 3) and ev.eval["scores"].shape == p.shape
    assert np.mean(p[0, :, 0, 0, 2]) == 0.834983498349835
    assert np.mean(p[1, :, 0, 0, 2]) == 0.5049504950495048
    assert r[0, 0, 0].tolist() == [0.5, 1.0, 1.0]
    assert np.all(r[1:, 0, 0] == 0.5)
    assert np.all(p[:, :, :, 3] == -1) and np.all(r[:, :, 3] == -1)                  # the large-area range holds no gt
    assert np.array_equal(p[:, :, :, 1], p[:, :, :, 0]) and np.array_equal(r[:, :, 1], r[:, :, 0])
    assert res["bbox"]["AP50"] == 83.4983498349835 and math.isnan(res["bbox"]["APl"])
    assert list(res["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]           # one category: no per-category rows


def test_dets_equal_to_the_gts_score_one():
    ev, res = _run(*cases.perfect())
    assert np.all(ev.eval["stats"] == 1.0), ev.eval["stats"]
    assert all(res["bbox"][k] == 100.0 for k in ("AP", "AP50", "AP75", "APs", "APm", "APl", "AP-cat10", "AP-cat20"))


@pytest.mark.parametrize("name,max_dets", [("edge", (1, 2, 5)), ("carry", (1, 10, 100)), ("many_gts", (1, 2, 5)), ("chunk", (1, 10, 100))] +
                         [(s, (1, 2, 5)) for s in range(6)] + [(100 + s, (1, 10, 100)) for s in range(3)] + [(200, (3,)), (201, (2, 4))])
def test_the_host_path_equals_the_loop_restatement(name, max_dets):
    if isinstance(name, int):
        gt, dets = cases.random_case(name, 10, 5, 30) if name >= 100 else cases.random_case(name)
    else:
        gt, dets = {"edge": cases.edge_cases, "carry": cases.carry_case, "many_gts": cases.many_gts_case,
                    "chunk": lambda: cases.carry_case(19, 41, 25)}[name]()
    ev, _ = _run(gt, dets, max_dets)
    _same(ev.eval, cocoeval_ref.evaluate(gt, dets, max_dets))


def test_the_edge_cases_hold_what_they_claim():
    gt, dets = cases.edge_cases()
    ev, res = _run(gt, dets, (1, 2, 5))
    p, r = ev.eval["precision"], ev.eval["recall"]
    assert np.all(p[:, :, 1] == -1) and np.all(r[:, 1] == -1)                         # only crowd gts
    assert np.all(p[:, :, 2, 0] == 0) and np.all(r[:, 2, 0] == 0)                     # gts and no det at all
    assert np.all(p[:, :, 3] == -1) and np.all(p[:, :, 5] == -1)                      # no cell; dets and no gt
    assert math.isnan(res["bbox"]["AP-cat7"]) and res["bbox"]["AP-cat11"] == 0.0
    # the later gt takes the det at equal IoU: with the earlier one taken, image 30's second det would be a false positive at 0.5
    only30 = [d for d in dets if d[0] == 30]
    gt30 = dict(gt, images=[im for im in gt["images"] if im["id"] == 30], annotations=[a for a in gt["annotations"] if a["image_id"] == 30])
    ev30, _ = _run(gt30, only30, (1, 2, 5))
    assert ev30.eval["recall"][0, 0, 0, 2] == 1.0 and np.all(ev30.eval["precision"][0, :, 0, 0, 2] == 1.0)


def test_derived_results_and_the_nan_rules():
    gt, dets = cases.edge_cases()
    names = ["a", "b", "c", "d", "e", "f"]
    ev, res = _run(gt, dets, (1, 2, 5), class_names=names, seen_names=["a", "e", "c"], unseen_names=["b", "a"])
    res = res["bbox"]
    p = ev.eval["precision"]
    ap50 = lambda k: float(np.mean(p[0, :, k, 0, -1]) * 100) if (p[0, :, k, 0, -1] > -1).any() else float("nan")
    assert [k for k in res if k.startswith("AP-")] == ["AP-" + n for n in names]
    assert res["AP-a"] == float(np.mean(p[:, :, 0, 0, -1]) * 100)
    assert res["AP50-seen"] == (ap50(0) + ap50(2) + ap50(4)) / 3                       # (class order, as the reference sums them)
    assert math.isnan(res["AP50-unseen"])                                              # "b" has no valid precision: the mean is nan
    assert res["AP"] == ev.eval["stats"][0] * 100 and res["APl"] == ev.eval["stats"][5] * 100
    _, res = _run(gt, dets, (1, 2, 5))                                                 # the categories' own names; no lists: nan
    assert "AP-cat3" in res["bbox"] and math.isnan(res["bbox"]["AP50-seen"]) and math.isnan(res["bbox"]["AP50-unseen"])
    ev, res = _run(gt, [], (1, 2, 5))                                                  # nothing processed: the all-nan dict
    assert ev.eval is None and list(res["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    assert all(math.isnan(v) for v in res["bbox"].values())


def test_constructor_and_process_checks(tmp_path):
    from locov_amd import COCOEvaluator
    gt, dets = cases.handworked()
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(gt))
    ev = COCOEvaluator(str(path))
    cases.feed(ev, dets)
    want = cocoeval_ref.evaluate(gt, dets)
    ev.evaluate()
    _same(ev.eval, want)
    ev.reset()
    assert ev.eval is None and math.isnan(ev.evaluate()["bbox"]["AP"])
    for bad in ((), (10, 1), (1, 1), (0, 5), (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="max_dets"):
            COCOEvaluator(gt, max_dets=bad)
    with pytest.raises(ValueError, match="class names"):
        COCOEvaluator(gt, class_names=["a", "b"])
    with pytest.raises(KeyError, match="not in the ground truth"):
        cases.feed(ev, [cases._det(77, 0, 0.5, [0, 0, 1, 1])])
    ev.reset()
    cases.feed(ev, dets + [cases._det(1, 5, 0.99, [0, 0, 10, 10]), cases._det(1, -1, 0.99, [0, 0, 10, 10])])   # classes outside the bank: unread
    ev.evaluate()
    _same(ev.eval, want)


class _Stub(torch.nn.Module):
    def __init__(self, dets):
        super().__init__()
        self.dets, self.calls = dets, []

    def forward(self, inputs):
        from locov_amd.structures import Boxes, Instances
        assert not self.training and not torch.is_grad_enabled()
        out = []
        for inp in inputs:
            self.calls.append(inp["image_id"])
            ds = [d for d in self.dets if d[0] == inp["image_id"]]
            inst = Instances((480, 640))
            inst.pred_boxes = Boxes(torch.from_numpy(np.stack([d[3] for d in ds]).reshape(-1, 4)) if ds else torch.zeros(0, 4))
            inst.scores = torch.tensor([float(d[2]) for d in ds], dtype=torch.float32)
            inst.pred_classes = torch.tensor([d[1] for d in ds], dtype=torch.int64)
            out.append(dict(instances=inst))
        return out


def test_inference_on_dataset_feeds_in_order_and_restores_the_mode():
    from locov_amd import COCOEvaluator, inference_on_dataset
    gt, dets = cases.random_case(3)
    ids = [im["id"] for im in gt["images"]]
    loader = [[dict(image_id=i) for i in ids[n:n + 2]] for n in range(0, len(ids), 2)]
    seen = []

    class Recording(COCOEvaluator):
        def process(self, inputs, outputs):
            seen.extend(i["image_id"] for i in inputs)
            super().process(inputs, outputs)

    ev = Recording(gt, max_dets=(1, 2, 5))
    with torch.no_grad():
        ev.process([dict(image_id=ids[0])], _Stub(dets).eval()([dict(image_id=ids[0])]))   # stale state: inference_on_dataset resets it
    seen.clear()
    for training in (True, False):
        model = _Stub(dets).train(training)
        res = inference_on_dataset(model, loader, ev)
        assert model.training is training and model.calls == ids and seen[-len(ids):] == ids
    by_image = sorted(dets, key=lambda d: ids.index(d[0]))                             # (stable: the order the stub emits)
    _same(ev.eval, cocoeval_ref.evaluate(gt, by_image, (1, 2, 5)))
    assert res["bbox"]["AP"] == ev.eval["stats"][0] * 100

    class Broken(torch.nn.Module):
        def forward(self, inputs):
            raise RuntimeError("boom")

    model = Broken().train()
    with pytest.raises(RuntimeError, match="boom"):
        inference_on_dataset(model, loader, ev)
    assert model.training
