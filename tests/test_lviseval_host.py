"""The LVIS box-AP evaluator's host path (numpy, float64: the definition) against the issue's hand-worked case and against the loop
restatement of the protocol in tests/lviseval_ref.py; the derived results, build_evaluator and inference_on_dataset.  No GPU needed."""
import json
import math

import numpy as np
import pytest
import torch

import lviseval_cases as cases
import lviseval_ref

KEYS = ("precision", "recall", "stats")
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"]


def _run(gt, dets, cap=300, **kw):
    from locov_amd.evaluation import LVISEvaluator
    ev = LVISEvaluator(gt, max_dets_per_image=cap, **kw)
    cases.feed(ev, dets)
    return ev, ev.evaluate()


def _same(got, want):
    assert sorted(got) == sorted(KEYS)
    for key in KEYS:
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key


def test_the_hand_worked_case_under_both_protocols():
    from locov_amd.evaluation import COCOEvaluator
    gt, dets = cases.handworked()
    ev, res = _run(gt, dets)
    p, r, stats = ev.eval["precision"], ev.eval["recall"], ev.eval["stats"]
    assert p.shape == (10, 101, 3, 4) and r.shape == (10, 3, 4) and stats.shape == (13,)
    assert np.all(p[:, :, 0, 0] == 0.5) and np.all(p[:, :, 0, 1] == 0.5) and np.all(r[:, 0, 0] == 1.0)     # category 1, "all" and "small"
    assert np.all(p[:, :, 0, 2:] == -1) and np.all(p[:, :, 1:] == -1) and np.all(r[:, 1:] == -1)           # E: a category with no gt
    res = res["bbox"]
    assert list(res) == METRICS
    assert all(res[k] == 50.0 for k in ("AP", "AP50", "AP75", "APs", "APf")), res
    assert all(res[k] == -100.0 for k in ("APm", "APl", "APr", "APc")), res
    assert stats[9:13].tolist() == [1.0, 1.0, -1.0, -1.0]
    _same(ev.eval, lviseval_ref.evaluate(gt, dets))
    coco = COCOEvaluator(gt)                                                          # A, B and C are false positives there
    cases.feed(coco, dets)
    assert coco.evaluate()["bbox"]["AP"] == 25.0


def test_the_cap_runs_across_the_categories_of_an_image():
    """The issue's cap example: .9 (class 0), .5 (class 1), .5 (class 0) under a cap of 2 keeps the first two."""
    from locov_amd import evaluation as E
    gt, dets = cases.cap_example()
    img, cls = np.zeros(3, dtype=np.int64), np.array([d[1] for d in dets])
    score = np.array([float(d[2]) for d in dets])
    assert E.limit_host(img, cls, score, 2, 2).tolist() == [True, True, False]
    assert E.limit_host(img, cls, score, 2, 3).all()
    assert E.limit_host(img, np.array([0, 7, 0]), score, 2, 2).tolist() == [True, False, True]   # a class outside the bank takes no place
    ev, _ = _run(gt, dets, 2)
    assert np.all(ev.eval["recall"][:, 0, 0] == 0.0) and np.all(ev.eval["recall"][:, 1, 0] == 1.0)   # the dropped det was category 1's
    _same(ev.eval, lviseval_ref.evaluate(gt, dets, 2))
    ev, _ = _run(gt, dets, 300)
    assert np.all(ev.eval["recall"][:, :, 0] == 1.0)


CASES = {"edge": cases.edge_cases, "straddle": cases.straddle_case}
CASES.update({f"random{s}": (lambda s=s: cases.random_case(s)) for s in range(4)})


@pytest.mark.parametrize("cap", [300, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_the_host_path_equals_the_loop_restatement(name, cap):
    gt, dets = CASES[name]()
    ev, _ = _run(gt, dets, cap)
    _same(ev.eval, lviseval_ref.evaluate(gt, dets, cap))


def test_the_shared_matching_is_one_function_under_both_switches():
    """With no ignore flag, no not-exhaustive entry and every cell listed, nothing the LVIS switches select can act (and without an
    iscrowd field nothing the COCO ones select can): match_host and match_host_lvis give the same bits on the same dets."""
    import copy
    from locov_amd import evaluation as E
    gt, dets = cases.random_case(2)
    gt = copy.deepcopy(gt)
    for a in gt["annotations"]:
        a["ignore"] = 0
    for im in gt["images"]:
        im["not_exhaustive_category_ids"] = []
        im["neg_category_ids"] = [c["id"] for c in gt["categories"]]
    coco, lvis = E._GroundTruth(gt), E._LVISGroundTruth(gt)
    assert not coco.crowd.any() and not lvis.ignore.any()
    dets = [d for d in dets if 0 <= d[1] < coco.n_categories]                          # (the LVIS path leaves the others out first)
    img = np.array([coco.image_rank[d[0]] for d in dets], dtype=np.int64)
    cls = np.array([d[1] for d in dets], dtype=np.int64)
    score = np.array([float(d[2]) for d in dets], dtype=np.float64)
    perm, det_off, _, _, _ = E.order_host(img, cls, score, coco.n_images, coco.n_categories)
    boxes = np.stack([d[3] for d in dets])[perm]
    bits, gt_ignore = E.match_host(coco, det_off, boxes, 300)
    bits_lvis, gt_ignore_lvis, listed = E.match_host_lvis(lvis, det_off, boxes, 300)
    assert np.array_equal(bits, bits_lvis) and np.array_equal(gt_ignore, gt_ignore_lvis)
    assert int(det_off[-1]) == len(dets) and listed[:int(det_off[-1])].all()
    assert (bits == 1).any() and (bits == 0).any()                                     # matched and counted; unmatched and counted
    assert ((np.diff(det_off) >= 2) & (np.diff(coco.offsets) >= 2)).any()              # a cell where the walk over the gts has a choice


def test_the_large_case_equals_the_loop_restatement():
    gt, dets = cases.large_case()
    ev, _ = _run(gt, dets)
    _same(ev.eval, lviseval_ref.evaluate(gt, dets))
    assert sum(1 for d in dets if d[0] <= 4 and d[1] == 0) > 1024 + 80                   # (more than a chunk even after the cap)


def test_the_edge_cases_hold_what_they_claim():
    from locov_amd import evaluation as E
    gt, dets = cases.edge_cases()
    ev, res = _run(gt, dets)
    p, r, stats = ev.eval["precision"], ev.eval["recall"], ev.eval["stats"]
    assert np.all(p[:, :, 2, 0] == 0) and np.all(r[:, 2, 0] == 0)                     # category 11: gts and no det at all
    assert np.all(p[:, :, 3] == -1) and np.all(r[:, 3] == -1)                         # category 20: no gt, dets in a negative cell
    g = E._LVISGroundTruth(gt)
    assert [grp.tolist() for grp in g.freq_groups] == [[], [1], [0, 2, 5]]            # no rare category; 20 and 42 in no group
    assert stats[6] == -1.0 and res["bbox"]["APr"] == -100.0
    assert stats[7] == float(np.mean(p[:, :, 1, 0])) and stats[8] == float(np.mean(p[:, :, [0, 2, 5], 0]))
    in_ap = np.ascontiguousarray(p[:, :, [0, 1, 2, 4, 5], 0]).ravel()                 # category 42 counts in AP only
    assert (p[:, :, 4, 0] > -1).all() and stats[0] == float(np.mean(in_ap))
    # category 7 (class 1): one gt with a det at IoU > 0.9, and image 4's negative cell: three false positives, each ignored outside
    # its own area range; the det in image 2's not-exhaustive cell (0.875, the category's best score) is unlisted and changes nothing
    one_tp = 1.0 / (0.0 + 1.0 + np.spacing(1))                                        # pr of a first det that is a true positive
    assert np.all(r[:9, 1, 0] == 1.0) and np.all(p[:9, :, 1, 0] == one_tp)            # (only 0.625 and lower are false positives)
    flags = g.cell_flags.reshape(g.n_categories, g.n_images)
    assert flags[1, g.image_rank[4]] == 1 and flags[3, g.image_rank[4]] == 1 and flags[0, g.image_rank[17]] == 2
    assert flags[1, g.image_rank[2]] == 2 and int(np.count_nonzero(flags)) == 4
    # the medium range of category 42: the first 40 x 40 det takes the (small, so ignored) gt and the second is a false positive
    only = [d for d in dets if d[1] == 4]
    ev42, _ = _run(gt, only)
    assert np.all(ev42.eval["recall"][:, 4, 2] == 1.0) and np.all(ev42.eval["precision"][:, :, 4, 2] == 0.5)
    # at a cap of 3, image 17 keeps 0.75 and the first two of its four 0.5s; the two classes outside the bank took no place
    img = np.array([g.image_rank[d[0]] for d in dets], dtype=np.int64)
    cls = np.array([d[1] for d in dets], dtype=np.int64)
    score = np.array([float(d[2]) for d in dets], dtype=np.float64)
    keep = E.limit_host(img, cls, score, g.n_categories, 3)
    assert keep[:7].tolist() == [False, False, True, True, True, False, False]


def test_result_keys_and_the_nan_rules():
    gt, dets = cases.edge_cases()
    ev, res = _run(gt, dets)
    assert list(res) == ["bbox"] and list(res["bbox"]) == METRICS
    assert all(res["bbox"][m] == ev.eval["stats"][i] * 100 for i, m in enumerate(METRICS))
    ev, res = _run(gt, [])                                                            # nothing processed: the all-nan dict
    assert ev.eval is None and list(res["bbox"]) == METRICS and all(math.isnan(v) for v in res["bbox"].values())
    only_unlisted = [d for d in dets if d[0] == 9 and d[1] == 5]                      # processed, and nothing takes part
    ev, res = _run(gt, only_unlisted)
    assert res["bbox"]["AP"] == 0.0 and res["bbox"]["APr"] == -100.0
    assert np.all(ev.eval["precision"][:, :, 5, 0] == 0) and np.all(ev.eval["recall"][:, 5, 0] == 0)


def test_constructor_and_process_checks(tmp_path):
    from locov_amd import LVISEvaluator
    gt, dets = cases.handworked()
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(gt))
    ev = LVISEvaluator(str(path))
    assert ev.max_dets_per_image == 300
    cases.feed(ev, dets)
    want = lviseval_ref.evaluate(gt, dets)
    ev.evaluate()
    _same(ev.eval, want)
    ev.reset()
    assert ev.eval is None and math.isnan(ev.evaluate()["bbox"]["APr"])
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="max_dets_per_image"):
            LVISEvaluator(gt, max_dets_per_image=bad)
    with pytest.raises(ValueError, match="class names"):
        LVISEvaluator(gt, class_names=["a", "b"])
    LVISEvaluator(gt, class_names=["a", "b", "c"])
    with pytest.raises(KeyError, match="not in the ground truth"):
        cases.feed(ev, [cases._det(77, 0, 0.5, [0, 0, 1, 1])])
    ev.reset()
    cases.feed(ev, dets + [cases._det(1, 5, 0.99, [0, 0, 10, 10]), cases._det(1, -1, 0.99, [0, 0, 10, 10])])   # classes outside the bank
    ev.evaluate()
    _same(ev.eval, want)


def test_build_evaluator_dispatches_on_the_dataset_name():
    import locov_amd
    from locov_amd import COCOEvaluator, LVISEvaluator, build_evaluator
    gt, _ = cases.handworked()
    for name in ("lvis_v1_val", "lvis_v1_train_norare", "my_lvis"):
        ev = build_evaluator(name, gt, max_dets_per_image=7)
        assert type(ev) is LVISEvaluator and ev.max_dets_per_image == 7
    for name in ("coco_2017_val", "coco_zeroshot_val", "LVIS"):
        ev = build_evaluator(name, gt, max_dets=(1, 5))
        assert type(ev) is COCOEvaluator and ev.max_dets == (1, 5)
    assert locov_amd.build_evaluator is build_evaluator and locov_amd.LVISEvaluator is LVISEvaluator


class _Stub(torch.nn.Module):
    def __init__(self, dets):
        super().__init__()
        self.dets = dets

    def forward(self, inputs):
        from locov_amd.structures import Boxes, Instances
        assert not self.training and not torch.is_grad_enabled()
        out = []
        for inp in inputs:
            ds = [d for d in self.dets if d[0] == inp["image_id"]]
            inst = Instances((480, 640))
            inst.pred_boxes = Boxes(torch.from_numpy(np.stack([d[3] for d in ds]).reshape(-1, 4)) if ds else torch.zeros(0, 4))
            inst.scores = torch.tensor([float(d[2]) for d in ds], dtype=torch.float32)
            inst.pred_classes = torch.tensor([d[1] for d in ds], dtype=torch.int64)
            out.append(dict(instances=inst))
        return out


def test_inference_on_dataset_works_with_the_lvis_evaluator():
    from locov_amd import LVISEvaluator, inference_on_dataset
    gt, dets = cases.random_case(3)
    ids = [im["id"] for im in gt["images"]]
    loader = [[dict(image_id=i) for i in ids[n:n + 2]] for n in range(0, len(ids), 2)]
    ev = LVISEvaluator(gt, max_dets_per_image=5)
    model = _Stub(dets).train()
    res = inference_on_dataset(model, loader, ev)
    assert model.training
    by_image = sorted(dets, key=lambda d: ids.index(d[0]))                             # (stable: the order the stub emits)
    _same(ev.eval, lviseval_ref.evaluate(gt, by_image, 5))
    assert res["bbox"]["APr"] == ev.eval["stats"][6] * 100


def test_ap75_reads_the_sixth_threshold():
    from locov_amd.evaluation import IOU_THRS
    assert IOU_THRS[5] == 0.75 and lviseval_ref.IOU_THRS[5] == 0.75 and IOU_THRS[0] == 0.5
