"""The device path of the COCO box-AP evaluator (csrc/coco_eval.hip) against the loop restatement of the protocol in
tests/cocoeval_ref.py, bit for bit: everything is float64 and integer, so there is no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import cocoeval_cases as cases
import cocoeval_ref

pytestmark = pytest.mark.gpu

KEYS = ("precision", "recall", "scores", "stats")
CASES = {
    "edge": (cases.edge_cases, (1, 2, 5)),
    "random0": (lambda: cases.random_case(0), (1, 2, 5)),
    "random1": (lambda: cases.random_case(1), (1, 2, 5)),
    "random2": (lambda: cases.random_case(2, 9, 5, 20), (1, 2, 5)),
    "random3": (lambda: cases.random_case(100, 10, 5, 30), (1, 10, 100)),
    "two_caps": (lambda: cases.random_case(201), (2, 4)),
    "carry": (cases.carry_case, (1, 10, 100)),
    "many_gts": (cases.many_gts_case, (1, 2, 5)),
    # the two sides of each size at which a kernel changes its path: 5 dets x G gts fit the cell's 8 KiB of LDS up to G = 78
    # (5 * G * 8 + G * 64 <= 8192); a category's dets fill one chunk of the accumulation up to 1 024
    "lds_78_gts": (lambda: cases.many_gts_case(17, 78), (1, 2, 5)),
    "workspace_79_gts": (lambda: cases.many_gts_case(17, 79), (1, 2, 5)),
    "chunk_1024_dets": (lambda: cases.carry_case(19, 32, 32), (1, 10, 100)),
    "chunk_1025_dets": (lambda: cases.carry_case(19, 41, 25), (1, 10, 100)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(gt, dets, max_dets, the reference's arrays): computed once and shared."""
    make, max_dets = CASES[name]
    gt, dets = make()
    want = cocoeval_ref.evaluate(gt, dets, max_dets)
    for v in want.values():
        v.setflags(write=False)
    return gt, dets, max_dets, want


def _run(gt, dets, max_dets, where="cuda", **kw):
    from locov_amd.evaluation import COCOEvaluator
    ev = COCOEvaluator(gt, max_dets=max_dets, **kw)
    cases.feed(ev, dets, where)
    res = ev.evaluate()
    return ev, res


@pytest.fixture
def launches(monkeypatch):
    """Counts the two kernels' launches, so that a test knows which path ran."""
    from locov_amd import ops
    n = dict(match=0, accumulate=0)
    match, accumulate = ops.coco_match, ops.coco_accumulate

    def spy_match(*a, **k):
        n["match"] += 1
        return match(*a, **k)

    def spy_accumulate(*a, **k):
        n["accumulate"] += 1
        return accumulate(*a, **k)

    monkeypatch.setattr(ops, "coco_match", spy_match)
    monkeypatch.setattr(ops, "coco_accumulate", spy_accumulate)
    return n


def _assert_same(got, want):
    for key in KEYS:
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape, key
        diff = np.argwhere(got[key] != want[key])
        assert diff.size == 0, f"{key}: {len(diff)} entries differ, first at {diff[0].tolist()}: {got[key][tuple(diff[0])]!r} != {want[key][tuple(diff[0])]!r}"


@pytest.mark.parametrize("name", ["edge", "random0", "random1", "random2", "random3", "two_caps", "lds_78_gts", "workspace_79_gts",
                                  "chunk_1024_dets", "chunk_1025_dets"])
def test_device_path_equals_the_protocol_bit_for_bit(name, launches, monkeypatch):
    monkeypatch.delenv("LOCOV_FUSED_COCOEVAL", raising=False)
    gt, dets, max_dets, want = _case(name)
    ev, _ = _run(gt, dets, max_dets)
    assert launches == dict(match=1, accumulate=1)                                   # the device path is the default
    _assert_same(ev.eval, want)


def test_the_match_kernel_equals_the_host_matching(monkeypatch):
    """The first kernel's own outputs (matched / ignored bits per det, ignore flags per gt) on the edge cases, where a difference
    names the cell it is in."""
    from locov_amd import evaluation as E, ops
    gt, dets, max_dets, _ = _case("edge")
    g = E._GroundTruth(gt)
    img = np.array([g.image_rank[d[0]] for d in dets], dtype=np.int64)
    cls = np.array([d[1] for d in dets], dtype=np.int64)
    score = np.array([float(d[2]) for d in dets], dtype=np.float64)
    boxes = np.stack([d[3] for d in dets])
    perm, det_off, rank, acc_index, cat_off = E.order_host(img, cls, score, g.n_images, g.n_categories)
    bits, gt_ignore = E.match_host(g, det_off, boxes[perm], max_dets[-1])
    up = lambda a: torch.from_numpy(a).cuda()
    o = ops.coco_order(up(img), up(cls), up(score), up(boxes), g.n_images, g.n_categories)
    assert np.array_equal(o.det_offsets.cpu().numpy(), det_off) and np.array_equal(o.boxes.cpu().numpy(), boxes[perm])
    assert np.array_equal(o.acc_index.cpu().numpy(), acc_index) and np.array_equal(o.cat_offsets.cpu().numpy(), cat_off)
    assert np.array_equal(o.acc_rank.cpu().numpy(), rank[acc_index]) and np.array_equal(o.acc_score.cpu().numpy(), score[perm][acc_index])
    d = g.on(torch.device("cuda", torch.cuda.current_device()))
    got_bits, got_ignore = ops.coco_match(o.det_offsets, d["offsets"], o.boxes, d["box"], d["area"], d["crowd"], E.AREA_RNG, E.IOU_THRS,
                                          max_dets[-1])
    assert np.array_equal(got_ignore.cpu().numpy(), gt_ignore)
    diff = np.argwhere(got_bits.cpu().numpy() != bits)
    assert diff.size == 0, f"det (cell order) {diff[0][0]}, (range, threshold) lane {diff[0][1]}"


def test_the_carry_across_chunks(launches):
    """One category, 3 000 dets under the caps (1, 10, 100): three chunks of the accumulation, with equal scores across their
    borders; twice, with equal bits."""
    gt, dets, max_dets, want = _case("carry")
    first, _ = _run(gt, dets, max_dets)
    _assert_same(first.eval, want)
    again, _ = _run(gt, dets, max_dets)
    assert launches == dict(match=2, accumulate=2)
    for key in KEYS:
        assert first.eval[key].tobytes() == again.eval[key].tobytes(), key


def test_a_cell_too_large_for_lds(launches):
    """150 gts in one cell: 5 x 150 doubles and 150 x 64 flags exceed the cell's 8 KiB, so the matrix lives in the workspace."""
    gt, dets, max_dets, want = _case("many_gts")
    ev, _ = _run(gt, dets, max_dets)
    assert launches == dict(match=1, accumulate=1)
    _assert_same(ev.eval, want)


def test_the_host_path_is_selected_by_the_environment(launches, monkeypatch):
    gt, dets, max_dets, want = _case("edge")
    monkeypatch.setenv("LOCOV_FUSED_COCOEVAL", "0")
    ev, res_host = _run(gt, dets, max_dets)
    assert launches == dict(match=0, accumulate=0)
    _assert_same(ev.eval, want)
    monkeypatch.delenv("LOCOV_FUSED_COCOEVAL")
    ev, res_dev = _run(gt, dets, max_dets)
    assert launches == dict(match=1, accumulate=1)
    _assert_same(ev.eval, want)
    assert repr(res_host) == repr(res_dev)                                           # (repr: nan compares unequal to itself)


def test_the_mark_hook_names_the_steps_and_changes_nothing(launches):
    """evaluate_device calls `mark` after each of its steps, in order, and returns the arrays it returns without one."""
    from locov_amd import evaluation as E
    gt, dets = cases.handworked()
    g = E._GroundTruth(gt)
    arrays = (np.array([g.image_rank[d[0]] for d in dets], dtype=np.int64), np.array([d[1] for d in dets], dtype=np.int64),
              np.array([float(d[2]) for d in dets], dtype=np.float64), np.stack([d[3] for d in dets]))
    tensors = [torch.from_numpy(a).cuda() for a in arrays]
    plain = E.evaluate_device(g, *tensors, (1, 10, 100))
    names = []
    marked = E.evaluate_device(g, *tensors, (1, 10, 100), mark=names.append)
    assert names == ["orderings", "match", "npig", "accumulate", "copy_and_means"]
    assert launches == dict(match=2, accumulate=2)
    for key in KEYS:
        assert marked[key].tobytes() == plain[key].tobytes(), key


def test_end_to_end_on_device_instances_equals_the_cpu_evaluator(launches):
    gt, dets, max_dets, _ = _case("random3")
    names = [f"n{i}" for i in range(len(gt["categories"]))]
    kw = dict(class_names=names, seen_names=names[:3], unseen_names=names[3:])
    dev, res_dev = _run(gt, dets, max_dets, "cuda", **kw)
    cpu, res_cpu = _run(gt, dets, max_dets, "cpu", **kw)
    assert launches == dict(match=1, accumulate=1)                                   # (the CPU tensors took the host path)
    _assert_same(dev.eval, cpu.eval)
    assert repr(res_dev) == repr(res_cpu) and "AP50-unseen" in res_dev["bbox"] and "AP-n0" in res_dev["bbox"]
    host_forced, _ = _run(gt, dets, max_dets, "cuda", device="cpu", **kw)            # device tensors, evaluated on the host
    _assert_same(host_forced.eval, cpu.eval)
    assert launches == dict(match=1, accumulate=1)
