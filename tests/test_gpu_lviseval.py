"""The device path of the LVIS box-AP evaluator (locov_lvis_match and the cap in ops.lvis_limit, with the COCO path's ordering and
accumulate kernel) against the host definition in locov_amd/evaluation.py and the loop restatement in tests/lviseval_ref.py, bit
for bit: everything is float64 and integer, so there is no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import lviseval_cases as cases
import lviseval_ref

pytestmark = pytest.mark.gpu

KEYS = ("precision", "recall", "stats")
CASES = {
    "handworked": (cases.handworked, 300),
    "cap_example": (cases.cap_example, 2),
    "edge": (cases.edge_cases, 300),
    "edge_cap3": (cases.edge_cases, 3),
    "straddle": (cases.straddle_case, 5),              # 5 dets x 78 gts in LDS, 5 x 79 in the workspace
    "large": (cases.large_case, 300),                  # a category with more than 1 024 listed dets
}
for _s in range(4):
    CASES[f"random{_s}"] = ((lambda s=_s: cases.random_case(s)), 300)
    CASES[f"random{_s}_cap3"] = ((lambda s=_s: cases.random_case(s)), 3)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(gt, dets, cap, the restatement's arrays): computed once and shared."""
    make, cap = CASES[name]
    gt, dets = make()
    want = lviseval_ref.evaluate(gt, dets, cap)
    for v in want.values():
        v.setflags(write=False)
    return gt, dets, cap, want


def _run(gt, dets, cap, where="cuda", **kw):
    from locov_amd.evaluation import LVISEvaluator
    ev = LVISEvaluator(gt, max_dets_per_image=cap, **kw)
    cases.feed(ev, dets, where)
    res = ev.evaluate()
    return ev, res


@pytest.fixture
def launches(monkeypatch):
    """Counts the two kernels' launches, so that a test knows which path ran."""
    from locov_amd import ops
    n = dict(match=0, coco_match=0, accumulate=0)
    match, coco_match, accumulate = ops.lvis_match, ops.coco_match, ops.coco_accumulate

    def spy_match(*a, **k):
        n["match"] += 1
        return match(*a, **k)

    def spy_coco_match(*a, **k):
        n["coco_match"] += 1
        return coco_match(*a, **k)

    def spy_accumulate(*a, **k):
        n["accumulate"] += 1
        return accumulate(*a, **k)

    monkeypatch.setattr(ops, "lvis_match", spy_match)
    monkeypatch.setattr(ops, "coco_match", spy_coco_match)
    monkeypatch.setattr(ops, "coco_accumulate", spy_accumulate)
    return n


def _assert_same(got, want):
    assert sorted(got) == sorted(KEYS)
    for key in KEYS:
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape, key
        diff = np.argwhere(got[key] != want[key])
        assert diff.size == 0, f"{key}: {len(diff)} entries differ, first at {diff[0].tolist()}: {got[key][tuple(diff[0])]!r} != {want[key][tuple(diff[0])]!r}"


def _arrays(gt, dets):
    from locov_amd import evaluation as E
    g = E._LVISGroundTruth(gt)
    img = np.array([g.image_rank[d[0]] for d in dets], dtype=np.int64)
    cls = np.array([d[1] for d in dets], dtype=np.int64)
    score = np.array([float(d[2]) for d in dets], dtype=np.float64)
    return g, img, cls, score, np.stack([d[3] for d in dets])


@pytest.mark.parametrize("name", [n for n in CASES if n not in ("straddle", "large")])
def test_device_path_equals_the_definition_and_the_restatement(name, launches, monkeypatch):
    from locov_amd import evaluation as E
    monkeypatch.delenv("LOCOV_FUSED_COCOEVAL", raising=False)
    gt, dets, cap, want = _case(name)
    ev, _ = _run(gt, dets, cap)
    assert launches == dict(match=1, coco_match=0, accumulate=1)                     # the device path is the default
    _assert_same(ev.eval, want)
    g, img, cls, score, boxes = _arrays(gt, dets)
    _assert_same(ev.eval, E.evaluate_host_lvis(g, img, cls, score, boxes, cap))


@pytest.mark.parametrize("name", ["edge", "edge_cap3", "random2_cap3", "straddle"])
def test_the_cap_and_the_match_kernel_equal_the_host_steps(name):
    """ops.lvis_limit against limit_host, and locov_lvis_match's own outputs against match_host_lvis on the capped dets in cell
    order: the listed dets' bits, 2 for every det of an unlisted cell, and the gts' ignore flags."""
    from locov_amd import evaluation as E, ops
    gt, dets, cap, _ = _case(name)
    g, img, cls, score, boxes = _arrays(gt, dets)
    up = lambda a: torch.from_numpy(a).cuda()
    K = g.n_categories
    keep = E.limit_host(img, cls, score, K, cap)
    want_cls = np.where(keep, cls, np.where((cls >= 0) & (cls < K), K, cls))          # past the cap: class K; outside the bank: as it was
    got_cls = ops.lvis_limit(up(img), up(cls), up(score), g.n_images, K, cap)
    assert np.array_equal(got_cls.cpu().numpy(), want_cls)
    perm, det_off, rank, acc_index, cat_off = E.order_host(img, want_cls, score, g.n_images, K)
    bits, gt_ignore, listed = E.match_host_lvis(g, det_off, boxes[perm], cap)
    assert listed.any() and (name == "straddle" or not listed[:int(det_off[-1])].all())   # listed and unlisted dets
    o = ops.coco_order(up(img), got_cls, up(score), up(boxes), g.n_images, K)
    assert np.array_equal(o.det_offsets.cpu().numpy(), det_off) and np.array_equal(o.boxes.cpu().numpy(), boxes[perm])
    d = g.on(torch.device("cuda", torch.cuda.current_device()))
    got_bits, got_ignore = ops.lvis_match(o.det_offsets, d["offsets"], d["cell_flags"], o.boxes, d["box"], d["area"], d["ignore"], E.AREA_RNG,
                                          E.IOU_THRS, cap)
    assert np.array_equal(got_ignore.cpu().numpy(), gt_ignore)
    got_bits = got_bits.cpu().numpy()
    diff = np.argwhere(got_bits[listed] != bits[listed])
    assert diff.size == 0, f"listed det {diff[0][0]}, (range, threshold) lane {diff[0][1]}"
    unlisted = ~listed
    unlisted[int(det_off[-1]):] = False                                               # (the trailing cell is never written)
    assert np.all(got_bits[unlisted] == 2)


def test_the_two_cells_on_either_side_of_the_lds_rule(launches):
    """At a cap of 5: 5 dets x 78 gts is the last cell whose IoU matrix and flags fit its 8 KiB of LDS; 5 x 79 lives in the workspace."""
    from locov_amd import evaluation as E
    gt, dets, cap, want = _case("straddle")
    sizes = sorted(sum(1 for a in gt["annotations"] if a["image_id"] == i and a["category_id"] == 1) for i in (1, 2))
    assert cases.fits_lds(cap, sizes[0]) and not cases.fits_lds(cap, sizes[1]) and sizes[1] == sizes[0] + 1
    ev, _ = _run(gt, dets, cap)
    assert launches == dict(match=1, coco_match=0, accumulate=1)
    _assert_same(ev.eval, want)
    g, img, cls, score, boxes = _arrays(gt, dets)
    _assert_same(ev.eval, E.evaluate_host_lvis(g, img, cls, score, boxes, cap))


def test_a_category_past_one_chunk_twice_with_equal_bits(launches):
    """More than 1 024 listed dets of one category at the default cap, unlisted and not-exhaustive-ignored dets on both sides of
    the accumulation's chunk boundary; twice, with equal bits."""
    from locov_amd import evaluation as E
    gt, dets, cap, want = _case("large")
    g, img, cls, score, boxes = _arrays(gt, dets)
    keep = E.limit_host(img, cls, score, g.n_categories, cap)
    assert all(np.count_nonzero(keep & (img == i)) == 300 for i in range(4))          # the cap acted on the four images
    mine = np.nonzero(keep & (cls == 0))[0]
    mine = mine[np.argsort(-score[mine], kind="stable")]
    listed, nel = img[mine] < 4, img[mine] == 1                                       # image 5: unlisted; image 2: not exhaustive
    assert np.count_nonzero(listed) > 1024
    for kind in (~listed, nel):
        assert kind[:1024].any() and kind[1024:].any()
    first, _ = _run(gt, dets, cap)
    _assert_same(first.eval, want)
    _assert_same(first.eval, E.evaluate_host_lvis(g, img, cls, score, boxes, cap))
    again, _ = _run(gt, dets, cap)
    assert launches == dict(match=2, coco_match=0, accumulate=2)
    for key in KEYS:
        assert first.eval[key].tobytes() == again.eval[key].tobytes(), key


def test_the_host_path_is_selected_by_the_environment(launches, monkeypatch):
    gt, dets, cap, want = _case("edge")
    monkeypatch.setenv("LOCOV_FUSED_COCOEVAL", "0")
    ev, res_host = _run(gt, dets, cap)
    assert launches == dict(match=0, coco_match=0, accumulate=0)
    _assert_same(ev.eval, want)
    monkeypatch.delenv("LOCOV_FUSED_COCOEVAL")
    ev, res_dev = _run(gt, dets, cap)
    assert launches == dict(match=1, coco_match=0, accumulate=1)
    _assert_same(ev.eval, want)
    assert repr(res_host) == repr(res_dev)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_one_device_to_host_copy(monkeypatch):
    """evaluate_device_lvis reads the device once: every synchronising call but Tensor.cpu raises, and Tensor.cpu is counted."""
    from locov_amd import evaluation as E
    gt, dets, cap, want = _case("edge_cap3")
    g, img, cls, score, boxes = _arrays(gt, dets)
    dev = torch.device("cuda", torch.cuda.current_device())
    g.on(dev)                                                                         # (the ground truth is uploaded once per device)
    args = [torch.from_numpy(a).to(dev) for a in (img, cls, score, boxes)]
    E.evaluate_device_lvis(g, *args, cap)                                             # (workspace and library are in place)
    torch.cuda.synchronize()
    copies = []
    real_cpu = torch.Tensor.cpu

    def counted_cpu(self, *a, **k):
        copies.append(self.numel() * self.element_size())
        torch.cuda.set_sync_debug_mode("default")
        try:
            return real_cpu(self, *a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("error")

    monkeypatch.setattr(torch.Tensor, "cpu", counted_cpu)
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = E.evaluate_device_lvis(g, *args, cap)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    T, R, K, A = 10, 101, g.n_categories, 4
    assert copies == [(T * R * K * A + T * K * A) * 8]                                # precision and recall, no scores
    _assert_same(got, want)


def test_the_mark_hook_names_the_steps_and_changes_nothing(launches):
    """evaluate_device_lvis calls `mark` after each of its steps, in order, and returns the arrays it returns without one."""
    from locov_amd import evaluation as E
    gt, dets, cap, want = _case("handworked")
    g, *arrays = _arrays(gt, dets)
    tensors = [torch.from_numpy(a).cuda() for a in arrays]
    plain = E.evaluate_device_lvis(g, *tensors, cap)
    names = []
    marked = E.evaluate_device_lvis(g, *tensors, cap, mark=names.append)
    assert names == ["cap", "orderings", "match", "npig", "accumulate", "copy", "means"]
    assert launches == dict(match=2, coco_match=0, accumulate=2)
    for key in KEYS:
        assert marked[key].tobytes() == plain[key].tobytes(), key
    _assert_same(marked, want)


def test_end_to_end_on_device_instances_equals_the_cpu_evaluator(launches):
    gt, dets, cap, _ = _case("random3")
    dev, res_dev = _run(gt, dets, cap, "cuda")
    cpu, res_cpu = _run(gt, dets, cap, "cpu")
    assert launches == dict(match=1, coco_match=0, accumulate=1)                     # (the CPU tensors took the host path)
    _assert_same(dev.eval, cpu.eval)
    assert repr(res_dev) == repr(res_cpu) and list(res_dev["bbox"])[-3:] == ["APr", "APc", "APf"]
    host_forced, _ = _run(gt, dets, cap, "cuda", device="cpu")                       # device tensors, evaluated on the host
    _assert_same(host_forced.eval, cpu.eval)
    assert launches == dict(match=1, coco_match=0, accumulate=1)
