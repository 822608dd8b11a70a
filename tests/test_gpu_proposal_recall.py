"""The device path of the proposal recall (locov_proposal_recall behind ops.proposal_recall, and the evaluators' "box_proposals")
against the host definition in locov_amd/evaluation.py and the literal restatement in tests/proposal_recall_ref.py, bit for bit:
everything is fp32 rounded step by step and integers, so there is no tolerance anywhere.  The cases (tests/proposal_recall_cases.py
names each situation): P < G, P == G, P > G; 101 proposals in one image; an image with gts and no proposal; only crowd gts; an
image never processed; areas of exactly 1024 and 9216; IoUs exactly on 0.5 and fp32(0.55); equal IoUs across gts and across
proposals; equal logits; a column whose cached row another gt takes; 65 gts x 300 proposals; an image at the kernel's row limit;
sizes past the kernel's limits (the host path, with an equal result); LOCOV_FUSED_COCOEVAL=0; four random seeds; image ids out of
order; ProposalNetwork on two toy images."""
import numpy as np
import pytest
import torch

import backbone_ref as br
import proposal_recall_cases as cases
import proposal_recall_ref as ref
from test_proposal_recall_host import CASES, assert_totals, case, definition, run, same_bits

pytestmark = pytest.mark.gpu

HOST_PATH = ("long_2049", "many_gts")                                                # past MAX_LIMIT / past MAX_GT: the definition runs


@pytest.fixture
def launches(monkeypatch):
    """Counts ops.proposal_recall's calls, so that a test knows which path ran."""
    from locov_amd import ops
    n = dict(recall=0)
    real = ops.proposal_recall

    def spy(*a, **k):
        n["recall"] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "proposal_recall", spy)
    return n


def _kernel(gt, props, limits, lvis=False):
    """ops.proposal_recall's own outputs on the case's arrays."""
    from locov_amd import evaluation as E, ops
    g = (E._LVISGroundTruth if lvis else E._GroundTruth)(gt)
    d = g.on(torch.device("cuda", torch.cuda.current_device()), by_image=True)
    img = np.concatenate([np.full(len(p[1]), g.image_rank[p[0]], dtype=np.int64) for p in props])
    up = lambda a: torch.from_numpy(a).cuda()
    totals, overlaps = ops.proposal_recall(up(img), up(np.concatenate([p[1] for p in props]).astype(np.float64)),
                                           up(np.concatenate([p[2] for p in props])), d["image_offsets"], d["image_box"], d["image_area"],
                                           d["image_skip"], g.image_index()["max_per_image"], E.PROPOSAL_AREA_RNG, limits, E.PROPOSAL_THRS)
    assert totals.dtype == torch.int64 and totals.is_cuda and overlaps.is_cuda
    return totals.cpu().numpy().reshape(4, len(limits), -1), overlaps.cpu().numpy()


@pytest.mark.parametrize("lvis", [False, True], ids=["coco", "lvis"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_evaluator_on_device_tensors_equals_the_restatement(name, lvis, launches, monkeypatch):
    monkeypatch.delenv("LOCOV_FUSED_COCOEVAL", raising=False)
    gt, props, limits, want = case(name, lvis)
    ev, res = run(gt, props, limits, lvis, where="cuda")
    assert launches["recall"] == (0 if name in HOST_PATH else 1)                      # the device path is the default, inside the limits
    assert_totals(ev, res, want)


@pytest.mark.parametrize("lvis", [False, True], ids=["coco", "lvis"])
@pytest.mark.parametrize("name", [n for n in CASES if n not in HOST_PATH])
def test_the_kernel_matches_as_the_definition_does(name, lvis):
    """The matching itself: every overlap in match order, zeros behind them and in the segments that take no part."""
    gt, props, limits, want = case(name, lvis)
    totals, overlaps = _kernel(gt, props, limits, lvis)
    same_bits(overlaps, want["gt_overlaps"], "gt_overlaps")
    same_bits(overlaps, definition(gt, props, limits, lvis)["gt_overlaps"], "gt_overlaps (definition)")
    same_bits(np.ascontiguousarray(totals[:, :, :-1]), want["counts"], "counts")
    same_bits(np.ascontiguousarray(totals[:, :, -1]), want["num_pos"], "num_pos")


def test_the_row_limit_is_the_last_size_the_kernel_takes(launches):
    from locov_amd import _lib
    assert CASES["long_2048"][1][-1] == _lib.PROPOSAL_RECALL_MAX_LIMIT and CASES["long_2049"][1][-1] == _lib.PROPOSAL_RECALL_MAX_LIMIT + 1
    assert len(case("long_2048")[1][0][1]) > _lib.PROPOSAL_RECALL_MAX_LIMIT          # more proposals than the limit keeps
    gt, props, _, _ = case("many_gts")
    assert max(sum(1 for a in gt["annotations"] if a["image_id"] == i) for i in (1, 2)) == _lib.PROPOSAL_RECALL_MAX_GT + 1
    for name, calls in (("long_2048", 1), ("long_2049", 0)):
        launches["recall"] = 0
        gt, props, limits, want = case(name)
        ev, res = run(gt, props, limits, where="cuda")
        assert launches["recall"] == calls
        assert_totals(ev, res, want)
    with pytest.raises(_lib.LocovError, match="per image"):                           # the entry point itself refuses, it never truncates
        _kernel(*case("long_2049")[:3])


def test_twice_with_equal_bits_and_on_ids_out_of_order():
    gt, props, limits, want = case("wide")
    first, again = _kernel(gt, props, limits), _kernel(gt, props, limits)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    gt, props, limits, want = case("random1")
    ids = [p[0] for p in props]
    assert ids != sorted(ids) and [im["id"] for im in gt["images"]] != sorted(ids)
    same_bits(_kernel(gt, props[::-1], limits)[1], want["gt_overlaps"], "gt_overlaps")           # the feed order of the images is free


def test_the_host_path_is_selected_by_the_environment(launches, monkeypatch):
    gt, props, limits, want = case("edge")
    monkeypatch.setenv("LOCOV_FUSED_COCOEVAL", "0")
    ev, res_host = run(gt, props, limits, where="cuda")
    assert launches["recall"] == 0
    assert_totals(ev, res_host, want)
    monkeypatch.delenv("LOCOV_FUSED_COCOEVAL")
    ev, res_dev = run(gt, props, limits, where="cuda")
    assert launches["recall"] == 1
    assert_totals(ev, res_dev, want)
    assert repr(res_host) == repr(res_dev)
    forced, res_forced = run(gt, props, limits, where="cuda", device="cpu")           # device tensors, evaluated on the host
    assert launches["recall"] == 1 and repr(res_forced) == repr(res_dev)
    cpu, res_cpu = run(gt, props, limits, where="cpu")
    assert launches["recall"] == 1 and repr(res_cpu) == repr(res_dev)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_one_device_to_host_copy_and_the_mark_hook(monkeypatch):
    """proposal_recall_device reads the device once: every synchronising call but Tensor.cpu raises, and Tensor.cpu is counted."""
    from locov_amd import evaluation as E
    gt, props, limits, want = case("random2")
    g = E._GroundTruth(gt)
    dev = torch.device("cuda", torch.cuda.current_device())
    g.on(dev, by_image=True)                                                          # (the ground truth is uploaded once per device)
    img = np.concatenate([np.full(len(p[1]), g.image_rank[p[0]], dtype=np.int64) for p in props])
    args = [torch.from_numpy(a).to(dev) for a in (img, np.concatenate([p[1] for p in props]).astype(np.float64), np.concatenate([p[2] for p in props]))]
    names = []
    E.proposal_recall_device(g, *args, limits, mark=names.append)                     # (the library is in place)
    assert names == ["orderings", "launch", "sum", "copy"]
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
        counts, num_pos = E.proposal_recall_device(g, *args, limits)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert copies == [4 * 2 * 11 * 8]                                                 # A x L x (T + 1) int64 totals
    same_bits(np.ascontiguousarray(counts), want["counts"], "counts")
    same_bits(np.ascontiguousarray(num_pos), want["num_pos"], "num_pos")


# ------------------------------------------------------------------------------------------------------ ProposalNetwork

@pytest.fixture(scope="module")
def model():
    import locov_amd as pkg
    torch.manual_seed(11)
    cfg = pkg.config.get_cfg()
    cfg.MODEL.BACKBONE["TRAIN_ON_DEVICE"] = True
    cfg.MODEL.META_ARCHITECTURE = "ProposalNetwork"
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.PIXEL_STD = [57.375, 57.12, 58.395]
    cfg.MODEL.RPN.PRE_NMS_TOPK_TEST, cfg.MODEL.RPN.POST_NMS_TOPK_TEST, cfg.MODEL.RPN.NMS_THRESH = 200, 50, 0.9
    m = pkg.build_model(cfg)
    assert type(m) is pkg.ProposalNetwork and m.device.type == "cuda"
    br.randomize_frozen_bn(m.backbone, 3)
    return m.eval()


def test_proposal_network_inference_equals_the_torch_postprocess_and_feeds_the_evaluator(model, launches):
    import locov_amd as pkg
    g = torch.Generator().manual_seed(5)
    inputs = []
    for n, ((h, w), (oh, ow)) in enumerate((((64, 96), (160, 321)), ((56, 80), (43, 53)))):
        inputs.append({"image": torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g), "height": oh, "width": ow, "image_id": 7 - n})
    with torch.no_grad():
        images = model.preprocess_image(inputs)
        raw, _ = model.proposal_generator(images, model.backbone(images.tensor), None)
        want = [pkg.detector_postprocess(r, d["height"], d["width"]) for r, d in zip(raw, inputs)]
        got = model(inputs)
    assert len(got) == 2 and all(set(o) == {"proposals"} for o in got)
    for o, w, d in zip(got, want, inputs):
        p = o["proposals"]
        assert len(w) >= 1 and len(p) == len(w) and p.image_size == (d["height"], d["width"])
        assert set(p.get_fields()) == {"proposal_boxes", "objectness_logits"}
        assert torch.equal(p.proposal_boxes.tensor.view(torch.int32), w.proposal_boxes.tensor.view(torch.int32))
        assert torch.equal(p.objectness_logits.view(torch.int32), w.objectness_logits.view(torch.int32))
        assert bool((p.objectness_logits[:-1] >= p.objectness_logits[1:]).all())      # the descending order is kept
    # a ground truth made of a few of the proposals themselves, so that the recall is neither 0 nor undefined
    anns = []
    for d, w in zip(inputs, want):
        for b in w.proposal_boxes.tensor[:3].cpu().tolist():
            anns.append(dict(id=len(anns) + 1, image_id=d["image_id"], category_id=1, bbox=[b[0], b[1], b[2] - b[0], b[3] - b[1]],
                             area=(b[2] - b[0]) * (b[3] - b[1]), iscrowd=0))
    gt = dict(images=[dict(id=d["image_id"], height=d["height"], width=d["width"]) for d in inputs], categories=[dict(id=1, name="a")],
              annotations=anns)
    ev = pkg.COCOEvaluator(gt)
    res = pkg.inference_on_dataset(model, [inputs], ev)
    assert launches["recall"] == 1 and list(res) == ["bbox", "box_proposals"] and not model.training
    props = [(d["image_id"], w.objectness_logits.cpu().numpy(), w.proposal_boxes.tensor.cpu().numpy()) for d, w in zip(inputs, want)]
    expected = ref.evaluate(gt, props)
    assert_totals(ev, res, expected)
    assert expected["num_pos"][0, 0] == len(anns) >= 2 and expected["counts"][0, 0, 0] >= 2
