"""The proposal recall ("box_proposals": AR, ARs, ARm, ARl at 100 and 1000 proposals per image) without a GPU: the host definition
in locov_amd/evaluation.py against the literal restatement of the public function in tests/proposal_recall_ref.py, bit for bit
(fp32 rounded step by step and integers: there is no tolerance anywhere); a hand-worked case; what evaluate() returns and when;
ProposalNetwork on recording stand-ins; the C entry point's argument errors."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import cocoeval_cases
import proposal_recall_cases as cases
import proposal_recall_ref as ref

P = ctypes.c_void_p

CASES = {
    "handworked": (cases.handworked, (100, 1000)),
    "edge": (cases.edge_cases, (100, 1000)),
    "limit101": (cases.limit_case, (100, 1000)),
    "wide": (cases.wide_case, (100, 1000)),
    "long_2048": (cases.long_case, (100, 2048)),
    "long_2049": (cases.long_case, (100, 2049)),
    "many_gts": (cases.many_gts_case, (100, 1000)),
}
for _s in range(4):
    CASES[f"random{_s}"] = ((lambda s=_s: cases.random_case(s)), (100, 1000))


@functools.lru_cache(maxsize=None)
def case(name, lvis=False):
    """(gt, props, limits, the restatement's arrays): computed once and shared."""
    make, limits = CASES[name]
    gt, props = make()
    want = ref.evaluate(gt, props, lvis=lvis, limits=limits)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return gt, props, limits, want


def run(gt, props, limits, lvis=False, where="cpu", **kw):
    from locov_amd.evaluation import COCOEvaluator, LVISEvaluator
    ev = (LVISEvaluator if lvis else COCOEvaluator)(gt, **kw)
    ev.proposal_limits = limits
    cases.feed(ev, props, where)
    return ev, ev.evaluate()


def definition(gt, props, limits, lvis=False):
    from locov_amd import evaluation as E
    g = (E._LVISGroundTruth if lvis else E._GroundTruth)(gt)
    img = np.concatenate([np.full(len(p[1]), g.image_rank[p[0]], dtype=np.int64) for p in props])
    return E.proposal_recall_host(g.image_index(), img, np.concatenate([p[1] for p in props]), np.concatenate([p[2] for p in props]), limits)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    diff = np.argwhere(got.view(np.uint8 if got.dtype.itemsize == 1 else f"u{got.dtype.itemsize}") !=
                       want.view(np.uint8 if want.dtype.itemsize == 1 else f"u{want.dtype.itemsize}"))
    assert diff.size == 0, f"{what}: {len(diff)} entries differ, first at {diff[0].tolist()}: {got[tuple(diff[0])]!r} != {want[tuple(diff[0])]!r}"


def assert_totals(ev, res, want):
    """The evaluator's totals and results against the restatement's."""
    for key in ("counts", "num_pos", "recalls", "ar"):
        same_bits(ev.proposal_eval[key], want[key], key)
    assert list(res["box_proposals"]) == list(want["results"]) and repr(dict(res["box_proposals"])) == repr(want["results"])


@pytest.mark.parametrize("lvis", [False, True], ids=["coco", "lvis"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_definition_equals_the_restatement(name, lvis):
    gt, props, limits, want = case(name, lvis)
    got = definition(gt, props, limits, lvis)
    same_bits(got["gt_overlaps"], want["gt_overlaps"], "gt_overlaps")
    same_bits(got["counts"], want["counts"], "counts")
    same_bits(got["num_pos"], want["num_pos"], "num_pos")
    assert want["num_pos"][0].min() > 0                                              # (a case that counts nothing would show nothing)
    ev, res = run(gt, props, limits, lvis)
    assert_totals(ev, res, want)


def test_the_handworked_case():
    gt, props, limits, _ = case("handworked")
    ev, res = run(gt, props, limits)
    got = definition(gt, props, limits)
    row = got["gt_overlaps"][0]
    assert row.tolist() == [np.float32(0.825), np.float32(0.5), np.float32(0.72)]     # image 1 in match order (largest first), image 2
    assert np.array_equal(got["gt_overlaps"][1], row)                                 # the same at 1000
    assert got["gt_overlaps"][2].tolist() == [0.5, 0.0, 0.0]                          # small: only A, in its image's first slot
    assert ev.proposal_eval["num_pos"].tolist() == [[3, 3], [1, 1], [1, 1], [1, 1]]
    assert ev.proposal_eval["counts"][:, 0].tolist() == [[3, 2, 2, 2, 2, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                                                         [1, 1, 1, 1, 1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
    mean = lambda counts, n: float((torch.tensor(counts).float() / float(n)).mean().item() * 100)
    expected = {"AR": mean([3, 2, 2, 2, 2, 1, 1, 0, 0, 0], 3), "ARs": mean([1, 0, 0, 0, 0, 0, 0, 0, 0, 0], 1),
                "ARm": mean([1, 1, 1, 1, 1, 1, 1, 0, 0, 0], 1), "ARl": mean([1, 1, 1, 1, 1, 0, 0, 0, 0, 0], 1)}
    assert abs(expected["AR"] - 1300 / 30) < 1e-4 and abs(expected["ARs"] - 10) < 1e-4 and abs(expected["ARm"] - 70) < 1e-4
    for limit in (100, 1000):
        for name, v in expected.items():
            assert res["box_proposals"][f"{name}@{limit}"] == v, (name, limit)


def test_the_result_keys_and_their_order():
    gt, props, limits, _ = case("edge")
    _, res = run(gt, props, limits)
    assert list(res) == ["bbox", "box_proposals"]
    assert list(res["box_proposals"]) == ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]
    assert all(type(v) is float for v in res["box_proposals"].values())
    _, res = run(gt, props, limits, lvis=True)
    assert list(res) == ["bbox", "box_proposals"] and len(res["box_proposals"]) == 8


def test_the_edge_cases_are_what_their_comments_say():
    from locov_amd import evaluation as E
    gt, props, limits, want = case("edge")
    _, _, _, want_lvis = case("edge", True)
    g = E._GroundTruth(gt)
    index = g.image_index()
    seg = lambda image_id, row=1: want["gt_overlaps"][row, index["offsets"][g.image_rank[image_id]]:index["offsets"][g.image_rank[image_id] + 1]]
    thrs = E.PROPOSAL_THRS
    assert thrs.dtype == np.float32 and thrs[0] == np.float32(0.5) and thrs[1] == np.float32(0.55) and len(thrs) == 10
    assert seg(21).tolist() == [thrs[1], thrs[0]]                                     # IoUs exactly on two thresholds
    assert seg(5).tolist() == [0.5, 0.0]                                              # the lower gt took the shared proposal
    assert seg(6).tolist() == [np.float32(0.6), np.float32(40) / np.float32(120)]     # the proposal fed first was taken
    assert seg(8).tolist() == [np.float32(400) / np.float32(420), np.float32(0.7)]    # the second gt looked again
    assert not seg(2).any() and not seg(12).any() and not seg(30).any()               # no proposal; never processed; crowd only
    off = np.asarray(index["offsets"])
    lvis_seg = want_lvis["gt_overlaps"][1, off[g.image_rank[30]]:off[g.image_rank[30] + 1]]
    assert lvis_seg.tolist() == [1.0, np.float32(0.9)]                                # LVIS counts them
    n_coco = sum(1 for a in gt["annotations"] if not a["iscrowd"] and a["image_id"] not in (2, 12))
    assert want["num_pos"][0].tolist() == [n_coco, n_coco] and want_lvis["num_pos"][0].tolist() == [n_coco + 3, n_coco + 3]
    # image 7: 1024 is small and medium, 9216 medium and large; the 50 x 50 box has its own area field (900: small)
    one = ref.evaluate(gt, [p for p in props if p[0] == 7])
    assert one["num_pos"][:, 0].tolist() == [3, 2, 2, 1]
    # P < G, P == G and P > G
    sizes = {p[0]: len(p[1]) for p in props}
    counted = {i: sum(1 for a in gt["annotations"] if a["image_id"] == i and not a["iscrowd"]) for i in (9, 4, 17)}
    assert sizes[9] < counted[9] and sizes[4] == counted[4] and sizes[17] > counted[17]
    assert [im["id"] for im in gt["images"]] != sorted(im["id"] for im in gt["images"])           # image ids out of order


def test_the_limit_drops_the_proposal_of_rank_101():
    gt, props, limits, want = case("limit101")
    assert len(props[0][1]) == 101 and props[0][1][-1] == props[0][1][-2]             # equal logits: the stable order decides
    assert want["counts"][0, 0, 0] == 1 and want["counts"][0, 1, 0] == 2
    ev, res = run(gt, props, limits)
    assert res["box_proposals"]["AR@100"] < res["box_proposals"]["AR@1000"]
    gt, props, limits, want = case("long_2048")
    assert want["gt_overlaps"][1, :3].tolist() == [np.float32(0.8), np.float32(0.75), 0.0]        # rank 2047 is kept, rank 2048 dropped
    assert case("long_2049")[3]["gt_overlaps"][1, :3].tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.75)]


def _with_dets(ev, dets, props, where="cpu"):
    """The dets (tests/cocoeval_cases.py's) and the proposals of an image in ONE output each, as a model that returns both would."""
    from locov_amd.structures import Boxes, Instances
    by_image = {}
    for d in dets:
        by_image.setdefault(d[0], []).append(d)
    prop_of = {p[0]: p for p in props}
    for image_id in sorted(set(by_image) | set(prop_of), reverse=True):
        out = {}
        if image_id in by_image:
            ds = by_image[image_id]
            out["instances"] = Instances((480, 640), pred_boxes=Boxes(torch.from_numpy(np.stack([d[3] for d in ds])).to(where)),
                                         scores=torch.tensor([float(d[2]) for d in ds], dtype=torch.float32, device=where),
                                         pred_classes=torch.tensor([d[1] for d in ds], dtype=torch.int64, device=where))
        if image_id in prop_of:
            _, logits, boxes = prop_of[image_id]
            out["proposals"] = Instances((480, 640), proposal_boxes=Boxes(torch.from_numpy(boxes).to(where)),
                                         objectness_logits=torch.from_numpy(logits).to(where))
        ev.process([dict(image_id=image_id)], [out])


def dets_and_proposals(seed=1):
    gt, dets = cocoeval_cases.random_case(seed)
    rng = np.random.default_rng(seed)
    props = []
    for im in gt["images"][:-1]:
        n = int(rng.integers(1, 20))
        xy = rng.integers(0, 500, (n, 2)).astype(np.float32) / 2
        wh = rng.integers(4, 300, (n, 2)).astype(np.float32) / 2
        props.append((im["id"], (rng.integers(-64, 64, n) / 64).astype(np.float32), np.concatenate([xy, xy + wh], axis=1)))
    return gt, dets, props


def test_bbox_is_unchanged_when_proposals_are_also_fed():
    from locov_amd.evaluation import COCOEvaluator
    gt, dets, props = dets_and_proposals()
    alone = COCOEvaluator(gt)
    _with_dets(alone, dets, [])
    res_alone = alone.evaluate()
    assert list(res_alone) == ["bbox"] and alone.proposal_eval is None                # no proposals fed: no "box_proposals"
    both = COCOEvaluator(gt)
    _with_dets(both, dets, props)
    res_both = both.evaluate()
    assert list(res_both) == ["bbox", "box_proposals"] and repr(res_both["bbox"]) == repr(res_alone["bbox"])
    for key in ("precision", "recall", "scores", "stats"):
        assert both.eval[key].tobytes() == alone.eval[key].tobytes(), key
    want = ref.evaluate(gt, props)
    assert_totals(both, res_both, want)
    # proposals only: "bbox" is the all-NaN result of an evaluator that saw nothing, "box_proposals" the same as above
    only = COCOEvaluator(gt)
    _with_dets(only, [], props)
    res_only = only.evaluate()
    assert only.eval is None and repr(res_only["bbox"]) == repr(COCOEvaluator(gt).evaluate()["bbox"])
    assert repr(res_only["box_proposals"]) == repr(res_both["box_proposals"])
    only.reset()
    assert only.proposal_eval is None and list(only.evaluate()) == ["bbox"]           # reset() clears the proposals too


def test_an_evaluator_that_saw_only_empty_proposals_reports_nan():
    from locov_amd.evaluation import COCOEvaluator
    gt, props, limits, _ = case("handworked")
    ev = COCOEvaluator(gt)
    cases.feed(ev, [(1, np.zeros(0, dtype=np.float32), np.zeros((0, 4), dtype=np.float32))])
    res = ev.evaluate()
    assert len(res["box_proposals"]) == 8 and all(np.isnan(v) for v in res["box_proposals"].values())
    assert not ev.proposal_eval["num_pos"].any()
    with pytest.raises(KeyError, match="not in the ground truth"):
        cases.feed(ev, [(77, props[0][1], props[0][2])])
    ev.proposal_limits = (1000, 100)
    with pytest.raises(ValueError, match="ascending"):
        ev.evaluate()


def test_the_by_image_index_is_built_on_demand():
    from locov_amd import evaluation as E
    gt, _, _, _ = case("edge")
    g = E._GroundTruth(gt)
    assert g._image_index is None
    index = g.image_index()
    assert index is g.image_index() and index["box"].dtype == np.float32 and index["area"].dtype == np.float32
    assert index["offsets"].dtype == np.int32 and index["offsets"][-1] == len(gt["annotations"]) and index["max_per_image"] == 4
    assert index["skip"] is index["crowd"] and E._LVISGroundTruth(gt).image_index()["skip"] is None
    first = gt["annotations"][0]
    rank = g.image_rank[first["image_id"]]
    x, y, w, h = first["bbox"]
    assert index["box"][index["offsets"][rank]].tolist() == [x, y, x + w, y + h]


# ------------------------------------------------------------------------------------------------------ ProposalNetwork

class _Backbone(nn.Module):
    size_divisibility = 16
    padding_constraints = {}

    def __init__(self, log):
        super().__init__()
        self.log = log
        self.w = nn.Parameter(torch.ones(1))

    def forward(self, x):
        self.log.append(("backbone", x))
        return {"res4": x[:, :1, ::16, ::16] * self.w}


class _Rpn(nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log = log
        self.b = nn.Parameter(torch.zeros(1))

    @staticmethod
    def raw(image_sizes):
        from locov_amd.structures import Boxes, Instances
        out = []
        for h, w in image_sizes:
            b = torch.tensor([[1.0, 2.0, w - 1.0, h - 2.0], [w + 5.0, 0.0, w + 9.0, 4.0], [3.0, 3.0, 10.0, 12.0], [0.5, 0.5, 7.25, 9.0]])
            out.append(Instances((h, w), proposal_boxes=Boxes(b), objectness_logits=torch.tensor([3.0, 2.0, 1.0, -1.0])))
        return out                                                                     # (the second box clips away)

    def forward(self, images, features, gt_instances=None):
        self.log.append(("rpn", images, features, gt_instances))
        losses = {"loss_rpn_cls": features["res4"].sum() * 0 + 3.0, "loss_rpn_loc": self.b.sum() + 4.0} if gt_instances is not None else {}
        return self.raw(images.image_sizes), losses


def _inputs(with_gt=False):
    from locov_amd.structures import Boxes, Instances
    g = torch.Generator().manual_seed(0)
    out = []
    for (h, w), (oh, ow) in (((40, 50), (80, 100)), ((33, 64), (66, 32))):
        d = {"image": torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g), "height": oh, "width": ow, "image_id": len(out) + 1}
        if with_gt:
            d["instances"] = Instances((h, w), gt_boxes=Boxes(torch.tensor([[2.0, 2.0, 20.0, 20.0]])), gt_classes=torch.tensor([1]))
        out.append(d)
    return out


def test_proposal_network_is_registered_and_runs_on_the_cpu():
    import locov_amd as pkg
    from locov_amd.meta_arch import META_ARCH_REGISTRY, ProposalNetwork, detector_postprocess
    from locov_amd.structures import Boxes, Instances
    assert "ProposalNetwork" in META_ARCH_REGISTRY and META_ARCH_REGISTRY.get("ProposalNetwork") is ProposalNetwork is pkg.ProposalNetwork
    log = []
    model = ProposalNetwork(backbone=_Backbone(log), proposal_generator=_Rpn(log), pixel_mean=[10.0, 20.0, 30.0], pixel_std=[2.0, 4.0, 8.0])
    assert sorted(model.state_dict()) == ["backbone.w", "proposal_generator.b"] and model.device == torch.device("cpu")
    inputs = _inputs()
    out = model.eval()(inputs)
    assert [e[0] for e in log] == ["backbone", "rpn"] and log[1][3] is None
    assert isinstance(out, list) and len(out) == 2 and all(set(o) == {"proposals"} for o in out)
    for o, r, d in zip(out, _Rpn.raw([(40, 50), (33, 64)]), inputs):
        want, got = detector_postprocess(r, d["height"], d["width"]), o["proposals"]
        assert type(got) is Instances and type(got.proposal_boxes) is Boxes and got.image_size == (d["height"], d["width"])
        assert len(got) == len(want) == 3 and set(got.get_fields()) == {"proposal_boxes", "objectness_logits"}
        assert torch.equal(got.proposal_boxes.tensor.view(torch.int32), want.proposal_boxes.tensor.view(torch.int32))
        assert got.objectness_logits.tolist() == [3.0, 1.0, -1.0]                     # the descending order is kept
    assert out[0]["proposals"].proposal_boxes.tensor[0].tolist() == [2.0, 4.0, 98.0, 76.0]
    # training: the proposal losses, and the gts reach the generator
    log.clear()
    losses = model.train()(_inputs(with_gt=True))
    assert list(losses) == ["loss_rpn_cls", "loss_rpn_loc"] and [float(v.detach()) for v in losses.values()] == [3.0, 4.0]
    assert [len(t) for t in log[1][3]] == [1, 1]
    sum(losses.values()).backward()
    assert model.backbone.w.grad is not None
    # its outputs feed the evaluator through inference_on_dataset
    gt = dict(images=[dict(id=1, height=80, width=100), dict(id=2, height=66, width=32)], categories=[dict(id=1, name="a")],
              annotations=[dict(id=1, image_id=1, category_id=1, bbox=[2.0, 4.0, 96.0, 72.0], area=96.0 * 72.0, iscrowd=0),
                           dict(id=2, image_id=2, category_id=1, bbox=[20.0, 40.0, 4.0, 10.0], area=40.0, iscrowd=0)])
    ev = pkg.COCOEvaluator(gt)
    res = pkg.inference_on_dataset(model, [inputs], ev)
    assert model.training and list(res) == ["bbox", "box_proposals"]
    assert ev.proposal_eval["num_pos"][0].tolist() == [2, 2] and ev.proposal_eval["counts"][0, 0].tolist() == [1] * 10


def test_build_model_builds_a_proposal_network():
    import locov_amd as pkg
    cfg = pkg.config.get_cfg()
    cfg.MODEL.META_ARCHITECTURE = "ProposalNetwork"
    cfg.MODEL.DEVICE = "cpu"
    model = pkg.build_model(cfg)
    assert type(model) is pkg.ProposalNetwork and not hasattr(model, "roi_heads")
    keys = list(model.state_dict())
    assert keys and all(k.startswith(("backbone.", "proposal_generator.")) for k in keys)
    assert any(k.startswith("backbone.") for k in keys) and any(k.startswith("proposal_generator.") for k in keys)


# ------------------------------------------------------------------------------------------------------ the C entry point

@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_constants_agree_with_the_header():
    from locov_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "locov_hip.h")).read()
    defs = dict(re.findall(r"#define LOCOV_(PROPOSAL_RECALL_[A-Z_]+) (\d+)", src))
    assert len(defs) == 3 and all(getattr(_lib, k) == int(v) for k, v in defs.items()), defs
    assert _lib.PROPOSAL_RECALL_MAX_LIMIT % 64 == 0 and _lib.PROPOSAL_RECALL_MAX_GT % 256 == 0 and _lib.ABI_VERSION == 8
    assert "locov_proposal_recall" in _lib.SIGNATURES


def _call(lib, prop_off=P(256), gt_off=P(512), n_images=3, n_prop=50, n_gt=7, max_gt=4, prop_boxes=P(1024), gt_boxes=P(2048), gt_area=P(4096),
          gt_skip=P(8192), areas=(0, 1e10, 0, 1024), n_areas=2, limits=(100, 1000), n_limits=2, thrs=(0.5, 0.75), n_thrs=2,
          overlaps=P(1 << 14), counts=P(1 << 15)):
    ar = (ctypes.c_float * len(areas))(*areas) if areas is not None else None
    lim = (ctypes.c_int * len(limits))(*limits) if limits is not None else None
    th = (ctypes.c_float * len(thrs))(*thrs) if thrs is not None else None
    return lib.locov_proposal_recall(prop_off, gt_off, n_images, n_prop, n_gt, max_gt, prop_boxes, gt_boxes, gt_area, gt_skip, ar, n_areas,
                                     lim, n_limits, th, n_thrs, overlaps, counts, None)


def test_proposal_recall_validates_its_arguments(lib):
    from locov_amd import _lib
    err = lib.locov_last_error
    assert _call(lib, n_images=0) == 0                                                                  # no images: a no-op
    assert _call(lib, n_prop=0, n_gt=0, prop_off=None, gt_off=None, counts=None) == 0                   # no proposal and no gt: a no-op
    for kw in (dict(n_images=-1), dict(n_prop=-1), dict(n_gt=-1), dict(max_gt=-1)):
        assert _call(lib, **kw) == -1 and b"negative" in err()
    assert _call(lib, n_areas=0) == -1 and b"area ranges" in err()
    assert _call(lib, n_areas=_lib.COCO_MAX_AREAS + 1) == -1 and b"area ranges" in err()
    assert _call(lib, n_limits=0) == -1 and b"proposal limits" in err()
    assert _call(lib, n_limits=_lib.PROPOSAL_RECALL_MAX_LIMITS + 1) == -1 and b"proposal limits" in err()
    assert _call(lib, n_thrs=0) == -1 and b"IoU thresholds" in err()
    assert _call(lib, n_thrs=_lib.COCO_MAX_THRESHOLDS + 1) == -1 and b"IoU thresholds" in err()
    for name in ("areas", "limits", "thrs"):
        assert _call(lib, **{name: None}) == -1 and b"null area range, limit or threshold" in err()
    assert _call(lib, areas=(0, 1e10, 1024, 0)) == -1 and b"not ascending" in err()
    assert _call(lib, limits=(1000, 100)) == -1 and b"positive and ascending" in err()
    assert _call(lib, limits=(100, 100)) == -1 and b"positive and ascending" in err()
    assert _call(lib, limits=(0, 100)) == -1 and b"positive and ascending" in err()
    assert _call(lib, limits=(100, _lib.PROPOSAL_RECALL_MAX_LIMIT + 1)) == -3 and b"per image" in err()  # LOCOV_ERR_UNSUPPORTED: never a truncation
    assert _call(lib, max_gt=_lib.PROPOSAL_RECALL_MAX_GT + 1) == -3 and b"per image" in err()
    assert _call(lib, n_images=_lib.COCO_MAX_BLOCKS // 4 + 1) == -3
    for name in ("prop_off", "gt_off", "counts"):
        assert _call(lib, **{name: None}) == -1 and b"null offsets or counts" in err()
    assert _call(lib, prop_boxes=None) == -1 and b"null proposal pointer" in err()
    for name in ("gt_boxes", "gt_area", "overlaps"):
        assert _call(lib, **{name: None}) == -1 and b"null gt pointer" in err()
    assert _call(lib, prop_boxes=P(1032)) == -1 and b"misaligned" in err()
    assert _call(lib, gt_boxes=P(2052)) == -1 and b"misaligned" in err()
    assert _call(lib, prop_off=P(258)) == -1 and b"misaligned" in err()
    with pytest.raises(_lib.LocovError, match="null offsets"):
        _lib.check(_call(lib, prop_off=None), "locov_proposal_recall")


def test_the_wrapper_refuses_cpu_tensors():
    from locov_amd import ops
    from locov_amd._lib import LocovError
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(LocovError, match="only run on a ROCm GPU"):
        ops.proposal_recall(z, torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4), torch.zeros(3, dtype=torch.int32), torch.zeros(1, 4),
                            torch.zeros(1), None, 1, [[0, 1e10]], (100, 1000), [0.5])
