"""The proposal side of the dataset mapper on the host (locov_amd/data.py): transform_proposals and change_proposals_as_gt against the
independent restatement of tests/proposal_ref.py on the whole case table, ProposalStore's packing, CocoImageDatasetMapper's dicts,
get_mapper and the config keys."""
import copy

import numpy as np
import pytest
import torch

import proposal_cases as pc
import proposal_ref
from locov_amd import data
from locov_amd.config import get_cfg
from locov_amd.structures import Boxes, Instances


@pytest.mark.parametrize("case", pc.CASES + (pc.CHUNKED,), ids=lambda c: c.name)
def test_the_definition_equals_the_restatement(case):
    want_all = pc.expected(data, case)
    for i, (im, got) in enumerate(zip(case.images, want_all)):
        rows = pc.rows(case, i)
        assert rows.dtype == np.dtype(case.dtype) and rows.shape == (im.n, 5)
        props, src = proposal_ref.transform_proposals(rows, im.hw, im.new_hw, im.flip, case.topk)
        ref = proposal_ref.change_proposals_as_gt({"proposals": props, "instances": None, "image_id": 3})
        assert ref["gt_obj"] is None and "proposals" not in ref and ref["image_id"] == 3
        gt = ref["instances"]
        assert list(gt.get_fields()) == ["objectness_logits", "gt_classes", "gt_boxes"]
        # torch.equal: the sign of a zero is not part of the contract (min / max of -0.0 and 0.0 may return either)
        assert torch.equal(got["prop_boxes"], props.proposal_boxes.tensor) and torch.equal(got["prop_logits"], props.objectness_logits), i
        assert torch.equal(got["prop_src"], src) and len(src) <= case.topk, i
        assert torch.equal(got["gt_boxes"], gt.gt_boxes.tensor) and torch.equal(got["gt_logits"], gt.objectness_logits), i
        assert torch.equal(got["gt_classes"], gt.gt_classes) and bool((got["gt_classes"] == 1).all()), i
        assert got["image_size"] == gt.image_size == pc.size_of(im)
        for k, dt in (("prop_boxes", torch.float32), ("prop_logits", torch.float32), ("gt_boxes", torch.float32), ("gt_logits", torch.float32),
                      ("gt_classes", torch.int64)):
            assert got[k].dtype == dt, k
        assert not torch.isnan(got["prop_boxes"]).any()              # a NaN end empties its row
        if im.kind == "all_kept":
            assert len(got["prop_src"]) == min(im.n, case.topk)
        if im.kind == "all_dropped":
            assert len(got["prop_src"]) == 0


def test_the_edge_rows_one_by_one():
    case = pc.Case("edges", "float64", 100, (pc.Image(pc.SPECIAL, (480, 640), (800, 1067), 0),), scattered=False)
    got = pc.expected(data, case)[0]
    assert got["prop_src"].tolist() == [2, 3, 4, 5, 8, 9, 10, 11]    # the empty, outside and NaN rows are gone; x1 > x2 is ordered
    assert got["gt_src"].tolist() == [2, 3, 4, 9, 11]                # below 0.7: row 5; at fp32(0.7): rows 8 and 10 (the double 0.7)
    boxes = dict(zip(got["prop_src"].tolist(), got["prop_boxes"].tolist()))
    assert boxes[11] == [0.0, 0.0, 1067.0, 800.0] and boxes[4][2] == 1067.0 and boxes[5][0] == 0.0 and boxes[5][3] == 800.0
    fx = 1067 * 1.0 / 640
    assert boxes[2][0] == float(np.float32(0.2 * 640 * fx)) and boxes[2][2] == float(np.float32(0.6 * 640 * fx))
    same = pc.Case("edges32", "float32", 100, case.images, scattered=False)
    assert pc.expected(data, same)[0]["gt_src"].tolist() == [2, 3, 4, 9, 11]
    # the fp32 rows take the factor rounded to fp32 FIRST (numpy's rule for array * Python float), not the double product rounded
    r = pc.rows(same, 0)
    assert pc.expected(data, same)[0]["prop_boxes"][0, 2].item() == float(r[2, 0] * np.float32(fx))
    flipped = pc.Case("edges_flipped", "float32", 100, (pc.Image(pc.SPECIAL, (480, 640), (800, 1067), 1),), scattered=False)
    x = pc.expected(data, flipped)[0]["prop_boxes"][0]
    assert x[0].item() == float(np.float32(1067) - r[2, 0] * np.float32(fx)) and x[2].item() == float(np.float32(1067) - r[2, 2] * np.float32(fx))


def test_transform_proposals_arguments():
    d = {"proposal_boxes": np.zeros((2, 4), np.float32), "proposal_bbox_mode": data.XYWH_ABS, "proposal_objectness_logits": np.zeros(2, np.float32)}
    with pytest.raises(NotImplementedError, match="proposal_bbox_mode"):
        data.transform_proposals(d, (4, 4), data.TransformList([]), 10)
    untouched = {"image_id": 1}
    data.transform_proposals(untouched, (4, 4), data.TransformList([]), 10)
    assert untouched == {"image_id": 1}
    boxes = np.array([[0, 0, 3, 3], [0, 0, 0.5, 0.5], [1, 1, 9, 9]], np.float32)
    d = {"proposal_boxes": boxes, "proposal_bbox_mode": data.XYXY_ABS, "proposal_objectness_logits": np.array([1, 2, 3], np.float64)}
    data.transform_proposals(d, (4, 4), data.TransformList([]), 10, min_box_size=1)
    assert set(d) == {"proposals"} and d["proposals"].objectness_logits.tolist() == [1.0, 3.0] and d["proposals"].objectness_logits.dtype == torch.float32
    assert d["proposals"].proposal_boxes.tensor.tolist() == [[0, 0, 3, 3], [1, 1, 4, 4]] and boxes[2, 2] == 9        # the input is left alone
    for missing in ("proposals", "instances"):
        full = {"proposals": d["proposals"], "instances": None}
        del full[missing]
        with pytest.raises(KeyError, match=missing):
            data.change_proposals_as_gt(full)


def test_proposal_store_packs_once():
    a = np.arange(35, dtype=np.float32).reshape(5, 7)               # more than five columns: the rest is ignored
    b = np.arange(10, dtype=np.float32).reshape(2, 5) + 100
    store = data.ProposalStore({7: a, "x": [b, "ignored"], 9: np.zeros((0, 5), np.float32)})
    assert len(store) == 3 and 7 in store and "x" in store and 8 not in store and store.rows is None and store.dtype == np.float32
    assert store[7] is a and np.array_equal(store["x"], b) and store[9].shape == (0, 5)             # a thin view on the CPU
    with pytest.raises(KeyError):
        store[8]
    mixed = data.ProposalStore({7: a, 8: b.astype(np.float64)})
    assert mixed.dtype == np.float64 and mixed[7].dtype == np.float64 and np.array_equal(mixed[7], a)
    with pytest.raises(ValueError, match="XYXY"):
        data.ProposalStore({1: np.zeros((3, 4), np.float32)})


# ---- the mappers -----------------------------------------------------------------------------------------------------------------

class Metadata:
    thing_classes = ["person", "bicycle", "car", "dog"]

    def __init__(self, **entries):
        self.entries = entries

    def get(self, name, default=None):
        return self.entries.get(name, default)


def _cfg(**model):
    cfg = get_cfg()
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.LOAD_OBJ_PROPOSALS = True
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TEST = (40, 48, 64), 90, 74
    for k, v in model.items():
        cfg.MODEL[k] = v
    return cfg


def _anno(box, category_id):
    return {"bbox": list(box), "bbox_mode": data.XYWH_ABS, "category_id": category_id}


def _dicts(n=3):
    rng = np.random.default_rng(4)
    return [{"image_raw": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), "height": 37, "width": 53, "image_id": 10 + i,
             "annotations": [_anno((4.0, 5.0, 20.0, 10.0), 3), _anno((1.0, 1.0, 30.0, 30.0), 1)]} for i in range(n)]


CASE = pc.Case("mapper", "float32", 2000, tuple(pc.Image(65, (37, 53), None, 0) for _ in range(3)))


def _metadata(n=3):
    return Metadata(captions_dict={10 + i: [f"caption {i}.{j}" for j in range(4)] for i in range(n)},
                    object_proposals={10 + i: pc.rows(CASE, i) for i in range(n)})


def test_coco_mapper_dicts_and_the_replayed_sample():
    mapper = data.CocoImageDatasetMapper(_cfg(), _metadata(), True, device="cpu", seed=5)
    assert mapper.proposal_topk == 2000 and isinstance(mapper.store, data.ProposalStore)
    dicts = _dicts()
    before = copy.deepcopy(dicts)
    sample = mapper.draw_sample(dicts)
    assert all(0 <= c < 4 for c in sample["caption"]) and len(set(mapper.draw_sample(dicts * 4)["caption"])) > 1
    first, again = mapper.map_batch(dicts, sample), mapper.map_batch(dicts, sample)
    for d, b in zip(dicts, before):
        assert d.keys() == b.keys() and d["annotations"] == b["annotations"]                           # the input is left alone
    for i, (a, b) in enumerate(zip(first, again)):
        assert set(a) == {"image", "height", "width", "image_id", "caption", "nouns", "nouns_id", "instances", "gt_obj"}
        assert a["caption"] == b["caption"] == f"caption {i}.{sample['caption'][i]}"
        assert a["nouns"] == ["dog", "bicycle"] and a["nouns_id"] == [3, 1]
        inst, obj = a["instances"], a["gt_obj"]
        assert isinstance(inst, Instances) and list(inst.get_fields()) == ["objectness_logits", "gt_classes", "gt_boxes"]
        assert isinstance(inst.gt_boxes, Boxes) and inst.gt_classes.dtype == torch.int64 and bool((inst.gt_classes == 1).all()) and len(inst) > 0
        assert obj.gt_classes.tolist() == [3, 1] and len(obj.gt_boxes) == 2 and inst.image_size == obj.image_size == tuple(a["image"].shape[1:])
        assert torch.equal(inst.gt_boxes.tensor, b["instances"].gt_boxes.tensor) and torch.equal(a["image"], b["image"])
        # the same lists by hand: the image's transforms on its rows, the config's cut, the threshold
        nh, nw = inst.image_size
        im = pc.Image(65, (37, 53), (nh, nw), int(sample["flip"][i]))
        props, _ = proposal_ref.transform_proposals(pc.rows(CASE, i), im.hw, im.new_hw, im.flip, 2000)
        want = proposal_ref.change_proposals_as_gt({"proposals": props, "instances": None})["instances"]
        assert torch.equal(inst.gt_boxes.tensor, want.gt_boxes.tensor) and torch.equal(inst.objectness_logits, want.objectness_logits)


def test_coco_mapper_caption_rules_topk_and_missing_entries():
    meta = _metadata()
    test_mapper = data.CocoImageDatasetMapper(_cfg(), meta, False, device="cpu")
    assert test_mapper.proposal_topk == 1000
    out = test_mapper(_dicts(1)[0])
    assert out["caption"] == "caption 0.0" and out["instances"].image_size == (74, 106)              # inference: the first caption
    cfg = _cfg()
    cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST = 2
    cut = data.CocoImageDatasetMapper(cfg, meta, False, device="cpu")(_dicts(1)[0])
    assert len(cut["instances"]) <= 2 and torch.equal(cut["instances"].gt_boxes.tensor, out["instances"].gt_boxes.tensor[:len(cut["instances"])])
    del meta.entries["captions_dict"][11]                                                           # no caption entry: "" and empty lists
    got = test_mapper.map_batch(_dicts(2))[1]
    assert got["caption"] == "" and got["nouns"] == [] and got["nouns_id"] == [] and len(got["gt_obj"]) == 2
    unknown = dict(_dicts(1)[0], image_id=99)                                                       # no proposal entry: KeyError, as in the reference
    with pytest.raises(KeyError, match="proposals"):
        test_mapper(unknown)
    without = dict(_dicts(1)[0])
    del without["annotations"]
    with pytest.raises(KeyError):
        data.CocoImageDatasetMapper(_cfg(), Metadata(object_proposals=meta.get("object_proposals")), False, device="cpu")(without)
    # a list-of-arrays entry and a ready-made store
    listed = Metadata(object_proposals=data.ProposalStore({10: [pc.rows(CASE, 0)]}))
    one = data.CocoImageDatasetMapper(_cfg(), listed, False, device="cpu")(_dicts(1)[0])
    assert torch.equal(one["instances"].gt_boxes.tensor, out["instances"].gt_boxes.tensor) and "caption" not in one and "nouns" not in one
    # without object_proposals in the metadata the mapper is the base mapper plus the captions
    plain = data.CocoImageDatasetMapper(_cfg(), Metadata(captions_dict=meta.get("captions_dict")), False, device="cpu")(_dicts(1)[0])
    assert "gt_obj" not in plain and plain["instances"].gt_classes.tolist() == [3, 1] and plain["caption"] == "caption 0.0"


def test_dataset_mapper_takes_the_key_and_maps_a_dict_that_carries_proposals():
    cfg = _cfg()
    mapper = data.DatasetMapper(cfg, False, device="cpu")
    assert mapper.proposal_topk == 1000 and data.DatasetMapper(get_cfg(), False, device="cpu").proposal_topk is None
    rows = pc.rows(CASE, 0)
    d = dict(_dicts(1)[0], proposal_boxes=rows[:, :4], proposal_objectness_logits=rows[:, 4], proposal_bbox_mode=data.XYXY_ABS)
    out = mapper(d)
    assert "proposal_boxes" in d and not {"proposal_boxes", "proposal_bbox_mode", "proposal_objectness_logits"} & set(out)
    props, _ = proposal_ref.transform_proposals(rows, (37, 53), (74, 106), 0, 1000)
    assert list(out["proposals"].get_fields()) == ["proposal_boxes", "objectness_logits"] and out["proposals"].image_size == (74, 106)
    assert torch.equal(out["proposals"].proposal_boxes.tensor, props.proposal_boxes.tensor) and out["instances"].gt_classes.tolist() == [3, 1]
    assert "proposals" not in mapper(_dicts(1)[0])                                                   # no proposals in the dict: none out
    off = get_cfg()
    off.MODEL.DEVICE = "cpu"
    assert "proposals" not in data.DatasetMapper(off, False)(d)                                      # the key is off: as before


def test_get_mapper_dispatch_and_refusals():
    cfg, meta = _cfg(), _metadata()
    assert type(data.get_mapper("coco_captions_train_seen_proposals", cfg, True, meta, device="cpu")) is data.CocoImageDatasetMapper
    lvis = data.get_mapper("lvis_v1_val", cfg, False, meta, device="cpu")
    assert type(lvis) is data.DatasetMapper and not lvis.is_train
    for name, word in (("vaw_train", "Vaw"), ("cc3m_noise", "Noise"), ("", "Noise")):
        with pytest.raises(NotImplementedError, match=word):
            data.get_mapper(name, cfg, True, meta)


def test_config_defaults_and_what_is_still_refused():
    cfg = get_cfg()
    assert cfg.MODEL.LOAD_OBJ_PROPOSALS is False
    assert (cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN, cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST) == (2000, 1000)
    # coco_lsm.yaml's mapper keys load without a refusal
    cfg.merge_from_dict({"MODEL": {"LOAD_OBJ_PROPOSALS": True}, "DATASETS": {"TRAIN": ("coco_captions_train_seen_proposals",)}})
    cfg.MODEL.DEVICE = "cpu"
    assert data.DatasetMapper(cfg, True).proposal_topk == 2000
    for key in ("MASK_ON", "KEYPOINT_ON"):
        with pytest.raises(NotImplementedError, match="MASK_ON"):
            data.DatasetMapper(_cfg(**{key: True}), True)
