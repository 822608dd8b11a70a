"""locov_amd/data.py on the host: the restatement of Pillow's bilinear resize (and the independent one of tests/resize_ref.py) against
bytes Pillow itself produced (tests/golden/g12_pil_resize.npz, and a live Pillow where it imports), Detectron2's shape rule and box
transforms against hand-computed values, and the mapper's dicts."""
import copy
import os

import numpy as np
import pytest
import torch

import resize_cases
import resize_ref
from locov_amd import data
from locov_amd.config import get_cfg


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "g12_pil_resize.npz")) as z:
        return {k: z[k] for k in z.files}


def _keys(golden):
    return sorted(k[3:] for k in golden if k.startswith("in:"))


def test_fixture_holds_every_small_case(golden):
    keys = _keys(golden)
    assert str(golden["pillow_version"])[0].isdigit()
    for name, size, new in resize_cases.SMALL_CASES:
        key = f"{name}/random/3"
        assert key in keys and golden["in:" + key].shape == size + (3,) and golden["out:" + key].shape == new + (3,)
        assert np.array_equal(golden["in:" + key], resize_cases.content("random", *size, 3, key))       # the tests can redraw the inputs
    assert {k.rsplit("/", 1)[1] for k in keys} == {"1", "3", "4"} and {k.split("/")[1] for k in keys} == {"random", "checker", "white"}


def test_both_restatements_give_pillows_bytes(golden):
    for key in _keys(golden):
        img, want = golden["in:" + key], golden["out:" + key]
        got = data.resize_bilinear_host(img, *want.shape[:2])
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), key
        assert np.array_equal(resize_ref.resize(img, *want.shape[:2]), want), key
    white = golden["out:upscale/white/3"]
    assert white.min() == 255                                   # the + 2^21 does not carry into 256


def test_both_restatements_equal_a_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    modes = {1: "L", 3: "RGB", 4: "CMYK"}                       # ("RGBA" resizes with premultiplied alpha: not an image array's resize)
    cases = [(n, s, o, 3) for n, s, o in resize_cases.SMALL_CASES + [resize_cases.REALISTIC]]
    cases += [resize_cases.CHANNEL_CASE + (c,) for c in (1, 4)]
    for name, (h, w), (nh, nw), c in cases:
        for kind in ("random", "checker", "white"):
            img = resize_cases.content(kind, h, w, c, name)
            im = Image.fromarray(img[:, :, 0] if c == 1 else img, modes[c])
            want = np.asarray(im.resize((nw, nh), Image.BILINEAR)).reshape(nh, nw, c)
            assert np.array_equal(data.resize_bilinear_host(img, nh, nw), want), (name, kind, c)
            if name != "realistic" or kind == "random":
                assert np.array_equal(resize_ref.resize(img, nh, nw), want), (name, kind, c)


def test_coefficients_agree_and_respect_the_tap_limit():
    for in_size, out_size in [(1, 3), (9, 2), (53, 87), (64, 17), (131, 200), (63, 8), (128, 16), (65, 8), (3000, 800)]:
        xmin, count, k = data.bilinear_coefficients(in_size, out_size)
        assert k.shape[1] == resize_ref.taps(in_size, out_size)
        for xx in range(out_size):
            m, ks = resize_ref.coefficients(in_size, out_size, xx)
            assert m == xmin[xx] and len(ks) == count[xx] and ks == list(k[xx, :len(ks)]) and not k[xx, len(ks):].any()
    assert resize_ref.taps(63, 8) == resize_ref.taps(128, 16) == resize_cases.MAX_TAPS and resize_ref.taps(65, 8) == resize_cases.MAX_TAPS + 2
    assert resize_ref.taps(3000, 800) == 9                      # a 4000 x 3000 photograph to 800 on the short side


def test_the_shape_rule():
    shape = data.ResizeShortestEdge.get_output_shape
    assert shape(480, 640, 800, 1333) == (800, 1067)            # 640 * 800 / 480 = 1066.67
    assert shape(640, 480, 800, 1333) == (1067, 800)
    assert shape(500, 1500, 800, 1333) == (444, 1333)           # 800 x 2400, then * 1333 / 2400: 444.33 x 1333
    assert shape(300, 300, 800, 1333) == (800, 800)             # a square image
    assert shape(1000, 1000, 1400, 1333) == (1333, 1333)        # ... limited by max_size
    assert shape(3000, 4000, 800, 1333) == (800, 1067)
    aug = data.ResizeShortestEdge((0,), 1333, "choice")
    t = aug.get_transform(37, 53, 0)                            # a size of 0: a no-op
    assert type(t) is data.NoOpTransform and t.output_shape(37, 53) == (37, 53)
    rng = data.random.Random(3)
    assert all(640 <= data.ResizeShortestEdge((640, 672), 1333, "range").draw(rng) <= 672 for _ in range(50))
    assert {data.ResizeShortestEdge((640, 672, 704), 1333, "choice").draw(rng) for _ in range(60)} == {640, 672, 704}
    with pytest.raises(AssertionError):
        data.ResizeShortestEdge((640, 672, 704), 1333, "range")


def _cfg(**inp):
    cfg = get_cfg()
    cfg.MODEL.DEVICE = "cpu"
    for k, v in inp.items():
        cfg.INPUT[k] = v
    return cfg


def test_build_augmentation_reads_the_config():
    cfg = get_cfg()
    assert (cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING, cfg.INPUT.MAX_SIZE_TRAIN) == ((800,), "choice", 1333)
    assert (cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, cfg.INPUT.RANDOM_FLIP) == (800, 1333, "horizontal")
    train, test = data.build_augmentation(cfg, True), data.build_augmentation(cfg, False)
    assert [type(a) for a in train] == [data.ResizeShortestEdge, data.RandomFlip] and [type(a) for a in test] == [data.ResizeShortestEdge]
    assert train[1].horizontal and not train[1].vertical and train[1].prob == 0.5 and not train[0].is_range
    assert test[0].short_edge_length == (800, 800) and test[0].max_size == 1333
    assert data.build_augmentation(_cfg(RANDOM_FLIP="vertical"), True)[1].vertical
    assert len(data.build_augmentation(_cfg(RANDOM_FLIP="none"), True)) == 1
    ranged = data.build_augmentation(_cfg(MIN_SIZE_TRAIN=(640, 800), MIN_SIZE_TRAIN_SAMPLING="range"), True)[0]
    assert ranged.is_range and ranged.short_edge_length == (640, 800)


@pytest.mark.parametrize("key,value", [("COLOR_JITTER", 0.4), ("RANDOM_GRAY_SCALE", True), ("GAUSSIAN_BLUR", True), ("RANDOM_ERASE", True),
                                       ("CROP", {"ENABLED": True})])
def test_what_is_not_built_is_refused(key, value):
    cfg = _cfg()
    cfg.merge_from_dict({"INPUT": {key: value}})
    with pytest.raises(NotImplementedError, match=key):
        data.build_augmentation(cfg, True)
    with pytest.raises(NotImplementedError, match=key):
        data.DatasetMapper(cfg, False)


def test_mask_and_keypoint_configs_are_refused():
    cfg = _cfg()
    cfg.MODEL.MASK_ON = True
    with pytest.raises(NotImplementedError, match="MASK_ON"):
        data.DatasetMapper(cfg, True)
    with pytest.raises(NotImplementedError, match="bbox_mode"):
        data.convert_to_xyxy([1, 2, 3, 4], 4)


# ---- boxes ---------------------------------------------------------------------------------------------------------------------
H, W, NH, NW = 480, 640, 800, 1067


def _anno(box, mode=data.XYWH_ABS, **kw):
    return dict({"bbox": list(box), "bbox_mode": mode, "category_id": 3}, **kw)


def test_box_transform_equals_the_closed_form():
    # XYWH with quarter-pixel values: exact in the fp32 the conversion runs in (BoxMode.convert on a list)
    x, y, w, h = 100.25, 50.5, 200.0, 120.75
    x1, y1, x2, y2 = x, y, x + w, y + h
    sx, sy = NW * 1.0 / W, NH * 1.0 / H
    resize = data.ResizeTransform(H, W, NH, NW)
    got = data.transform_instance_annotations(_anno((x, y, w, h)), data.TransformList([resize]), (NH, NW))
    assert got["bbox_mode"] == data.XYXY_ABS and got["bbox"].dtype == np.float64
    assert got["bbox"].tolist() == [x1 * sx, y1 * sy, x2 * sx, y2 * sy]
    got = data.transform_instance_annotations(_anno((x, y, w, h)), data.TransformList([data.NoOpTransform(), data.HFlipTransform(W)]), (H, W))
    assert got["bbox"].tolist() == [W - x2, y1, W - x1, y2]
    got = data.transform_instance_annotations(_anno((x, y, w, h)), data.TransformList([data.VFlipTransform(H)]), (H, W))
    assert got["bbox"].tolist() == [x1, H - y2, x2, H - y1]
    got = data.transform_instance_annotations(_anno((x, y, w, h)), data.TransformList([resize, data.HFlipTransform(NW)]), (NH, NW))
    assert got["bbox"].tolist() == [NW - x2 * sx, y1 * sy, NW - x1 * sx, y2 * sy]
    # XYXY passes through; a box over the border is clipped at 0 and at (w, h, w, h)
    got = data.transform_instance_annotations(_anno((-5.0, 10.0, 700.0, 500.0), data.XYXY_ABS), data.TransformList([resize]), (NH, NW))
    assert got["bbox"].tolist() == [0.0, 10.0 * sy, float(NW), float(NH)]
    assert data.convert_to_xyxy([1, 2, 3, 4], data.XYWH_ABS) == [1, 2, 4, 6]                        # ints stay ints
    assert data.convert_to_xyxy([0.1, 0.0, 0.2, 1.0], data.XYWH_ABS)[2] == float(np.float32(0.1) + np.float32(0.2))


def _dict(rng, captions=True):
    d = {"image_raw": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), "height": 37, "width": 53, "image_id": 7,
         "annotations": [_anno((4.0, 5.0, 20.0, 10.0)), _anno((1.0, 1.0, 30.0, 30.0), iscrowd=1), _anno((10.0, 10.0, 0.0, 5.0)),
                         _anno((60.0, 3.0, 5.0, 5.0)), _anno((2.0, 3.0, 40.0, 30.0), data.XYXY_ABS, category_id=9, iscrowd=0)]}
    if captions:
        d["caption"] = ["a first caption", "a second caption", "a third caption"]
    return d


def test_mapper_drops_crowd_and_empty_boxes_and_leaves_its_input_alone():
    cfg = _cfg(MIN_SIZE_TEST=74, MAX_SIZE_TEST=1333)
    mapper = data.DatasetMapper(cfg, False, device="cpu")
    src = _dict(np.random.default_rng(0))
    before = copy.deepcopy(src)
    out = mapper(src)
    assert src.keys() == before.keys() and src["annotations"] == before["annotations"] and np.array_equal(src["image_raw"], before["image_raw"])
    assert "annotations" not in out and "image_raw" not in out and (out["height"], out["width"]) == (37, 53)
    assert out["image"].dtype == torch.uint8 and tuple(out["image"].shape) == (3, 74, 106)
    assert np.array_equal(out["image"].numpy(), resize_ref.resize_flip_chw(src["image_raw"], 74, 106))
    inst = out["instances"]                 # the crowd box, the zero-width box and the box outside the image (empty once clipped) are gone
    assert inst.image_size == (74, 106) and inst.gt_boxes.tensor.dtype == torch.float32
    assert inst.gt_boxes.tensor.tolist() == [[8.0, 10.0, 48.0, 30.0], [4.0, 6.0, 80.0, 60.0]] and inst.gt_classes.tolist() == [3, 9]
    assert out["caption"] == "a first caption"                                                       # inference: element 0


def test_a_replayed_sample_reproduces_a_batch():
    cfg = _cfg(MIN_SIZE_TRAIN=(40, 48, 64), MAX_SIZE_TRAIN=90)
    mapper = data.DatasetMapper(cfg, True, device="cpu", seed=11)
    rng = np.random.default_rng(1)
    dicts = [_dict(rng) for _ in range(6)]
    sample = mapper.draw_sample(dicts)
    assert set(sample) == {"short_edge", "flip", "caption"} and all(len(v) == 6 for v in sample.values())
    first, again = mapper.map_batch(dicts, sample), mapper.map_batch(dicts, sample)
    other = mapper.map_batch(dicts)
    assert any(a["image"].shape != o["image"].shape or not torch.equal(a["image"], o["image"]) for a, o in zip(first, other))
    for i, (a, b, d) in enumerate(zip(first, again, dicts)):
        assert torch.equal(a["image"], b["image"]) and a["caption"] == b["caption"] == d["caption"][sample["caption"][i]]
        assert torch.equal(a["instances"].gt_boxes.tensor, b["instances"].gt_boxes.tensor)
        nh, nw = data.ResizeShortestEdge.get_output_shape(37, 53, sample["short_edge"][i], 90)
        assert np.array_equal(a["image"].numpy(), resize_ref.resize_flip_chw(d["image_raw"], nh, nw, int(sample["flip"][i])))
        x1, x2 = 4.0 * (nw / 53), 24.0 * (nw / 53)
        want = [nw - x2, nw - x1] if sample["flip"][i] else [x1, x2]
        assert a["instances"].gt_boxes.tensor[0, 0::2].tolist() == [float(np.float32(v)) for v in want]
    forced = dict(sample, flip=[True] * 6, short_edge=[0] * 6, caption=[2] * 6)                       # size 0: only the flip
    for a, d in zip(mapper.map_batch(dicts, forced), dicts):
        assert np.array_equal(a["image"].numpy(), d["image_raw"][:, ::-1].transpose(2, 0, 1)) and a["caption"] == "a third caption"


def test_image_size_rules_black_image_and_iterate_batches(tmp_path):
    cfg = _cfg(MIN_SIZE_TEST=0)
    mapper = data.DatasetMapper(cfg, False, device="cpu")
    raw = np.random.default_rng(2).integers(0, 256, (5, 8, 3), dtype=np.uint8)
    assert [mapper({"image_raw": raw, **kw})[k] for kw in ({}, {"height": 8, "width": 5}, {"height": 9, "width": 9})
            for k in ("height", "width")] == [5, 8] * 3                                                # filled, swapped, overwritten
    out = mapper({"file_name": str(tmp_path / "missing.jpg"), "height": 4, "width": 6, "caption": ["x", "y"]})
    assert tuple(out["image"].shape) == (3, 4, 6) and not out["image"].any() and out["caption"] == "A black image."
    assert mapper({"image_raw": torch.from_numpy(raw)})["image"].equal(torch.from_numpy(raw).permute(2, 0, 1))
    with pytest.raises(TypeError):
        mapper({"image_raw": raw.astype(np.float32)})
    batches = list(data.iterate_batches([{"image_raw": raw, "image_id": i} for i in range(5)], mapper, 2))
    assert [[d["image_id"] for d in b] for b in batches] == [[0, 1], [2, 3], [4]]


def test_mapper_reads_a_file_in_the_configured_order(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rgb = np.random.default_rng(3).integers(0, 256, (6, 7, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "a.png")
    out = data.DatasetMapper(_cfg(MIN_SIZE_TEST=0), False, device="cpu")({"file_name": str(tmp_path / "a.png")})
    assert np.array_equal(out["image"].numpy(), rgb[:, :, ::-1].transpose(2, 0, 1)) and (out["height"], out["width"]) == (6, 7)   # BGR
