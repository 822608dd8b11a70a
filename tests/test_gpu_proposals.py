"""The proposal side of the dataset mapper on the device (csrc/proposal_map.hip: locov_map_proposals; ops.map_proposals; data.py:
CocoImageDatasetMapper) against the HOST DEFINITION of locov_amd/data.py on the case table of tests/proposal_cases.py -- never
against the kernel itself.  Equality is torch.equal: the values are the definition's own roundings, and only the sign of a zero is
outside the contract."""
import numpy as np
import pytest
import torch

import backbone_ref as br
import lsm_model_cases as mc
import proposal_cases as pc

pytestmark = pytest.mark.gpu

FIELDS = ("prop_boxes", "prop_logits", "prop_src", "gt_boxes", "gt_logits", "gt_classes", "gt_src")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _garbage(pkg, total, n_images):
    bufs = pkg.ops.proposal_buffers(total, n_images, "cuda")
    for b in bufs:
        b.view(torch.uint8).fill_(0xA5)                              # (a NaN-free pattern nothing below produces: -2.87e-16 / a huge int)
    return bufs


def _run(pkg, case, out=None):
    rows, starts, counts = pc.store(case)
    rows = torch.from_numpy(rows).cuda()
    got = pkg.ops.map_proposals(rows, starts, counts, [pc.factors_of(im) for im in case.images], [im.flip for im in case.images],
                                [pc.size_of(im) for im in case.images], case.topk, pc.THR, out=out)
    return got, counts


def _check(pkg, case):
    total, n_images = sum(im.n for im in case.images), len(case.images)
    bufs = _garbage(pkg, total, n_images)
    got, counts = _run(pkg, case, out=bufs)
    want = pc.expected(pkg.data, case)
    assert len(got) == len(want) == n_images
    kept = bufs.counts.cpu()
    assert kept.dtype == torch.int32 and tuple(kept.shape) == (n_images, 2)
    at = 0
    for i, (g, w, n) in enumerate(zip(got, want, counts)):
        assert kept[i].tolist() == [len(w["prop_src"]), len(w["gt_src"])], (case.name, i)
        for k in FIELDS:
            view = getattr(g, k)
            assert view.is_cuda and view.dtype == w[k].dtype and torch.equal(view.cpu(), w[k]), (case.name, i, k)
            seg = getattr(bufs, k)[at:at + n]
            assert len(view) == 0 or view.data_ptr() == seg.data_ptr()              # a view of the caller's buffer, at the image's segment
            tail = seg[len(w[k]):].cpu()                                            # behind the count: zeros, src -1, classes 0
            assert bool((tail == (-1 if k.endswith("src") else 0)).all()), (case.name, i, k)
        at += n
    fresh, _ = _run(pkg, case)                                                      # a second call, fresh buffers: the same bits
    for g, f in zip(got, fresh):
        for k in FIELDS:
            a, b = getattr(g, k), getattr(f, k)
            assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (case.name, k)


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_map_proposals_equals_the_host_definition(pkg, case):
    _check(pkg, case)


def test_more_than_one_call_of_images(pkg):
    assert len(pc.CHUNKED.images) == pkg.ops.IMAGE_BATCH_MAX_IMAGES + 1
    _check(pkg, pc.CHUNKED)


def test_empty_batches(pkg):
    rows = torch.zeros((0, 5), device="cuda")
    assert pkg.ops.map_proposals(rows, [], [], [], [], [], 10, pc.THR) == []
    got = pkg.ops.map_proposals(rows, [0, 0], [0, 0], [(1.0, 1.0)] * 2, [0, 1], [(4, 4)] * 2, 10, pc.THR)
    assert len(got) == 2 and all(len(v) == 0 for g in got for v in g)
    with pytest.raises(TypeError):
        pkg.ops.map_proposals(rows.half(), [0], [0], [(1.0, 1.0)], [0], [(4, 4)], 10, pc.THR)
    with pytest.raises(ValueError):
        pkg.ops.map_proposals(torch.zeros((4, 5), device="cuda"), [2], [3], [(1.0, 1.0)], [0], [(4, 4)], 10, pc.THR)


# ---- the mapper and the model ----------------------------------------------------------------------------------------------------

class Metadata:
    thing_classes = ["c0", "c1", "c2", "c3", "c4"]

    def __init__(self, **entries):
        self.entries = entries

    def get(self, name, default=None):
        return self.entries.get(name, default)


SIZES = [(80, 96), (64, 80), (97, 131)]


def _dataset(n_rows, dtype="float32", n=3):
    case = pc.Case(f"mapper_{n_rows}_{dtype}", dtype, 2000, tuple(pc.Image(n_rows, s, None, 0) for s in SIZES[:n]))
    rng = np.random.default_rng(6)
    dicts = []
    for i, (h, w) in enumerate(SIZES[:n]):
        annos = [{"bbox": [w * 0.1, h * 0.2, w * 0.5, h * 0.55], "bbox_mode": 1, "category_id": i % 5},
                 {"bbox": [1.0, 2.0, w - 3.0, h - 2.0], "bbox_mode": 0, "category_id": 4}]
        dicts.append({"image_raw": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "image_id": 100 + i, "annotations": annos})
    meta = Metadata(captions_dict={100 + i: [mc.captions()[i % 2], mc.captions()[(i + 1) % 2]] for i in range(n)},
                    object_proposals={100 + i: pc.rows(case, i) for i in range(n)})
    return dicts, meta


def _same(got, want):
    assert got.keys() == want.keys() and "proposals" not in got and {"instances", "gt_obj", "caption", "nouns", "nouns_id"} <= set(got)
    for k in got:
        if k == "image":
            assert got[k].is_cuda and torch.equal(got[k].cpu(), want[k])
        elif k in ("instances", "gt_obj"):
            a, b = got[k], want[k]
            assert a.image_size == b.image_size and list(a.get_fields()) == list(b.get_fields())
            for name, v in a.get_fields().items():
                v, w = getattr(v, "tensor", v), getattr(b.get(name), "tensor", b.get(name))
                assert v.is_cuda == (k == "instances") and v.dtype == w.dtype and torch.equal(v.cpu(), w), (k, name)
        else:
            assert got[k] == want[k], k


@pytest.mark.parametrize("dtype,is_train", [("float32", True), ("float64", True), ("float32", False)])
def test_coco_mapper_on_the_device_equals_its_host_path(pkg, dtype, is_train, monkeypatch):
    cfg = pkg.config.get_cfg()
    cfg.MODEL.LOAD_OBJ_PROPOSALS = True
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = (96, 128, 160), 224, 128, 224
    cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST = 40                                 # (a cut that bites, at inference)
    dicts, meta = _dataset(257, dtype)
    dev = pkg.data.CocoImageDatasetMapper(cfg, meta, is_train, device="cuda", seed=4)
    host = pkg.data.CocoImageDatasetMapper(cfg, meta, is_train, device="cpu")
    assert dev.store.rows.is_cuda and tuple(dev.store.rows.shape) == (3 * 257, 5) and host.store.rows is None
    sample = dev.draw_sample(dicts)
    if is_train:
        sample["flip"] = [True, False, True]
    calls = []
    real = pkg.ops.map_proposals
    monkeypatch.setattr(pkg.ops, "map_proposals", lambda *a, **k: calls.append(a[0].data_ptr()) or real(*a, **k))
    want = host.map_batch(dicts, sample)
    for g, w in zip(dev.map_batch(dicts, sample), want):
        _same(g, w)
    assert calls == [dev.store.rows.data_ptr()]                                      # one call for the batch, on the store's own rows
    assert any(0 < len(w["instances"]) < 257 for w in want)
    monkeypatch.setenv("LOCOV_FUSED_PROPOSALS", "0")                                 # the definition, moved to the device
    for g, w in zip(dev.map_batch(dicts, sample), want):
        _same(g, w)
    assert len(calls) == 1
    monkeypatch.setenv("LOCOV_FUSED_PROPOSALS", "1")
    # a store that lives on the host: the batch's rows are packed and uploaded once, then the same launch
    packed = pkg.data.CocoImageDatasetMapper(cfg, Metadata(captions_dict=meta.get("captions_dict"), object_proposals=host.store), is_train,
                                             device="cuda")
    for g, w in zip(packed.map_batch(dicts, sample), want):
        _same(g, w)
    assert len(calls) == 2 and calls[1] != calls[0]


def test_dataset_mapper_with_proposals_in_the_dict(pkg):
    cfg = pkg.config.get_cfg()
    cfg.MODEL.LOAD_OBJ_PROPOSALS = True
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 128, 224
    dicts, meta = _dataset(65)
    for d in dicts:
        rows = meta.get("object_proposals")[d["image_id"]]
        d.update(proposal_boxes=rows[:, :4], proposal_objectness_logits=rows[:, 4], proposal_bbox_mode=pkg.data.XYXY_ABS)
    del dicts[1]["proposal_boxes"]                                                   # an image without proposals between two with
    got = pkg.data.DatasetMapper(cfg, False, device="cuda").map_batch(dicts)
    want = pkg.data.DatasetMapper(cfg, False, device="cpu").map_batch(dicts)
    assert "proposals" not in got[1] and "proposals" not in want[1]
    for g, w in zip(got[::2], want[::2]):
        a, b = g["proposals"], w["proposals"]
        assert a.image_size == b.image_size and list(a.get_fields()) == list(b.get_fields()) == ["proposal_boxes", "objectness_logits"]
        assert a.proposal_boxes.tensor.is_cuda and torch.equal(a.proposal_boxes.tensor.cpu(), b.proposal_boxes.tensor)
        assert torch.equal(a.objectness_logits.cpu(), b.objectness_logits) and 0 < len(b) < 65


def test_training_forward_on_the_mapped_pseudo_ground_truth(pkg):
    cfg = mc.toy_cfg(pkg, "cuda", **{"MODEL.LOAD_OBJ_PROPOSALS": True, "MODEL.LANGUAGE_BACKBONE.FREEZE": False})
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = (160,), 400
    torch.manual_seed(11)
    model = pkg.build_model(cfg, tokenizer=mc.ToyTokenizer())
    br.randomize_frozen_bn(model.backbone, 3)
    model.roi_heads.box_predictor.set_class_embeddings(torch.randn(6, mc.HIDDEN) * 0.05)
    model.roi_heads.num_classes = model.roi_heads.box_predictor.num_classes
    dicts, meta = _dataset(65, n=2)
    dev = pkg.data.get_mapper("coco_captions_train_seen_proposals", cfg, True, meta, device="cuda")
    host = pkg.data.get_mapper("coco_captions_train_seen_proposals", cfg, True, meta, device="cpu")
    assert type(dev) is pkg.data.CocoImageDatasetMapper and dev.proposal_topk == 2000
    sample = dict(dev.draw_sample(dicts), flip=[True, False])
    mapped = dev.map_batch(dicts, sample)
    moved = [dict(d, image=d["image"].cuda(), instances=d["instances"].to("cuda")) for d in host.map_batch(dicts, sample)]
    for g, w in zip(mapped, moved):
        assert 0 < len(g["instances"]) < 65 and g["instances"].gt_boxes.tensor.is_cuda
        assert torch.equal(g["instances"].gt_boxes.tensor, w["instances"].gt_boxes.tensor) and torch.equal(g["image"], w["image"])
    from locov_amd.language_backbone import MAX_LENGTH
    draws = np.random.default_rng(3).random((2, 2, MAX_LENGTH))
    draws[0, 0, 2], draws[0, 1, 1] = 0.01, 0.02                                      # (a masked word in each caption: lsm_model_cases.mlm_draws)
    step = {"mlm_draws": torch.from_numpy(draws).cuda()}
    model.train()
    try:
        losses = []
        for batch in (mapped, moved):
            torch.manual_seed(21)
            losses.append(model(batch, sample=step)[1])
        assert list(losses[0]) == list(losses[1]) and "loss_rpn_cls" in losses[0] and "box_kd_loss" in losses[0]
        for k, v in losses[0].items():
            assert v.dim() == 0 and bool(torch.isfinite(v)), k
            assert torch.equal(v.detach().view(torch.int32), losses[1][k].detach().view(torch.int32)), k       # identical inputs: a condition
    finally:
        model.zero_grad(set_to_none=True)
        model.eval()
