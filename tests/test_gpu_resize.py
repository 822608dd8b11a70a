"""csrc/image_resize.hip on the device: ops.resize_flip_images against tests/resize_ref.py (the plain-loop restatement of Pillow's 8-bit
bilinear resize, itself checked against Pillow's bytes in tests/test_resize_host.py), and DatasetMapper on the device against its
host path.  Every comparison is exact equality of bytes.  Outputs are carved from one buffer pre-filled with 0xA5, with a guard
region behind each: every output byte must be written and no guard byte touched."""
import numpy as np
import pytest
import torch

import backbone_ref as br
import lsm_model_cases as mc
import resize_cases as rc
import resize_ref

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
_REF = {}


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _want(img, size, flip):
    """resize_ref's answer, computed once per (image, size) and shared by the flips and tests that ask for it again."""
    key = (img.shape, size, img.tobytes())
    if key not in _REF:
        _REF[key] = resize_ref.resize(img, *size)
        _REF[key].setflags(write=False)
    out = _REF[key]
    out = out[:, ::-1] if flip == 1 else out[::-1] if flip == 2 else out
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def _offset_copy(img, offset):
    """The image on the device, its first byte `offset` bytes into a fresh allocation."""
    store = torch.zeros(img.size + 16, dtype=torch.uint8, device="cuda")
    view = store[offset:offset + img.size].view(img.shape)
    view.copy_(torch.from_numpy(img))
    assert view.is_contiguous() and view.data_ptr() % 16 == offset
    return view


def _run(pkg, images, sizes, flips, offset=0):
    """One call for the batch; checks every output byte and every guard byte, and that a second call gives the same bits."""
    C = images[0].shape[2]
    dev = [_offset_copy(x, offset) for x in images]
    lengths = [C * h * w for h, w in sizes]
    buf = torch.full((sum(lengths) + GUARD * len(sizes),), FILL, dtype=torch.uint8, device="cuda")
    outs, at = [], 0
    for n, (h, w) in zip(lengths, sizes):
        outs.append(buf[at:at + n].view(C, h, w))
        at += n + GUARD
    got = pkg.ops.resize_flip_images(dev, sizes, flips, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    want = np.full(buf.numel(), FILL, dtype=np.uint8)
    at = 0
    for x, n, size, flip in zip(images, lengths, sizes, flips):
        want[at:at + n] = _want(x, size, flip).reshape(-1)
        at += n + GUARD
    first = buf.cpu().numpy()
    bad = np.flatnonzero(first != want)
    assert bad.size == 0, f"{bad.size} differing bytes, the first at {bad[:5]} (got {first[bad[:5]]}, want {want[bad[:5]]})"
    for x, d in zip(images, dev):
        assert np.array_equal(d.cpu().numpy(), x)                                    # the inputs are left as they were
    fresh = pkg.ops.resize_flip_images(dev, sizes, flips)                            # fresh torch.empty outputs
    for f, o in zip(fresh, outs):
        assert f.dtype == torch.uint8 and torch.equal(f, o)


ALL_CASES = rc.SMALL_CASES + [rc.REALISTIC]
SUPPORTED = [c for c in ALL_CASES if c[0] != "over_limit"]


@pytest.mark.parametrize("name,size,new", SUPPORTED, ids=[c[0] for c in SUPPORTED])
def test_resize_gives_pillows_bytes(pkg, name, size, new):
    assert pkg.ops.resize_supported(size, new, 3)
    kinds = ("random",) if name == "realistic" else ("random", "checker", "white")
    for kind in kinds:
        _run(pkg, [rc.content(kind, *size, 3, f"{name}/{kind}/3")], [new], [0])


def test_white_stays_white_and_the_checkerboard_on_the_realistic_shape(pkg):
    _, size, new = rc.REALISTIC
    white = pkg.ops.resize_flip_images([torch.full(size + (3,), 255, dtype=torch.uint8, device="cuda")], [new])[0]
    assert int(white.min()) == 255                                                   # the + 2^21 never carries into 256
    checker = rc.content("checker", 97, 131, 3, "")
    _run(pkg, [checker], [(160, 203)], [1])


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("offset", [0, 1])
def test_channel_counts_and_odd_bases(pkg, channels, offset):
    name, size, new = rc.CHANNEL_CASE
    images = [rc.content("random", *size, channels, f"{name}/random/{channels}"), rc.content("random", 37, 53, channels, "odd")]
    _run(pkg, images, [new, (61, 87)], [0, 0], offset=offset)


@pytest.mark.parametrize("flip", [0, 1, 2], ids=["none", "horizontal", "vertical"])
def test_flips_with_a_resize_and_with_an_identity_size(pkg, flip):
    img = rc.content("random", 37, 53, 3, "upscale/random/3")
    _run(pkg, [img, img, rc.content("random", 20, 30, 3, "tile_plus_1/random/3")], [(61, 87), (37, 53), (17, 65)], [flip] * 3, offset=flip)


def test_one_call_with_five_images_of_mixed_sizes_and_flips(pkg):
    by_name = {c[0]: c for c in rc.SMALL_CASES}
    picks = ["mixed", "many_taps", "two_tiles_minus_1", "tap_limit_bands", "row"]
    images = [rc.content("random", *by_name[n][1], 3, f"{n}/random/3") for n in picks]
    _run(pkg, images, [by_name[n][2] for n in picks], [1, 2, 0, 1, 2], offset=1)


def test_one_call_with_the_most_images(pkg):
    n = pkg.ops.IMAGE_BATCH_MAX_IMAGES
    assert n == 64
    images = [rc.content("random", 1 + i % 5, 1 + i % 7, 3, i) for i in range(n)]
    sizes = [(1 + (3 * i) % 7, 1 + (5 * i) % 9) for i in range(n)]
    _run(pkg, images, sizes, [i % 3 for i in range(n)])
    with pytest.raises(ValueError, match="at most 64"):
        pkg.ops.resize_flip_images([torch.zeros(2, 2, 3, dtype=torch.uint8, device="cuda")] * (n + 1), [(2, 2)] * (n + 1))


def test_past_the_tap_limit_the_wrapper_refuses_and_the_mapper_takes_the_host_path(pkg):
    name, size, new = next(c for c in rc.SMALL_CASES if c[0] == "over_limit")
    img = rc.content("random", *size, 3, f"{name}/random/3")
    assert not pkg.ops.resize_supported(size, new, 3)
    with pytest.raises(ValueError, match="limits"):
        pkg.ops.resize_flip_images([torch.from_numpy(img).cuda()], [new])
    cfg = pkg.config.get_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 8, 20
    mapper = pkg.data.DatasetMapper(cfg, False, device="cuda")
    tall = rc.content("random", 200, 20, 3, "tall")                                  # 200 x 20 at 8, at most 20: 20 x 2, a factor of 10
    out = mapper({"image_raw": tall})
    assert tuple(out["image"].shape) == (3, 20, 2) and not pkg.ops.resize_supported((200, 20), (20, 2), 3)
    assert out["image"].is_cuda and np.array_equal(out["image"].cpu().numpy(), _want(tall, (20, 2), 0))


# ---- the mapper and the model --------------------------------------------------------------------------------------------------

def _dicts(n=5):
    rng = np.random.default_rng(12)
    out = []
    for i, (h, w) in enumerate([(97, 131), (120, 90), (64, 64), (37, 53), (150, 200)][:n]):
        annos = [{"bbox": [w * 0.1, h * 0.2, w * 0.5, h * 0.55], "bbox_mode": 1, "category_id": i % 5},
                 {"bbox": [w * 0.4, h * 0.1, w * 0.3, h * 0.3], "bbox_mode": 1, "category_id": (i + 2) % 5, "iscrowd": i % 2},
                 {"bbox": [1.0, 2.0, w - 3.0, h - 2.0], "bbox_mode": 0, "category_id": 4}]
        out.append({"image_raw": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "image_id": i, "annotations": annos,
                    "caption": [f"w{10 + i} w11 w12", f"w{20 + i} w21"]})
    return out


def _same_dicts(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "image":
            assert a[k].dtype == b[k].dtype == torch.uint8 and a[k].shape == b[k].shape and torch.equal(a[k].cpu(), b[k].cpu())
        elif k == "instances":
            assert a[k].image_size == b[k].image_size and torch.equal(a[k].gt_classes, b[k].gt_classes)
            assert torch.equal(a[k].gt_boxes.tensor.view(torch.int32), b[k].gt_boxes.tensor.view(torch.int32))
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("is_train", [True, False], ids=["train", "test"])
def test_mapper_on_the_device_equals_its_host_path(pkg, is_train, monkeypatch):
    cfg = pkg.config.get_cfg()
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = (96, 128, 160), 224, 128, 224
    dev, host = pkg.data.DatasetMapper(cfg, is_train, device="cuda", seed=4), pkg.data.DatasetMapper(cfg, is_train, device="cpu")
    dicts = _dicts()
    sample = dev.draw_sample(dicts)
    if is_train:
        sample["flip"] = [True, False, True, True, False]
    calls = []
    real = pkg.ops.resize_flip_images
    monkeypatch.setattr(pkg.ops, "resize_flip_images", lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
    got, want = dev.map_batch(dicts, sample), host.map_batch(dicts, sample)
    assert calls == [5]                                                              # one launch for the batch
    for g, w, d in zip(got, want, dicts):
        assert g["image"].is_cuda and not w["image"].is_cuda and (g["height"], g["width"]) == d["image_raw"].shape[:2]
        _same_dicts(g, w)
    monkeypatch.setenv("LOCOV_FUSED_RESIZE", "0")                                    # the definition, moved to the device
    for g, w in zip(dev.map_batch(dicts, sample), want):
        assert g["image"].is_cuda
        _same_dicts(g, w)
    assert calls == [5]


def test_inference_from_raw_images_is_the_same_from_both_paths(pkg):
    cfg = mc.toy_cfg(pkg, "cuda", arch="GeneralizedRCNN")
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 160, 224
    torch.manual_seed(11)
    model = pkg.build_model(cfg)
    br.randomize_frozen_bn(model.backbone, 3)
    model.roi_heads.box_predictor.set_class_embeddings(torch.randn(6, mc.HIDDEN) * 0.05)
    model.roi_heads.num_classes = model.roi_heads.box_predictor.num_classes
    model.eval()
    dicts = _dicts(2)
    dev, host = pkg.data.DatasetMapper(cfg, False, device="cuda"), pkg.data.DatasetMapper(cfg, False, device="cpu")
    with torch.no_grad():
        got = [model.inference(b) for b in pkg.data.iterate_batches(dicts, dev, 2)]
        want = [model.inference(b) for b in pkg.data.iterate_batches(dicts, host, 2)]
    assert len(got) == len(want) == 1 and len(got[0]) == 2
    for g, w, d in zip(got[0], want[0], dicts):
        a, b = g["instances"], w["instances"]
        assert a.image_size == b.image_size == d["image_raw"].shape[:2] and len(a) == len(b) >= 1
        assert torch.equal(a.pred_boxes.tensor.view(torch.int32), b.pred_boxes.tensor.view(torch.int32))
        assert torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)) and torch.equal(a.pred_classes, b.pred_classes)
