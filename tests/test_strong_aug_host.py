"""locov_amd/strong_augment.py on the host: the restatement of the reference's strong augmentation (and the independent one of
tests/strong_aug_ref.py) against bytes Pillow itself produced (tests/golden/g13_pil_strong_aug.npz, and a live Pillow where it
imports), the erasers against the torch expression, torchvision's draw rules, and the mapper with train_aug on the CPU."""
import os
import random

import numpy as np
import pytest
import torch

import strong_aug_cases as sc
import strong_aug_ref as ref
from locov_amd import data
from locov_amd import strong_augment as sa
from locov_amd.config import get_cfg


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "g13_pil_strong_aug.npz")) as z:
        return {k: z[k] for k in z.files}


def _op(mod, img, name, value):
    """One recorded operation through a restatement (sa or ref: the same function names)."""
    if name == "L":
        return mod.luma(img)
    if name == "HSV":
        return mod.rgb_to_hsv(img)
    if name == "RGB_from_HSV":
        return mod.hsv_to_rgb(img)
    if name == "blur":
        return mod.gaussian_blur(img, value)
    op = {"brightness": sc.BRIGHTNESS, "contrast": sc.CONTRAST, "color": sc.SATURATION, "hue": sc.HUE}[name]
    return mod.adjust(img, op, value)


def _chain(mod, img, d, noise=None):
    return sa.apply_host(img, d, noise) if mod is sa else ref.apply(img, d, noise)


def test_both_restatements_give_pillows_bytes(golden):
    assert str(golden["pillow_version"])[0].isdigit()
    img = sc.content(*sc.SMALL, "ops")
    for name, value in sc.OP_CASES:
        want = golden[f"op:{name}/{value}"]
        for mod in (sa, ref):
            got = _op(mod, img, name, value)
            assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (name, value, mod.__name__)
    for name, (h, w), kind, d in sc.CHAIN_CASES:
        want = golden[f"chain:{name}"]
        for mod in (sa, ref):
            assert np.array_equal(_chain(mod, sc.content(h, w, name, kind), d), want), (name, mod.__name__)
    for h, w in sc.BLUR_SIZES:
        for sigma in sc.SIGMAS:
            want = golden[f"blur_sizes:{h}x{w}/{sigma}"]
            for mod in (sa, ref):
                assert np.array_equal(mod.gaussian_blur(sc.content(h, w, f"blur{h}x{w}"), sigma), want), (h, w, sigma, mod.__name__)
    assert golden["chain:white_blur"].min() == 255              # ww * 255 * (2 radius + 1) + fw * 510 + 2^23 does not fall short of 255
    assert len(golden) == 1 + len(sc.OP_CASES) + len(sc.CHAIN_CASES) + len(sc.BLUR_SIZES) * len(sc.SIGMAS)


def test_conversions_equal_a_live_pillow_on_every_colour():
    Image = pytest.importorskip("PIL.Image")
    v = np.arange(1 << 24, dtype=np.uint32)
    colours = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    im = Image.fromarray(colours, "RGB")
    want = {"L": np.asarray(im.convert("L")), "HSV": np.asarray(im.convert("HSV")),
            "RGB_from_HSV": np.asarray(Image.fromarray(colours, "HSV").convert("RGB"))}
    for name, w in want.items():
        for mod in (sa, ref):
            bad = np.count_nonzero(_op(mod, colours, name, None) != w)
            assert bad == 0, f"{name} ({mod.__name__}): {bad} differing bytes of {w.size}"


def test_blur_equals_a_live_pillow_across_sigma():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter
    sigmas = np.linspace(0.1, 2.0, 200)
    for h, w in sc.BLUR_SIZES:
        img = sc.content(h, w, f"blur{h}x{w}")
        for sigma in sigmas:
            want = np.asarray(Image.fromarray(img, "RGB").filter(ImageFilter.GaussianBlur(radius=float(sigma))))
            assert np.array_equal(sa.gaussian_blur(img, float(sigma)), want), (h, w, sigma)
            assert np.array_equal(ref.gaussian_blur(img, float(sigma)), want), (h, w, sigma)
    assert float(sa.box_radius(2.0)) == ref.box_radius(2.0) == 1.375 and sa.blur_reach(2.0) == 2 and sa.blur_reach(0.1) == 1
    assert all(float(sa.box_radius(float(s))) == ref.box_radius(float(s)) for s in sigmas)


def test_enhancers_equal_a_live_pillow_across_factors():
    pytest.importorskip("PIL.Image")
    from PIL import Image, ImageEnhance
    img = sc.content(64, 96, "enhance", "smooth")
    im = Image.fromarray(img, "RGB")
    factors = sorted(set(np.linspace(0.0, 2.0, 47).tolist() + [0.0, 0.9999999, 1.0, 1.0000001, 1.5, 2.0]))
    assert len(factors) == 50 and factors[0] == 0.0 and 1.0 in factors and max(factors) > 1
    for f in factors:
        for op, enhancer in ((sc.BRIGHTNESS, ImageEnhance.Brightness), (sc.CONTRAST, ImageEnhance.Contrast), (sc.SATURATION, ImageEnhance.Color)):
            want = np.asarray(enhancer(im).enhance(f))
            assert np.array_equal(sa.adjust(img, op, f), want) and np.array_equal(ref.adjust(img, op, f), want), (op, f)


def test_erasers_equal_the_torch_expression():
    img = sc.content(19, 23, "erase")
    rects = [(2, 3, 5, 7), None, (4, 6, 15, 17)]                # the second reaches the last row and column; they overlap
    noise = sc.noise(3 * (5 * 7 + 15 * 17), "erase")
    d = sc.draws(erase=rects)
    assert sa.noise_count(d) == noise.size
    want = ref.erase(img, rects, noise)
    got = sa.apply_host(img, d, noise)
    assert np.array_equal(got, want)
    mask = np.zeros((19, 23), bool)
    mask[2:7, 3:10] = mask[4:19, 6:23] = True
    assert np.array_equal(got[~mask], img[~mask]) and (got[mask] != img[mask]).any()          # ToTensor -> ToPILImage: the identity
    assert np.array_equal(got[4:19, 6:23], sa.noise_bytes(noise[105:]).reshape(3, 15, 17).transpose(1, 2, 0))    # the later eraser wins
    every = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    assert np.array_equal(ref.erase(every, [], noise), every)
    assert sa.noise_bytes(np.array([-1.0, -0.5, 1.5, 0.999, -3.0], np.float32)).tolist() == [1, 129, 126, 254, 3]
    assert np.array_equal(sa.apply_host(img, sc.draws(sc.PERMUTATIONS[3], sc.FACTOR_SETS[0], sigma=1.3, erase=rects), noise),
                          ref.apply(img, sc.draws(sc.PERMUTATIONS[3], sc.FACTOR_SETS[0], sigma=1.3, erase=rects), noise))
    with pytest.raises(ValueError, match="noise"):
        sa.apply_host(img, d, noise[:-1])
    with pytest.raises(TypeError):
        sa.apply_host(img[:, :, :1], sc.draws())


def _cfg(**inp):
    cfg = get_cfg()
    cfg.MODEL.DEVICE = "cpu"
    for k, v in inp.items():
        cfg.INPUT[k] = v
    return cfg


ALL_ON = dict(COLOR_JITTER=0.4, RANDOM_GRAY_SCALE=True, GAUSSIAN_BLUR=True, RANDOM_ERASE=True)


def test_build_complete_augmentation_follows_the_config():
    assert sa.build_complete_augmentation(_cfg(**ALL_ON), False) is None
    assert sa.build_complete_augmentation(_cfg(), True) is None
    aug = sa.build_complete_augmentation(_cfg(**ALL_ON), True)
    assert aug.color_jitter == 0.4 and aug.gray_scale and aug.gaussian_blur
    assert [(e.p, e.scale, e.ratio) for e in aug.erasers] == [(0.7, (0.05, 0.2), (0.3, 3.3)), (0.5, (0.02, 0.2), (0.1, 6)), (0.3, (0.02, 0.2), (0.05, 8))]
    only = sa.build_complete_augmentation(_cfg(GAUSSIAN_BLUR=True), True)
    assert only.color_jitter == 0 and not only.gray_scale and only.gaussian_blur and only.erasers == []


def test_the_draw_rules():
    aug = sa.build_complete_augmentation(_cfg(**ALL_ON), True)
    rng = random.Random(5)
    seen = {"jitter": 0, "gray": 0, "blur": 0, "erase": [0, 0, 0], "orders": set()}
    n = 600
    for _ in range(n):
        d = aug.draw(rng, 60, 90)
        assert sorted(d["order"]) == [1, 2, 3, 4] and len(d["erase"]) == 3
        if d["jitter"]:
            assert all(0.6 <= d[k] <= 1.4 for k in ("brightness", "contrast", "saturation")) and -0.1 <= d["hue"] <= 0.1
            seen["orders"].add(tuple(d["order"]))
        else:
            assert (d["brightness"], d["contrast"], d["saturation"], d["hue"]) == (1.0, 1.0, 1.0, 0.0)
        assert (0.1 <= d["sigma"] <= 2.0) if d["blur"] else d["sigma"] == 0.0
        for k, e in enumerate(d["erase"]):
            if e is not None:
                i, j, eh, ew = e
                assert eh < 60 and ew < 90 and 0 <= i <= 60 - eh and 0 <= j <= 90 - ew
                assert eh * ew <= 0.2 * 5400 + 0.5 * (60 + 90) + 1       # (sqrt(A r) + 1/2)(sqrt(A / r) + 1/2) with both roots below the sides
                seen["erase"][k] += 1
        for k in ("jitter", "gray", "blur"):
            seen[k] += bool(d[k])
    # p = 0.8, 0.2, 0.5 and 0.7, 0.5, 0.3 (less the rare eraser that does not fit in ten attempts): six sigma of a binomial of 600
    for got, p in zip([seen["jitter"], seen["gray"], seen["blur"]] + seen["erase"], (0.8, 0.2, 0.5, 0.7, 0.5, 0.3)):
        assert abs(got - n * p) <= 6 * (n * p * (1 - p)) ** 0.5 + 0.02 * n, (got, p)
    assert len(seen["orders"]) == 24
    wide = sa.StrongAugmentation(1.5)                                                            # lower end: max(0, 1 - cj)
    assert all(0.0 <= wide.draw(rng, 4, 4)["brightness"] <= 2.5 for _ in range(50))


class _CountingRandom(random.Random):
    calls = 0

    def uniform(self, a, b):
        self.calls += 1
        return super().uniform(a, b)


def test_an_eraser_takes_ten_attempts_and_may_not_fit():
    eraser = sa.RandomErasing(1.0, (0.9, 1.0), (0.01, 0.011))       # 90 % of the area at 1 : 100: wider than any 8 x 8 image
    rng = _CountingRandom(1)
    assert eraser.get_params(rng, 8, 8) is None and rng.calls == 20  # ten attempts, two uniform draws each
    rng = _CountingRandom(2)
    rect = sa.RandomErasing(1.0, (0.05, 0.2), (0.3, 3.3)).get_params(rng, 40, 40)
    assert rect is not None and rng.calls == 2
    aug = sa.StrongAugmentation(erasers=[eraser])
    assert aug.draw(random.Random(3), 8, 8)["erase"] == [None]
    assert sa.StrongAugmentation(erasers=[sa.RandomErasing(0.0, (0.05, 0.2), (0.3, 3.3))]).draw(random.Random(3), 40, 40)["erase"] == [None]
    # eh < h and ew < w, strictly: on one row nothing fits
    assert sa.RandomErasing(1.0, (0.02, 0.2), (0.3, 3.3)).get_params(random.Random(4), 1, 50) is None


def _dict(rng):
    return {"image_raw": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), "height": 37, "width": 53, "image_id": 7,
            "annotations": [{"bbox": [4.0, 5.0, 20.0, 10.0], "bbox_mode": data.XYWH_ABS, "category_id": 3}],
            "caption": ["a first caption", "a second caption"]}


@pytest.mark.parametrize("key,value", [("COLOR_JITTER", 0.4), ("RANDOM_GRAY_SCALE", True), ("GAUSSIAN_BLUR", True), ("RANDOM_ERASE", True)])
def test_without_train_aug_the_keys_stay_refused(key, value):
    cfg = _cfg(**{key: value})
    for build in (lambda: data.build_augmentation(cfg, True), lambda: data.DatasetMapper(cfg, True), lambda: data.DatasetMapper(cfg, True, train_aug=None),
                  lambda: data.CocoImageDatasetMapper(cfg, {}, True), lambda: data.get_mapper("lvis_v1_train", cfg, True)):
        with pytest.raises(NotImplementedError, match=key):
            build()
    aug = sa.build_complete_augmentation(cfg, True)
    assert data.DatasetMapper(cfg, True, "cpu", 0, train_aug=aug).train_aug is aug
    assert data.get_mapper("lvis_v1_train", cfg, True, device="cpu", train_aug=aug).train_aug is aug
    assert data.get_mapper("coco_2017_train", cfg, True, metadata={}, device="cpu", train_aug=aug).train_aug is aug
    cfg.merge_from_dict({"INPUT": {"CROP": {"ENABLED": True}}})
    with pytest.raises(NotImplementedError, match="CROP"):
        data.DatasetMapper(cfg, True, "cpu", 0, train_aug=aug)


def test_a_replayed_sample_reproduces_a_strong_batch():
    cfg = _cfg(MIN_SIZE_TRAIN=(40, 48, 64), MAX_SIZE_TRAIN=90, **ALL_ON)
    aug = sa.build_complete_augmentation(cfg, True)
    mapper = data.DatasetMapper(cfg, True, device="cpu", seed=11, train_aug=aug)
    plain = data.DatasetMapper(_cfg(MIN_SIZE_TRAIN=(40, 48, 64), MAX_SIZE_TRAIN=90), True, device="cpu", seed=11)
    rng = np.random.default_rng(1)
    dicts = [_dict(rng) for _ in range(8)]
    sample = mapper.draw_sample(dicts)
    assert set(sample) == {"short_edge", "flip", "caption", "strong", "erase_seed"} and len(sample["strong"]) == 8
    assert set(plain.draw_sample(dicts)) == {"short_edge", "flip", "caption"}
    first, again = mapper.map_batch(dicts, sample), mapper.map_batch(dicts, sample)
    base = plain.map_batch(dicts, {k: sample[k] for k in ("short_edge", "flip", "caption")})
    noise = mapper.erase_noise(sample).numpy()
    gen = torch.Generator(device="cpu")
    gen.manual_seed(sample["erase_seed"])
    assert np.array_equal(noise, torch.randn(noise.size, generator=gen).numpy())
    at, changed = 0, 0
    for a, b, p, s in zip(first, again, base, sample["strong"]):
        assert torch.equal(a["image"], b["image"]) and a["image"].dtype == torch.uint8 and a["image"].shape == p["image"].shape
        assert tuple(a["image"].shape[1:]) == a["instances"].image_size
        n = sa.noise_count(s)
        want = sa.apply_host(p["image"].numpy().transpose(1, 2, 0), s, noise[at:at + n])
        at += n
        assert np.array_equal(a["image"].numpy(), want.transpose(2, 0, 1))
        changed += not torch.equal(a["image"], p["image"])
        assert torch.equal(a["instances"].gt_boxes.tensor, p["instances"].gt_boxes.tensor) and a["caption"] == p["caption"]
    assert changed >= 6 and at == noise.size
    given = dict(sample, erase_noise=torch.from_numpy(noise.copy()), erase_seed=0)                # carried noise wins over the seed
    assert all(torch.equal(a["image"], b["image"]) for a, b in zip(first, mapper.map_batch(dicts, given)))
    # inference: train_aug is not applied and nothing is drawn for it
    test_mapper = data.DatasetMapper(cfg, False, device="cpu", seed=11, train_aug=aug)
    assert test_mapper.train_aug is None and set(test_mapper.draw_sample(dicts)) == {"short_edge", "flip", "caption"}


def test_the_draws_follow_the_image_the_batch_will_hold(tmp_path, monkeypatch):
    """A file is decoded once, by draw_sample; a file whose header parses but whose decode fails takes the reference's black-image
    fallback at the dict's size, and the erasers are drawn for THAT size."""
    Image = pytest.importorskip("PIL.Image")
    rgb = sc.content(30, 44, "file")
    Image.fromarray(rgb, "RGB").save(tmp_path / "good.png")
    whole = (tmp_path / "good.png").read_bytes()
    (tmp_path / "cut.png").write_bytes(whole[:len(whole) // 2])
    with Image.open(tmp_path / "cut.png") as im:
        assert im.size == (44, 30)                                  # the header alone still parses
    cfg = _cfg(MIN_SIZE_TRAIN=(0,), FORMAT="RGB", RANDOM_ERASE=True, GAUSSIAN_BLUR=True)
    aug = sa.build_complete_augmentation(cfg, True)
    for eraser in aug.erasers:
        eraser.p = 1.0
    mapper = data.DatasetMapper(cfg, True, device="cpu", seed=4, train_aug=aug)
    reads = []
    plain_read = data._read_file
    monkeypatch.setattr(data, "_read_file", lambda path, fmt: (reads.append(path), plain_read(path, fmt))[1])
    dicts = [{"file_name": str(tmp_path / "good.png"), "caption": ["a", "b"]},
             {"file_name": str(tmp_path / "cut.png"), "height": 12, "width": 70, "caption": ["a", "b"]},
             {"file_name": str(tmp_path / "missing.png"), "height": 9, "width": 8, "caption": ["a", "b"]}]
    sample = mapper.draw_sample(dicts)
    out = mapper.map_batch(dicts, sample)
    assert reads == [d["file_name"] for d in dicts] and mapper._decoded == {}                     # each decoded (or tried) once
    assert [tuple(o["image"].shape) for o in out] == [(3, 30, 44), (3, 12, 70), (3, 9, 8)]
    assert [o["caption"] for o in out[1:]] == ["A black image."] * 2 and out[0]["caption"] in ("a", "b")
    for s, (h, w) in zip(sample["strong"], [(30, 44), (12, 70), (9, 8)]):
        assert all(e is None or (e[0] + e[2] <= h and e[1] + e[3] <= w) for e in s["erase"])
    again = mapper.map_batch(dicts, sample)                                                       # a replay reads the files itself
    assert all(torch.equal(a["image"], b["image"]) for a, b in zip(out, again)) and len(reads) == 6


def test_train_aug_none_leaves_the_stream_of_draws_alone():
    cfg = _cfg(MIN_SIZE_TRAIN=(40, 48, 64), MAX_SIZE_TRAIN=90)
    rng = np.random.default_rng(2)
    dicts = [_dict(rng) for _ in range(4)]
    a = data.DatasetMapper(cfg, True, device="cpu", seed=3)
    b = data.DatasetMapper(cfg, True, device="cpu", seed=3, train_aug=None)
    for _ in range(3):
        sa_, sb = a.draw_sample(dicts), b.draw_sample(dicts)
        assert sa_ == sb
        assert all(torch.equal(x["image"], y["image"]) for x, y in zip(a.map_batch(dicts, sa_), b.map_batch(dicts, sb)))
