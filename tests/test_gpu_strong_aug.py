"""csrc/image_augment.hip on the device: ops.augment_images against locov_amd.strong_augment.apply_host (the definition, itself
pinned to Pillow's bytes by tests/test_strong_aug_host.py), and DatasetMapper with train_aug on the device against its host path.
Every comparison is exact equality of bytes.  Outputs are carved from one buffer pre-filled with 0xA5, with a guard region behind
each: every output byte must be written and no guard byte touched."""
import numpy as np
import pytest
import torch

import strong_aug_cases as sc
from locov_amd import strong_augment as sa

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _planar(img):
    return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda()


def _run(pkg, images, draws, noise=None, want=None):
    """One call for the batch (HWC numpy images); checks every output byte against the definition and every guard byte, and that
    a second call gives the same bits.  Image i's noise block follows image i - 1's."""
    counts = [sa.noise_count(d) for d in draws]
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int)
    noise = np.zeros(0, np.float32) if noise is None else noise
    assert noise.size >= sum(counts)
    if want is None:
        want = [sa.apply_host(x, d, noise[o:o + c]) for x, d, o, c in zip(images, draws, offsets, counts)]
    dev = [_planar(x) for x in images]
    lengths = [x.size for x in images]
    buf = torch.full((sum(lengths) + GUARD * len(images),), FILL, dtype=torch.uint8, device="cuda")
    outs, at = [], 0
    for n, x in zip(lengths, images):
        outs.append(buf[at:at + n].view(3, x.shape[0], x.shape[1]))
        at += n + GUARD
    dev_noise = torch.from_numpy(noise).cuda() if sum(counts) else None
    got = pkg.ops.augment_images(dev, draws, dev_noise, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    expect = np.full(buf.numel(), FILL, dtype=np.uint8)
    at = 0
    for n, w in zip(lengths, want):
        expect[at:at + n] = w.transpose(2, 0, 1).reshape(-1)
        at += n + GUARD
    first = buf.cpu().numpy()
    bad = np.flatnonzero(first != expect)
    assert bad.size == 0, f"{bad.size} differing bytes, the first at {bad[:5]} (got {first[bad[:5]]}, want {expect[bad[:5]]})"
    for x, d in zip(images, dev):
        assert np.array_equal(d.cpu().numpy(), x.transpose(2, 0, 1))          # the inputs are untouched
    fresh = pkg.ops.augment_images(dev, draws, dev_noise)
    assert all(torch.equal(f, o) for f, o in zip(fresh, outs))
    return want


@pytest.mark.parametrize("size", sc.SIZES)
def test_blur_at_every_sigma(pkg, size):
    h, w = size
    plain = sc.content(h, w, f"gpu-blur{size}")
    _run(pkg, [plain] * len(sc.SIGMAS), [sc.draws(sigma=s) for s in sc.SIGMAS])
    smooth = sc.content(h, w, f"gpu-blur-jitter{size}", "smooth")
    _run(pkg, [smooth] * len(sc.SIGMAS), [sc.draws(sc.PERMUTATIONS[7 + n], sc.FACTOR_SETS[n % 2], gray=n == 3, sigma=s)
                                          for n, s in enumerate(sc.SIGMAS)])


@pytest.mark.parametrize("size", sc.SIZES)
def test_jitter_without_blur_at_every_size(pkg, size):
    h, w = size
    img = sc.content(h, w, f"gpu-jitter{size}")
    _run(pkg, [img] * 4, [sc.draws(sc.PERMUTATIONS[n * 5], sc.FACTOR_SETS[n % 3]) for n in range(4)])


def test_every_permutation(pkg):
    """All 24 orders at the three factor sets, on several tiles with partial edges and three contrast partials."""
    images = {kind: sc.content(70, 150, "gpu-permutations", kind) for kind in ("random", "smooth")}
    cases = [(images["random" if n % 2 else "smooth"], sc.draws(p, f)) for n, p in enumerate(sc.PERMUTATIONS) for f in sc.FACTOR_SETS]
    assert len(cases) == 72
    for lo in range(0, len(cases), sc.MAX_IMAGES):
        part = cases[lo:lo + sc.MAX_IMAGES]
        _run(pkg, [x for x, _ in part], [d for _, d in part])


def test_contrast_alone_first_and_last(pkg):
    img = sc.content(70, 150, "gpu-contrast", "smooth")
    orders = [[sc.CONTRAST], [sc.CONTRAST, sc.BRIGHTNESS, sc.SATURATION, sc.HUE], [sc.BRIGHTNESS, sc.SATURATION, sc.HUE, sc.CONTRAST]]
    _run(pkg, [img] * 6, [sc.draws(o, f) for o in orders for f in sc.FACTOR_SETS[:2]])
    big = sc.content(131, 257, "gpu-contrast-big")                                  # nine partials, the last one short
    want = _run(pkg, [big], [sc.draws([sc.CONTRAST], (1.0, 0.25, 1.0, 0.0))])
    mean = sa.contrast_mean(big)
    assert abs(int(want[0].astype(np.int64).mean()) - mean) <= 2 and want[0].std() < big.std() / 3


@pytest.mark.parametrize("value", [0, 255])
def test_constant_images_through_every_operation(pkg, value):
    img = sc.content(33, 70, None, value)
    ds = [sc.draws([op], f) for op in (sc.BRIGHTNESS, sc.CONTRAST, sc.SATURATION, sc.HUE) for f in sc.FACTOR_SETS[:2]]
    ds += [sc.draws(gray=True), sc.draws(sigma=2.0), sc.draws(sigma=0.1), sc.draws(sc.PERMUTATIONS[11], sc.FACTOR_SETS[1], gray=True, sigma=1.3)]
    want = _run(pkg, [img] * len(ds), ds)
    assert (want[-3] == value).all() and (want[-2] == value).all()                  # 255 through the blur stays 255


@pytest.fixture(scope="module")
def every_colour():
    """The 4096 x 4096 image of all 2^24 colours (no subsampling) and its HSV form by the definition, computed once; a shift then
    costs the definition one HSV -> RGB pass."""
    v = np.arange(1 << 24, dtype=np.uint32)
    colours = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    return colours, sa.rgb_to_hsv(colours), _planar(colours)


@pytest.mark.parametrize("shift", [-25, 0, 25])
def test_hue_only_over_every_colour(pkg, every_colour, shift):
    colours, hsv, dev = every_colour
    shifted = hsv.copy()
    shifted[..., 0] = (hsv[..., 0].astype(np.int32) + shift) & 255
    want = sa.hsv_to_rgb(shifted)
    hue = shift / 255.0
    assert sa.hue_shift(hue) == shift & 255
    got = pkg.ops.augment_images([dev], [sc.draws([sc.HUE], (1.0, 1.0, 1.0, hue))])[0].permute(1, 2, 0).cpu().numpy()
    bad = np.count_nonzero(got != want)
    assert bad == 0, f"{bad} differing bytes of {want.size}"


def test_grayscale_with_and_without_jitter(pkg):
    img = sc.content(70, 150, "gpu-gray")
    want = _run(pkg, [img] * 3, [sc.draws(gray=True), sc.draws(sc.PERMUTATIONS[20], sc.FACTOR_SETS[0], gray=True),
                                 sc.draws(sc.PERMUTATIONS[2], sc.FACTOR_SETS[1], gray=True)])
    assert all((w[..., 0] == w[..., 1]).all() and (w[..., 1] == w[..., 2]).all() for w in want)


def test_erasers(pkg):
    h, w = 70, 150
    img = sc.content(h, w, "gpu-erase")
    edge = [(h - 20, w - 31, 20, 31)]                                                # its last row and column are the image's
    three = [(5, 10, 30, 40), (20, 30, 30, 100), (25, 35, 40, 10)]                   # overlapping: the later wins
    cases = [sc.draws(erase=[None, None, None]), sc.draws(erase=edge), sc.draws(erase=three), sc.draws(erase=[None, three[1], None]),
             sc.draws(sc.PERMUTATIONS[6], sc.FACTOR_SETS[0], gray=True, sigma=2.0, erase=three), sc.draws(sigma=1.3, erase=edge),
             sc.draws(erase=[(0, 0, 0, 5), (1, 1, 69, 149)])]                        # an empty rectangle; the largest one that fits
    noise = sc.noise(sum(sa.noise_count(d) for d in cases), "gpu-erase")
    want = _run(pkg, [img] * len(cases), cases, noise)
    assert np.array_equal(want[0], img) and np.array_equal(want[1][:h - 20], img[:h - 20]) and (want[1][h - 1, w - 1] != img[h - 1, w - 1]).any()
    first = 3 * 20 * 31
    block = sa.noise_bytes(noise[first + 3 * (30 * 40 + 30 * 100):first + sa.noise_count(cases[2])]).reshape(3, 40, 10)
    assert np.array_equal(want[2][25:65, 35:45], block.transpose(1, 2, 0))


def test_five_images_of_mixed_sizes_and_groups(pkg):
    sizes = [(1, 1), (37, 53), (70, 150), (33, 65), (9, 200)]
    ds = [sc.draws(sc.PERMUTATIONS[13], sc.FACTOR_SETS[0]),
          sc.draws(sigma=0.45, erase=[(1, 2, 30, 40)]),
          sc.draws(sc.PERMUTATIONS[4], sc.FACTOR_SETS[1], gray=True, sigma=2.0, erase=[(0, 0, 10, 10), None, (60, 100, 10, 50)]),
          sc.draws(gray=True),
          sc.draws()]                                                                # nothing applied: a copy
    noise = sc.noise(sum(sa.noise_count(d) for d in ds), "gpu-mixed")
    images = [sc.content(h, w, f"gpu-mixed{n}", "smooth" if n % 2 else "random") for n, (h, w) in enumerate(sizes)]
    want = _run(pkg, images, ds, noise)
    assert np.array_equal(want[4], images[4])


def test_the_maximum_number_of_images(pkg):
    rng = np.random.default_rng(64)
    images, ds = [], []
    for n in range(sc.MAX_IMAGES):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 81))
        images.append(sc.content(h, w, f"gpu-max{n}", "smooth" if n % 3 == 0 else "random"))
        erase = [(h // 3, w // 4, h // 2, w // 2)] if n % 4 == 1 else []
        ds.append(sc.draws(sc.PERMUTATIONS[n % 24] if n % 5 else (), sc.FACTOR_SETS[n % 3], gray=n % 7 == 0,
                           sigma=sc.SIGMAS[n % 5] if n % 2 else None, erase=erase))
    noise = sc.noise(sum(sa.noise_count(d) for d in ds), "gpu-max")
    _run(pkg, images, ds, noise)
    with pytest.raises(ValueError, match="at most"):
        pkg.ops.augment_images([_planar(images[0])] * (sc.MAX_IMAGES + 1), [ds[0]] * (sc.MAX_IMAGES + 1))


def test_what_the_wrapper_refuses(pkg):
    dev = _planar(sc.content(9, 11, "gpu-refuse"))
    assert pkg.ops.augment_supported(2.0) and pkg.ops.augment_supported(0.1) and not pkg.ops.augment_supported(2.5)
    with pytest.raises(ValueError, match="augment_supported"):
        pkg.ops.augment_images([dev], [sc.draws(sigma=2.5)])
    with pytest.raises(ValueError, match="noise"):
        pkg.ops.augment_images([dev], [sc.draws(erase=[(0, 0, 3, 3)])])
    with pytest.raises(ValueError, match="noise"):
        pkg.ops.augment_images([dev], [sc.draws(erase=[(0, 0, 3, 3)])], torch.zeros(26, device="cuda"))
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        pkg.ops.augment_images([dev[:2]], [sc.draws()])
    with pytest.raises(ValueError, match="not the image itself"):
        pkg.ops.augment_images([dev], [sc.draws()], out=[dev])
    with pytest.raises(pkg._lib.LocovError, match="leaves the image"):
        pkg.ops.augment_images([dev], [sc.draws(erase=[(5, 5, 5, 5)])], torch.zeros(75, device="cuda"))


# ---- the mapper ----------------------------------------------------------------------------------------------------------------

def _cfg(device, **inp):
    from locov_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.DEVICE = device
    for k, v in dict(MIN_SIZE_TRAIN=(40, 48, 64), MAX_SIZE_TRAIN=90, **inp).items():
        cfg.INPUT[k] = v
    return cfg


ALL_ON = dict(COLOR_JITTER=0.4, RANDOM_GRAY_SCALE=True, GAUSSIAN_BLUR=True, RANDOM_ERASE=True)


def _dicts(n, seed):
    rng = np.random.default_rng(seed)
    return [{"image_raw": rng.integers(0, 256, (37 + i, 53 + 2 * i, 3), dtype=np.uint8), "image_id": i,
             "annotations": [{"bbox": [4.0, 5.0, 20.0, 10.0], "bbox_mode": 1, "category_id": 3}], "caption": ["one", "two"]} for i in range(n)]


def test_map_batch_on_the_device_equals_the_host_path(pkg, monkeypatch):
    from locov_amd import data
    cfg = _cfg("cuda", **ALL_ON)
    aug = sa.build_complete_augmentation(cfg, True)
    on_device = data.DatasetMapper(cfg, True, device="cuda", seed=5, train_aug=aug)
    on_host = data.DatasetMapper(cfg, True, device="cpu", seed=5, train_aug=aug)
    dicts = _dicts(10, 3)
    sample = on_device.draw_sample(dicts)
    assert sum(s["jitter"] for s in sample["strong"]) and sum(s["blur"] for s in sample["strong"]) and sum(
        any(e is not None for e in s["erase"]) for s in sample["strong"])
    noise = on_device.erase_noise(sample)
    assert noise.is_cuda and noise.numel() == sum(sa.noise_count(s) for s in sample["strong"]) > 0
    assert torch.equal(noise, on_device.erase_noise(sample))                        # the seed replays it
    launches = pkg._lib.load().locov_launch_count()
    got = on_device.map_batch(dicts, sample)
    assert pkg._lib.load().locov_launch_count() - launches <= 3                     # the resize's one and the augmentation's two
    want = on_host.map_batch(dicts, dict(sample, erase_noise=noise.cpu()))          # the noise is copied back for the host side
    for g, w in zip(got, want):
        assert g["image"].is_cuda and torch.equal(g["image"].cpu(), w["image"])
        assert torch.equal(g["instances"].gt_boxes.tensor.cpu(), w["instances"].gt_boxes.tensor) and g["caption"] == w["caption"]
    assert all(torch.equal(a["image"], b["image"]) for a, b in zip(got, on_device.map_batch(dicts, sample)))
    # a sigma the kernel does not take is served by the host definition, image by image
    wide = dict(sample, strong=[dict(s, blur=True, sigma=2.5 + 0.1 * i) if i % 2 else s for i, s in enumerate(sample["strong"])])
    got = on_device.map_batch(dicts, wide)
    want = on_host.map_batch(dicts, dict(wide, erase_noise=noise.cpu()))
    assert all(g["image"].is_cuda and torch.equal(g["image"].cpu(), w["image"]) for g, w in zip(got, want))
    monkeypatch.setenv("LOCOV_FUSED_AUGMENT", "0")
    launches = pkg._lib.load().locov_launch_count()
    off = on_device.map_batch(dicts, sample)
    assert pkg._lib.load().locov_launch_count() - launches == 1                     # the resize alone
    assert all(torch.equal(a["image"], b["image"]) for a, b in zip(off, on_device.map_batch(dicts, dict(sample, erase_noise=noise))))


def test_without_train_aug_the_bytes_are_the_existing_path(pkg):
    from locov_amd import data
    cfg = _cfg("cuda")
    dicts = _dicts(6, 4)
    plain = data.DatasetMapper(cfg, True, device="cuda", seed=9)
    none = data.DatasetMapper(cfg, True, device="cuda", seed=9, train_aug=None)
    built = data.DatasetMapper(cfg, True, device="cuda", seed=9, train_aug=sa.build_complete_augmentation(cfg, True))     # all off: None
    sample = plain.draw_sample(dicts)
    assert none.draw_sample(dicts) == sample == built.draw_sample(dicts) and set(sample) == {"short_edge", "flip", "caption"}
    launches = pkg._lib.load().locov_launch_count()
    want = plain.map_batch(dicts, sample)
    assert pkg._lib.load().locov_launch_count() - launches == 1
    for other in (none, built):
        assert all(torch.equal(a["image"], b["image"]) for a, b in zip(want, other.map_batch(dicts, sample)))
    # identity draws through the kernel are a copy of the existing path's bytes
    same = pkg.ops.augment_images([w["image"] for w in want], [sc.draws() for _ in want])
    assert all(torch.equal(a, w["image"]) for a, w in zip(same, want))


def test_a_batch_past_one_call_with_a_host_image_in_each_stage(pkg, monkeypatch):
    """The mapper's own dispatch: IMAGE_BATCH_MAX_IMAGES + 2 images, one outside ops.resize_supported and another outside
    ops.augment_supported.  Each stage sends 64 and 1 images through its op and one through the host definition, and every
    image is the CPU mapper's, byte for byte."""
    import random
    from locov_amd import data
    cfg = _cfg("cuda", **ALL_ON)
    cfg.INPUT.MIN_SIZE_TRAIN = (10, 14, 20)
    aug = sa.build_complete_augmentation(cfg, True)
    on_device = data.DatasetMapper(cfg, True, device="cuda", seed=21, train_aug=aug)
    on_host = data.DatasetMapper(cfg, True, device="cpu", seed=21, train_aug=aug)
    n, big, wide = pkg.ops.IMAGE_BATCH_MAX_IMAGES + 2, 40, 13
    rng = np.random.default_rng(8)
    dicts = [{"image_raw": rng.integers(0, 256, (90, 90, 3) if i == big else (12 + i % 3, 16 + i % 5, 3), dtype=np.uint8), "image_id": i}
             for i in range(n)]
    sample = on_device.draw_sample(dicts)
    sample["short_edge"][big] = 10                                                   # 90 -> 10: 19 taps a side
    sample["strong"][big] = aug.draw(random.Random(3), 10, 10)
    sample["strong"][wide] = dict(sample["strong"][wide], blur=True, sigma=3.0)
    assert not pkg.ops.resize_supported((90, 90), (10, 10), 3) and not pkg.ops.augment_supported(3.0)
    assert all(pkg.ops.augment_supported(s["sigma"]) for i, s in enumerate(sample["strong"]) if s["blur"] and i != wide)
    sample["erase_noise"] = on_device.erase_noise(sample).cpu()
    want = on_host.map_batch(dicts, sample)
    calls = {"resize_flip_images": [], "augment_images": []}
    for name, seen in calls.items():
        monkeypatch.setattr(pkg.ops, name, lambda images, *a, _op=getattr(pkg.ops, name), _seen=seen, **k: (_seen.append(len(images)), _op(images, *a, **k))[1])
    got = on_device.map_batch(dicts, sample)
    assert calls == {"resize_flip_images": [64, 1], "augment_images": [64, 1]}
    assert len(got) == n and tuple(got[big]["image"].shape) == (3, 10, 10)
    for g, w in zip(got, want):
        assert g["image"].is_cuda and g["image"].dtype == torch.uint8 and torch.equal(g["image"].cpu(), w["image"])
