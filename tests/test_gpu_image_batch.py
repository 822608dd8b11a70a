"""csrc/image_batch.hip on the device: ops.preprocess_images against the CPU torch expression (x - pixel_mean) / pixel_std followed
by ImageList.from_tensors, and ops.detector_rescale against the CPU chain Boxes.scale -> Boxes.clip -> Boxes.nonempty.  Every
comparison is of int32 bit patterns: both kernels are specified to give the torch ops' bits."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

MEAN, STD = [103.530, 116.280, 123.675], [57.375, 57.12, 58.395]          # a pixel_std far from 1: the division rounds


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _draw(sizes, dtype, channels=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return [torch.randint(0, 256, (channels, h, w), dtype=torch.uint8, generator=g) for h, w in sizes]
    return [torch.rand((channels, h, w), generator=g) * 255.0 for h, w in sizes]      # (x - mean is 0 or far above the subnormals)


def _reference(pkg, images, mean, std, divisibility=0, pad_value=0.0, constraints=None):
    """The definition, on the CPU."""
    m, s = torch.tensor(mean).view(-1, 1, 1), torch.tensor(std).view(-1, 1, 1)
    return pkg.structures.ImageList.from_tensors([(x - m) / s for x in images], divisibility, pad_value, constraints)


def _check_preprocess(pkg, images, mean=MEAN, std=STD, divisibility=0, pad_value=0.0, constraints=None, device_images=None):
    want = _reference(pkg, images, mean, std, divisibility, pad_value, constraints)
    dev = device_images if device_images is not None else [x.cuda() for x in images]
    out = torch.full(tuple(want.tensor.shape), float("nan"), device="cuda")                  # NaN shows an element nobody wrote
    got, sizes = pkg.ops.preprocess_images(dev, mean, std, divisibility, pad_value, constraints, out=out)
    assert got is out and sizes == want.image_sizes and tuple(got.shape) == tuple(want.tensor.shape)
    assert not torch.isnan(got).any()
    assert torch.equal(_bits(got), _bits(want.tensor))
    again, _ = pkg.ops.preprocess_images(dev, mean, std, divisibility, pad_value, constraints)     # a fresh torch.empty
    assert torch.equal(_bits(again), _bits(want.tensor))
    return want


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["uint8", "fp32"])
@pytest.mark.parametrize("sizes,divisibility,pad_value", [
    ([(16, 16)], 0, 0.0),                                                 # N = 1, nothing padded
    ([(37, 53)], 0, 0.0),                                                 # N = 1, rows of 53: no quad is row-aligned
    ([(37, 53), (40, 41), (5, 64)], 0, 0.0),
    ([(37, 53), (40, 41), (5, 64)], 32, 0.0),
    ([(37, 53), (40, 41), (5, 64)], 32, -3.25),
    ([(37, 53), (40, 41)], 0, 1.5),                                       # batch width 53: not a multiple of 4
    ([(9, 1), (1, 11)], 0, 0.0),                                          # one pixel wide, one pixel high; 2 * 3 * 9 * 11 % 4 != 0
    ([(9, 1), (1, 11)], 0, 7.0),
    ([(3, 3)], 0, 0.0),                                                   # 27 elements: the last quad is cut short
], ids=["1img", "1img_w53", "3img", "3img_div32", "3img_div32_pad", "2img_w53_pad", "thin", "thin_pad", "tail"])
def test_preprocess_images_gives_the_bits_of_the_torch_expression(pkg, dtype, sizes, divisibility, pad_value):
    _check_preprocess(pkg, _draw(sizes, dtype, seed=len(sizes) + divisibility), divisibility=divisibility, pad_value=pad_value)


@pytest.mark.parametrize("dtype,channels,sizes", [
    (torch.uint8, 3, [(611, 1013), (640, 801), (333, 1001)]),             # 5.8e6 elements in rows of 1013
    (torch.float32, 4, [(181 - i % 3, 183 - i % 5) for i in range(64)]),  # 8.5e6 elements in the most planes a call can have, 256
], ids=["large_rows", "many_planes"])
def test_preprocess_images_over_thousands_of_workgroups(pkg, dtype, channels, sizes):
    """Sizes near the real ones: every wave of 5 000 and more workgroups finds its plane, row and column."""
    _check_preprocess(pkg, _draw(sizes, dtype, channels=channels, seed=channels), mean=MEAN[:channels] + [99.5] * (channels - 3),
                      std=STD[:channels] + [61.25] * (channels - 3), pad_value=0.5)


def test_preprocess_images_is_exhaustive_over_uint8(pkg):
    """One 3 x 16 x 16 image holding all 256 values in every channel: every (value, channel) pair the kernel can meet."""
    image = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).repeat(3, 1, 1)
    image[1] = image[1].flip(-1)
    image[2] = image[2].t().clone()
    assert all(len(torch.unique(image[c])) == 256 for c in range(3))
    _check_preprocess(pkg, [image])
    _check_preprocess(pkg, [image], mean=[0.0, 0.0, 0.0], std=[255.0, 3.0, 0.1])


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["uint8", "fp32"])
def test_preprocess_images_reads_a_source_at_an_odd_offset(pkg, dtype):
    """A contiguous view that starts one element into its storage: an odd byte for uint8, 4 bytes off a 16-byte line for fp32."""
    images = _draw([(21, 40), (24, 37)], dtype, seed=7)
    dev = []
    for k, x in enumerate(images):
        store = torch.zeros(x.numel() + 8, dtype=dtype, device="cuda")
        view = store[1 + 2 * k:1 + 2 * k + x.numel()].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 == (1 + 2 * k) * x.element_size()
        dev.append(view)
    _check_preprocess(pkg, images, device_images=dev)


def test_preprocess_images_channel_counts_square_size_and_limits(pkg):
    _check_preprocess(pkg, _draw([(7, 9), (8, 5)], torch.uint8, channels=1), mean=[10.0], std=[3.0])
    _check_preprocess(pkg, _draw([(7, 9), (8, 5)], torch.float32, channels=4), mean=[1.0, 2.0, 3.0, 4.0], std=[3.0, 5.0, 7.0, 9.0], pad_value=2.0)
    _check_preprocess(pkg, _draw([(7, 9), (8, 5)], torch.uint8), constraints={"square_size": 20, "size_divisibility": 8})
    sizes = [(1 + i % 5, 1 + i % 7) for i in range(64)]                   # the most images one call takes
    _check_preprocess(pkg, _draw(sizes, torch.uint8, seed=64))
    with pytest.raises(ValueError, match="limits"):
        pkg.ops.preprocess_images([x.cuda() for x in _draw(sizes + [(2, 2)], torch.uint8)], MEAN, STD)
    with pytest.raises(ValueError, match="limits"):
        pkg.ops.preprocess_images([torch.zeros(5, 4, 4, device="cuda")], [0.0] * 5, [1.0] * 5)
    with pytest.raises(TypeError):
        pkg.ops.preprocess_images([torch.zeros(3, 4, 4, device="cuda"), torch.zeros(3, 4, 4, dtype=torch.uint8, device="cuda")], MEAN, STD)


class _NoBackbone(nn.Module):
    size_divisibility = 32
    padding_constraints = {}


def test_preprocess_image_chooses_the_kernel_or_the_torch_expression(pkg, monkeypatch):
    """model.preprocess_image: 64 device images of one dtype go through the kernel; 65 images, or mixed dtypes, through the torch
    expression -- and give the bits the kernel would."""
    model = pkg.GeneralizedRCNN(backbone=_NoBackbone(), proposal_generator=None, roi_heads=nn.Identity(), pixel_mean=MEAN, pixel_std=STD).cuda()
    assert model.device.type == "cuda"
    calls = []
    real = pkg.ops.preprocess_images
    monkeypatch.setattr(pkg.ops, "preprocess_images", lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
    sizes = [(3 + i % 5, 2 + i % 7) for i in range(65)]
    images = _draw(sizes, torch.uint8, seed=65)
    want = _reference(pkg, images, MEAN, STD, 32)
    got = model.preprocess_image([{"image": x} for x in images[:64]])              # CPU inputs are moved to the model's device
    assert calls == [64] and got.tensor.is_cuda and got.image_sizes == want.image_sizes[:64]
    assert torch.equal(_bits(got.tensor), _bits(want.tensor[:64]))
    got = model.preprocess_image([{"image": x.cuda()} for x in images])
    assert calls == [64] and got.image_sizes == want.image_sizes                     # 65 images: the torch expression
    assert torch.equal(_bits(got.tensor), _bits(want.tensor))
    mixed = [images[0], images[1].float(), images[2]]
    got = model.preprocess_image([{"image": x} for x in mixed])
    assert calls == [64]
    assert torch.equal(_bits(got.tensor), _bits(_reference(pkg, mixed, MEAN, STD, 32).tensor))
    got = model.preprocess_image([{"image": x.float()} for x in images[:3]])         # fp32 of one dtype: the kernel again
    assert calls == [64, 3]
    assert torch.equal(_bits(got.tensor), _bits(_reference(pkg, [x.float() for x in images[:3]], MEAN, STD, 32).tensor))


# ------------------------------------------------------------------------------------------------------ detector_rescale

def _boxes(n, size, seed):
    """n XYXY boxes around an (h, w) image: most inside, some hanging over an edge, some outside, some of zero width / height."""
    g = torch.Generator().manual_seed(seed)
    h, w = size
    xy = torch.rand(n, 2, generator=g) * torch.tensor([w * 1.3, h * 1.3]) - torch.tensor([w * 0.15, h * 0.15])
    wh = torch.rand(n, 2, generator=g) * torch.tensor([w * 0.4, h * 0.4])
    b = torch.cat([xy, xy + wh], dim=1)
    kind = torch.randint(0, 8, (n,), generator=g)
    b[kind == 0, 2] = b[kind == 0, 0]                                     # zero width
    b[kind == 1, 3] = b[kind == 1, 1]                                     # zero height
    return b


def _inside(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    h, w = size
    xy = torch.rand(n, 2, generator=g) * torch.tensor([w * 0.5, h * 0.5])
    return torch.cat([xy, xy + 1.0 + torch.rand(n, 2, generator=g) * torch.tensor([w * 0.4, h * 0.4])], dim=1)


def _outside(n, size, seed):
    b = _inside(n, size, seed)
    b[:, 0::2] += size[1] + 5.0                                           # right of the image: empty once clipped
    return b


def _cpu_chain(pkg, boxes, image_size, out_size):
    """Boxes.scale -> Boxes.clip -> Boxes.nonempty on the CPU, as detector_postprocess forms them."""
    b = pkg.structures.Boxes(boxes.clone())
    b.scale(out_size[1] / image_size[1], out_size[0] / image_size[0])
    b.clip(out_size)
    keep = b.nonempty()
    return b.tensor[keep], keep.nonzero().flatten()


def _check_rescale(pkg, per_image, image_sizes, out_sizes):
    sizes = [len(b) for b in per_image]
    cat = torch.cat(per_image).cuda() if per_image else torch.zeros(0, 4, device="cuda")
    out, src, counts = pkg.ops.detector_rescale(cat, sizes, image_sizes, out_sizes)
    assert tuple(out.shape) == (sum(sizes), 4) and src.dtype == torch.int64 and tuple(src.shape) == (sum(sizes),)
    assert isinstance(counts, list) and len(counts) == len(sizes)
    lo = 0
    for b, n, kept, isz, osz in zip(per_image, sizes, counts, image_sizes, out_sizes):
        want_boxes, want_rows = _cpu_chain(pkg, b, isz, osz)
        assert kept == len(want_rows)
        assert torch.equal(src[lo:lo + kept].cpu(), want_rows)                                  # the kept rows, in their order
        assert torch.equal(_bits(out[lo:lo + kept]), _bits(want_boxes))
        assert not _bits(out[lo + kept:lo + n]).any() and bool((src[lo + kept:lo + n] == -1).all())     # the tail: zeros, -1
        lo += n
    out2, src2, counts2 = pkg.ops.detector_rescale(cat, sizes, image_sizes, out_sizes)
    assert counts2 == counts and torch.equal(_bits(out2), _bits(out)) and torch.equal(src2, src)
    return counts


NET, SMALL = (800, 1333), (480, 640)                                      # 480 / 800, 640 / 1333: neither is an fp32 number


@pytest.mark.parametrize("rows", [1, 100, 1000])
@pytest.mark.parametrize("image_size,out_size", [(NET, SMALL), (SMALL, NET), (NET, NET)], ids=["down", "up", "same"])
def test_detector_rescale_one_image(pkg, rows, image_size, out_size):
    counts = _check_rescale(pkg, [_boxes(rows, image_size, rows)], [image_size], [out_size])
    if rows > 1:
        assert 0 < counts[0] < rows                                       # something is dropped, something is kept


def test_detector_rescale_batch_with_every_kind_of_image(pkg):
    nan_rows = _inside(300, NET, 3)
    nan_rows[5, 0] = float("nan")                                         # one NaN coordinate each: the row is dropped, as the chain drops it
    nan_rows[290, 3] = float("nan")
    per_image = [torch.zeros(0, 4), _outside(70, NET, 1), _inside(257, NET, 2), nan_rows, _boxes(1000, (600, 900), 4),
                 torch.zeros(0, 4), _boxes(513, SMALL, 5)]
    image_sizes = [NET, NET, NET, NET, (600, 900), SMALL, SMALL]
    out_sizes = [SMALL, SMALL, (1213, 2017), SMALL, (427, 640), NET, NET]
    counts = _check_rescale(pkg, per_image, image_sizes, out_sizes)
    assert counts[0] == 0 and counts[1] == 0 and counts[2] == 257 and counts[3] == 298 and counts[5] == 0
    assert 0 < counts[4] < 1000 and 0 < counts[6] < 513


def test_detector_rescale_64_images_and_no_rows(pkg):
    per_image = [_boxes(1 + 3 * i, NET, 100 + i) for i in range(64)]
    _check_rescale(pkg, per_image, [NET] * 64, [SMALL if i % 2 else (1000, 1666) for i in range(64)])
    assert _check_rescale(pkg, [torch.zeros(0, 4)] * 3, [NET] * 3, [SMALL] * 3) == [0, 0, 0]
    with pytest.raises(ValueError):
        pkg.ops.detector_rescale(torch.zeros(65, 4, device="cuda"), [1] * 65, [NET] * 65, [SMALL] * 65)
    with pytest.raises(ValueError):
        pkg.ops.detector_rescale(torch.zeros(5, 4, device="cuda"), [2, 2], [NET] * 2, [SMALL] * 2)


def test_postprocess_gathers_only_where_a_row_was_dropped(pkg):
    """GeneralizedRCNN._postprocess on device results: an image that loses nothing keeps its field tensors (no gather), the others
    hold the kept rows; all of it equals the single-image torch function."""
    Boxes, Instances = pkg.structures.Boxes, pkg.structures.Instances
    raw = [_inside(40, NET, 11), _boxes(90, NET, 12), _outside(8, NET, 13)]
    results = [Instances(NET, pred_boxes=Boxes(b.cuda()), scores=torch.rand(len(b)).cuda(), pred_classes=torch.arange(len(b)).cuda()) for b in raw]
    inputs = [{"height": 480, "width": 640}, {"height": 1213, "width": 2017}, {}]
    got = pkg.GeneralizedRCNN._postprocess(results, inputs, [NET] * 3)
    for g, r, (h, w) in zip(got, results, [(480, 640), (1213, 2017), NET]):
        g = g["instances"]
        want = pkg.detector_postprocess(r, h, w)
        assert type(g) is Instances and type(g.pred_boxes) is Boxes and g.image_size == (h, w) and len(g) == len(want)
        assert torch.equal(_bits(g.pred_boxes.tensor), _bits(want.pred_boxes.tensor))
        assert torch.equal(_bits(g.scores), _bits(want.scores)) and torch.equal(g.pred_classes, want.pred_classes)
    assert got[0]["instances"].scores is results[0].scores and len(got[0]["instances"]) == 40
    assert 0 < len(got[1]["instances"]) < 90 and len(got[2]["instances"]) == 0
    assert torch.equal(_bits(results[1].pred_boxes.tensor), _bits(raw[1]))          # the inputs are left as they were
