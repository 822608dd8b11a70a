"""The C4 backbone on the device: the fused stem kernel (csrc/resnet_stem.hip) against float64 element by element with
tests/split_ref.py's gate, its write footprint and launch-size independence, the whole R50-C4 on the device path against the
float64 restatement (tests/backbone_ref.py) with the project's end-to-end gate, and the path selection / the seam to the RPN and
the ROI heads."""
import pytest
import torch
import torch.nn.functional as F

import backbone_ref as br
import split_ref as sr

pytestmark = pytest.mark.gpu

# the end-to-end gate of tests/test_gpu_split_f64.py: device error against float64 <= LOGIT_MULT x the torch-fp32 CPU evaluation's own
# error + LOGIT_FLOOR x max |ref|.  Measured on an MI355X (docs/experiments.md, "ResNet C4 backbone on the device"): the device error is
# 1.86x the CPU evaluation's on 2 x 3 x 67 x 97 (7.68e-4 against 4.13e-4 at max |ref| 404) and 1.20x on 1 x 3 x 64 x 96 (6.78e-4 against
# 5.64e-4 at 327): under half of the allowance.
LOGIT_MULT = 4.0
LOGIT_FLOOR = 2.0 ** -20

STEM_CASES = [(1, 1, 1), (1, 2, 3), (1, 5, 8), (2, 37, 51), (1, 40, 64), (2, 38, 50), (3, 70, 131), (1, 129, 260)]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _stem(pkg, args, **kw):
    return pkg.ops.resnet_stem(*[a.cuda() for a in args], **kw)


def _gate(pkg, name, args):
    N, _, H, W = args[0].shape
    got = _stem(pkg, args)
    assert tuple(got.shape) == (N, (H + 3) // 4, (W + 3) // 4, 64) and got.is_contiguous() and got.dtype == torch.float32
    ref = br.stem(*args)
    q = sr.gate_ratio(got, ref)
    print(f"SPLITGATE stem[{name}] {q:.4f}")
    assert q <= 1.0, f"stem {name}: err / bound = {q:.3g}"
    return got, ref


@pytest.mark.parametrize("shape", STEM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_stem_against_float64(pkg, shape):
    _gate(pkg, "x".join(map(str, shape)), br.stem_inputs(*shape, seed=sum(shape)))


def test_stem_large_negative_shift_gives_exact_zero(pkg):
    args = br.stem_inputs(2, 37, 51, seed=7, variant="neg_shift")
    got, ref = _gate(pkg, "2x37x51 shift -1e3", args)
    assert float(got[..., [5, 17, 40]].abs().max()) == 0.0 and float(ref.ref[..., [5, 17, 40]].abs().max()) == 0.0
    assert float(got.max()) > 0


@pytest.mark.parametrize("shape", [(1, 40, 64), (2, 37, 51)], ids=lambda s: "x".join(map(str, s)))
def test_stem_single_pixels_at_the_corners(pkg, shape):
    args = br.stem_inputs(*shape, seed=11, variant="corners")
    got, ref = _gate(pkg, "x".join(map(str, shape)) + " corners", args)
    # away from the corners the convolution sees zeros only: relu(shift) exactly, on both sides
    mid = got[:, 3:-3, 3:-3, :].cpu()
    assert torch.equal(mid, torch.relu(args[3]).expand_as(mid))


@pytest.mark.parametrize("band", [4, 5, 7, 18])
def test_stem_band_height_does_not_change_a_bit(pkg, band, monkeypatch):
    """The launch picks the band of pooled rows a wave walks from the problem size (csrc/resnet_stem.hip stem_band); small inputs
    get bands of one row.  LOCOV_STEM_BAND forces taller ones: 4 (nine conv rows: a second patch of one row), 5, 7 (18 rows =
    7 + 7 + 4: a short last band) and 18 (the whole column, five patches) -- same bits, and the float64 gate again."""
    args = br.stem_inputs(2, 70, 131, seed=9)
    monkeypatch.delenv("LOCOV_STEM_BAND", raising=False)
    want = _stem(pkg, args)
    monkeypatch.setenv("LOCOV_STEM_BAND", str(band))
    got, _ = _gate(pkg, f"2x70x131 band {band}", args)
    assert torch.equal(got, want)


def test_stem_writes_nothing_outside_out(pkg):
    args = br.stem_inputs(2, 37, 51, seed=3)
    want = _stem(pkg, args)
    n, margin, fill = want.numel(), 4096, -7.25
    buf = torch.full((n + 2 * margin,), fill, device="cuda")
    out = buf[margin:margin + n].view(want.shape)
    got = _stem(pkg, args, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)
    assert bool((buf[:margin] == fill).all()) and bool((buf[margin + n:] == fill).all())


def test_stem_image_result_does_not_depend_on_the_launch(pkg):
    x, w, s, b = br.stem_inputs(3, 70, 131, seed=5)
    batch = _stem(pkg, (x, w, s, b))
    alone = _stem(pkg, (x[1:2].contiguous(), w, s, b))
    assert torch.equal(batch[1:2], alone)


@pytest.fixture(scope="module")
def r50(pkg):
    """R50-C4, He-initialised, random FrozenBN statistics, nothing trainable; built on the CPU."""
    torch.manual_seed(0)
    cfg = pkg.config.get_cfg()
    cfg.MODEL.BACKBONE.FREEZE_AT = 5
    return br.randomize_frozen_bn(pkg.build_backbone(cfg), 1).eval()


@pytest.mark.parametrize("shape,want", [((2, 3, 67, 97), (2, 1024, 5, 7)), ((1, 3, 64, 96), (1, 1024, 4, 6))])
def test_whole_backbone_on_the_device_path(pkg, r50, shape, want, monkeypatch):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[2]))
    ref = br.net(r50.state_dict(), x)["res4"]
    with torch.no_grad():
        cpu = r50.cpu()(x)["res4"]
    model = r50.cuda()
    count = pkg._lib.load().locov_launch_count

    def no_torch_conv(*a, **k):
        raise AssertionError("F.conv2d called on the device path")

    before = count()
    with monkeypatch.context() as m:
        m.setattr(F, "conv2d", no_torch_conv)
        with torch.no_grad():
            out = model(x.cuda())
    assert count() - before >= 1 + 3 * 13 + 3 + 2 + 1             # the stem, 13 blocks' convolutions, 3 shortcuts, 2 strides, the transpose
    got = out["res4"]
    assert list(out) == ["res4"] and tuple(got.shape) == want and got.is_contiguous() and got.dtype == torch.float32
    top = float(ref.abs().max())
    err_dev, err_cpu = float((got.double().cpu() - ref).abs().max()), float((cpu.double() - ref).abs().max())
    print(f"SPLITGATE backbone{list(shape)} device err {err_dev:.3e} torch-fp32-cpu err {err_cpu:.3e} max|ref| {top:.3e} "
          f"ratio {err_dev / max(err_cpu, 1e-300):.3f}")
    assert top > 0 and err_dev <= LOGIT_MULT * err_cpu + LOGIT_FLOOR * top
    r50.cpu()


def test_trainable_res4_takes_the_torch_path(pkg):
    torch.manual_seed(4)
    model = pkg.build_backbone(pkg.config.get_cfg()).cuda()      # FREEZE_AT 2: res3, res4 train
    x = torch.randn(1, 3, 33, 35).cuda()
    assert not model.device_path_ok(x)
    count = pkg._lib.load().locov_launch_count
    before = count()
    out = model(x)["res4"]
    assert count() == before and out.requires_grad and tuple(out.shape) == (1, 1024, 3, 3)
    out.sum().backward()
    assert model.res4[0].conv1.weight.grad is not None and float(model.res4[0].conv1.weight.grad.abs().max()) > 0
    with torch.no_grad():
        assert model.device_path_ok(x)


def test_res4_feeds_the_rpn_and_the_roi_heads(pkg):
    from locov_amd.structures import ImageList, Instances
    torch.manual_seed(6)
    cfg = pkg.config.get_cfg()
    cfg.MODEL.RPN.POST_NMS_TOPK_TEST = 50
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = 96
    cfg.MODEL.ROI_HEADS.NAME = "EmbeddingRes5ROIHeads"
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0
    backbone = br.randomize_frozen_bn(pkg.build_backbone(cfg), 2).cuda().eval()
    rpn = pkg.build_proposal_generator(cfg, backbone.output_shape()).cuda().eval()
    heads = pkg.build_roi_heads(cfg, backbone.output_shape()).cuda().eval()
    heads.box_predictor.set_class_embeddings(torch.randn(81, 96) * 0.05)
    heads.num_classes = heads.box_predictor.num_classes
    x = torch.randn(1, 3, 160, 224).cuda()
    images = ImageList(x, [(160, 224)])
    with torch.no_grad():
        feats = backbone(images.tensor)
        assert tuple(feats["res4"].shape) == (1, 1024, 10, 14) and feats["res4"].is_contiguous() and feats["res4"].dtype == torch.float32
        props, _ = rpn(images, feats)
        inst, losses = heads(images, feats, props, None)
    assert losses == {} and len(inst) == 1 and isinstance(inst[0], Instances) and inst[0].image_size == (160, 224)
