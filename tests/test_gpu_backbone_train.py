"""Training through the C4 backbone on the device (MODEL.BACKBONE.TRAIN_ON_DEVICE): the stem's training forward (the selection it
saves) and its weight-gradient kernel (csrc/resnet_stem.hip) against float64 with tests/split_ref.py's gate, and the whole R50-C4
forward + backward on the device path against the float64 restatement of tests/backbone_train_ref.py evaluated on the device's
own active sets (the convention of tests/test_gpu_res5_train.py).

Measured on an MI355X (docs/experiments.md, "Training through the C4 backbone on the device"): see the figures there."""
import pytest
import torch
import torch.nn.functional as F

import backbone_ref as br
import backbone_train_ref as btr
import split_ref as sr

pytestmark = pytest.mark.gpu

# the forward gate of tests/test_gpu_backbone.py::test_whole_backbone_on_the_device_path, and the same margin for the gradients
LOGIT_MULT = 4.0
LOGIT_FLOOR = 2.0 ** -20
FLIP_CAP = 1e-4                                           # share of active-set / selection units that may differ from float64's own (test_gpu_res5_train.py)

STEM_CASES = [(1, 1, 1), (1, 2, 3), (1, 5, 8), (2, 37, 51), (1, 40, 64), (2, 38, 50), (3, 70, 131), (1, 129, 260)]
EXACT_CASES = STEM_CASES[:6]                              # no window whose float64 top-two gap is within the summed bounds
_id = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


# ---------------------------------------------------------------------------------------------------------------- the stem
_STEM = {}


def _stem_case(pkg, shape):
    """Inputs, the device's (y, sel) and the float64 conv map with its bound, once per shape (left unchanged by the tests)."""
    if shape not in _STEM:
        args = br.stem_inputs(*shape, seed=sum(shape))
        x, w, scale, shift = args
        y, sel = pkg.ops.resnet_stem_train(*[a.cuda() for a in args])
        xd, wd = x.double(), w.double()
        cl = lambda t: t.permute(0, 2, 3, 1)
        S = cl(F.conv2d(xd.abs(), wd.abs(), stride=2, padding=3))
        conv = sr.Ref(cl(F.conv2d(xd, wd, stride=2, padding=3)), S, torch.zeros_like(S), br.STEM_K)
        act = sr.epilogue(conv, scale=scale, shift=shift, relu=True)           # channels-last [N,CH,CW,64]
        _STEM[shape] = dict(args=args, y=y, sel=sel, act=act.ref.permute(0, 3, 1, 2).contiguous(),
                            bound=sr.bound(act).permute(0, 3, 1, 2).contiguous())
    return _STEM[shape]


@pytest.mark.parametrize("shape", STEM_CASES, ids=_id)
def test_stem_train_forward_and_selection(pkg, shape):
    c = _stem_case(pkg, shape)
    N, H, W = shape
    PH, PW = pkg.ops.resnet_stem_shape(H, W)
    y, sel = c["y"], c["sel"]
    assert tuple(y.shape) == tuple(sel.shape) == (N, PH, PW, 64) and sel.dtype == torch.uint8 and sel.is_contiguous()
    assert torch.equal(y, pkg.ops.resnet_stem(*[a.cuda() for a in c["args"]]))
    yc, sc = y.cpu().permute(0, 3, 1, 2), sel.cpu().permute(0, 3, 1, 2)          # NCHW views
    assert int(sc.max()) <= 9
    keep = sc < 9
    assert bool((yc[~keep] == 0).all()) and bool((yc[keep] > 0).all())
    # the selected conv position holds the pooled value: |y - act64[selected]| <= that position's bound (no tie handling needed)
    CH, CW = c["act"].shape[2:]
    idx, keep2 = btr.pool_index(sc, CH, CW)
    assert torch.equal(keep, keep2)
    at = c["act"].flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    bd = c["bound"].flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    err = (yc.double() - at).abs()
    assert bool((err[keep] <= bd[keep]).all()), f"worst err / bound {float((err[keep] / bd[keep]).max()):.3g}"
    # against float64's own selection
    own = btr.pool_select(c["act"])
    diff, total = int((own != sc).sum()), sc.numel()
    print(f"STEMSEL {_id(shape)}: {diff} of {total} selections differ from float64's own ({diff / total:.2e})")
    assert diff <= FLIP_CAP * total
    if shape in EXACT_CASES:
        assert diff == 0


def test_stem_sel_of_an_image_does_not_depend_on_the_batch(pkg):
    c = _stem_case(pkg, (3, 70, 131))
    x, w, s, b = c["args"]
    y1, sel1 = pkg.ops.resnet_stem_train(x[1:2].contiguous().cuda(), w.cuda(), s.cuda(), b.cuda())
    assert torch.equal(sel1, c["sel"][1:2]) and torch.equal(y1, c["y"][1:2])


@pytest.mark.parametrize("band", [4, 5, 7, 18])
def test_stem_sel_band_height_does_not_change_a_bit(pkg, band, monkeypatch):
    """As tests/test_gpu_backbone.py::test_stem_band_height_does_not_change_a_bit, for sel: bands taller than the one row a small
    input gets carry the open window's selection across conv rows, patches and (18 rows = 7 + 7 + 4) a short last band."""
    c = _stem_case(pkg, (3, 70, 131))
    monkeypatch.setenv("LOCOV_STEM_BAND", str(band))
    y, sel = pkg.ops.resnet_stem_train(*[a.cuda() for a in c["args"]])
    assert torch.equal(y, c["y"]) and torch.equal(sel, c["sel"])


def test_stem_train_writes_nothing_outside_y_and_sel(pkg):
    c = _stem_case(pkg, (2, 37, 51))
    args = [a.cuda() for a in c["args"]]
    n, margin, fill, bfill = c["y"].numel(), 4096, -7.25, 77
    buf = torch.full((n + 2 * margin,), fill, device="cuda")
    sbuf = torch.full((n + 2 * margin,), bfill, dtype=torch.uint8, device="cuda")
    out, sel_out = buf[margin:margin + n].view(c["y"].shape), sbuf[margin:margin + n].view(c["sel"].shape)
    y, sel = pkg.ops.resnet_stem_train(*args, out=out, sel_out=sel_out)
    assert y.data_ptr() == out.data_ptr() and sel.data_ptr() == sel_out.data_ptr()
    assert torch.equal(y, c["y"]) and torch.equal(sel, c["sel"])
    assert bool((buf[:margin] == fill).all()) and bool((buf[margin + n:] == fill).all())
    assert bool((sbuf[:margin] == bfill).all()) and bool((sbuf[margin + n:] == bfill).all())


def _wgrad_gate(pkg, name, c, g):
    """dw of the device for g against float64 of the formula on the DEVICE's sel: split_ref's gate with K = N CH CW."""
    x, _, scale, _ = c["args"]
    N, _, CH, CW = c["act"].shape
    dw = pkg.ops.resnet_stem_wgrad(x.cuda(), g.cuda(), c["sel"], scale.cuda())
    assert tuple(dw.shape) == (64, 3, 7, 7) and dw.dtype == torch.float32 and dw.is_contiguous()
    ref, S, _ = btr.stem_wgrad(x, g, c["sel"], scale)
    q = sr.gate_ratio(dw, sr.Ref(ref, S, torch.zeros_like(S), N * CH * CW))
    print(f"SPLITGATE stem_wgrad[{name}] {q:.4f}")
    assert q <= 1.0, f"stem_wgrad {name}: err / bound = {q:.3g}"
    return dw, ref


def _random_g(c, seed):
    g = torch.randn(c["y"].shape, generator=torch.Generator().manual_seed(seed))
    return torch.where(c["y"].cpu() == 0, torch.zeros_like(g), g)


@pytest.mark.parametrize("shape", STEM_CASES, ids=_id)
def test_stem_wgrad_against_float64(pkg, shape):
    c = _stem_case(pkg, shape)
    g = _random_g(c, 1000 + sum(shape))
    dw, ref = _wgrad_gate(pkg, _id(shape), c, g)
    assert float(ref.abs().max()) > 0
    x, _, scale, _ = c["args"]
    again = pkg.ops.resnet_stem_wgrad(x.cuda(), g.cuda(), c["sel"], scale.cuda())
    assert torch.equal(again, dw)                          # fixed-order reduction: the same bits
    zero = pkg.ops.resnet_stem_wgrad(x.cuda(), torch.zeros_like(g).cuda(), c["sel"], scale.cuda())
    assert float(zero.abs().max()) == 0.0


@pytest.mark.parametrize("band,blocks", [(3, 512), (9, 512), (20, 2), (64, 1)])
def test_stem_wgrad_band_height_and_rounds(pkg, band, blocks, monkeypatch):
    """The launch picks the band of conv rows a wave walks and the number of persistent workgroups from the problem size
    (csrc/resnet_stem.hip wgrad_plan): these inputs get bands of one row in one round.  LOCOV_STEM_WGRAD_BAND /
    LOCOV_STEM_WGRAD_BLOCKS force what a training-size batch gets: 3 rows, 9 (a second patch of one row), 20 rows (35 = 20 + 15: a
    short last band) on two workgroups (four rounds, dead waves in the last) and the whole column (five patches) on one
    workgroup.  Another order of the same sums: the float64 gate again, and the same bits twice."""
    c = _stem_case(pkg, (3, 70, 131))
    g = _random_g(c, 77)
    monkeypatch.setenv("LOCOV_STEM_WGRAD_BAND", str(band))
    monkeypatch.setenv("LOCOV_STEM_WGRAD_BLOCKS", str(blocks))
    dw, _ = _wgrad_gate(pkg, f"3x70x131 band {band} blocks {blocks}", c, g)
    x, _, scale, _ = c["args"]
    assert torch.equal(pkg.ops.resnet_stem_wgrad(x.cuda(), g.cuda(), c["sel"], scale.cuda()), dw)


def test_stem_wgrad_ignores_g_where_nothing_was_selected(pkg):
    c = _stem_case(pkg, (2, 37, 51))
    x, _, scale, _ = c["args"]
    g = _random_g(c, 5)
    want = pkg.ops.resnet_stem_wgrad(x.cuda(), g.cuda(), c["sel"], scale.cuda())
    noisy = torch.where(c["sel"].cpu() == 9, torch.full_like(g, 3.5), g)
    assert int((c["sel"] == 9).sum()) > 0
    assert torch.equal(pkg.ops.resnet_stem_wgrad(x.cuda(), noisy.cuda(), c["sel"], scale.cuda()), want)


@pytest.mark.parametrize("shape", [(2, 37, 51), (1, 40, 64)], ids=_id)
def test_stem_wgrad_of_single_elements(pkg, shape):
    """One pooled pixel (all of its channels) at each image corner and in the middle: dw[o] = scale[o] g[o] x-patch at the conv
    position channel o selected -- patches that hang over every image edge."""
    c = _stem_case(pkg, shape)
    N, PH, PW, _ = c["y"].shape
    for p, q in ((0, 0), (0, PW - 1), (PH - 1, 0), (PH - 1, PW - 1), (PH // 2, PW // 2)):
        g = torch.zeros(c["y"].shape)
        g[N - 1, p, q, :] = torch.randn(64, generator=torch.Generator().manual_seed(p * PW + q)) + 2.0
        dw, ref = _wgrad_gate(pkg, f"{_id(shape)} one at ({p},{q})", c, g)
        sel = c["sel"][N - 1, p, q].cpu()
        assert bool((ref[sel == 9] == 0).all()) and bool((dw.cpu()[sel == 9] == 0).all())
        assert float(ref[sel < 9].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- the whole backbone
SHAPES = [((2, 3, 67, 97), (2, 1024, 5, 7)), ((1, 3, 64, 96), (1, 1024, 4, 6))]


def _build(pkg, freeze_at):
    """R50-C4, He-initialised, random FrozenBN statistics (the model of tests/test_gpu_backbone.py), built on the CPU."""
    torch.manual_seed(0)
    cfg = pkg.config.get_cfg()
    cfg.MODEL.BACKBONE.FREEZE_AT = freeze_at
    cfg.MODEL.BACKBONE.TRAIN_ON_DEVICE = True
    return br.randomize_frozen_bn(pkg.build_backbone(cfg), 1).eval()


@pytest.fixture(scope="module")
def r50(pkg):
    return _build(pkg, 0)


@pytest.fixture(scope="module")
def r50_frozen2(pkg):
    return _build(pkg, 2)


_CPU = {}


def _cpu_side(sd, shape):
    """Per input, once: x, G, the float64 forward, the torch-fp32 CPU evaluation (forward error; gradients against float64 on ITS
    own sets, per tensor relative to the largest entry) and float64's own sets."""
    if shape not in _CPU:
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[2]))
        ref = br.net(sd, x)["res4"]
        G = torch.randn(ref.shape, generator=torch.Generator().manual_seed(shape[3]))
        y32, g32, sets32 = btr.grads(sd, x, G, dtype=torch.float32)
        _, g64_on32, _ = btr.grads(sd, x, G, sets=sets32)
        _, _, sets64 = btr.grads(sd, x, G)
        _CPU[shape] = dict(x=x, G=G, ref=ref, err_cpu=float((y32.double() - ref).abs().max()), g32=g32, g64_on32=g64_on32, sets64=sets64)
    return _CPU[shape]


def _device_sets(pkg, model, out, shape):
    """ResNet.saved_training_state in the layout of backbone_train_ref's sets (NCHW)."""
    state = model.saved_training_state(out)
    N = shape[0]
    H, W = pkg.ops.resnet_stem_shape(shape[2], shape[3])
    sets = {}
    if "stem" in state:
        assert tuple(state["stem"].shape) == (N, H, W, 64)
        sets["stem"] = state["stem"].cpu().permute(0, 3, 1, 2).contiguous()
    for si, name in enumerate(("res2", "res3", "res4")):
        if si > 0:
            H, W = (H + 1) // 2, (W + 1) // 2
        for b, (_, y1, y2, o) in enumerate(state.get(name, [])):
            for key, t in (("y1", y1), ("y2", y2), ("out", o)):
                sets[f"{name}.{b}.{key}"] = (t.cpu() > 0).view(N, H, W, t.shape[1]).permute(0, 3, 1, 2).contiguous()
    return sets


def _step(pkg, model, c, monkeypatch):
    """One forward + backward of (res4 . G).sum() on the device with torch's convolution and max-pool forbidden -> (res4, the
    device's sets, read between the two: backward frees what the nodes saved)."""
    count = pkg._lib.load().locov_launch_count

    def forbidden(*a, **k):
        raise AssertionError("torch's convolution / max-pool called on the device training path")

    model.zero_grad(set_to_none=True)
    x = c["x"].cuda()
    assert model.train_path_ok(x) and not model.device_path_ok(x)
    before = count()
    with monkeypatch.context() as m:
        m.setattr(F, "conv2d", forbidden)
        m.setattr(F, "max_pool2d", forbidden)
        out = model(x)["res4"]
        mid = count()
        sets = _device_sets(pkg, model, out, tuple(x.shape))
        (out * c["G"].cuda()).sum().backward()
    assert mid > before and count() > mid
    assert out.requires_grad and out.is_contiguous() and out.dtype == torch.float32
    return out, sets


def _check(pkg, model, out, sets, c, shape, sd, trained):
    """The forward gate, the flips cap and the gradient gate for the parameters under the prefixes `trained`."""
    ref, top = c["ref"], float(c["ref"].abs().max())
    err_dev = float((out.detach().double().cpu() - ref).abs().max())
    print(f"SPLITGATE backbone-train{list(shape)} device err {err_dev:.3e} torch-fp32-cpu err {c['err_cpu']:.3e} max|ref| {top:.3e}")
    assert top > 0 and err_dev <= LOGIT_MULT * c["err_cpu"] + LOGIT_FLOOR * top
    diff, total = btr.set_flips(sets, c["sets64"])
    print(f"BACKBONE-TRAIN{list(shape)} {diff} of {total} active-set units differ from float64's own")
    assert total > 0 and diff <= FLIP_CAP * total
    _, g64, used = btr.grads(sd, c["x"], c["G"], sets=sets)
    assert all(torch.equal(used[k], sets[k]) for k in sets)
    keys = [k for k in g64 if k.startswith(trained)]
    got = {k: dict(model.named_parameters())[k].grad for k in keys}
    assert all(g is not None for g in got.values())
    dev, at_dev = btr.worst_relative(got, g64, keys)
    cpu, at_cpu = btr.worst_relative(c["g32"], c["g64_on32"], keys)
    print(f"GRADGATE backbone-train{list(shape)} {len(keys)} tensors: device {dev:.3e} ({at_dev}) torch-fp32-cpu {cpu:.3e} ({at_cpu}) "
          f"ratio {dev / max(cpu, 1e-300):.3f}")
    assert dev <= LOGIT_MULT * cpu + LOGIT_FLOOR


@pytest.mark.parametrize("shape,want", SHAPES)
def test_whole_backbone_trains_on_the_device(pkg, r50, shape, want, monkeypatch):
    sd = {k: v.cpu() for k, v in r50.state_dict().items()}
    c = _cpu_side(sd, shape)
    model = r50.cuda()
    out, sets = _step(pkg, model, c, monkeypatch)
    assert tuple(out.shape) == want
    _check(pkg, model, out, sets, c, shape, sd, ("stem.", "res2.", "res3.", "res4."))
    assert len(sets) == 1 + 3 * 13 and len([p for p in model.parameters() if p.grad is not None]) == 1 + 3 * 13 + 3
    r50.cpu()


def test_freeze_at_2_runs_the_frozen_prefix_on_the_inference_kernels(pkg, r50_frozen2, monkeypatch):
    shape = SHAPES[1][0]
    sd = {k: v.cpu() for k, v in r50_frozen2.state_dict().items()}
    c = _cpu_side(sd, shape)                               # (the same weights and statistics as r50: the same seed)
    model = r50_frozen2.cuda()
    calls = []
    stem_fwd, stage_fwd = pkg.ops.resnet_stem, type(model.res2).forward_rows
    monkeypatch.setattr(pkg.ops, "resnet_stem", lambda *a, **k: (calls.append("stem"), stem_fwd(*a, **k))[1])
    monkeypatch.setattr(pkg.ops, "resnet_stem_train", lambda *a, **k: pytest.fail("a frozen stem under autograd"))
    monkeypatch.setattr(type(model.res2), "forward_rows", lambda self, *a, **k: (calls.append(self), stage_fwd(self, *a, **k))[1])
    out, sets = _step(pkg, model, c, monkeypatch)
    assert calls[0] == "stem" and calls[1] is model.res2 and len(calls) == 2
    _check(pkg, model, out, sets, c, shape, sd, ("res3.", "res4."))
    assert not any(k == "stem" or k.startswith("res2.") for k in sets) and len(sets) == 3 * 10
    assert all(p.grad is None for p in list(model.stem.parameters()) + list(model.res2.parameters()))
    r50_frozen2.cpu()


def test_flag_off_launches_nothing(pkg, r50):
    model = r50.cuda()
    x = torch.randn(1, 3, 33, 35).cuda()
    count = pkg._lib.load().locov_launch_count
    model.train_on_device = False
    try:
        assert not model.train_path_ok(x) and not model.device_path_ok(x)
        before = count()
        out = model(x)["res4"]
        assert count() == before and out.requires_grad and tuple(out.shape) == (1, 1024, 3, 3)
    finally:
        model.train_on_device = True
        r50.cpu()


def test_a_second_step_at_another_size(pkg, r50, monkeypatch):
    """The steps allocate per call: a step at one image size, then one at another in the same process -- both pass the gates."""
    sd = {k: v.cpu() for k, v in r50.state_dict().items()}
    model = r50.cuda()
    for shape, want in (SHAPES[1], SHAPES[0]):
        c = _cpu_side(sd, shape)
        out, sets = _step(pkg, model, c, monkeypatch)
        assert tuple(out.shape) == want
        _check(pkg, model, out, sets, c, shape, sd, ("stem.", "res2.", "res3.", "res4."))
    r50.cpu()
