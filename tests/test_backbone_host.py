"""locov_amd.backbone without a GPU: the Detectron2 surface (state-dict keys, output_shape, freeze, unsupported keys), the torch
path against the float64 restatement of tests/backbone_ref.py, and the argument checks of locov_resnet_stem_fwd / ops.resnet_stem."""
import ctypes

import pytest
import torch

import backbone_ref as br
from locov_amd import _lib, ops
from locov_amd.backbone import BasicStem, ResNet, build_backbone, build_resnet_backbone
from locov_amd.config import get_cfg
from locov_amd.structures import ShapeSpec

# fp32 torch path against float64: a convolution's relative error is ~ u sqrt(K) (u = 2^-24, K <= 2304: 3e-6); over the 43
# convolutions of R50-C4 in sequence a random walk gives 2e-5 and strictly linear growth 1.3e-4 -- 1e-4 of the largest value
NET_TOL = 1e-4


def _norm_keys(prefix, ch):
    return {f"{prefix}.norm.{k}": (ch,) for k in ("weight", "bias", "running_mean", "running_var")}


def d2_r50_c4_keys():
    """[D2-upstream] the state dict of build_resnet_backbone for R50-C4 (OUT_FEATURES ["res4"]), written out."""
    keys = {"stem.conv1.weight": (64, 3, 7, 7), **_norm_keys("stem.conv1", 64)}
    cin = 64
    for stage, blocks, mid, out in (("res2", 3, 64, 256), ("res3", 4, 128, 512), ("res4", 6, 256, 1024)):
        for b in range(blocks):
            pre = f"{stage}.{b}"
            if b == 0:
                keys[f"{pre}.shortcut.weight"] = (out, cin, 1, 1)
                keys.update(_norm_keys(f"{pre}.shortcut", out))
            keys[f"{pre}.conv1.weight"] = (mid, cin, 1, 1)
            keys.update(_norm_keys(f"{pre}.conv1", mid))
            keys[f"{pre}.conv2.weight"] = (mid, mid, 3, 3)
            keys.update(_norm_keys(f"{pre}.conv2", mid))
            keys[f"{pre}.conv3.weight"] = (out, mid, 1, 1)
            keys.update(_norm_keys(f"{pre}.conv3", out))
            cin = out
    return keys


@pytest.fixture(scope="module")
def r50():
    torch.manual_seed(0)
    return br.randomize_frozen_bn(build_backbone(get_cfg()), 1).eval()


def test_state_dict_is_detectron2s(r50):
    want = d2_r50_c4_keys()
    got = {k: tuple(v.shape) for k, v in r50.state_dict().items()}
    assert got == want
    assert len(want) == 5 * (1 + 3 * 13 + 3)
    assert not any(k.startswith(("res5.", "linear.")) for k in got)
    fresh = build_resnet_backbone(get_cfg(), ShapeSpec(channels=3))
    assert fresh.load_state_dict(r50.state_dict(), strict=True).missing_keys == []
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), r50.state_dict().values()))
    assert isinstance(r50, ResNet) and isinstance(r50.stem, BasicStem) and r50.stage_names == ("res2", "res3", "res4")


def test_output_shape_and_divisibility(r50):
    assert r50.output_shape() == {"res4": ShapeSpec(channels=1024, stride=16)}
    assert r50.size_divisibility == 0
    cfg = get_cfg()
    cfg.MODEL.RESNETS.OUT_FEATURES = ["res2", "res5"]
    cfg.MODEL.RESNETS.DEPTH = 101
    m = build_backbone(cfg)
    assert m.output_shape() == {"res2": ShapeSpec(channels=256, stride=4), "res5": ShapeSpec(channels=2048, stride=32)}
    assert [len(s) for s in m.stages] == [3, 4, 23, 3]


@pytest.mark.parametrize("freeze_at", [0, 1, 2, 3])
def test_freeze_at(freeze_at):
    cfg = get_cfg()
    cfg.MODEL.BACKBONE.FREEZE_AT = freeze_at
    m = build_backbone(cfg)
    assert all(p.requires_grad == (freeze_at < 1) for p in m.stem.parameters())
    for k in (2, 3, 4):
        ps = list(getattr(m, f"res{k}").parameters())
        assert ps and all(p.requires_grad == (freeze_at < k) for p in ps), k


def test_default_freeze_at_is_2():
    cfg = get_cfg()
    assert cfg.MODEL.BACKBONE.FREEZE_AT == 2 and cfg.MODEL.BACKBONE.NAME == "build_resnet_backbone"
    assert cfg.MODEL.RESNETS.DEPTH == 50 and cfg.MODEL.RESNETS.OUT_FEATURES == ["res4"]
    assert cfg.MODEL.RESNETS.STEM_OUT_CHANNELS == 64 and cfg.MODEL.RESNETS.RES5_DILATION == 1


@pytest.mark.parametrize("key,value,word", [("DEPTH", 18, "DEPTH"), ("DEPTH", 34, "DEPTH"), ("RES5_DILATION", 2, "RES5_DILATION"),
                                            ("DEFORM_ON_PER_STAGE", [False, False, True, False], "DEFORM_ON_PER_STAGE")])
def test_unsupported_keys_raise_by_name(key, value, word):
    cfg = get_cfg()
    cfg.MODEL.RESNETS[key] = value
    with pytest.raises(NotImplementedError, match=word):
        build_backbone(cfg)


@pytest.mark.parametrize("shape,want", [((2, 3, 67, 97), (2, 1024, 5, 7)), ((1, 3, 64, 96), (1, 1024, 4, 6))])
def test_torch_path_against_float64(r50, shape, want):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[2]))
    with torch.no_grad():
        got = r50(x)
    assert list(got) == ["res4"] and tuple(got["res4"].shape) == want and got["res4"].dtype == torch.float32
    ref = br.net(r50.state_dict(), x)["res4"]
    err, top = float((got["res4"].double() - ref).abs().max()), float(ref.abs().max())
    print(f"BACKBONE torch-fp32 cpu {shape}: err {err:.3e} max|ref| {top:.3e} ratio {err / top:.3e}")
    assert top > 0 and err <= NET_TOL * top


def test_gradients_reach_res3_under_freeze_at_2():
    torch.manual_seed(2)
    m = build_backbone(get_cfg())
    out = m(torch.randn(1, 3, 33, 35))["res4"]
    assert tuple(out.shape) == (1, 1024, 3, 3) and out.requires_grad
    out.sum().backward()
    assert m.res3[0].conv1.weight.grad is not None and float(m.res3[0].conv1.weight.grad.abs().max()) > 0
    assert m.res4[5].conv3.weight.grad is not None
    assert m.res2[0].conv1.weight.grad is None and m.stem.conv1.weight.grad is None


def test_stem_entry_point_validates_without_a_gpu():
    lib = _lib.load()
    assert "locov_resnet_stem_fwd" in _lib.SIGNATURES and lib.locov_abi_version() == 8
    buf = (ctypes.c_float * 64)()                          # any non-null, 16-byte-aligned host address: nothing is dereferenced
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    stem = lib.locov_resnet_stem_fwd
    assert stem(None, 1, 8, 8, p, p, p, 64, p, None) == -1 and b"null pointer" in lib.locov_last_error()
    assert stem(p, 1, 8, 8, p, p, p, 64, None, None) == -1 and b"null pointer" in lib.locov_last_error()
    assert stem(p, 1, 8, 8, p, p, p, 32, p, None) == -1 and b"Cout" in lib.locov_last_error()
    assert stem(p, 1, 0, 8, p, p, p, 64, p, None) == -1 and stem(p, -1, 8, 8, p, p, p, 64, p, None) == -1
    assert stem(p, 1, 8, 8, p, p, p, 64, ctypes.c_void_p(p.value + 4), None) == -1 and b"misaligned" in lib.locov_last_error()
    assert stem(p, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, p, p, p, 64, p, None) == -1 and b"overflow" in lib.locov_last_error()
    assert stem(None, 0, 8, 8, None, None, None, 64, None, None) == 0


def test_ops_resnet_stem_has_no_cpu_fallback():
    x, w, s, b = br.stem_inputs(1, 8, 8, 0)
    with pytest.raises(_lib.LocovError, match="no CPU fallback"):
        ops.resnet_stem(x, w, s, b)
