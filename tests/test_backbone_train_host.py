"""The backbone's device training path without a GPU: the MODEL.BACKBONE.TRAIN_ON_DEVICE key and ResNet.train_on_device, the silent
torch path for CPU tensors with the flag on, the argument checks of locov_resnet_stem_fwd_sel / locov_resnet_stem_wgrad
(+ _workspace_bytes) and their ops wrappers, and the autograd restatement of tests/backbone_train_ref.py against
tests/backbone_ref.py."""
import ctypes

import pytest
import torch

import backbone_ref as br
import backbone_train_ref as btr
from locov_amd import _lib, ops
from locov_amd.backbone import ResNet, build_backbone
from locov_amd.config import get_cfg


def test_key_defaults_to_false_and_reaches_the_module():
    cfg = get_cfg()
    assert cfg.MODEL.BACKBONE.TRAIN_ON_DEVICE is False
    m = build_backbone(cfg)
    assert m.train_on_device is False
    cfg.MODEL.BACKBONE.TRAIN_ON_DEVICE = True
    on = build_backbone(cfg)
    assert on.train_on_device is True
    m.train_on_device = True                               # an attribute: may be set afterwards
    assert m.train_on_device is True
    assert ResNet(on.stem, [list(s) for s in on.stages]).train_on_device is False
    assert ResNet(on.stem, [list(s) for s in on.stages], train_on_device=True).train_on_device is True


def test_cpu_tensors_take_the_torch_path_with_the_flag_on():
    torch.manual_seed(3)
    cfg = get_cfg()
    cfg.MODEL.BACKBONE.FREEZE_AT = 0
    m = br.randomize_frozen_bn(build_backbone(cfg), 3)
    x = torch.randn(1, 3, 33, 35)
    assert not m.train_path_ok(x) and not m.device_path_ok(x)

    def run():
        m.zero_grad(set_to_none=True)
        out = m(x)["res4"]
        out.sum().backward()
        return out.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}
    out_off, g_off = run()
    m.train_on_device = True
    assert not m.train_path_ok(x)
    out_on, g_on = run()
    assert torch.equal(out_on, out_off) and set(g_on) == set(g_off) and len(g_on) == 1 + 3 * 13 + 3
    assert all(torch.equal(g_on[k], g_off[k]) for k in g_off)


def _aligned(n=64):
    buf = (ctypes.c_float * (n + 8))()                     # any non-null, 16-byte-aligned host address: nothing is dereferenced
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)


def test_stem_fwd_sel_validates_without_a_gpu():
    lib = _lib.load()
    assert "locov_resnet_stem_fwd_sel" in _lib.SIGNATURES and lib.locov_abi_version() == 8
    _, p = _aligned()
    stem = lib.locov_resnet_stem_fwd_sel
    assert stem(None, 1, 8, 8, p, p, p, 64, p, p, None) == -1 and b"null pointer" in lib.locov_last_error()
    assert stem(p, 1, 8, 8, p, p, p, 64, p, None, None) == -1 and b"null pointer" in lib.locov_last_error()
    assert stem(p, 1, 8, 8, p, p, p, 32, p, p, None) == -1 and b"Cout" in lib.locov_last_error()
    assert stem(p, 1, 0, 8, p, p, p, 64, p, p, None) == -1 and stem(p, -1, 8, 8, p, p, p, 64, p, p, None) == -1
    assert stem(p, 1, 8, 8, p, p, p, 64, ctypes.c_void_p(p.value + 4), p, None) == -1 and b"misaligned" in lib.locov_last_error()
    assert stem(p, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, p, p, p, 64, p, p, None) == -1 and b"overflow" in lib.locov_last_error()
    assert b"locov_resnet_stem_fwd_sel" in lib.locov_last_error()
    assert stem(None, 0, 8, 8, None, None, None, 64, None, None, None) == 0


def test_stem_wgrad_validates_without_a_gpu():
    lib = _lib.load()
    assert "locov_resnet_stem_wgrad" in _lib.SIGNATURES and "locov_resnet_stem_wgrad_workspace_bytes" in _lib.SIGNATURES
    _, p = _aligned()
    wg, need = lib.locov_resnet_stem_wgrad, lib.locov_resnet_stem_wgrad_workspace_bytes
    part = 147 * 64 * 4                                    # one workgroup's partial
    assert need(0, 8, 8) == 0 and need(1, 0, 8) == 0 and need(-1, 8, 8) == 0
    assert need(1, 8, 8) == part                           # 4 x 4 conv positions: one wave
    assert need(1, 1, 1) == part
    big = need(4, 800, 1333)
    assert big % part == 0 and part < big <= 512 * part and need(64, 800, 1333) <= 512 * part      # bounded whatever N is
    n = need(1, 8, 8)
    for bad in range(6):                                   # x, g, sel, scale, dw, workspace
        args = [p, 1, 8, 8, p, p, p, 64, p, p, n, None]
        args[(0, 4, 5, 6, 8, 9)[bad]] = None
        assert wg(*args) == -1 and b"null pointer" in lib.locov_last_error(), bad
    assert wg(p, 1, 8, 8, p, p, p, 32, p, p, n, None) == -1 and b"Cout" in lib.locov_last_error()
    assert wg(p, 1, 8, 0, p, p, p, 64, p, p, n, None) == -1 and wg(p, -1, 8, 8, p, p, p, 64, p, p, n, None) == -1
    off = ctypes.c_void_p(p.value + 2)
    assert wg(p, 1, 8, 8, off, p, p, 64, p, p, n, None) == -1 and b"misaligned" in lib.locov_last_error()
    assert wg(p, 1, 8, 8, p, p, p, 64, off, p, n, None) == -1 and b"misaligned" in lib.locov_last_error()
    assert wg(p, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, p, p, p, 64, p, p, 2 ** 62, None) == -1 and b"overflow" in lib.locov_last_error()
    assert wg(p, 1, 8, 8, p, p, p, 64, p, p, n - 1, None) == -1 and b"workspace" in lib.locov_last_error()
    assert wg(None, 0, 8, 8, None, None, None, 64, None, None, 0, None) == 0


def test_ops_wrappers_have_no_cpu_fallback():
    x, w, s, b = br.stem_inputs(1, 8, 8, 0)
    with pytest.raises(_lib.LocovError, match="no CPU fallback"):
        ops.resnet_stem_train(x, w, s, b)
    with pytest.raises(_lib.LocovError, match="no CPU fallback"):
        ops.resnet_stem_wgrad(x, torch.zeros(1, 2, 2, 64), torch.zeros(1, 2, 2, 64, dtype=torch.uint8), s)


@pytest.fixture(scope="module")
def r50():
    torch.manual_seed(0)
    cfg = get_cfg()
    cfg.MODEL.BACKBONE.FREEZE_AT = 0
    return br.randomize_frozen_bn(build_backbone(cfg), 1).eval()


@pytest.mark.parametrize("shape", [(2, 3, 67, 97), (1, 3, 64, 96)])
def test_replaying_its_own_sets_is_backbone_ref(r50, shape):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[2]))
    want = br.net(r50.state_dict(), x)
    own, sets, _ = btr.net(r50.state_dict(), x)
    again, used, _ = btr.net(r50.state_dict(), x, sets=sets)
    assert set(sets) == {"stem"} | {f"res{k}.{b}.{n}" for k, nb in ((2, 3), (3, 4), (4, 6)) for b in range(nb) for n in ("y1", "y2", "out")}
    for name in ("stem", "res2", "res3", "res4"):
        assert torch.equal(own[name].detach(), want[name]) and torch.equal(again[name].detach(), want[name]), name
    assert btr.set_flips(sets, used) == (0, sum(v.numel() for v in sets.values()))


def test_reference_gradients_are_torch_autograds(r50):
    """The restatement's float32 gradients on its own sets against the module's torch path (F.relu / F.max_pool2d under autograd):
    the same function, so the same gradients up to the order of a few fp32 sums."""
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(64))
    G = torch.randn(1, 1024, 4, 6, generator=torch.Generator().manual_seed(1))
    r50.zero_grad(set_to_none=True)
    for p in r50.parameters():
        p.requires_grad_(True)
    (r50(x)["res4"] * G).sum().backward()
    _, g32, _ = btr.grads(r50.state_dict(), x, G, dtype=torch.float32)
    mine = {k: p.grad for k, p in r50.named_parameters()}
    assert set(mine) == set(g32)
    worst, at = btr.worst_relative(g32, {k: v.double() for k, v in mine.items()})
    print(f"BACKBONE-TRAIN ref fp32 against module autograd: worst {worst:.3e} at {at}")
    assert worst <= 1e-4                                    # (a flipped unit would show as ~1e-3; rounding sits near 1e-6)
    r50.zero_grad(set_to_none=True)


def test_stem_wgrad_formula_is_autograds():
    """backbone_train_ref.stem_wgrad (the formula of the header) against autograd through conv, fold, ReLU and max-pool."""
    x, w, scale, shift = br.stem_inputs(2, 37, 51, seed=90)
    wd = w.double().requires_grad_(True)
    pre = torch.nn.functional.conv2d(x.double(), wd, stride=2, padding=3) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    act = torch.relu(pre)
    sel = btr.pool_select(act)
    y = torch.nn.functional.max_pool2d(act, 3, 2, 1)
    assert torch.equal(btr.pool_gather(act, sel).detach(), y.detach())
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    (y * g).sum().backward()
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous()
    dw, S, _ = btr.stem_wgrad(x, cl(g), cl(sel), scale)
    assert float((dw - wd.grad).abs().max()) <= 1e-12 * float(S.max())
