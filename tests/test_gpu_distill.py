"""GPU checks of the one-launch distillation losses (ops.distill_loss = locov_distill_loss_fwd / _bwd) and of GroundingHead's
cross-entropy tail with its distributions (ops.grounding_ce_dist = locov_grounding_ce_dist_fwd / _bwd), the LSM configuration
configs/coco_lsm.yaml trains with (MMSS_HEAD.DISTILLATION_LOSS on): values against the reference's own vectors
(tests/golden/g5_distill_losses.npz), gradients against float64 autograd of the torch code, launch counts, and the fused tail
against LOCOV_FUSED_LOSSES=0."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["MultiDistillLoss", "MultiDistillLossJS", "MultiDistillLossL2"]


@pytest.fixture(scope="module")
def dl():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import _lib, distill_losses
    _lib.load()
    return distill_losses


def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


# ---------------------------------------------------------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("tt", [True, False])
@pytest.mark.parametrize("detach", [True, False])
def test_matches_reference_values_on_the_device(dl, golden_dir, name, tt, detach):
    g5 = np.load(os.path.join(golden_dir, "g5_distill_losses.npz"))
    for c in range(int(g5["num_cases"])):
        trans, w2r, r2w = (torch.from_numpy(g5[f"c{c}_{k}"]).cuda().requires_grad_(True) for k in ("trans", "w2r", "r2w"))
        mod = getattr(dl, name)(float(g5[f"c{c}_temp"]), loss_weight=0.7, detach_teacher=detach, transformer_teacher=tt)
        mod(trans, w2r, r2w)                                             # (warm: the first call loads the code object)
        got, names = _device_kernels(lambda: mod(trans, w2r, r2w))
        assert len(names) == 1 and "distill_loss_kernel" in names[0], names        # the HIP kernel, and no aten kernel
        want = float(g5[f"c{c}_{name}_tt{int(tt)}"])
        got = float(got.detach())
        assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), (c, got, want)


# ---------------------------------------------------------------------------------------------------------------- 2. gradients
def _costs(B, seed, scale=(3.0, 2.0, 0.5)):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, B, generator=g, dtype=torch.float64) * scale[0],
            torch.randn(B, B, generator=g, dtype=torch.float64) * scale[1] + 1.0,
            torch.randn(B, B, generator=g, dtype=torch.float64) * scale[2] - 1.0)


def _run(mod, costs, device, dtype):
    xs = [c.to(device=device, dtype=dtype).clone().requires_grad_(True) for c in costs]
    loss = mod(*xs)
    loss.backward()
    return loss.detach(), [x.grad for x in xs]


def _compare(dl, name, costs, temp, tt, detach, rtol=1e-4, atol=1e-7, finite_only=False, hard=False):
    """fused fp32 on the device against float64 autograd of the torch code on the CPU.  hard: logits z = -cost / temperature of
    O(100) and more, whose fp32 rounding alone moves exp(z - max) by |z| * 2^-23 relative -- the absolute tolerance grows with it
    (4 |z|max 2^-23 of the largest gradient)."""
    mod = getattr(dl, name)(temp, loss_weight=0.7, detach_teacher=detach, transformer_teacher=tt)
    got, g_got = _run(mod, costs, "cuda", torch.float32)
    want, g_want = _run(mod, costs, "cpu", torch.float64)
    assert torch.isfinite(got)
    assert abs(float(got) - float(want)) <= 2e-5 * max(1.0, abs(float(want))), (float(got), float(want))
    teacher = {0} if tt else {1, 2}
    for k, (a, b) in enumerate(zip(g_got, g_want)):
        if detach and k in teacher:
            assert a is None and b is None, k                          # the detached teacher gets no gradient
            continue
        assert a is not None and b is not None, k
        assert bool(torch.isfinite(a).all()), k
        a, b = a.cpu().double(), b
        if finite_only:
            keep = torch.isfinite(b)
            a, b = a[keep], b[keep]
        zmax = max(float(c.abs().max()) for c in costs) / temp
        tol = max(atol, 4 * 2.0 ** -23 * zmax * float(b.abs().max())) if hard and b.numel() else atol
        torch.testing.assert_close(a, b, rtol=rtol, atol=tol, msg=lambda m: f"input {k}: {m}")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("B", [1, 2, 4, 7, 32, 64, 65])
def test_gradients_match_float64_autograd(dl, name, B, monkeypatch):
    if B > 64:                                                        # beyond LOCOV_DISTILL_MAX_B: the torch code, still right
        from locov_amd import ops

        def refuse(*a, **k):
            raise AssertionError("B = 65 must take the torch path")
        monkeypatch.setattr(ops, "distill_loss", refuse)
    for temp in (1.0, 10.0):
        costs = _costs(B, seed=B * 7 + int(temp))
        for tt in (True, False):
            for detach in (True, False):
                _compare(dl, name, costs, temp, tt, detach)


# ---------------------------------------------------------------------------------------------------------------- 3. hard inputs
@pytest.mark.parametrize("name", NAMES)
def test_filled_pairs_and_underflowing_softmax(dl, name):
    B = 8
    trans, w2r, r2w = _costs(B, seed=5)
    # a caption without words next to an image without regions: GroundingHead's max + 100 fill in a row and a column
    for c in (w2r, r2w):
        fill = float(c.max()) + 100.0
        c[2, :] = fill
        c[:, 5] = fill
    for temp in (1.0, 10.0):
        for tt in (True, False):
            _compare(dl, name, (trans, w2r, r2w), temp, tt, False, hard=True)
    # costs spread so wide that fp32 softmax underflows to exact zeros (float64 does not): finite, and the finite limit
    wide = _costs(B, seed=6, scale=(60.0, 60.0, 60.0))
    for tt in (True, False):
        _compare(dl, name, wide, 1.0, tt, False, finite_only=True, hard=True)
    # ... and wider than float64's range: torch's teacher gradient turns NaN there; the kernel's stays finite
    wider = _costs(B, seed=7, scale=(600.0, 600.0, 600.0))
    for tt in (True, False):
        _compare(dl, name, wider, 1.0, tt, False, finite_only=True, hard=True)


# ---------------------------------------------------------------------------------------------------------------- 4. launch counts
def _cfg(words=True, regions=True):
    ns = types.SimpleNamespace
    g = ns(LOCAL_METRIC="dot", GLOBAL_METRIC="aligned_local", ALIGNMENT="softmax", ALIGNMENT_TEMPERATURE=10.0,
           LOSS="cross_entropy", NEGATIVE_MINING="random", TRIPLET_MARGIN=1.0, ALIGN_WORDS_TO_REGIONS=words,
           ALIGN_REGIONS_TO_WORDS=regions, TEXT_INPUT="input_embeddings")
    return ns(MODEL=ns(MMSS_HEAD=ns(GROUNDING=g, DISTILLATION_LOSS=True)))


def _synth(rng, B, NR, T, V, L):
    d = {"region_features": rng.standard_normal((B, NR, V)).astype(np.float32),
         "region_mask": np.ones((B, NR), np.uint8),
         "input_embeddings": rng.standard_normal((B, T, L)).astype(np.float32),
         "attention_mask": np.ones((B, T), np.int64), "special_tokens_mask": np.zeros((B, T), np.int64)}
    d["special_tokens_mask"][:, 0] = 1
    for b in range(B):
        n = max(T - 2 * b - 1, 3)
        d["attention_mask"][b, n:] = 0
        d["special_tokens_mask"][b, n - 1:] = 1
    return d


def _inputs(d):
    img = {"region_features": torch.from_numpy(d["region_features"]).cuda().requires_grad_(True),
           "region_mask": torch.from_numpy(d["region_mask"]).cuda()}
    cap = {"input_embeddings": torch.from_numpy(d["input_embeddings"]).cuda().requires_grad_(True),
           "attention_mask": torch.from_numpy(d["attention_mask"]).cuda(),
           "special_tokens_mask": torch.from_numpy(d["special_tokens_mask"]).cuda()}
    return img, cap


def test_launch_counts(dl):
    from locov_amd.grounding_head import GroundingHead
    costs = [c.float().cuda().requires_grad_(True) for c in _costs(4, seed=1)]
    for name in NAMES:
        for tt in (True, False):
            mod = getattr(dl, name)(10.0, transformer_teacher=tt)
            mod(*costs).backward()                                       # (warm)
            loss, fwd = _device_kernels(lambda: mod(*costs))
            assert len(fwd) == 1 and "distill_loss_kernel" in fwd[0], fwd
            _, bwd = _device_kernels(lambda: loss.backward())
            assert sum("locov" in n for n in bwd) == 1 and sum("distill_loss_kernel" in n for n in bwd) == 1, bwd
    rng = np.random.default_rng(2)
    B, NR, T, V, L = 4, 17, 9, 64, 32
    d = _synth(rng, B, NR, T, V, L)
    head = GroundingHead(_cfg(), V, L).cuda()
    trans = costs[0]
    kd = dl.MultiDistillLoss(10.0, transformer_teacher=False)

    def fwd():
        _, losses, dist = head(*_inputs(d))
        return sum(losses.values()) + kd(trans, dist["w2r"], dist["r2w"])
    fwd().backward()                                                     # (warm)
    total, f = _device_kernels(fwd)
    assert sum("grounding_ce_dist_kernel" in n for n in f) == 1, f
    assert not any("grounding_ce_kernel" in n for n in f), f
    assert sum("distill_loss_kernel" in n for n in f) == 1, f
    _, b = _device_kernels(lambda: total.backward())
    assert sum("grounding_ce_dist_kernel" in n for n in b) == 1, b
    assert sum("distill_loss_kernel" in n for n in b) == 1, b


# ---------------------------------------------------------------------------------------------------------------- 5. GroundingHead
@pytest.mark.parametrize("words,regions", [(True, True), (True, False), (False, True)])
def test_grounding_head_with_distributions_fused_vs_torch(dl, monkeypatch, words, regions):
    from locov_amd.grounding_head import GroundingHead
    rng = np.random.default_rng(11)
    B, NR, T, V, L = 6, 23, 9, 48, 32
    d = _synth(rng, B, NR, T, V, L)
    d["region_mask"][4, :] = 0                       # an image without regions
    d["attention_mask"][3, :] = 0                    # a caption without words: the (3, 4) pair is filled with max + 100
    trans0 = torch.from_numpy(rng.standard_normal((B, B)).astype(np.float32) * 3.0).cuda()
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("LOCOV_FUSED_LOSSES", fused)
        torch.manual_seed(5)
        head = GroundingHead(_cfg(words, regions), V, L).cuda()
        img, cap = _inputs(d)
        trans = trans0.clone().requires_grad_(True)
        info, losses, dist = head(img, cap)
        assert list(dist) == ["w2r", "r2w"]
        assert (dist["w2r"] is None) == (not words) and (dist["r2w"] is None) == (not regions)
        a = dist["w2r"] if words else dist["r2w"]
        b = dist["r2w"] if regions else dist["w2r"]
        kd = dl.MultiDistillLoss(10.0, transformer_teacher=False)(trans, a, b)      # the distributions carry gradient (g_pw != 0)
        w = torch.linspace(0.5, 2.0, len(losses)).tolist()
        (sum(v * k for v, k in zip(losses.values(), w)) + kd).backward()
        outs.append((info, losses, dist, kd.detach(), img["region_features"].grad, cap["input_embeddings"].grad,
                     head.v2l_projection.weight.grad, head.v2l_projection.bias.grad, trans.grad))
    (ia, la, da, ka, *ga), (ib, lb, db, kb, *gb) = outs
    assert list(la) == list(lb) and list(ia) == list(ib) and len(la) == 2 * (words + regions)
    for k in la:
        assert abs(float(la[k]) - float(lb[k])) <= 1e-6 * max(1.0, abs(float(lb[k]))), k
    assert abs(float(ka) - float(kb)) <= 1e-5 * max(1.0, abs(float(kb)))
    for k in ia:
        assert float(ia[k]) == float(ib[k]), k
    for k in da:
        assert (da[k] is None and db[k] is None) or torch.equal(da[k], db[k]), k                  # bit-identical distributions
    if words and regions:
        assert float(da["w2r"][3, 4]) == float(da["w2r"].max())                                   # (the filled pair)
    for x, y in zip(ga, gb):
        torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------- 6. the whole tail
def _tool():
    spec = importlib.util.spec_from_file_location("lsm_distill_tail", os.path.join(ROOT, "tools", "lsm_distill_tail.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_reference_config_tail_matches_torch_and_does_not_sync(monkeypatch):
    tool = _tool()
    tail = tool.Tail(4, torch.device("cuda"))
    res = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("LOCOV_FUSED_LOSSES", fused)
        tail.step()                                                      # (warm: workspaces, code objects)
        torch.cuda.synchronize()
        if fused == "1":                                                 # the fused tail enqueues without a host sync
            torch.cuda.set_sync_debug_mode("error")
        try:
            losses, grads = tail.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        res[fused] = (losses, grads)
    (lf, gf), (lt, gt) = res["1"], res["0"]
    assert list(lf) == list(lt) and {"kd_loss", "box_kd_loss", "mixbox_kd_loss"} <= set(lf)
    for k in lf:
        assert abs(float(lf[k]) - float(lt[k])) <= 1e-5 * max(1.0, abs(float(lt[k]))), (k, float(lf[k]), float(lt[k]))
    for x, y in zip(gf, gt):
        torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-7)
