"""GPU checks of GroundingHead's variants on the kernels: ALIGNMENT "hardmax" and a single alignment direction in the alignment kernel
(ops.grounding_costs(alignment=, words=, regions=) = locov_grounding_align_fwd / _bwd), LOSS "triplet" as one launch each way
(ops.grounding_triplet = locov_grounding_triplet_fwd / _bwd).  Values and gradients against the float64 re-statement
tests/grounding_variants_ref.py (itself pinned to the reference's vectors by tests/test_grounding_variants_capi.py), softmax through
the new export bit for bit against the old one, the module against its LOCOV_FUSED_LOSSES=0 self, launch counts and host reads."""
import types

import numpy as np
import pytest
import torch

import grounding_variants_ref as gvr

pytestmark = pytest.mark.gpu

TEMP = 10.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import _lib, ops
    _lib.load()
    return ops


# ---------------------------------------------------------------------------------------------------------------- 1. hardmax
# (B, T, NR): one entry; small odd sizes; NR past the 64 lanes of a wave; NR past the 256 threads of the workgroup; a tile above
# 64 KB (the raised dynamic-LDS limit).  The seeds are ones for which every top-two gap is >= 1e-4 (asserted below).
HARD_SHAPES = [(1, 1, 1, 0), (2, 5, 3, 0), (3, 11, 70, 0), (2, 3, 300, 0), (2, 70, 250, 1)]
_HARD_CACHE = {}


def _hard_case(B, T, NR, seed, empty):
    """Inputs and the float64 reference (costs and dS for each choice of directions), computed once per case."""
    key = (B, T, NR, seed, empty)
    if key in _HARD_CACHE:
        return _HARD_CACHE[key]
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + T + NR)
    S = torch.randn(B * T, B * NR, generator=g) * 3.0
    cmask, rmask = torch.ones(B, T), torch.ones(B, NR)
    for c in range(B):                                           # ragged: caption c loses its last c words, image i a third per i
        cmask[c, max(T - c, 1):] = 0
        rmask[c, max(NR - (c * NR) // 3, 1):] = 0
    if empty:                                                    # a caption without words, an image without regions, the pair of both
        cmask[B - 1, :] = 0
        rmask[0, :] = 0
    gw, gr = torch.randn(B, B, generator=g), torch.randn(B, B, generator=g)
    ref = {}
    for words, regions in ((True, True), (True, False), (False, True)):
        S64 = S.double().requires_grad_(True)
        w2r, r2w = gvr.costs(S64, cmask.double(), rmask.double(), TEMP, "hardmax", words, regions)
        total = (w2r * gw.double()).sum() if words else 0
        total = total + ((r2w * gr.double()).sum() if regions else 0)
        total.backward()
        ref[(words, regions)] = (w2r.detach() if words else None, r2w.detach() if regions else None, S64.grad)
    _HARD_CACHE[key] = (S, cmask, rmask, gw, gr, ref)
    return _HARD_CACHE[key]


@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("B,T,NR,seed", HARD_SHAPES)
def test_hardmax_costs_and_gradients_match_float64(ops, B, T, NR, seed, empty):
    S, cmask, rmask, gw, gr, ref = _hard_case(B, T, NR, seed, empty)
    gap = gvr.top_two_gap(S, cmask, rmask, TEMP)                 # in float64, before the device is touched: no row or column excluded
    assert gap >= 1e-4, gap
    for (words, regions), (w2r, r2w, dS) in ref.items():
        Sd = S.cuda().requires_grad_(True)
        got_w, got_r = ops.grounding_costs(Sd, cmask.cuda(), rmask.cuda(), TEMP, alignment="hardmax", words=words, regions=regions)
        assert (got_w is None) == (not words) and (got_r is None) == (not regions)
        total = 0
        for got, want, up in ((got_w, w2r, gw), (got_r, r2w, gr)):
            if got is None:
                continue
            np.testing.assert_allclose(got.detach().cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5, err_msg=str((words, regions)))
            total = total + (got * up.cuda()).sum()
        total.backward()
        np.testing.assert_allclose(Sd.grad.cpu().numpy(), dS.numpy(), atol=2e-6, rtol=1e-3, err_msg=str((words, regions)))


def test_hardmax_ties_go_to_the_lowest_index(ops):
    """torch's argmax rule: equal similarities choose the first valid candidate; the gradient lands there alone."""
    B, T, NR = 1, 3, 130
    S = torch.zeros(T, NR)
    S[1, 70] = S[1, 5] = 2.0                                     # two equal maxima in a row; everything equal in the columns
    cmask, rmask = torch.ones(B, T), torch.ones(B, NR)
    rmask[0, 0] = 0                                              # region 0 is masked: the lowest VALID index is 1
    Sd = S.cuda().requires_grad_(True)
    w2r, r2w = ops.grounding_costs(Sd, cmask.cuda(), rmask.cuda(), 1.0, alignment="hardmax")
    w2r.sum().backward()
    want = torch.zeros(T, NR)
    want[0, 1] = want[1, 5] = want[2, 1] = -1.0 / T
    assert torch.equal(Sd.grad.cpu() != 0, want != 0)
    torch.testing.assert_close(Sd.grad.cpu(), want, rtol=1e-6, atol=0)
    Sd.grad = None
    ops.grounding_costs(Sd, cmask.cuda(), rmask.cuda(), 1.0, alignment="hardmax")[1].sum().backward()
    want = torch.zeros(T, NR)
    want[0, 1:] = -1.0 / (NR - 1)                                # every valid column's first maximum is word 0 ...
    want[0, 5] = want[0, 70] = 0
    want[1, 5] = want[1, 70] = -1.0 / (NR - 1)                   # ... except the two columns whose maximum is word 1
    assert torch.equal(Sd.grad.cpu() != 0, want != 0)
    torch.testing.assert_close(Sd.grad.cpu(), want, rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------------------- 2. softmax parity
@pytest.mark.parametrize("B,T,NR", [(3, 11, 70), (2, 70, 250)])
def test_softmax_through_the_new_export_is_bit_identical(ops, B, T, NR):
    from locov_amd import _lib
    S, cmask, rmask, gw, gr, _ = _hard_case(B, T, NR, 0, True)
    # the old exports, locov_grounding_fwd / _bwd, called on the device tensors themselves (no ops function goes through them now)
    lib, p = _lib.load(), ops._ptr
    Sc, cm, rm, gwc, grc = S.cuda(), cmask.cuda(), rmask.cuda(), gw.cuda(), gr.cuda()
    w2r, r2w, dS = torch.empty(B, B, device="cuda"), torch.empty(B, B, device="cuda"), torch.empty_like(Sc)
    assert lib.locov_grounding_fwd(p(Sc), B, T, NR, p(cm), p(rm), TEMP, p(w2r), p(r2w), ops._stream(Sc)) == 0, lib.locov_last_error()
    assert lib.locov_grounding_bwd(p(Sc), B, T, NR, p(cm), p(rm), TEMP, p(gwc), p(grc), p(dS), ops._stream(Sc)) == 0, lib.locov_last_error()
    outs = [(w2r.cpu().numpy(), r2w.cpu().numpy(), dS.cpu().numpy())]
    Sd = S.cuda().requires_grad_(True)
    w2r, r2w = ops._GroundingAlignFn.apply(Sd, cm, rm, B, T, NR, TEMP, ops.GROUNDING_ALIGNMENTS["softmax"], True, True)
    ((w2r * gwc).sum() + (r2w * grc).sum()).backward()
    outs.append((w2r.detach().cpu().numpy(), r2w.detach().cpu().numpy(), Sd.grad.cpu().numpy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    # one direction of the softmax: the same numbers as that direction of the two-way launch (costs exactly; dS against float64)
    for words, regions in ((True, False), (False, True)):
        Sd = S.cuda().requires_grad_(True)
        got = ops.grounding_costs(Sd, cmask.cuda(), rmask.cuda(), TEMP, words=words, regions=regions)
        k = 0 if words else 1
        assert got[1 - k] is None
        np.testing.assert_array_equal(got[k].detach().cpu().numpy(), outs[0][k])
        (got[k] * (gw if words else gr).cuda()).sum().backward()
        S64 = S.double().requires_grad_(True)
        want = gvr.costs(S64, cmask.double(), rmask.double(), TEMP, "softmax", words, regions)[k]
        (want * (gw if words else gr).double()).sum().backward()
        np.testing.assert_allclose(Sd.grad.cpu().numpy(), S64.grad.numpy(), atol=2e-6, rtol=1e-3)


# ---------------------------------------------------------------------------------------------------------------- 3. the tails
_TRIPLET_CACHE = {}
# |loss - float64| and |dcost - float64| allowed.  Cross-entropy: the kernels before the tails were given one frame measured
# 3.22e-7 at worst on exactly these inputs (a loss at B = 64; the largest dcost error was 1.20e-7); four times that, rounded up to
# one digit, leaves room for a later reordering of the fp32 sums and stays below the 2e-5 the golden-vector tests accept.
TAIL_TOL = {"triplet": 2e-6, "cross_entropy": 2e-6}


def _triplet_inputs(B):
    """Costs whose entries are pairwise >= 1e-3 apart (min and max unambiguous), masks with an all-empty pair where B allows, given
    indices and upstream gradients."""
    if B in _TRIPLET_CACHE:
        return _TRIPLET_CACHE[B]
    g = torch.Generator().manual_seed(50 + B)
    step = max(1.5e-3, min(0.5, 6.0 / (B * B)))
    costs = [((torch.randperm(B * B, generator=g).double() - B * B / 2) * step + off).float().view(B, B) for off in (0.25, -0.4)]
    for c in costs:
        flat = c.double().flatten().sort().values
        assert B == 1 or float((flat[1:] - flat[:-1]).min()) >= 1e-3
    T, NR = 4, 6
    cmask, rmask = torch.ones(B, T), torch.ones(B, NR)
    cmask[:, 3:] = 0
    if B >= 2:
        cmask[1, :] = 0                                           # caption 1 has no words, image 0 no regions: pair (1, 0) is filled
        rmask[0, :] = 0
    neg = torch.randint(max(B - 1, 1), (2, 2, B), generator=g)
    ups = torch.rand(4, generator=g) + 0.5
    gpw = [torch.randn(B, B, generator=g) for _ in range(2)]
    _TRIPLET_CACHE[B] = (costs, cmask, rmask, neg, ups, gpw)
    return _TRIPLET_CACHE[B]


def _triplet_reference(B, mining, margin, have, with_dist):
    costs, cmask, rmask, neg, ups, gpw = _triplet_inputs(B)
    cs = [c.double().requires_grad_(True) if on else None for c, on in zip(costs, have)]
    vals, pws, total = [], [], 0
    for k, c in enumerate(cs):
        if c is None:
            vals += [0.0] * 4
            pws.append(None)
            continue
        lc, li, ac, ai, pw = gvr.tail(c, cmask.double(), rmask.double(), "cross_entropy" if mining == "cross_entropy" else "triplet",
                                      mining, margin, neg[k])
        vals += [float(v.detach()) for v in (lc, li, ac, ai)]
        pws.append(pw.detach())
        total = total + ups[2 * k].double() * lc + ups[2 * k + 1].double() * li
        if with_dist:
            total = total + (pw * gpw[k].double()).sum()
    total.backward()
    return vals, pws, [c.grad if c is not None else None for c in cs]


TAIL_CASES = [(m, g) for m in ("hardest", "easiest", "given") for g in (0.5, 2.0)] + [("cross_entropy", None)]


@pytest.mark.parametrize("mining,margin", TAIL_CASES, ids=[m if g is None else f"{m}-{g}" for m, g in TAIL_CASES])
@pytest.mark.parametrize("B", [1, 2, 3, 64])
def test_triplet_tail_matches_float64(ops, B, mining, margin):
    """mining "cross_entropy": the same inputs and checks through the cross-entropy tail (ops.grounding_ce / grounding_ce_dist)."""
    costs, cmask, rmask, neg, ups, gpw = _triplet_inputs(B)
    tol = TAIL_TOL["cross_entropy" if mining == "cross_entropy" else "triplet"]
    for have in ((True, True), (True, False), (False, True)):
        for with_dist in (False, True):
            want_vals, want_pw, want_grad = _triplet_reference(B, mining, margin, have, with_dist)
            cs = [c.cuda().requires_grad_(True) if on else None for c, on in zip(costs, have)]
            if mining == "cross_entropy":
                res = (ops.grounding_ce_dist if with_dist else ops.grounding_ce)(cs[0], cs[1], cmask.cuda(), rmask.cuda())
            else:
                res = ops.grounding_triplet(cs[0], cs[1], cmask.cuda(), rmask.cuda(), mining, margin,
                                            neg_idx=neg.cuda() if mining == "given" else None, with_dist=with_dist)
            vals, pws = (res[0], res[1:]) if with_dist else (res, (None, None))
            tag = str((have, with_dist))
            got_vals = [float(v.detach()) for v in vals]
            print(B, mining, margin, tag, "max |loss - f64| =", max(abs(a - b) for a, b in zip(got_vals, want_vals)))
            for k in range(8):
                if k % 4 < 2:
                    assert abs(got_vals[k] - want_vals[k]) <= tol, (tag, k, got_vals[k], want_vals[k])
                else:
                    assert got_vals[k] == float(np.float32(want_vals[k])), (tag, k, got_vals[k], want_vals[k])     # the accuracies, exactly
            total = 0
            for k, c in enumerate(cs):
                if c is None:
                    assert pws[k] is None
                    continue
                total = total + ups[2 * k].item() * vals[4 * k] + ups[2 * k + 1].item() * vals[4 * k + 1]
                if with_dist:
                    # the filled costs, bit for bit what torch makes of the same fp32 input
                    ok = (cmask.sum(1)[:, None] > 0) | (rmask.sum(1)[None, :] > 0)
                    fill = torch.where(ok.cuda(), c.detach(), c.detach().max() + 100.0)
                    assert torch.equal(pws[k].detach(), fill), tag
                    if B >= 2:
                        assert float(pws[k][1, 0]) == float(c.detach().max() + 100.0)
                    total = total + (pws[k] * gpw[k].cuda()).sum()
            total.backward()
            for k, c in enumerate(cs):
                if c is not None:
                    err = float((c.grad.cpu().double() - want_grad[k]).abs().max())
                    print(B, mining, margin, tag, "max |dcost - f64| =", err)
                    assert err <= tol, (tag, k, err)


# ---------------------------------------------------------------------------------------------------------------- 4. the module
def _cfg(distill, **over):
    ns = types.SimpleNamespace
    g = ns(LOCAL_METRIC="dot", GLOBAL_METRIC="aligned_local", ALIGNMENT="softmax", ALIGNMENT_TEMPERATURE=10.0,
           LOSS="cross_entropy", NEGATIVE_MINING="random", TRIPLET_MARGIN=1.0, ALIGN_WORDS_TO_REGIONS=True,
           ALIGN_REGIONS_TO_WORDS=True, TEXT_INPUT="input_embeddings")
    for k, v in over.items():
        setattr(g, k, v)
    return ns(MODEL=ns(MMSS_HEAD=ns(GROUNDING=g, DISTILLATION_LOSS=distill)))


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
    d["region_mask"][1, NR // 3:] = 0
    return d


def _inputs(d):
    img = {"region_features": torch.from_numpy(d["region_features"]).cuda().requires_grad_(True),
           "region_mask": torch.from_numpy(d["region_mask"]).cuda()}
    cap = {"input_embeddings": torch.from_numpy(d["input_embeddings"]).cuda().requires_grad_(True),
           "attention_mask": torch.from_numpy(d["attention_mask"]).cuda(),
           "special_tokens_mask": torch.from_numpy(d["special_tokens_mask"]).cuda()}
    return img, cap


MODULE_CONFIGS = {
    "hardmax_ce": (True, dict(ALIGNMENT="hardmax")),
    "softmax_triplet_hardest": (True, dict(LOSS="triplet", NEGATIVE_MINING="hardest", TRIPLET_MARGIN=0.5)),
    "hardmax_triplet_random": (True, dict(ALIGNMENT="hardmax", LOSS="triplet", NEGATIVE_MINING="random", TRIPLET_MARGIN=2.0)),
    "regions_only_hardmax": (False, dict(ALIGNMENT="hardmax", ALIGN_WORDS_TO_REGIONS=False)),
}


@pytest.mark.parametrize("name", list(MODULE_CONFIGS))
def test_grounding_head_fused_equals_the_torch_chain(ops, monkeypatch, name):
    from locov_amd.grounding_head import GroundingHead
    distill, over = MODULE_CONFIGS[name]
    rng = np.random.default_rng(11)
    B, NR, T, V, L = 6, 23, 9, 48, 32
    d = _synth(rng, B, NR, T, V, L)
    d["region_mask"][4, :] = 0                       # an image without regions
    d["attention_mask"][3, :] = 0                    # a caption without words: the (3, 4) pair is filled with max + 100
    calls = {"variant": 0, "general": 0}
    for which in ("_variant", "_general"):
        def spy(self, *a, _orig=getattr(GroundingHead, which), _k=which[1:], **k):
            calls[_k] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(GroundingHead, which, spy)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("LOCOV_FUSED_LOSSES", fused)
        torch.manual_seed(5)
        head = GroundingHead(_cfg(distill, **over), V, L).cuda()
        img, cap = _inputs(d)
        torch.manual_seed(9)                         # random mining: the same draws in the same order on both paths
        res = head(img, cap)
        assert len(res) == (3 if distill else 2)
        info, losses = res[0], res[1]
        total = sum(v * k for v, k in zip(losses.values(), torch.linspace(0.5, 2.0, len(losses)).tolist()))
        if distill:
            assert list(res[2]) == ["w2r", "r2w"]
            total = total + (res[2]["w2r"] * 0.01).sum() - (res[2]["r2w"] * 0.02).sum()
        total.backward()
        after = torch.rand(3, device="cuda")         # the RNG stream after the step is the same as well
        outs.append((info, losses, res[2] if distill else None, after, img["region_features"].grad, cap["input_embeddings"].grad,
                     head.v2l_projection.weight.grad, head.v2l_projection.bias.grad))
    assert calls == {"variant": 1, "general": 1}
    (ia, la, da, ra, *ga), (ib, lb, db, rb, *gb) = outs
    assert list(la) == list(lb) and list(ia) == list(ib) and len(la) == (4 if distill else 2)
    assert all(k.startswith("Triplet Loss" if over.get("LOSS") == "triplet" else "CE_loss") for k in la)
    for k in la:
        assert abs(float(la[k]) - float(lb[k])) <= 2e-5, (k, float(la[k]), float(lb[k]))
    for k in ia:
        assert float(ia[k]) == float(ib[k]), k
    assert torch.equal(ra, rb)
    if distill:
        for k in da:
            torch.testing.assert_close(da[k], db[k], rtol=2e-5, atol=2e-5)
        assert float(da["w2r"][3, 4]) == float(da["w2r"].max())
    for x, y in zip(ga, gb):
        assert float((x - y).abs().max()) <= 2e-5 * float(y.abs().max()), (float((x - y).abs().max()), float(y.abs().max()))


def test_what_general_answers_stays_on_general(ops, monkeypatch):
    """reconstruction_mse, the random alignments, and a configuration `_general` answers with an exception never reach the kernels'
    variant path."""
    from locov_amd.grounding_head import GroundingHead
    monkeypatch.setattr(GroundingHead, "_variant", lambda *a, **k: pytest.fail("the variant path was taken"))
    rng = np.random.default_rng(3)
    d = _synth(rng, 3, 9, 8, 64, 32)
    for over in (dict(GLOBAL_METRIC="reconstruction_mse", ALIGN_REGIONS_TO_WORDS=False), dict(ALIGNMENT="random_categorical"),
                 dict(ALIGNMENT="random_top3", LOSS="triplet", NEGATIVE_MINING="hardest")):
        both = over.get("ALIGN_REGIONS_TO_WORDS", True)
        out = GroundingHead(_cfg(both, **over), 64, 32).cuda()(*_inputs(d))
        assert all(bool(torch.isfinite(v)) for v in out[1].values())
    with pytest.raises(KeyError):
        GroundingHead(_cfg(True, ALIGNMENT="hardmax", ALIGN_WORDS_TO_REGIONS=False), 64, 32).cuda()(*_inputs(d))
    with pytest.raises(NotImplementedError):
        GroundingHead(_cfg(False, LOSS="triplet", NEGATIVE_MINING="semi_hard"), 64, 32).cuda()(*_inputs(d))


# ---------------------------------------------------------------------------------------------------------------- 5. launches, host reads
def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_launch_counts_and_no_host_read(ops, monkeypatch):
    from locov_amd.grounding_head import GroundingHead
    rng = np.random.default_rng(2)
    B, NR, T, V, L = 4, 17, 9, 64, 32
    d = _synth(rng, B, NR, T, V, L)
    monkeypatch.setenv("LOCOV_FUSED_LOSSES", "1")
    head = GroundingHead(_cfg(True, ALIGNMENT="hardmax", LOSS="triplet", NEGATIVE_MINING="hardest"), V, L).cuda()

    inputs = _inputs(d)                                                  # (made once: the upload itself waits for the host)

    def fwd(h=head):
        _, losses, dist = h(*inputs)
        return sum(losses.values()) + (dist["w2r"] * 0.01).sum()
    fwd().backward()                                                     # (warm)
    total, f = _device_kernels(fwd)
    assert sum("grounding_kernel" in n for n in f) == 1, f
    assert sum("grounding_triplet_kernel" in n for n in f) == 1, f
    _, b = _device_kernels(lambda: total.backward())
    assert sum("grounding_kernel" in n for n in b) == 1, b
    assert sum("grounding_triplet_kernel" in n for n in b) == 1, b
    assert not any("grounding_ce" in n for n in f + b), f + b
    rand = GroundingHead(_cfg(True, ALIGNMENT="hardmax", LOSS="triplet", NEGATIVE_MINING="random"), V, L).cuda()
    fwd(rand).backward()                                                 # (warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                              # the fused step enqueues without a host read
    try:
        fwd().backward()
        fwd(rand).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # the torch chain of the same configuration reads the host (masked_select's data-dependent size)
    monkeypatch.setenv("LOCOV_FUSED_LOSSES", "0")
    fwd().backward()                                                     # (warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            fwd()
    finally:
        torch.cuda.set_sync_debug_mode("default")
