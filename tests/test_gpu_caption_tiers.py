"""The caption kernels (locov_amd/csrc/caption.hip) on every branch of their launch code: the five forward instantiations filled and
entered at their edges, the scalar tiers reached through one misaligned operand at a time, the rank kernel past one round of its
1024 threads and at its limit of 8192 tokens, the scatter kernel past one grid of 16384 waves (and at the production vocabulary),
the null-gradient arms of the LayerNorm backward, and N = 0.  The inputs and the branch each one reaches are tests/caption_cases.py
(checked without a GPU by tests/test_caption_cases.py); the helpers and the gates are those of tests/test_gpu_caption.py:

  integers, gather, gather-only weight gradient   bit-identical to tests/caption_ref.py (the 2690-token run of the padding id at
                                                  N = 8192 included: the kernel adds in ascending position from 0.0f)
  LayerNorm forward and backward                  error against float64 <= 2 x the error of the CPU torch fp32 expression + one fp32
                                                  ulp of the largest reference magnitude

A misaligned operand is placed on the device at the same offset from a 16-byte boundary as in the case, and every test asserts that
ops._dev hands that very pointer on (a copy would be aligned, and the vector tier would run instead).  Misaligned runs are gated like
the others, not compared bitwise with the aligned run: the two tiers sum the row in different orders.

Found by these cases: nothing -- every branch computes what the restatement computes.  (Three in-bounds changes to the launch code,
<1,16> up to H = 1026, <4,4> up to H = 1028 and a scatter stride of waves + 1, fail 12 of the 73 cases and no others.)  Worst measured
ratio error / gate per group, MI355X (docs/experiments.md, "Caption kernels across their tiers"):
  forward, aligned operands          0.57 ((2, 5, 258, 40) with the keep mask; kernel 9.75e-7, CPU torch fp32 6.13e-7)
  forward, one operand misaligned    0.51
  backward at length                 0.42 (N = 8192; kernel 4.12e-6, CPU torch autograd 3.92e-6)
  backward, one gradient null        0.55"""
import ctypes

import numpy as np
import pytest
import torch

import caption_cases as cc
import caption_ref as cr
from test_gpu_caption import ULP, _bwd_direct, _check_ints, _dev, _ln_args, _mlm, _torch_cpu_ln, ops  # noqa: F401 (ops: the fixture)

pytestmark = pytest.mark.gpu

FORWARD = list(cc.FORWARD) + list(cc.PREDICATE)
OK = 0                                                      # LOCOV_OK


def _place(ops, case, layer_norm=True, keep=True):
    """_dev's tensors with every misaligned operand of the case placed at its offset; asserts the tier that this launch reaches."""
    packed, draws, t = _dev(case)
    for k in case["misalign"]:
        t[k] = cc.on_device(case[k])
    t["keep"] = cc.on_device(case["keep"])
    for k, x in t.items():
        handed = ops._dev(x, k, torch.uint8 if k == "keep" else torch.float32)
        assert handed.data_ptr() == x.data_ptr() and x.data_ptr() % 16 == case[k].ctypes.data % 16, k
        assert (x.data_ptr() % (4 if k == "keep" else 16) != 0) == (k in case["misalign"]), k
    H, mis = case["shape"][2], case["misalign"]
    tier = cc.fwd_tier(H, cc.aligned(case, layer_norm, keep))
    if case["name"] in FORWARD:                             # the name's tier, unless this launch does not take the misaligned operand
        takes = not mis or mis == ("W",) or (layer_norm and (keep or mis != ("keep",)))
        assert tier == (case["name"].split("_")[0] if takes else cc.fwd_tier(H, True))
    return packed, draws, t, tier


def _ln(case, t, keep):
    args = _ln_args(case, t, False)
    args["keep"] = t["keep"] if keep else None
    return args


@pytest.mark.parametrize("name", FORWARD)
def test_forward_integers_and_gather_are_bit_identical_on_every_tier(ops, name):
    case = cc.case(name)
    B, T, H, V = case["shape"]
    packed, draws, t, tier = _place(ops, case, layer_norm=False)
    ints, emb, enc = ops.caption_embed(packed, draws, T, t["W"], mlm=_mlm(ops, case))
    assert enc is None
    _check_ints(case, ints)
    ids = case["want"][0]
    assert np.array_equal(emb.cpu().numpy().view(np.int32), case["W"][ids.reshape(-1)].view(np.int32))
    print(f"caption gather {name} {case['shape']}: tier {tier}")
    if "W" in case["misalign"]:                             # the same values from an aligned table: the vector tier, the same bits
        W = torch.from_numpy(case["W"]).cuda()
        assert W.data_ptr() % 16 == 0 and tier[0] == "s" and cc.fwd_tier(H, True)[0] == "v"
        ints2, emb2, _ = ops.caption_embed(packed, draws, T, W, mlm=_mlm(ops, case))
        assert torch.equal(ints, ints2) and torch.equal(emb.view(torch.int32), emb2.view(torch.int32))


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", FORWARD)
def test_layer_norm_forward_within_twice_the_cpu_torch_error_on_every_tier(ops, name, keep):
    case = cc.case(name)
    B, T, H, V = case["shape"]
    packed, draws, t, tier = _place(ops, case, keep=keep)
    ints, emb, enc = ops.caption_embed(packed, draws, T, t["W"], mlm=_mlm(ops, case), **_ln(case, t, keep))
    _check_ints(case, ints)
    ids = case["want"][0]
    assert np.array_equal(emb.cpu().numpy().view(np.int32), case["W"][ids.reshape(-1)].view(np.int32))
    y64, _, _ = cr.layer_norm_fwd(ids, case["types"], case["W"], case["P"], case["Tt"], case["gamma"], case["beta"], case["eps"],
                                  case["keep"] if keep else None, case["p_drop"])
    err_torch = float(np.abs(_torch_cpu_ln(case, ids, keep).numpy() - y64).max())
    got = enc.cpu().numpy().reshape(B, T, H)
    err_kernel = float(np.abs(got - y64).max())
    gate = 2 * err_torch + ULP(y64)
    print(f"caption LayerNorm forward {name} {case['shape']} keep={keep} tier {tier}: kernel {err_kernel:.3e}, CPU torch fp32 {err_torch:.3e} "
          f"(vs float64), ratio to the gate {err_kernel / gate:.3f}")
    assert err_kernel <= gate
    if keep:
        assert np.array_equal(got == 0, (case["keep"] == 0) | (y64 == 0))


@pytest.mark.parametrize("name", list(cc.RANK) + list(cc.GRID) + list(cc.PRODUCTION))
def test_gather_backward_is_the_sequential_scatter_past_one_round_and_one_grid(ops, name):
    case = cc.case(name)
    B, T, H, V = case["shape"]
    packed, draws, t = _dev(case)
    if not case["rule"]:
        draws = None                                        # the tokenizer's ids: every planted id keeps its token
    ids = case["want_bwd"][0]
    g = np.random.default_rng(5).standard_normal((B * T, H)).astype(np.float32)
    gd = torch.from_numpy(g).cuda()
    want = cr.scatter(ids, g, V)
    nan = lambda: torch.full((V, H), float("nan"), device="cuda")
    if name in cc.PRODUCTION:                               # 94 MB: one run, through the C entry point
        ints, _, _ = ops.caption_embed(packed, draws, T, t["W"], mlm=_mlm(ops, case))
        runs = [_bwd_direct(ops, ints, T, H, V, gd, nan()).cpu().numpy()]
    else:
        W = t["W"].clone().requires_grad_(True)
        ints, emb, _ = ops.caption_embed(packed, draws, T, W, mlm=_mlm(ops, case))
        emb.backward(gd)
        assert np.array_equal(W.grad.cpu().numpy().view(np.int32), want.view(np.int32))
        runs = [_bwd_direct(ops, ints, T, H, V, gd, nan()).cpu().numpy() for _ in range(2)]
    assert np.array_equal(ints[0].cpu().numpy().reshape(B, T), ids)
    # rows of unused ids are exactly zero even when the buffer held NaN; two runs give the same bits
    used = np.zeros(V, dtype=bool)
    used[ids.reshape(-1)] = True
    assert not used.all() and np.isfinite(runs[0]).all() and not runs[0][~used].any()
    for r in runs:
        assert np.array_equal(r.view(np.int32), want.view(np.int32))
    for row in (0,) + cc.MARK_ROWS + (V - 1,):              # either side of one and two grids of 16384 waves, and the last row
        if row < V:
            assert np.array_equal(runs[0][row].view(np.int32), want[row].view(np.int32)), row
    if "plant_pos" in case:
        planted = [int(ids[i, j]) for i, j in case["plant_pos"]]
        assert planted == list(cc.CASES[name][1]["plant_ids"]) and used[0]
        assert all(np.all(runs[0][row] != 0) for row in planted + [0])                     # each of them received its gradient
    longest = int(np.bincount(ids.reshape(-1)).max())
    print(f"caption gather backward {name} {case['shape']}: {cc.rank_rounds(B * T)} rank round(s), scatter {cc.scatter_form(H, V, True)}, "
          f"longest run {longest}, bit-identical")
    if name == "rank8_n8192_long_run":
        assert longest > 2000 and longest == int((ids == 0).sum())


def test_backward_of_no_tokens_writes_every_row_as_zeros(ops):
    from locov_amd import _lib
    lib = _lib.load()
    V, H = 20000, 8
    dW = torch.full((V, H), float("nan"), device="cuda")
    assert lib.locov_caption_embed_bwd_workspace_bytes(0, H, 0) == 0
    status = lib.locov_caption_embed_bwd(None, 0, 0, H, V, None, None, None, None, None, None, None, 0.0, None, None,
                                         ctypes.c_void_p(dW.data_ptr()), None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == OK, lib.locov_last_error()
    assert cc.scatter_form(H, V, True) == ("vec4", True)
    assert not dW.cpu().numpy().view(np.int32).any()


def _ln_backward_reference(case, ids, keep, g_enc, g_in):
    """(float64 weight gradient, CPU torch autograd fp32 weight gradient); either gradient may be None."""
    B, T, H, V = case["shape"]
    dx = np.zeros((B, T, H))
    Wc = torch.from_numpy(case["W"]).clone().requires_grad_(True)
    loss = 0
    if g_enc is not None:
        _, xhat, rstd = cr.layer_norm_fwd(ids, case["types"], case["W"], case["P"], case["Tt"], case["gamma"], case["beta"], case["eps"])
        dx = dx + cr.layer_norm_bwd(g_enc, xhat, rstd, case["gamma"], case["keep"] if keep else None, case["p_drop"])
        loss = loss + (_torch_cpu_ln(case, ids, keep, Wc) * torch.from_numpy(g_enc)).sum()
    if g_in is not None:
        dx = dx + g_in.astype(np.float64)
        loss = loss + (Wc[torch.from_numpy(ids)] * torch.from_numpy(g_in)).sum()
    loss.backward()
    return cr.scatter(ids, dx, V, dtype=np.float64), Wc.grad.numpy()


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", list(cc.LN_BWD))
def test_layer_norm_backward_within_twice_the_cpu_autograd_error_at_length(ops, name, keep):
    case = cc.case(name)
    B, T, H, V = case["shape"]
    packed, draws, t, _ = _place(ops, case, keep=keep)
    if not case["rule"]:
        draws = None
    ids = case["want_bwd"][0]
    rng = np.random.default_rng(6)
    g_enc, g_in = rng.standard_normal((B, T, H)).astype(np.float32), rng.standard_normal((B, T, H)).astype(np.float32)
    want, torch_grad = _ln_backward_reference(case, ids, keep, g_enc, g_in)
    err_torch = float(np.abs(torch_grad - want).max())

    def run():
        W = t["W"].clone().requires_grad_(True)
        ints, emb, enc = ops.caption_embed(packed, draws, T, W, mlm=_mlm(ops, case), **_ln(case, t, keep))
        assert np.array_equal(ints[0].cpu().numpy().reshape(B, T), ids)
        torch.autograd.backward([enc, emb], [torch.from_numpy(g_enc).cuda().view(B * T, H), torch.from_numpy(g_in).cuda().view(B * T, H)])
        return W.grad.cpu().numpy()
    a, b = run(), run()
    err_kernel = float(np.abs(a - want).max())
    gate = 2 * err_torch + ULP(want)
    print(f"caption LayerNorm backward {name} {case['shape']} keep={keep}: kernel {err_kernel:.3e}, CPU torch autograd fp32 {err_torch:.3e} "
          f"(vs float64), ratio to the gate {err_kernel / gate:.3f}, {cc.rank_rounds(B * T)} rank round(s), longest run "
          f"{int(np.bincount(ids.reshape(-1)).max())}")
    assert err_kernel <= gate
    assert np.array_equal(a.view(np.int32), b.view(np.int32))                              # reproducible bits
    used = np.zeros(V, dtype=bool)
    used[ids.reshape(-1)] = True
    assert not used.all() and not a[~used].any()


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("arm", ["encoded_tokens only", "input_embeddings only"])
def test_layer_norm_backward_with_one_gradient_null(ops, arm, keep):
    """Through the C entry points, the other gradient pointer null, so that caption_ln_bwd_kernel takes its g_in == nullptr and
    g_enc == nullptr arms (under autograd the wrapper is handed a zero tensor for an output without a gradient)."""
    from locov_amd import _lib
    lib = _lib.load()
    case = cc.case("ln_null_arms_h64")
    B, T, H, V = case["shape"]
    N = B * T
    packed, draws, t, _ = _place(ops, case, keep=keep)
    ids = case["want"][0]
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    kp = t["keep"] if keep else None
    m = _mlm(ops, case)
    ints = torch.empty((6, N), dtype=torch.int64, device="cuda")
    emb, enc = torch.empty((N, H), device="cuda"), torch.empty((N, H), device="cuda")
    mean, rstd = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    _lib.check(lib.locov_caption_embed_fwd(p(packed), p(draws), N, T, H, V, p(t["W"]), p(t["P"]), t["P"].shape[0], p(t["Tt"]), 2, p(t["gamma"]),
                                           p(t["beta"]), case["eps"], p(kp), case["p_drop"], m.p, m.p_mask, m.p_mask_noise, m.mask_id, m.len_tok, 6,
                                           p(ints), p(emb), p(enc), p(mean), p(rstd), stream), "locov_caption_embed_fwd")
    _check_ints(case, ints)
    g = np.random.default_rng(7).standard_normal((B, T, H)).astype(np.float32)
    g_enc, g_in = (g, None) if arm == "encoded_tokens only" else (None, g)
    want, torch_grad = _ln_backward_reference(case, ids, keep, g_enc, g_in)
    err_torch = float(np.abs(torch_grad - want).max())
    gd = torch.from_numpy(g).cuda().view(N, H)
    ws = torch.empty(int(lib.locov_caption_embed_bwd_workspace_bytes(N, H, 1)), dtype=torch.uint8, device="cuda")

    def run():
        dW = torch.full((V, H), float("nan"), device="cuda")
        _lib.check(lib.locov_caption_embed_bwd(p(ints), N, T, H, V, p(t["W"]), p(t["P"]), p(t["Tt"]), p(t["gamma"]), p(mean), p(rstd), p(kp),
                                               case["p_drop"], p(gd) if g_enc is not None else None, p(gd) if g_in is not None else None, p(dW),
                                               p(ws), ws.numel(), stream), "locov_caption_embed_bwd")
        return dW.cpu().numpy()
    a, b = run(), run()
    err_kernel = float(np.abs(a - want).max())
    gate = 2 * err_torch + ULP(want)
    print(f"caption LayerNorm backward, {arm}, keep={keep}: kernel {err_kernel:.3e}, CPU torch autograd fp32 {err_torch:.3e} (vs float64), "
          f"ratio to the gate {err_kernel / gate:.3f}")
    assert np.isfinite(a).all() and err_kernel <= gate
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    if g_enc is None:                                       # dx is g_in itself: the fp32 sequential scatter, bit for bit
        assert np.array_equal(a.view(np.int32), cr.scatter(ids, g, V).view(np.int32))
