"""The caption kernels on the device (csrc/caption.hip, ops.caption_embed, language_backbone.BertEmbedding) against the numpy
restatement tests/caption_ref.py.

Integers, the gather and the gather-only weight gradient are bit-identical to the restatement (the kernel copies values and adds
gradient rows in the restatement's order, from 0).  The LayerNorm path is gated on its error against float64: at most 2 x the error
of the CPU torch fp32 expression on the same inputs (both are fp32 sums over H terms in different orders) plus one fp32 ulp of the
largest reference magnitude (so that the gate is not zero where torch happens to be exact).  Both errors are printed.

Shapes (B, T, H, V): (3, 7, 768, 50) -- 21 tokens, a partial last workgroup, three float4 per lane; (2, 5, 64, 50) -- the float4
path with one vector in sixteen lanes; (3, 7, 100, 37) -- the scalar path with a partial wave.  Backward also (4, 12, 64, 50), where
one word appears ten times."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import caption_ref as cr

pytestmark = pytest.mark.gpu

SHAPES = [(3, 7, 768, 50), (2, 5, 64, 50), (3, 7, 100, 37)]
ULP = lambda ref: float(np.spacing(np.float32(np.abs(ref).max())))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import _lib, ops
    _lib.load()
    return ops


_CASES = {}


def _case(shape, p_noise=0.05):
    key = (shape, p_noise)
    if key not in _CASES:
        c = cr.make_case(*shape, seed=sum(shape), p_noise=p_noise)
        c["want"] = cr.expected_ints(c)
        _CASES[key] = c
    return _CASES[key]


def _dev(case):
    B, T = case["ids"].shape
    packed = torch.from_numpy(np.stack([case[k] for k in ("ids", "types", "attn", "special")]).reshape(4, B * T).astype(np.int32)).cuda()
    draws = torch.from_numpy(case["draws"].reshape(2, B * T)).cuda()
    t = {k: torch.from_numpy(case[k]).cuda() for k in ("W", "P", "Tt", "gamma", "beta")}
    return packed, draws, t


def _mlm(ops, case):
    return ops.CaptionMlm(cr.P, cr.P_MASK, cr.P_MASK + case["p_noise"], case["mask_id"], case["len_tok"])


def _ln_args(case, t, keep):
    return dict(position=t["P"], token_type=t["Tt"], ln_weight=t["gamma"], ln_bias=t["beta"], eps=case["eps"],
                keep=torch.from_numpy(case["keep"]).cuda() if keep else None, p_drop=case["p_drop"])


def _torch_cpu_ln(case, ids, keep, W=None):
    """The CPU torch fp32 expression (the module's definition) on the restatement's ids."""
    c = {k: torch.from_numpy(case[k]) for k in ("W", "P", "Tt", "gamma", "beta")}
    W = c["W"] if W is None else W
    ids, types = torch.from_numpy(ids), torch.from_numpy(case["types"])
    x = (W[ids] + c["Tt"][types]) + c["P"][:ids.shape[1]]
    y = F.layer_norm(x, (x.shape[-1],), c["gamma"], c["beta"], case["eps"])
    if keep:
        y = y * torch.from_numpy(case["keep"]).float() * (1.0 / (1.0 - case["p_drop"]))
    return y


def _check_ints(case, ints, rows=6):
    B, T = case["ids"].shape
    ids, special, target, mlm_mask = case["want"]
    want = [ids, case["types"], case["attn"], special, target, mlm_mask][:rows]
    assert ints.dtype == torch.int64 and tuple(ints.shape) == (rows, B * T)
    for k, w in enumerate(want):
        assert np.array_equal(ints[k].cpu().numpy().reshape(B, T), w), k


@pytest.mark.parametrize("p_noise", [0.0, 0.05])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_integers_and_gather_are_bit_identical(ops, shape, p_noise):
    case = _case(shape, p_noise)
    B, T, H, V = shape
    packed, draws, t = _dev(case)
    ints, emb, enc = ops.caption_embed(packed, draws, T, t["W"], mlm=_mlm(ops, case))
    assert enc is None
    _check_ints(case, ints)
    ids, _, target, mlm_mask = case["want"]
    assert mlm_mask.sum() >= 3 and (ids == case["mask_id"]).any() and (p_noise == 0.0 or (ids == case["len_tok"] - 1).any())
    assert (ids == 0).sum() >= B * (T // 3) and (case["ids"] == 7).sum() >= 2              # duplicated ids: the padding, one word
    assert np.array_equal(emb.cpu().numpy().view(np.int32), case["W"][ids.reshape(-1)].view(np.int32))
    # masked language modelling inactive (draws None): nothing changes; configured off: four integer rows
    ints0, emb0, _ = ops.caption_embed(packed, None, T, t["W"], mlm=_mlm(ops, case))
    assert np.array_equal(ints0[0].cpu().numpy(), case["ids"].reshape(-1)) and np.array_equal(ints0[4].cpu().numpy(), case["ids"].reshape(-1))
    assert not ints0[5].any() and np.array_equal(ints0[3].cpu().numpy(), case["special"].reshape(-1))
    ints4, _, _ = ops.caption_embed(packed, None, T, t["W"], with_targets=False)
    assert tuple(ints4.shape) == (4, B * T) and torch.equal(ints4, ints0[:4])
    assert np.array_equal(emb0.cpu().numpy().view(np.int32), case["W"][case["ids"].reshape(-1)].view(np.int32))


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_layer_norm_forward_within_twice_the_cpu_torch_error(ops, shape, keep):
    case = _case(shape)
    B, T, H, V = shape
    packed, draws, t = _dev(case)
    ints, emb, enc = ops.caption_embed(packed, draws, T, t["W"], mlm=_mlm(ops, case), **_ln_args(case, t, keep))
    _check_ints(case, ints)
    ids = case["want"][0]
    assert np.array_equal(emb.cpu().numpy().view(np.int32), case["W"][ids.reshape(-1)].view(np.int32))
    y64, _, _ = cr.layer_norm_fwd(ids, case["types"], case["W"], case["P"], case["Tt"], case["gamma"], case["beta"], case["eps"],
                                  case["keep"] if keep else None, case["p_drop"])
    err_torch = float(np.abs(_torch_cpu_ln(case, ids, keep).numpy() - y64).max())
    err_kernel = float(np.abs(enc.cpu().numpy().reshape(B, T, H) - y64).max())
    print(f"caption LayerNorm forward {shape} keep={keep}: kernel {err_kernel:.3e}, CPU torch fp32 {err_torch:.3e} (vs float64)")
    assert err_kernel <= 2 * err_torch + ULP(y64)
    if keep:
        assert np.array_equal(enc.cpu().numpy().reshape(B, T, H) == 0, (case["keep"] == 0) | (y64 == 0))


def _bwd_direct(ops, ints, T, H, V, g, dW):
    from locov_amd import _lib
    lib = _lib.load()
    N = ints.shape[1]
    ws = torch.empty(int(lib.locov_caption_embed_bwd_workspace_bytes(N, H, 0)), dtype=torch.uint8, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    _lib.check(lib.locov_caption_embed_bwd(p(ints), N, T, H, V, None, None, None, None, None, None, None, 0.0, None, p(g), p(dW), p(ws), ws.numel(),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locov_caption_embed_bwd")
    return dW


@pytest.mark.parametrize("shape", SHAPES + [(4, 12, 64, 50)])
def test_gather_backward_is_the_sequential_scatter_bit_for_bit(ops, shape):
    case = _case(shape)
    B, T, H, V = shape
    packed, draws, t = _dev(case)
    W = t["W"].clone().requires_grad_(True)
    ints, emb, _ = ops.caption_embed(packed, draws, T, W, mlm=_mlm(ops, case))
    ids = case["want"][0]
    if shape[1] == 12:
        assert (case["ids"] == 7).sum() == 10 and (ids == 7).sum() >= 4                    # one word ten times (the rule replaces some)
    g = np.random.default_rng(5).standard_normal((B * T, H)).astype(np.float32)
    emb.backward(torch.from_numpy(g).cuda())
    want = cr.scatter(ids, g, V)
    assert np.array_equal(W.grad.cpu().numpy().view(np.int32), want.view(np.int32))
    # rows of unused ids are exactly zero even when the buffer held NaN; two runs give the same bits
    gd = torch.from_numpy(g).cuda()
    runs = [_bwd_direct(ops, ints, T, H, V, gd, torch.full((V, H), float("nan"), device="cuda")).cpu().numpy() for _ in range(2)]
    unused = np.setdiff1d(np.arange(V), ids.reshape(-1))
    assert len(unused) > 0 and not runs[0][unused].any() and np.isfinite(runs[0]).all()
    assert np.array_equal(runs[0].view(np.int32), want.view(np.int32)) and np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32))


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [(4, 12, 64, 50)])
def test_layer_norm_backward_within_twice_the_cpu_autograd_error(ops, shape, keep):
    case = _case(shape)
    B, T, H, V = shape
    packed, draws, t = _dev(case)
    ids = case["want"][0]
    rng = np.random.default_rng(6)
    g_enc, g_in = rng.standard_normal((B, T, H)).astype(np.float32), rng.standard_normal((B, T, H)).astype(np.float32)
    # float64 reference: LN backward of the restatement, plus the input_embeddings gradient, scattered in float64
    _, xhat, rstd = cr.layer_norm_fwd(ids, case["types"], case["W"], case["P"], case["Tt"], case["gamma"], case["beta"], case["eps"])
    dx = cr.layer_norm_bwd(g_enc, xhat, rstd, case["gamma"], case["keep"] if keep else None, case["p_drop"]) + g_in.astype(np.float64)
    want = cr.scatter(ids, dx, V, dtype=np.float64)
    # yardstick: CPU torch autograd in fp32
    Wc = torch.from_numpy(case["W"]).clone().requires_grad_(True)
    ((_torch_cpu_ln(case, ids, keep, Wc) * torch.from_numpy(g_enc)).sum() + (Wc[torch.from_numpy(ids)] * torch.from_numpy(g_in)).sum()).backward()
    err_torch = float(np.abs(Wc.grad.numpy() - want).max())

    def run():
        W = t["W"].clone().requires_grad_(True)
        _, emb, enc = ops.caption_embed(packed, draws, T, W, mlm=_mlm(ops, case), **_ln_args(case, t, keep))
        torch.autograd.backward([enc, emb], [torch.from_numpy(g_enc).cuda().view(B * T, H), torch.from_numpy(g_in).cuda().view(B * T, H)])
        return W.grad.cpu().numpy()
    a, b = run(), run()
    err_kernel = float(np.abs(a - want).max())
    print(f"caption LayerNorm backward {shape} keep={keep}: kernel {err_kernel:.3e}, CPU torch autograd fp32 {err_torch:.3e} (vs float64)")
    assert err_kernel <= 2 * err_torch + ULP(want)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))                              # reproducible bits
    unused = np.setdiff1d(np.arange(V), ids.reshape(-1))
    assert not a[unused].any()


def _module(case, shape, add_pos, freeze=True):
    from locov_amd.config import get_cfg
    from locov_amd.language_backbone import build_language_backbone
    from lsm_model_cases import SizedTokenizer
    B, T, H, V = shape
    cfg = get_cfg()
    cfg.MODEL.DEVICE = "cuda"
    lb, tr = cfg.MODEL.LANGUAGE_BACKBONE, cfg.MODEL.MMSS_HEAD.TRANSFORMER
    lb.TYPE, lb.PRETRAINED, lb.ADD_POSITION_EMBEDDING, lb.FREEZE = "build_bertemb_backbone", False, add_pos, freeze
    tr.MASKED_LANGUAGE_MODELING, tr.MASKED_LANGUAGE_MODELING_PROB, tr.MASKED_LANGUAGE_MODELING_PROB_MASK = True, cr.P, cr.P_MASK
    tr.MASKED_LANGUAGE_MODELING_PROB_NOISE = case["p_noise"]
    tr.BERT_CONFIG.update(vocab_size=V, hidden_size=H, max_position_embeddings=case["P"].shape[0])
    m = build_language_backbone(cfg, SizedTokenizer(case["len_tok"], case["mask_id"]))
    body = m.body
    with torch.no_grad():
        body.embeddings.copy_(torch.from_numpy(case["W"]))
        body.bert_model.position_embeddings.weight.copy_(torch.from_numpy(case["P"]))
        body.bert_model.token_type_embeddings.weight.copy_(torch.from_numpy(case["Tt"]))
        body.bert_model.LayerNorm.weight.copy_(torch.from_numpy(case["gamma"]))
        body.bert_model.LayerNorm.bias.copy_(torch.from_numpy(case["beta"]))
    return m


@pytest.mark.parametrize("add_pos", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_module_kernel_path_equals_its_torch_expression_on_the_device(ops, shape, add_pos, monkeypatch):
    case = _case(shape)
    B, T, H, V = shape
    m = _module(case, shape, add_pos).train()
    draws = torch.from_numpy(case["draws"]).cuda()
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("LOCOV_FUSED_CAPTION", fused)
        torch.manual_seed(9)                                                               # the same keep mask on both paths
        out[fused] = m.body.forward_tokenized(cr.tokenized(case), draws)
    a, b = out["1"], out["0"]
    assert list(a) == list(b) == ["input_ids", "token_type_ids", "attention_mask", "special_tokens_mask", "target_ids", "mlm_mask",
                                  "encoded_tokens", "input_embeddings"]
    ids, special, target, mlm_mask = case["want"]
    for k, w in (("input_ids", ids), ("special_tokens_mask", special), ("target_ids", target), ("mlm_mask", mlm_mask),
                 ("token_type_ids", case["types"]), ("attention_mask", case["attn"])):
        assert a[k].dtype == b[k].dtype == torch.int64 and tuple(a[k].shape) == (B, T)
        assert torch.equal(a[k], b[k]) and np.array_equal(a[k].cpu().numpy(), w), k
    assert torch.equal(a["input_embeddings"].view(torch.int32), b["input_embeddings"].view(torch.int32))
    if not add_pos:
        assert a["encoded_tokens"] is a["input_embeddings"] and b["encoded_tokens"] is b["input_embeddings"]
        return
    torch.manual_seed(9)
    keep = (torch.rand((B, T, H), device="cuda") >= m.body.bert_model.dropout.p).cpu().numpy().astype(np.uint8)
    y64, _, _ = cr.layer_norm_fwd(ids, case["types"], case["W"], case["P"], case["Tt"], case["gamma"], case["beta"], case["eps"], keep,
                                  m.body.bert_model.dropout.p)
    kcase = dict(case, keep=keep, p_drop=m.body.bert_model.dropout.p)
    err_torch = float(np.abs(_torch_cpu_ln(kcase, ids, True).numpy() - y64).max())
    for name, o in (("kernel", a), ("device torch expression", b)):
        err = float(np.abs(o["encoded_tokens"].cpu().numpy() - y64).max())
        print(f"module {shape} {name}: {err:.3e} vs float64 (CPU torch fp32 {err_torch:.3e})")
        if name == "kernel":
            assert err <= 2 * err_torch + ULP(y64)


def test_module_trains_the_word_table_and_takes_the_torch_expression_beyond_the_limits(ops):
    from locov_amd._lib import LocovError
    shape = (2, 5, 64, 50)
    case = _case(shape)
    m = _module(case, shape, True, freeze=False).train()
    out = m.body.forward_tokenized(cr.tokenized(case), torch.from_numpy(case["draws"]).cuda())
    (out["encoded_tokens"].sum() + out["input_embeddings"].square().sum()).backward()
    g = m.body.embeddings.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert [n for n, p in m.named_parameters() if p.grad is not None] == ["body.embeddings"]
    # more tokens than the kernel takes: an error of the entry point, the torch expression in the module
    N = ops.CAPTION_MAX_TOKENS + 1
    W = torch.randn(10, 8, device="cuda")
    with pytest.raises(LocovError, match="over the limits"):
        ops.caption_embed(torch.zeros((4, N), dtype=torch.int32, device="cuda"), None, N, W, with_targets=False)
    big = {"input_ids": [[5] * N], "token_type_ids": [[0] * N], "attention_mask": [[1] * N], "special_tokens_mask": [[0] * N]}
    m2 = _module(case, shape, False).eval()
    got = m2.body.forward_tokenized(big)
    assert tuple(got["input_embeddings"].shape) == (1, N, 64) and torch.equal(got["input_embeddings"][0, -1], m2.body.embeddings[5])
