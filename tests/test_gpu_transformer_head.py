"""locov_amd.TransformerHead on the device against the float64 re-statement (tests/transformer_ref.py) on the weights and inputs of
tests/golden/g10_transformer_head.npz -- the reference's own run, which tests/test_transformer_head_host.py pins the re-statement to.

Gate per quantity: 8 x the fixture's recorded max |reference fp32 - float64| for that quantity plus one fp32 ulp of its largest
magnitude (the recorded diff is ONE draw of fp32 rounding through another summation order over two layers)."""
import functools
import json
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import transformer_ref as tr
from test_transformer_head_host import CASES, G10, inputs, make_head, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cuda(inp):
    return {k: v.to(DEV) for k, v in inp.items()}


def _head(tag="h2", distill=True, **over):
    head = make_head(tag, distill, **over)
    head.load_state_dict(state_dict(), strict=True)
    return head.to(DEV)


@functools.lru_cache(maxsize=None)
def _f64(tag, B, zero):
    heads = json.loads(str(G10["cfg_" + tag]))["BERT_CONFIG"]["num_attention_heads"]
    sd = {k: v.double().requires_grad_(k in tr.GRAD_NAMES) for k, v in state_dict().items()}
    losses, info, pw = tr.head_forward(sd, inputs(B, zero), heads, 2)
    if not zero:
        sum(losses.values()).backward()
    return ({k: v.detach() for k, v in losses.items()}, info, pw.detach(), {n: sd[n].grad for n in tr.GRAD_NAMES})


def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


@pytest.mark.parametrize("tag,B,zero", [c for c in CASES if not c[2]])
def test_matches_float64(tag, B, zero):
    p = f"{tag}_b{B}_"
    want_losses, want_info, want_pw, want_grads = _f64(tag, B, False)
    head = _head(tag)
    assert head.heads.predictions.decoder.weight is head.backbone.embeddings          # .to(device) keeps the tie
    inp = _cuda(inputs(B))
    info, losses, dist = head(inp, inp)
    assert list(losses) == list(want_losses) and list(info) == list(want_info) and list(dist) == ["trans"]
    sum(losses.values()).backward()
    failed = []

    def gate(name, got, want, recorded):
        err = float((got.detach().cpu().double() - want).abs().max())
        bound = 8.0 * float(recorded) + _ulp(want.abs().max())
        print(f"{p}{name}: err {err:.3e}  recorded fp32-f64 diff {float(recorded):.3e}  bound {bound:.3e}")
        if not err <= bound:
            failed.append((name, err, bound))
    gate("trans", dist["trans"], want_pw, G10[p + "trans_f64_diff"])
    for (name, got), rec in zip(losses.items(), G10[p + "losses_f64_diff"]):
        gate(name, got, want_losses[name], rec)
    params = dict(head.named_parameters())
    for name in tr.GRAD_NAMES:
        gate("grad " + name, params[name].grad, want_grads[name], G10[p + "grad_f64_diff/" + name])
    for name, got in info.items():                                                     # the three accuracies: exact
        assert np.float32(float(got)) == np.float32(float(want_info[name])) == G10[p + "info"][list(info).index(name)], name
    assert head.log_info.keys() == {**losses, **info}.keys()
    assert not failed, failed


def test_all_zero_mlm_mask_gives_nan_loss_and_zero_accuracy():
    p = "h2_b3_zero_"
    head = _head("h2")
    inp = _cuda(inputs(3, True))
    info, losses, dist = head(inp, inp)
    assert np.isnan(G10[p + "losses"][0]) and G10[p + "info"][0] == 0.0               # as pinned from the reference
    assert torch.isnan(losses["Masked Language Modeling Loss"]) and float(info["Masked Language Modeling Accuracy"]) == 0.0
    want = _f64("h2", 3, True)
    icm = "Image Caption Matching Loss"
    assert abs(float(losses[icm]) - float(want[0][icm])) <= 8.0 * float(G10[p + "losses_f64_diff"][1]) + _ulp(want[0][icm])
    assert float((dist["trans"].cpu().double() - want[2]).abs().max()) <= 8.0 * float(G10[p + "trans_f64_diff"]) + _ulp(want[2].abs().max())


def test_weights_are_read_at_call_time_and_the_decoder_gradient_reaches_the_embeddings():
    head, other = _head("h2"), torch.nn.Linear(40, 64).to(DEV)
    inp = _cuda(inputs(3))
    before = head(inp, inp)[2]["trans"].detach().clone()
    head.v2l_projection.weight = other.weight                                          # the meta-architecture's tying
    head.v2l_projection.bias = other.bias
    _, losses, dist = head(inp, inp)
    assert not torch.equal(dist["trans"], before)
    sum(losses.values()).backward()
    assert other.weight.grad is not None and float(other.weight.grad.abs().max()) > 0
    emb = head.backbone.embeddings
    assert emb.grad is not None and float(emb.grad.abs().max()) > 0
    assert head.heads.predictions.bias.grad is not None and float(head.heads.predictions.bias.grad.abs().max()) > 0


def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_launch_counts_and_no_host_read(monkeypatch):
    monkeypatch.delenv("LOCOV_FUSED_ATTENTION", raising=False)
    head = _head("h2")
    inp = _cuda(inputs(3))                                                             # (made once: the upload itself waits for the host)

    def fwd():
        _, losses, dist = head(inp, inp)
        return sum(losses.values()) + (dist["trans"] * 0.01).sum()
    fwd().backward()                                                                   # (warm)
    total, f = _device_kernels(fwd)
    assert sum("mha_fwd_kernel" in n for n in f) == 2, f                               # one launch per layer
    assert not any("mha_bwd_kernel" in n for n in f), f
    _, b = _device_kernels(lambda: total.backward())
    assert sum("mha_bwd_kernel" in n for n in b) == 4, b                               # dQ, then dK / dV, per layer
    assert not any("mha_fwd_kernel" in n for n in b), b
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                            # forward and backward enqueue without a host read
    try:
        fwd().backward()
        head.train()
        fwd().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_no_s_by_s_tensor_is_allocated(monkeypatch):
    """Peak memory of the attention core, forward + backward, at the LSM shape (16, 8, 170, 96) against the composed path: the fused
    core allocates its row-sized results (ctx, dQ, dK, dV) and two [N, H, S] vectors, nothing of size [N, H, S, S]."""
    from locov_amd import transformer_head as th
    nseq, H, S, d = 16, 8, 170, 96
    g = torch.Generator().manual_seed(5)
    E = H * d
    q, k, v = (torch.randn(nseq * S, E, generator=g).to(DEV).requires_grad_(True) for _ in range(3))
    bias = torch.ones(nseq, S, device=DEV)
    gout = torch.randn(nseq * S, E, generator=g).to(DEV)
    s_by_s, rows, vec = nseq * H * S * S * 4, nseq * S * E * 4, nseq * H * S * 4

    def peak():
        q.grad = k.grad = v.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        th.attention_core(q, k, v, bias, H).backward(gout)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    monkeypatch.setenv("LOCOV_FUSED_ATTENTION", "0")
    composed = peak()
    monkeypatch.delenv("LOCOV_FUSED_ATTENTION")
    fused = peak()
    print(f"peak bytes above the operands: fused {fused}, composed {composed}; one [N, H, S, S] fp32 tensor {s_by_s}, one row matrix {rows}")
    # (slack: a quarter of one [N, H, S, S] tensor -- allocator rounding and bookkeeping fit, a tensor of that size does not)
    assert fused <= 4 * rows + 2 * vec + s_by_s // 4
    assert composed - fused >= s_by_s                                                  # the composed path keeps at least the probabilities


def test_training_dropout_is_reproducible_under_a_seed():
    p0 = _head("h2").train()
    drop = _head("h2", **{"BERT_CONFIG": {**json.loads(str(G10["cfg_h2"]))["BERT_CONFIG"], "attention_probs_dropout_prob": 0.1}}).train()
    inp = _cuda(inputs(3))

    def run(head, seed):
        head.zero_grad()
        torch.manual_seed(seed)
        _, losses, dist = head(inp, inp)
        sum(losses.values()).backward()
        return [dist["trans"].detach().clone()] + [v.detach().clone() for v in losses.values()] + \
            [dict(head.named_parameters())[n].grad.clone() for n in tr.GRAD_NAMES]
    a, b, c = run(drop, 7), run(drop, 7), run(p0, 7)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[3], c[3])
    assert all(torch.isfinite(x).all() for x in a)


@pytest.mark.parametrize("cls", ["MultiDistillLoss", "MultiDistillLossJS", "MultiDistillLossL2"])
def test_distillation_wiring_end_to_end(cls):
    """distill_prop_mmss_gcnn.py:424-442 with real costs: the module's `trans` and GroundingHead's w2r / r2w on the same batch."""
    from locov_amd import distill_losses
    from locov_amd.grounding_head import GroundingHead
    g = ns(LOCAL_METRIC="dot", GLOBAL_METRIC="aligned_local", ALIGNMENT="softmax", ALIGNMENT_TEMPERATURE=10.0, LOSS="cross_entropy",
           NEGATIVE_MINING="random", TRIPLET_MARGIN=1.0, ALIGN_WORDS_TO_REGIONS=True, ALIGN_REGIONS_TO_WORDS=True,
           TEXT_INPUT="input_embeddings")
    grounding = GroundingHead(ns(MODEL=ns(MMSS_HEAD=ns(GROUNDING=g, DISTILLATION_LOSS=True))), 40, 64).to(DEV)
    trans_head = _head("h2")
    trans_head.v2l_projection.weight = grounding.v2l_projection.weight                  # TIE_VL_PROJECTION_WEIGHTS
    trans_head.v2l_projection.bias = grounding.v2l_projection.bias
    inp = _cuda(inputs(3))
    cap = {**inp, "input_embeddings": inp["encoded_tokens"], "special_tokens_mask": torch.zeros_like(inp["attention_mask"])}
    _, g_losses, g_dist = grounding(inp, cap)
    _, t_losses, t_dist = trans_head(inp, cap)
    loss = getattr(distill_losses, cls)(10.0)(t_dist["trans"], g_dist["w2r"], g_dist["r2w"])
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    (loss + sum(g_losses.values()) + sum(v for v in t_losses.values())).backward()
    for p in (grounding.v2l_projection.weight, trans_head.pooler.dense.weight, trans_head.encoder.layer[0].attention.self.key.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    only = torch.autograd.grad(getattr(distill_losses, cls)(10.0)(trans_head(inp, cap)[2]["trans"], g_dist["w2r"].detach(),
                                                                   g_dist["r2w"].detach()), trans_head.pooler.dense.weight)[0]
    assert float(only.abs().max()) > 0                                                 # the distillation loss itself reaches the transformer
