"""TransformerHead at the LSM shape (configs/coco_lsm.yaml: B = 4 per GPU, T = 70 caption tokens, NR = 100 regions, hidden 768,
8 heads of dim 96, intermediate 768, 6 layers, vocabulary 30 522, both dropouts 0.1), forward + backward.

    python tools/transformer_head_step.py [--batch 4] [--iters 30] [--warmup 5] [--out records.json]

Two pairs, each alternating its two sides in one process (device events, median and the 10th / 90th percentile):
  * the attention core alone, 16 sequences of 170 tokens, with a dropout keep mask: ops.mha (csrc/mha.hip) against the composed
    torch chain (LOCOV_FUSED_ATTENTION=0);
  * the whole head in training mode with the LM head on the B * T tokens of the matching pairs (the product) against the whole head
    with the LM head on all B^2 * T tokens and the diagonal taken afterwards, as the reference runs it.  The latter exists in this
    tool only (`forward_all_tokens`).
Also printed: the device kernels one forward + backward enqueues on each side (torch.profiler, a run of its own), peak memory above
the resident state, and the attention kernels' achieved FLOP/s (the MFMA work they execute: 4 N H S^2 d forward, 18 N H S^2 d for the two
backward launches, whose three sweeps each recompute S and dP) over the pair's device-event time, as a fraction of the f32-MFMA rate given with --peak-tflops.
Needs a ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

T, NR, V_DIM, L, LOC, HEADS, LAYERS, INTER, VOCAB = 70, 100, 2048, 768, 2, 8, 6, 768, 30522


def _cfg():
    ns = types.SimpleNamespace
    bert = dict(vocab_size=VOCAB, hidden_size=L, num_hidden_layers=LAYERS, num_attention_heads=HEADS, intermediate_size=INTER,
                hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, initializer_range=0.02, layer_norm_eps=1e-12)
    t = ns(MVM_LOSS="", MMM_LOSS="cross_entropy", MVM_LOSS_NUM_NEGATIVE=128, BERT_CONFIG=bert, pretrained_weights=False)
    return ns(MODEL=ns(MMSS_HEAD=ns(TRANSFORMER=t, DISTILLATION_LOSS=True)))


class _Backbone(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embeddings = torch.nn.Parameter(torch.randn(VOCAB, L) * 0.02)


class _Env:
    def __init__(self, fused: bool):
        self.fused = fused

    def __enter__(self):
        self.old = os.environ.get("LOCOV_FUSED_ATTENTION")
        os.environ["LOCOV_FUSED_ATTENTION"] = "1" if self.fused else "0"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("LOCOV_FUSED_ATTENTION", None)
        else:
            os.environ["LOCOV_FUSED_ATTENTION"] = self.old


def make_inputs(B, device, seed):
    g = torch.Generator().manual_seed(seed)
    cmask = torch.ones(B, T, dtype=torch.int64)
    for b in range(B):
        cmask[b, int(torch.randint(12, T, (1,), generator=g)):] = 0
    mlm = ((torch.rand(B, T, generator=g) < 0.15) & (cmask > 0)).to(torch.int64)
    mlm[:, 1] = 1
    d = {"region_features": torch.relu(torch.randn(B, NR, V_DIM, generator=g)) * 0.05, "region_mask": torch.ones(B, NR, dtype=torch.uint8),
         "region_loc": torch.rand(B, NR, LOC, generator=g), "encoded_tokens": torch.randn(B, T, L, generator=g),
         "attention_mask": cmask, "mlm_mask": mlm, "target_ids": torch.randint(0, VOCAB, (B, T), generator=g)}
    return {k: v.to(device) for k, v in d.items()}


def forward_all_tokens(head, inp):
    """The head's forward with the LM head on all B^2 * T tokens, the diagonal pairs taken from its scores (transformer_head.py:182-206
    of the reference); everything else as the product.  Returns the summed losses."""
    from locov_amd.transformer_head import _lin
    B = inp["region_features"].shape[0]
    cmask, rmask = inp["attention_mask"].float(), inp["region_mask"].float()
    img = head.visual_emb(_lin(inp["region_features"], head.v2l_projection), inp["region_loc"])
    P, S = B * B, T + NR
    img = img[None].expand(B, B, NR, L).reshape(P, NR, L)
    cap = inp["encoded_tokens"][:, None].expand(B, B, T, L).reshape(P, T, L)
    bias = torch.cat([cmask[:, None].expand(B, B, T).reshape(P, T), rmask[None].expand(B, B, NR).reshape(P, NR)], dim=1).contiguous()
    seq = head.encoder(torch.cat([cap, img], dim=1).reshape(P * S, L), bias).view(P, S, L)
    scores = head.heads.predictions(seq[:, :T].reshape(P * T, L))                          # [B^2 * T, vocabulary]
    scores = torch.diagonal(scores.view(B, B, T, VOCAB), dim1=0, dim2=1).permute(2, 0, 1)
    target = torch.where(inp["mlm_mask"] > 0, inp["target_ids"], torch.full_like(inp["target_ids"], -1))
    mlm = F.cross_entropy(scores.reshape(-1, VOCAB), target.reshape(-1), ignore_index=-1)
    pw = _lin(head.pooler(seq[:, 0]), head.heads.bi_seq_relationship)[:, 0].reshape(B, B)
    return mlm + torch.diag(-torch.log_softmax(-pw, dim=0)).mean() + torch.diag(-torch.log_softmax(-pw, dim=1)).mean()


def head_step(head, inputs, all_tokens: bool):
    def step(i):
        inp = inputs[i % len(inputs)]
        head.zero_grad(set_to_none=True)
        if all_tokens:
            forward_all_tokens(head, inp).backward()
        else:
            _, losses, dist = head(inp, inp)
            sum(losses.values()).backward()
    return step


def core_step(B, device, fused: bool, seed=0):
    from locov_amd import transformer_head as th
    n, S, E = B * B, T + NR, L
    g = torch.Generator().manual_seed(seed)
    sets = []
    for _ in range(3):                                                                      # fresh operands from call to call
        qkv = torch.randn(n * S, 3 * E, generator=g).to(device).requires_grad_(True)
        sets.append((qkv, torch.ones(n, S, device=device), (torch.rand(n, HEADS, S, S, generator=g) >= 0.1).to(torch.uint8).to(device),
                     torch.randn(n * S, E, generator=g).to(device)))

    def step(i):
        qkv, bias, keep, gout = sets[i % len(sets)]
        qkv.grad = None
        with _Env(fused):
            th.attention_core(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], bias, HEADS, keep=keep, p_drop=0.1).backward(gout)
    return step


def alternate(sides, iters, warmup):
    """sides: name -> step(i).  Device-event time of each call, the sides alternating (and swapping order) in one process."""
    ms = {k: [] for k in sides}
    names = list(sides)
    for it in range(warmup + iters):
        for name in (names if it % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sides[name](it)
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[name].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
            for k, v in ms.items()}


def kernels_and_peak(step):
    from torch.profiler import ProfilerActivity, profile
    step(0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(1)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        step(2)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    mha = [e for e in ev if "mha_" in e.name]
    return {"device_kernels": len(ev), "locov_mha_kernels": len(mha), "mha_kernel_us": float(sum(e.device_time for e in mha)),
            "peak_bytes": int(peak)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="f32-input MFMA peak: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz")
    ap.add_argument("--skip-head", action="store_true")
    ap.add_argument("--out", default=None, help="also write the record as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("transformer_head_step: needs a ROCm GPU")
    from locov_amd.transformer_head import TransformerHead
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B = args.batch
    rec = {"B": B, "T": T, "NR": NR, "device": torch.cuda.get_device_name(dev)}

    core = {"fused": core_step(B, dev, True), "composed": core_step(B, dev, False)}
    rec["core_kernels"] = {k: kernels_and_peak(s) for k, s in core.items()}
    rec["core"] = alternate(core, args.iters, args.warmup)
    flops = 22.0 * (B * B) * HEADS * (T + NR) ** 2 * (L // HEADS)
    rec["core_mha_flops"] = flops
    rec["core_fused_tflops_over_event_time"] = flops / (rec["core"]["fused"]["median_ms"] * 1e-3) / 1e12
    kus = rec["core_kernels"]["fused"]["mha_kernel_us"]
    if kus > 0:
        rec["core_fused_tflops_over_kernel_time"] = flops / (kus * 1e-6) / 1e12
        rec["core_fused_fraction_of_f32_mfma_peak"] = rec["core_fused_tflops_over_kernel_time"] / args.peak_tflops
    print(json.dumps({k: rec[k] for k in rec if k.startswith("core")}), flush=True)

    if not args.skip_head:
        torch.manual_seed(0)
        head = TransformerHead(_cfg(), V_DIM, L, LOC, _Backbone()).to(dev).train()
        inputs = [make_inputs(B, dev, s) for s in range(3)]
        sides = {"diagonal_lm_head": head_step(head, inputs, False), "all_tokens_lm_head": head_step(head, inputs, True)}
        rec["head_kernels"] = {k: kernels_and_peak(s) for k, s in sides.items()}
        rec["head"] = alternate(sides, args.iters, args.warmup)
        with _Env(False):
            rec["head_composed_attention"] = alternate({"diagonal_lm_head": sides["diagonal_lm_head"]}, max(args.iters // 2, 1), 2)
        print(json.dumps({k: rec[k] for k in rec if k.startswith("head")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
