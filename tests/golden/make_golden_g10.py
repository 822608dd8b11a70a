#!/usr/bin/env python
"""
Generates tests/golden/g10_transformer_head.npz by running the REFERENCE's own TransformerHead under autograd on the CPU
(ovr/modeling/mmss_heads/transformer_head.py:22-303 over the installed `transformers` BERT layers, loaded as make_golden.py loads
the grounding head).

    python tests/golden/make_golden_g10.py            # needs the reference checkout (LOCOV_REFERENCE) and `transformers`

One state dict (hidden 64, 2 layers, intermediate 64, vocabulary 100, v_dim 40, loc_dim 2, both dropouts 0.0, MMM_LOSS
"cross_entropy", DISTILLATION_LOSS on) is run as two configurations that differ in the number of heads only -- "h2": 2 heads of
dim 32, "h1": 1 head of dim 64 -- so that two head dims of the attention kernel are pinned by the same 290 KB of weights.
(The attention kernel takes head dims 32, 64, 96 and 128: 4 heads at hidden 64 would be dim 16, and a second state dict at hidden
256 does not fit a committed file.)

The query / key weights of every layer (std 0.25), the value / attention-output weights (std 0.15), every bias and LayerNorm
parameter and the inputs are redrawn: with the reference's init (std 0.02, zero biases) the softmax is nearly uniform, the
attention output drowns in the residual and an attention bug would not show.  The script asserts that the mean attention entropy is
below 0.7 log S.  heads.predictions.decoder.bias is made the same parameter as heads.predictions.bias, the tying of the library
the reference was written against (the installed one leaves them apart, both zero at init, so the reference's values are the same).

Cases: B in {1, 3} with T = 12 tokens and NR = 27 regions (S = 39), ragged caption and region masks including a caption with one
real token, and for "h2", B = 3 once more with an all-zero mlm_mask ("_zero": NaN MLM loss, accuracy 0, no gradients stored).

Stored: `keys` (the state-dict key list) and `sd/<key>`; `cfg` (json); per B the inputs `b<B>_<name>`; per case `<tag>_b<B>_`:
trans, loss_names / losses, info_names / info, `grad/<name>` of (sum of the two losses) for transformer_ref.GRAD_NAMES; and for
every stored output `<...>_f64_diff...` = max |reference fp32 - float64 restatement (tests/transformer_ref.py)|, what a gate on
these vectors has to leave room for.  The fixture holds inputs, weights, outputs and names only.
"""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg          # noqa: E402  (its loaders; it writes nothing on import)
import transformer_ref as tr      # noqa: E402

HIDDEN, LAYERS, INTER, VOCAB, V_DIM, LOC_DIM, T, NR = 64, 2, 64, 100, 40, 2, 12, 27
HEADS = {"h2": 2, "h1": 1}


class _N(dict):
    __getattr__ = dict.__getitem__


def _cfg(heads):
    bert = dict(vocab_size=VOCAB, hidden_size=HIDDEN, num_hidden_layers=LAYERS, num_attention_heads=heads, intermediate_size=INTER,
                hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, max_position_embeddings=512,
                type_vocab_size=2, initializer_range=0.02, layer_norm_eps=1e-12, pad_token_id=0)
    t = dict(MVM_LOSS="", MMM_LOSS="cross_entropy", MVM_LOSS_NUM_NEGATIVE=128, BERT_CONFIG=bert, pretrained_weights=False)
    return t, _N(MODEL=_N(MMSS_HEAD=_N(TRANSFORMER=_N({**t, "BERT_CONFIG": _N(bert)}), DISTILLATION_LOSS=True)))


class _Backbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.embeddings = nn.Parameter(torch.zeros(VOCAB, HIDDEN))


def _inputs(B, g):
    cmask = torch.ones(B, T, dtype=torch.int64)
    rmask = torch.ones(B, NR, dtype=torch.uint8)
    for i in range(B):
        cmask[i, T - 4 * i:] = 0
        rmask[i, NR - 7 * i:] = 0
    if B > 1:
        cmask[B - 1, 1:] = 0                                   # a caption with one real token
    mlm = ((torch.rand(B, T, generator=g) < 0.4) & (cmask > 0)).to(torch.int64)
    mlm[:, 0] = 1
    return {"region_features": torch.randn(B, NR, V_DIM, generator=g), "region_mask": rmask,
            "region_loc": torch.rand(B, NR, LOC_DIM, generator=g), "mvm_mask": torch.zeros(B, NR),
            "target_region_features": torch.zeros(B, NR, V_DIM), "encoded_tokens": torch.randn(B, T, HIDDEN, generator=g),
            "attention_mask": cmask, "mlm_mask": mlm, "target_ids": torch.randint(0, VOCAB, (B, T), generator=g)}


IMAGE_KEYS = ("region_features", "region_mask", "region_loc", "mvm_mask", "target_region_features")


def main():
    assert os.path.isdir(mg.REF), f"reference not found at {mg.REF}"
    mg.install_standins()
    mg.cuda_to_cpu_shim()
    mg.load("ovr.misc", "ovr/misc.py")
    mg.load("ovr.modeling.logged_module", "ovr/modeling/logged_module.py")
    mg.load("ovr.modeling.mmss_heads.grounding_head", "ovr/modeling/mmss_heads/grounding_head.py")
    th = mg.load("ovr.modeling.mmss_heads.transformer_head", "ovr/modeling/mmss_heads/transformer_head.py")

    g = torch.Generator().manual_seed(mg.SEED + 10)
    out = {"seed": mg.SEED + 10}
    heads_of = {}
    for tag, h in HEADS.items():
        plain, cfg = _cfg(h)
        torch.manual_seed(mg.SEED + 10)
        head = th.TransformerHead(cfg, V_DIM, HIDDEN, LOC_DIM, _Backbone())
        head.heads.predictions.decoder.bias = head.heads.predictions.bias
        heads_of[tag] = head
        out["cfg_" + tag] = np.asarray(json.dumps(plain))
    first = heads_of["h2"]
    with torch.no_grad():
        for name, p in first.named_parameters():
            if name.endswith("LayerNorm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif ".attention.self.query." in name or ".attention.self.key." in name:
                p.copy_(0.25 * torch.randn(p.shape, generator=g))
            elif ".attention.self.value." in name or ".attention.output.dense." in name:
                p.copy_(0.15 * torch.randn(p.shape, generator=g))
            elif name == "backbone.embeddings":
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif name.startswith("v2l_projection") or name.startswith("visual_emb"):
                p.copy_(0.15 * torch.randn(p.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in first.state_dict().items()}
    heads_of["h1"].load_state_dict(sd, strict=True)
    out["keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        out["sd/" + k] = v.numpy()
    assert sd["heads.predictions.decoder.weight"].data_ptr() != 0 and torch.equal(sd["heads.predictions.decoder.weight"], sd["backbone.embeddings"])

    inputs = {}
    for B in (1, 3):
        inputs[B] = _inputs(B, g)
        for k, v in inputs[B].items():
            out[f"b{B}_{k}"] = v.numpy()

    for tag, h in HEADS.items():
        head = heads_of[tag]
        for B, zero in ((1, False), (3, False)) + (((3, True),) if tag == "h2" else ()):
            inp = dict(inputs[B])
            if zero:
                inp["mlm_mask"] = torch.zeros_like(inp["mlm_mask"])
            head.zero_grad()
            info, losses, dist = head({k: inp[k] for k in IMAGE_KEYS}, {k: v for k, v in inp.items() if k not in IMAGE_KEYS})
            sd64 = {k: v.double().clone().requires_grad_(k in tr.GRAD_NAMES) for k, v in sd.items()}
            l64, i64, pw64 = tr.head_forward(sd64, inp, h, LAYERS)
            p = f"{tag}_b{B}_" + ("zero_" if zero else "")
            out[p + "trans"] = dist["trans"].detach().numpy()
            out[p + "trans_f64_diff"] = np.float64((dist["trans"].detach().double() - pw64.detach()).abs().max())
            assert list(losses) == list(l64) and list(info) == list(i64)
            out[p + "loss_names"] = np.array(list(losses))
            out[p + "losses"] = np.array([float(v.detach()) for v in losses.values()], np.float32)
            out[p + "losses_f64_diff"] = np.array([abs(float(v.detach()) - float(l64[k].detach())) for k, v in losses.items()], np.float64)
            out[p + "info_names"] = np.array(list(info))
            out[p + "info"] = np.array([float(v) for v in info.values()], np.float32)
            assert [np.float32(float(v)) for v in info.values()] == [np.float32(float(v)) for v in i64.values()], (p, info, i64)
            print(p, {k: float(v.detach()) for k, v in losses.items()}, {k: float(v) for k, v in info.items()},
                  "f64 diff trans", float(out[p + "trans_f64_diff"]), "losses", out[p + "losses_f64_diff"])
            if zero:
                assert np.isnan(out[p + "losses"][0]) and out[p + "info"][0] == 0.0
                continue
            ent, log_s = tr.attention_entropy(sd, inp, h, LAYERS)
            assert ent < 0.7 * log_s, (p, ent, log_s)
            sum(losses.values()).backward()
            sum(l64.values()).backward()
            params = dict(head.named_parameters())
            for name in tr.GRAD_NAMES:
                got, want = params[name].grad, sd64[name].grad
                out[p + "grad/" + name] = got.numpy().copy()
                out[p + "grad_f64_diff/" + name] = np.float64((got.double() - want).abs().max())
                print(f"   {name}: max|grad| {float(got.abs().max()):.4g}  max|fp32 - f64| {float(out[p + 'grad_f64_diff/' + name]):.3g}")
            print(f"   attention entropy {ent:.3f} of log S = {log_s:.3f}")
    path = os.path.join(HERE, "g10_transformer_head.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
