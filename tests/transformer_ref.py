"""Re-statement of TransformerHead (ovr/modeling/mmss_heads/transformer_head.py:105-254 over a BERT encoder) with plain torch
ops in whatever dtype its inputs have -- float64 is the yardstick of tests/test_gpu_mha.py and tests/test_gpu_transformer_head.py,
float32 on the CPU is the "same precision, other summation order" chain their gates are sized from.  Written from the
arithmetic, reads nothing of the reference:

    scores = q k^T / sqrt(d) + mask            the raw 0 / 1 attention mask is ADDED (padded keys are not excluded)
    a = LN(dense(ctx) + x);  x' = LN(dense(gelu(dense(a))) + a)          post-LN, erf-GELU, LayerNorm eps 1e-12
    pooled = tanh(dense(x[:, 0]));  LM head = dense -> gelu -> LN -> decoder (weight backbone.embeddings, bias heads.predictions.bias)
    cost = bi_seq_relationship(pooled)[:, 0] as [B, B], rows = captions

tests/test_transformer_head_host.py pins it to the reference's own outputs (tests/golden/g10_transformer_head.npz)."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-12
GRAD_NAMES = ("v2l_projection.weight", "encoder.layer.0.attention.self.query.weight", "encoder.layer.1.output.dense.weight",
              "pooler.dense.weight", "backbone.embeddings")


def attention(q, k, v, bias, num_heads, scale=None, keep=None, p_drop=0.0):
    """dropout(softmax(q k^T * scale + bias[n, key])) v for q, k, v [Nseq * S, H * d] and bias [Nseq, S]; keep: [Nseq, H, S, S]."""
    nseq, S = bias.shape
    E = q.shape[1]
    d = E // num_heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    heads = lambda t: t.reshape(nseq, S, num_heads, d).permute(0, 2, 1, 3)
    p = torch.softmax(torch.matmul(heads(q), heads(k).transpose(-1, -2)) * scale + bias.to(q.dtype)[:, None, None, :], dim=-1)
    if keep is not None:
        p = p * keep.to(p.dtype) / (1.0 - p_drop)
    return torch.matmul(p, heads(v)).permute(0, 2, 1, 3).reshape(nseq * S, E)


def _lin(x, sd, name):
    return x @ sd[name + ".weight"].t() + sd[name + ".bias"]


def _ln(x, sd, name):
    return F.layer_norm(x, x.shape[-1:], sd[name + ".weight"], sd[name + ".bias"], EPS)


def head_forward(sd, inputs, num_heads, num_layers, mmm_loss="cross_entropy"):
    """sd: name -> tensor (the module's state dict; those that require grad receive gradients), inputs: the forward's input keys.
    Returns (losses, other_info, pw_cost) with the reference's key strings."""
    dt = sd["v2l_projection.weight"].dtype
    cap = inputs["encoded_tokens"].to(dt)
    cmask = inputs["attention_mask"].to(dt)
    rmask = inputs["region_mask"].to(dt)
    mlm_mask, target_ids = inputs["mlm_mask"], inputs["target_ids"]
    target = torch.where(mlm_mask > 0, target_ids, torch.full_like(target_ids, -1))
    B, NR, _ = inputs["region_features"].shape
    T = cmask.shape[1]
    img = _lin(inputs["region_features"].to(dt), sd, "v2l_projection")
    img = _ln(_lin(img, sd, "visual_emb.image_embeddings") + _lin(inputs["region_loc"].to(dt), sd, "visual_emb.image_location_embeddings"),
              sd, "visual_emb.LayerNorm")
    E = img.shape[-1]
    if mmm_loss == "cross_entropy":                         # pair p = i * B + j is (caption i, image j)
        P = B * B
        img = img[None].expand(B, B, NR, E).reshape(P, NR, E)
        cap = cap[:, None].expand(B, B, T, E).reshape(P, T, E)
        rmask = rmask[None].expand(B, B, NR).reshape(P, NR)
        cmask = cmask[:, None].expand(B, B, T).reshape(P, T)
    else:
        P = B
    S = T + NR
    x = torch.cat([cap, img], dim=1).reshape(P * S, E)
    bias = torch.cat([cmask, rmask], dim=1)
    for i in range(num_layers):
        pre = f"encoder.layer.{i}."
        q, k, v = (_lin(x, sd, pre + "attention.self." + n) for n in ("query", "key", "value"))
        ctx = attention(q, k, v, bias, num_heads)
        a = _ln(_lin(ctx, sd, pre + "attention.output.dense") + x, sd, pre + "attention.output.LayerNorm")
        x = _ln(_lin(F.gelu(_lin(a, sd, pre + "intermediate.dense")), sd, pre + "output.dense") + a, sd, pre + "output.LayerNorm")
    x = x.reshape(P, S, E)
    pooled = torch.tanh(_lin(x[:, 0], sd, "pooler.dense"))
    seq_t = x[:, :T]
    if mmm_loss == "cross_entropy":
        eye = torch.arange(B)
        seq_t = seq_t.reshape(B, B, T, E)[eye, eye]
    h = _ln(F.gelu(_lin(seq_t, sd, "heads.predictions.transform.dense")), sd, "heads.predictions.transform.LayerNorm")
    logits = h @ sd["backbone.embeddings"].t() + sd["heads.predictions.bias"]
    V = logits.shape[-1]
    mlm = F.cross_entropy(logits.reshape(-1, V), target.reshape(-1), ignore_index=-1)
    losses = {"Masked Language Modeling Loss": mlm}
    acc_num = (logits.argmax(dim=-1) == target).to(dt).sum()
    acc_den = (target >= 0).to(dt).sum()
    info = {"Masked Language Modeling Accuracy": torch.where(acc_den > 0, acc_num / acc_den.clamp(min=1), acc_den)}
    pw = None
    if mmm_loss == "cross_entropy":
        pw = _lin(pooled, sd, "heads.bi_seq_relationship")[:, 0].reshape(B, B)
        eye = torch.arange(B)
        losses["Image Caption Matching Loss"] = torch.diag(-torch.log_softmax(-pw, dim=0)).mean() + \
            torch.diag(-torch.log_softmax(-pw, dim=1)).mean()
        info["Batch Accuracy (Choose Caption)"] = (pw.argmin(dim=0) == eye).to(dt).mean()
        info["Batch Accuracy (Choose Image)"] = (pw.argmin(dim=1) == eye).to(dt).mean()
    else:
        losses["Image Caption Matching Loss"] = torch.zeros((), dtype=dt)
    return losses, info, pw


def attention_entropy(sd, inputs, num_heads, num_layers):
    """Mean entropy of the attention rows over layers, pairs, heads and queries (float64), and log S: what the fixture's generator
    asserts on, so that the pinned outputs depend on where the attention looks."""
    sd = {k: v.double() for k, v in sd.items()}
    ent = []
    orig = torch.softmax

    def spy(x, dim=-1, **kw):
        p = orig(x, dim=dim, **kw)
        if p.dim() == 4:
            ent.append(-(p * torch.log(p.clamp(min=1e-300))).sum(-1).mean())
        return p

    torch.softmax = spy
    try:
        head_forward(sd, inputs, num_heads, num_layers)
    finally:
        torch.softmax = orig
    S = inputs["attention_mask"].shape[1] + inputs["region_mask"].shape[1]
    return float(torch.stack(ent).mean()), math.log(S)
