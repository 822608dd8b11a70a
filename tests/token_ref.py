"""float64 torch restatement of the multi-token class scoring, differentiable by autograd.

Written from the algorithm as the header comment of locov_amd/csrc/token_attention.hip states it -- per region r and class k
with n_k real tokens, over the class's Tmax padded slots:
    s_t = sim[r, off_k + t] / temperature                       (cosine: NaN -> 0 first)
    d_t = -s_t (dot)  |  (1 - sim) / temperature (cosine)
    masked s_t = s_t for t < n_k, else gmin - 100                (gmin = min of the zero-padded tensor, a constant)
    a = softmax_t(masked s)  |  one_hot(argmax_t masked s)
    att_t = a_t [t < n_k];   score = -sum_t att_t d_t
It is the yardstick of the GPU tests of the backward kernel; tests/test_token_attention_bwd_capi.py pins it to the vectors
recorded from the reference (g6 forward, g9 gradients) on the CPU."""
import numpy as np
import torch


def layout(ntok, background=True):
    """Column layout of a bank whose classes come in index order: (tok_off [K1], num_tok [K1], Ttot).  A token-less class
    (and the background row) owns one column."""
    counts = [int(n) for n in ntok] + ([0] if background else [])
    off, pos = [], 0
    for n in counts:
        off.append(pos)
        pos += max(n, 1)
    return np.asarray(off, np.int32), np.asarray(counts, np.int32), pos


def padded_min(sim, tok_off, num_tok, tmax, temperature, cosine):
    """gmin: the minimum of the zero-padded [R, K1, Tmax] tensor of s -- every column of sim / temperature (NaN -> 0 under
    cosine), and 0 when any class has a padded slot.  Same dtype as sim, detached."""
    v = sim.detach()
    if cosine:
        v = torch.where(torch.isnan(v), torch.zeros_like(v), v)
    g = (v / temperature).min()
    if any(max(int(n), 1) < tmax for n in num_tok):
        g = torch.minimum(g, torch.zeros_like(g))
    return g


def token_attention(sim, tok_off, num_tok, tmax, temperature, cosine=False, hardmax=False, gmin=None):
    """sim [R, Ttot] (any float dtype; may require grad) -> (scores [R, K1], att [R, K1, tmax]) in float64."""
    sim = sim.double()
    off = torch.as_tensor(np.asarray(tok_off), dtype=torch.int64)
    n = torch.as_tensor(np.asarray(num_tok), dtype=torch.int64)
    if gmin is None:
        gmin = padded_min(sim, tok_off, num_tok, tmax, temperature, cosine)
    gmin = torch.as_tensor(gmin).detach().double().reshape(())
    v = torch.where(torch.isnan(sim), torch.zeros_like(sim), sim) if cosine else sim
    t = torch.arange(tmax)
    mask = t[None, :] < n[:, None]                                              # [K1, tmax]
    cols = (off[:, None] + t[None, :]).clamp(max=sim.shape[1] - 1)
    pad = torch.where(mask[None], v[:, cols], torch.zeros((), dtype=torch.float64))   # [R, K1, tmax]
    s = pad / temperature
    d = ((1.0 - pad) if cosine else -pad) / temperature
    masked = torch.where(mask[None], s, gmin - 100.0)
    if hardmax:
        a = torch.nn.functional.one_hot(masked.argmax(dim=2), tmax).double()
    else:
        a = torch.softmax(masked, dim=2)
    att = a * mask[None].double()
    return -(att * d).sum(dim=2), att


def hardmax_gap(sim, tok_off, num_tok, cosine=False):
    """Smallest gap between the two largest real-token similarities of any (region, class) with at least two tokens."""
    v = sim.detach().double()
    if cosine:
        v = torch.where(torch.isnan(v), torch.zeros_like(v), v)
    gap = float("inf")
    for o, n in zip(np.asarray(tok_off), np.asarray(num_tok)):
        if n >= 2:
            top = v[:, int(o):int(o) + int(n)].topk(2, dim=1).values
            gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
    return gap


def normalize(x, eps=1e-12):
    """F.normalize(p=2, dim=1), differentiable."""
    return x / x.norm(dim=1, keepdim=True).clamp_min(eps)


def grounding_module(image_emb, embs, metric="dot", align="softmax", temperature=1.0, background=True):
    """The module on a bank of per-class token matrices `embs` ([n_k, D] each, index order; normalised per token under
    cosine, as set_class_embeddings does) -- image_emb [R, D] is what the module receives (already normalised under cosine).
    Returns (scores, att, sim) in float64."""
    cosine = metric == "cosine"
    image_emb = image_emb.double()
    pieces = [torch.as_tensor(e).double().reshape(-1, image_emb.shape[1]) for e in embs]
    ntok = [p.shape[0] for p in pieces]
    assert all(ntok), "a token-less class owns no row of the bank (only the background row does)"
    if background:
        pieces.append(torch.zeros(1, image_emb.shape[1], dtype=torch.float64))
    bank = torch.cat(pieces, 0)
    if cosine:
        bank = normalize(bank)
    sim = image_emb @ bank.t()
    off, cnt, _ = layout(ntok, background)
    tmax = max(max(ntok), 1)
    scores, att = token_attention(sim, off, cnt, tmax, temperature, cosine=cosine, hardmax=align == "hardmax")
    return scores, att, sim
