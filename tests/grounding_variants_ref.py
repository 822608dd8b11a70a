"""float64 torch re-statement of GroundingHead.forward's variants (ovr/modeling/mmss_heads/grounding_head.py:150-251 the
alignment and the [caption, image] costs, :279-343 the triplet loss, :264-277 the cross-entropy one, :357-377 the accuracies) for
LOCAL_METRIC "dot", GLOBAL_METRIC "aligned_local", ALIGNMENT softmax | hardmax, LOSS cross_entropy | triplet, either direction
optional.  It is the yardstick of tests/test_gpu_grounding_variants.py; tests/test_grounding_variants_capi.py ties it to the
reference's own outputs (tests/golden/g8_grounding_variants.npz).  Everything is differentiable torch in the dtype of its inputs."""
import torch


def pair_blocks(S, B, T, NR):
    """S [B*T, B*NR] -> [B (caption), B (image), T, NR]."""
    return S.view(B, T, B, NR).permute(0, 2, 1, 3)


def masked_similarity(S, cmask, rmask, temperature):
    """:152-160: similarities over the temperature, the pairs outside the masks filled with (global min - 100)."""
    B, T = cmask.shape
    NR = rmask.shape[1]
    sim = pair_blocks(S, B, T, NR) / temperature
    valid = (cmask[:, None, :, None] * rmask[None, :, None, :]) > 0
    return sim, torch.where(valid, sim, sim.min().detach() - 100.0)


def costs(S, cmask, rmask, temperature, alignment="softmax", words=True, regions=True):
    """:162-236: (cost_w2r, cost_r2w) [B, B] before the all-empty fill; None for a direction that is off."""
    sim, masked = masked_similarity(S, cmask, rmask, temperature)
    T, NR = cmask.shape[1], rmask.shape[1]

    def attention(dim, n):
        if alignment == "softmax":
            return torch.softmax(masked, dim=dim)
        if alignment == "hardmax":                                   # argmax: the first index on ties
            hot = torch.nn.functional.one_hot(masked.argmax(dim=dim), n).to(sim.dtype)      # [..., n] appended last
            return hot if dim == 3 else hot.permute(0, 1, 3, 2)
        raise NotImplementedError(alignment)

    dist = -sim
    nw = cmask.sum(1).clamp(min=1)[:, None]
    nr = rmask.sum(1).clamp(min=1)[None, :]
    w2r = r2w = None
    if words:
        w2r = (attention(3, NR) * cmask[:, None, :, None] * dist).sum((2, 3)) / nw
    if regions:
        r2w = (attention(2, T) * rmask[None, :, None, :] * dist).sum((2, 3)) / nr
    return w2r, r2w


def top_two_gap(S, cmask, rmask, temperature):
    """The smallest gap between the best and the second-best candidate over every valid word's valid regions and every valid
    region's valid words (rows / columns with one candidate have none): hardmax is only well-posed in fp32 above it."""
    _, masked = masked_similarity(S.double(), cmask.double(), rmask.double(), temperature)
    B, T = cmask.shape
    NR = rmask.shape[1]
    gap = float("inf")
    for c in range(B):
        for i in range(B):
            wv, rv = cmask[c] > 0, rmask[i] > 0
            blk = masked[c, i][wv][:, rv]
            if blk.shape[0] and blk.shape[1] >= 2:
                top = blk.topk(2, dim=1).values
                gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
            if blk.shape[1] and blk.shape[0] >= 2:
                top = blk.topk(2, dim=0).values
                gap = min(gap, float((top[0] - top[1]).min()))
    return gap


def filled(cost, cmask, rmask):
    """:240-251: pairs with neither words nor regions get max + 100 (a detached constant)."""
    ok = (cmask.sum(1)[:, None] > 0) | (rmask.sum(1)[None, :] > 0)
    return torch.where(ok, cost, cost.max().detach() + 100.0)


def without_diagonal(m, dim):
    """The n x n matrix without its diagonal: n x (n - 1) for dim 1, (n - 1) x n for dim 0, the other entries in order."""
    n = m.shape[0]
    keep = ~torch.eye(n, dtype=torch.bool)
    if dim == 1:
        return m[keep].reshape(n, n - 1)
    return m.t()[keep].reshape(n, n - 1).t()


def tail(cost, cmask, rmask, loss="cross_entropy", mining="hardest", margin=1.0, neg_idx=None):
    """One direction's [B, B] cost -> (loss choose caption, loss choose image, accuracy choose caption, accuracy choose image,
    the filled cost).  neg_idx (mining "given"): (index [B] for choose caption, index [B] for choose image) into the matrix without
    its diagonal."""
    B = cost.shape[0]
    pw = filled(cost, cmask, rmask)
    eye = torch.arange(B)
    if loss == "cross_entropy":
        lc = torch.diag(-torch.log_softmax(-pw, dim=0)).mean()
        li = torch.diag(-torch.log_softmax(-pw, dim=1)).mean()
    elif loss == "triplet":
        pos = torch.diag(pw)
        if B < 2:
            ncap = nimg = pos + margin
        else:
            cap_all, img_all = without_diagonal(pw, 0), without_diagonal(pw, 1)
            if mining == "hardest":
                ncap, nimg = cap_all.min(dim=0).values, img_all.min(dim=1).values
            elif mining == "easiest":
                ncap, nimg = cap_all.max(dim=0).values, img_all.max(dim=1).values
            elif mining == "given":
                ncap = cap_all.gather(0, neg_idx[0].view(1, B))[0]
                nimg = img_all.gather(1, neg_idx[1].view(B, 1))[:, 0]
            else:
                raise NotImplementedError(mining)
        lc = torch.relu(pos - ncap + margin).mean()
        li = torch.relu(pos - nimg + margin).mean()
    else:
        raise NotImplementedError(loss)
    ac = (pw.argmin(dim=0) == eye).to(cost.dtype).mean()
    ai = (pw.argmin(dim=1) == eye).to(cost.dtype).mean()
    return lc, li, ac, ai, pw


def head_forward(region, rmask, cap, att, spec, w, b, cfg):
    """The whole forward for a configuration dictionary (the keys of MODEL.MMSS_HEAD.GROUNDING): (losses, info, {"w2r", "r2w"})
    with the reference's names in the reference's order."""
    B, NR, _ = region.shape
    T = cap.shape[1]
    cmask = (att * (1 - spec)).to(region.dtype)
    rmask = rmask.to(region.dtype)
    img = region @ w.t() + b
    S = cap.reshape(B * T, -1) @ img.reshape(B * NR, -1).t()
    words, regions = cfg["ALIGN_WORDS_TO_REGIONS"], cfg["ALIGN_REGIONS_TO_WORDS"]
    w2r, r2w = costs(S, cmask, rmask, cfg["ALIGNMENT_TEMPERATURE"], cfg["ALIGNMENT"], words, regions)
    name = {"cross_entropy": "CE_loss", "triplet": "Triplet Loss"}[cfg["LOSS"]]
    losses, info, pw = {}, {}, {"w2r": None, "r2w": None}
    for on, tag, key, cost in ((words, "Words", "w2r", w2r), (regions, "Regions", "r2w", r2w)):
        if not on:
            continue
        lc, li, ac, ai, pw[key] = tail(cost, cmask, rmask, cfg["LOSS"], cfg["NEGATIVE_MINING"], cfg["TRIPLET_MARGIN"])
        losses[f"{name} (Align {tag}, Choose Caption)"] = lc
        losses[f"{name} (Align {tag}, Choose Image)"] = li
        info[f"Batch Accuracy (Align {tag}, Choose Caption)"] = ac
        info[f"Batch Accuracy (Align {tag}, Choose Image)"] = ai
    return losses, info, pw
