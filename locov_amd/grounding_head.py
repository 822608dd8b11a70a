"""GroundingHead of the LSM branch on the gfx950 kernels.

Mirrors ovr/modeling/mmss_heads/grounding_head.py:51-392 (class, constructor arguments, config
keys, `v2l_projection` parameter name, forward signature, returned dictionaries and their keys).

The combination configs/coco_lsm.yaml selects -- LOCAL_METRIC "dot", GLOBAL_METRIC "aligned_local",
ALIGNMENT "softmax", LOSS "cross_entropy" -- is the hot path: instead of materialising B^2 copies of
the captions, regions and masks (:119-144) and running ~30 elementwise launches on [B^2, T, NR]
tensors with a host sync per logged tensor (`LoggedModule.log`), the region embeddings and the
caption tokens meet in ONE [B*T, B*NR] GEMM and one fused kernel reduces each T x NR block to its
two cost entries (csrc/grounding.hip).  The B x B cross-entropy tail is one more launch each way
(csrc/losses.hip), with or without the distributions DISTILLATION_LOSS asks for.

ALIGNMENT "hardmax" (:169-174), LOSS "triplet" with hardest / easiest / random negatives (:279-343) and
a single alignment direction run on the same kernels: the alignment kernel takes the rule and the
directions (ops.grounding_costs(alignment=, words=, regions=)), hardmax costs feed the same
cross-entropy tail, and the triplet tail is one launch each way (ops.grounding_triplet) with no host
read.  NEGATIVE_MINING "random" draws its indices here, with the torch.randint calls `_general` makes in
the same order, so a seeded run keeps its RNG stream, and hands them to the kernel.

Out of scope for the kernels, still on `_general` (the reference's statements on the [B^2, T, NR] view
with device tensor ops after the same single similarity GEMM; configuration options off the shipped
path, kept for drop-in completeness and pinned to the reference's own outputs, tests/golden G8):
GLOBAL_METRIC reconstruction_mse (:215-224) -- it needs the embeddings inside the tile, and its region
direction only broadcasts for B^2 == NR in the reference; ALIGNMENT random_categorical / random_top3
(:175-208) -- torch.multinomial's draw cannot be reproduced inside a kernel.  `_general` also answers
every configuration it answers with an exception (e.g. DISTILLATION_LOSS with one direction off:
KeyError), B above GROUNDING_CE_MAX_B and LOCOV_FUSED_LOSSES=0.  What the reference itself rejects is
rejected the same way: LOCAL_METRIC other than "dot" (NotImplementedError, :149), LOSS "matching" with
the dot metric (Exception, :258-262), unknown names (NotImplementedError).
"""
from __future__ import annotations

from typing import Dict

import os

import torch
from torch import nn

from . import ops

__all__ = ["GroundingHead", "build_grounding_head"]


def _get(cfg, name, default):
    return getattr(cfg, name) if hasattr(cfg, name) else default


class GroundingHead(nn.Module):
    def __init__(self, config, v_dim, l_dim, *args, **kwargs):
        super().__init__()
        g = config.MODEL.MMSS_HEAD.GROUNDING
        self.config = g
        self.v_dim, self.l_dim = v_dim, l_dim
        self.v2l_projection = nn.Linear(self.v_dim, self.l_dim)
        self.local_metric = g.LOCAL_METRIC
        self.global_metric = g.GLOBAL_METRIC
        self.alignment = g.ALIGNMENT
        self.temperature = g.ALIGNMENT_TEMPERATURE
        self.loss_type = g.LOSS
        self.negative_mining = _get(g, "NEGATIVE_MINING", "random")
        self.margin = _get(g, "TRIPLET_MARGIN", 1.0)
        self.align_words = g.ALIGN_WORDS_TO_REGIONS
        self.align_regions = g.ALIGN_REGIONS_TO_WORDS
        assert self.align_words or self.align_regions
        self.return_dist = config.MODEL.MMSS_HEAD.DISTILLATION_LOSS
        self.grounding_text_input = _get(g, "TEXT_INPUT", "input_embeddings")
        self.log_info: Dict[str, object] = {}          # LoggedModule.log_info (filled lazily, no host syncs)
        self._fused = (self.local_metric, self.global_metric, self.alignment, self.loss_type) == \
            ("dot", "aligned_local", "softmax", "cross_entropy")
        # the variants the kernels also take (hardmax, triplet); what `_general` answers with an exception stays there
        self._fused_variant = not self._fused and (self.local_metric, self.global_metric) == ("dot", "aligned_local") and \
            self.alignment in ("softmax", "hardmax") and self.loss_type in ("cross_entropy", "triplet") and \
            (self.loss_type != "triplet" or self.negative_mining in ("hardest", "easiest", "random")) and \
            not (self.return_dist and not (self.align_words and self.align_regions))

    def forward(self, input_image, input_caption):
        caption_emb = input_caption[self.grounding_text_input]                       # [B, T, L]
        caption_mask = (input_caption["attention_mask"] * (1 - input_caption["special_tokens_mask"])
                        ).to(torch.float32)                                          # :94-96
        region_features = input_image["region_features"]                             # [B, NR, V]
        region_mask = input_image["region_mask"].to(torch.float32)
        B, NR, V = region_features.shape
        T = caption_mask.shape[1]

        # :111 image_emb = v2l_projection(region_features); weights read at call time (tied to emb_pred)
        image_emb = ops.linear_autograd(region_features.reshape(B * NR, V).contiguous().float(),
                                        self.v2l_projection.weight, self.v2l_projection.bias)   # [B*NR, L]
        cap = caption_emb.reshape(B * T, -1).contiguous().float()
        if self.local_metric != "dot":
            raise NotImplementedError                                                 # :146-149
        # :147 all B^2 caption x image token-region similarities as one NT GEMM
        S = ops.linear_autograd(cap, image_emb, None)                                 # [B*T, B*NR]
        if self._fused_variant and S.is_cuda and S.dtype == torch.float32 and B <= ops.GROUNDING_CE_MAX_B and \
                os.environ.get("LOCOV_FUSED_LOSSES", "1") != "0":
            return self._variant(S, caption_mask, region_mask, B)
        if not self._fused:
            return self._general(S, cap.view(B, T, -1), image_emb.view(B, NR, -1), caption_mask, region_mask, caption_mask.sum(dim=1),
                                 region_mask.sum(dim=1))
        # :150-228 temperature, masked softmax both ways, aligned-local distances -> [caption, image] costs
        cost_w2r, cost_r2w = ops.grounding_costs(S, caption_mask, region_mask, self.temperature)
        if S.is_cuda and B <= ops.GROUNDING_CE_MAX_B and os.environ.get("LOCOV_FUSED_LOSSES", "1") != "0":
            # :239-290, :357-377 in one launch (ops.grounding_ce = locov_grounding_ce_fwd / _bwd): the (max + 100) replacement, both
            # log-softmaxes, the diagonal means and the batch accuracies of both alignments; with the distributions requested the
            # same launch also writes the filled costs (ops.grounding_ce_dist = locov_grounding_ce_dist_fwd / _bwd)
            return self._ce_tail(cost_w2r if self.align_words else None, cost_r2w if self.align_regions else None, caption_mask,
                                 region_mask)
        losses, other_info = {}, {}
        # :232-243 pairs with neither words nor regions get (max + 100)
        num_words, num_regions = caption_mask.sum(dim=1), region_mask.sum(dim=1)
        ok = (num_words[:, None] > 0) | (num_regions[None, :] > 0)
        eye = torch.arange(B, device=S.device)
        pw = {}
        for on, tag, cost in ((self.align_words, "Words", cost_w2r), (self.align_regions, "Regions", cost_r2w)):
            if not on:
                continue
            cost = torch.where(ok, cost, cost.max().detach() + 100.0)
            pw[tag] = cost
            logits_cap = torch.log_softmax(-cost, dim=0)                              # :264-277
            logits_img = torch.log_softmax(-cost, dim=1)
            losses[f"CE_loss (Align {tag}, Choose Caption)"] = torch.diag(-logits_cap).mean()
            losses[f"CE_loss (Align {tag}, Choose Image)"] = torch.diag(-logits_img).mean()
            other_info[f"Batch Accuracy (Align {tag}, Choose Caption)"] = (cost.argmin(dim=0) == eye).float().mean()
            other_info[f"Batch Accuracy (Align {tag}, Choose Image)"] = (cost.argmin(dim=1) == eye).float().mean()
        self.log_info = {**losses, **other_info}
        if self.return_dist:
            return other_info, losses, {"w2r": pw.get("Words"), "r2w": pw.get("Regions")}
        return other_info, losses

    # ------------------------------------------------------------------ hardmax / triplet / one direction on the kernels
    def _variant(self, S, caption_mask, region_mask, B):
        """:150-343 for ALIGNMENT softmax | hardmax and LOSS cross_entropy | triplet: one alignment launch, one tail launch."""
        c0, c1 = ops.grounding_costs(S, caption_mask, region_mask, self.temperature, alignment=self.alignment,
                                     words=self.align_words, regions=self.align_regions)
        if self.loss_type == "cross_entropy":
            return self._ce_tail(c0, c1, caption_mask, region_mask)
        mining, neg_idx = self.negative_mining, None
        if B < 2:
            mining = "hardest"                                # (:296 negative = positive + margin whatever the mining; nothing is drawn)
        elif mining == "random":
            # the draws of `_general`, same calls in the same order: per direction that is on, (1, B) then (B, 1)
            draws = [None] * 4
            for k, on in enumerate((self.align_words, self.align_regions)):
                if on:
                    draws[2 * k] = torch.randint(B - 1, (1, B), device=S.device).view(B)
                    draws[2 * k + 1] = torch.randint(B - 1, (B, 1), device=S.device).view(B)
            spare = next(d for d in draws if d is not None)                      # (a direction that is off is not read)
            mining, neg_idx = "given", torch.stack([d if d is not None else spare for d in draws]).view(2, 2, B)
        res = ops.grounding_triplet(c0, c1, caption_mask, region_mask, mining, self.margin, neg_idx, with_dist=self.return_dist)
        return self._tail_result("Triplet Loss", *(res if self.return_dist else (res, None, None)))

    def _ce_tail(self, c0, c1, caption_mask, region_mask):
        """The cross-entropy tail on the costs that are on, with the filled costs where the distributions are returned."""
        if self.return_dist:
            return self._tail_result("CE_loss", *ops.grounding_ce_dist(c0, c1, caption_mask, region_mask))
        return self._tail_result("CE_loss", ops.grounding_ce(c0, c1, caption_mask, region_mask), None, None)

    def _tail_result(self, name, vals, pw0, pw1):
        """The tail's 8 scalars (ops.grounding_ce's layout) and filled costs as forward returns them; fills log_info."""
        losses, other_info = {}, {}
        for k, (on, tag) in enumerate(((self.align_words, "Words"), (self.align_regions, "Regions"))):
            if not on:
                continue
            losses[f"{name} (Align {tag}, Choose Caption)"] = vals[4 * k]
            losses[f"{name} (Align {tag}, Choose Image)"] = vals[4 * k + 1]
            other_info[f"Batch Accuracy (Align {tag}, Choose Caption)"] = vals[4 * k + 2]
            other_info[f"Batch Accuracy (Align {tag}, Choose Image)"] = vals[4 * k + 3]
        self.log_info = {**losses, **other_info}
        if self.return_dist:
            return other_info, losses, {"w2r": pw0, "r2w": pw1}
        return other_info, losses

    # ------------------------------------------------------------------ the reference's other variants (:146-343)
    def _general(self, S, cap, img, caption_mask, region_mask, num_words, num_regions):
        """S [B*T, B*NR] = every caption token against every region of every image; cap [B,T,L], img [B,NR,L].
        Pair p = i * B + j is (caption i, image j), as the reference's repeat / reshape lays them out (:119-144)."""
        import torch.nn.functional as F
        B, T, L = cap.shape
        NR = img.shape[1]
        if self.loss_type in ("cross_entropy", "triplet"):
            local_similarity = S.view(B, T, B, NR).permute(0, 2, 1, 3).reshape(B * B, T, NR)
            image_emb = img.permute(0, 2, 1)[None].expand(B, B, L, NR).reshape(B * B, L, NR)
            caption_emb = cap[:, None].expand(B, B, T, L).reshape(B * B, T, L)
            region_mask = region_mask[None].expand(B, B, NR).reshape(B * B, NR)
            caption_mask = caption_mask[:, None].expand(B, B, T).reshape(B * B, T)
            num_regions = num_regions[None, :].expand(B, B).reshape(B * B)
            num_words = num_words[:, None].expand(B, B).reshape(B * B)
        else:                                             # "matching": matching pairs only (the diagonal blocks)
            idx = torch.arange(B, device=S.device)
            local_similarity = S.view(B, T, B, NR)[idx, :, idx, :]
            image_emb, caption_emb = img.permute(0, 2, 1), cap
        local_distance = -local_similarity
        local_similarity = local_similarity / self.temperature                        # :151-152
        local_distance = local_distance / self.temperature
        local_similarity = torch.where((caption_mask[:, :, None] * region_mask[:, None, :]) > 0, local_similarity,
                                       local_similarity.min().detach() - 100.0)       # :155-159
        # one alignment rule for both directions: a distribution over the LAST dimension -- regions for every word (w2r), and,
        # on the transposed similarities, words for every region (r2w; :161-208 spell the two cases out separately)
        def align(sim):
            n = sim.shape[-1]
            if self.alignment == "softmax":
                return F.softmax(sim, dim=-1)
            if self.alignment == "hardmax":
                return F.one_hot(sim.argmax(dim=-1), n).to(torch.float32)
            if self.alignment == "random_categorical":
                return F.one_hot(_choose_one(F.softmax(sim, dim=-1)), n).to(torch.float32)
            if self.alignment == "random_top3":
                top = F.one_hot(torch.topk(sim, k=3, dim=-1).indices, n).to(torch.float32).sum(dim=-2)
                return F.one_hot(_choose_one(top), n).to(torch.float32)
            raise NotImplementedError

        attention_w2r = align(local_similarity) if self.align_words else None                                   # [P, T, NR]
        attention_r2w = align(local_similarity.transpose(1, 2)).transpose(1, 2) if self.align_regions else None   # [P, T, NR]
        ones_w, ones_r = torch.ones_like(num_words), torch.ones_like(num_regions)
        global_dist_w2r = global_dist_r2w = None
        if self.global_metric == "reconstruction_mse":                                # :215-224 (the reference's own broadcasting)
            if self.align_words:
                caption_rec = torch.bmm(attention_w2r, image_emb.transpose(1, 2))
                global_dist_w2r = (((caption_rec - caption_emb) ** 2).mean(dim=2) * caption_mask).sum(dim=1) / torch.max(num_words, other=ones_w)
            if self.align_regions:
                image_rec = torch.bmm(caption_emb.transpose(1, 2), attention_r2w)
                global_dist_r2w = ((image_rec - image_emb) ** 2).mean(dim=2).mean(dim=1)
                global_dist_r2w = (global_dist_r2w * region_mask).sum(dim=1) / torch.max(num_regions, other=ones_r)
        elif self.global_metric == "aligned_local":                                   # :226-236
            if self.align_words:
                global_dist_w2r = (attention_w2r * caption_mask[:, :, None] * local_distance).sum(dim=(1, 2)) / torch.max(num_words, other=ones_w)
            if self.align_regions:
                global_dist_r2w = (attention_r2w * region_mask[:, None, :] * local_distance).sum(dim=(1, 2)) / torch.max(num_regions, other=ones_r)
        else:
            raise NotImplementedError
        ok = (num_words > 0) + (num_regions > 0)                                      # :240-251
        if self.align_words:
            global_dist_w2r = torch.where(ok, global_dist_w2r, global_dist_w2r.max().detach() + 100.0)
        if self.align_regions:
            global_dist_r2w = torch.where(ok, global_dist_r2w, global_dist_r2w.max().detach() + 100.0)

        losses, other_info, pw = {}, {}, {}
        eye = torch.arange(B, device=S.device)
        if self.loss_type == "matching":                                              # :258-262: undefined for the (only) dot metric
            raise Exception("Matching loss is not defined for dot product because dot product is unbounded")
        for on, tag, dist in ((self.align_words, "Words", global_dist_w2r), (self.align_regions, "Regions", global_dist_r2w)):
            if not on:
                continue
            cost = dist.reshape(B, B)
            pw[tag] = cost
            if self.loss_type == "cross_entropy":                                     # :264-277
                losses[f"CE_loss (Align {tag}, Choose Caption)"] = torch.diag(-torch.log_softmax(-cost, dim=0)).mean()
                losses[f"CE_loss (Align {tag}, Choose Image)"] = torch.diag(-torch.log_softmax(-cost, dim=1)).mean()
            elif self.loss_type == "triplet":                                         # :279-343
                positive = torch.diag(cost)
                neg_cap_all, neg_img_all = _remove_diag(cost, 0), _remove_diag(cost, 1)
                if B < 2:
                    neg_cap = neg_img = positive + self.margin
                elif self.negative_mining == "hardest":
                    neg_cap, neg_img = neg_cap_all.min(dim=0).values, neg_img_all.min(dim=1).values
                elif self.negative_mining == "easiest":
                    neg_cap, neg_img = neg_cap_all.max(dim=0).values, neg_img_all.max(dim=1).values
                elif self.negative_mining == "random":
                    neg_cap = neg_cap_all.gather(index=torch.randint(B - 1, (1, B), device=S.device), dim=0)[0, :]
                    neg_img = neg_img_all.gather(index=torch.randint(B - 1, (B, 1), device=S.device), dim=1)[:, 0]
                else:
                    raise NotImplementedError
                losses[f"Triplet Loss (Align {tag}, Choose Caption)"] = torch.mean(F.relu(positive - neg_cap + self.margin))
                losses[f"Triplet Loss (Align {tag}, Choose Image)"] = torch.mean(F.relu(positive - neg_img + self.margin))
            else:
                raise NotImplementedError
            other_info[f"Batch Accuracy (Align {tag}, Choose Caption)"] = (cost.argmin(dim=0) == eye).float().mean()
            other_info[f"Batch Accuracy (Align {tag}, Choose Image)"] = (cost.argmin(dim=1) == eye).float().mean()
        self.log_info = {**losses, **other_info}
        if self.return_dist:
            return other_info, losses, {"w2r": pw["Words"], "r2w": pw["Regions"]}     # (:381: both directions, like the reference)
        return other_info, losses


def _choose_one(p: torch.Tensor) -> torch.Tensor:
    """grounding_head.py:15-28: one index per row of the last dimension, drawn from the (unnormalised) weights."""
    shape = p.shape
    return torch.multinomial(p.reshape(-1, shape[-1]), num_samples=1).squeeze(-1).reshape(shape[:-1])


def _remove_diag(m: torch.Tensor, dim: int) -> torch.Tensor:
    """grounding_head.py:31-48: the N x N matrix without its diagonal, as N x (N-1) (dim 1) or (N-1) x N (dim 0)."""
    n = m.shape[0]
    mask = ~torch.eye(n, dtype=torch.bool, device=m.device)
    if dim == 1:
        return torch.masked_select(m, mask).reshape(n, n - 1)
    return torch.masked_select(m.t(), mask).reshape(n, n - 1).t()


def build_grounding_head(name, cfg, v_dim, l_dim, *args, **kwargs):
    if name != "GroundingHead":
        raise KeyError(f"No object named '{name}' found in 'MMSS_HEADS' registry!")
    return GroundingHead(cfg, v_dim, l_dim)
