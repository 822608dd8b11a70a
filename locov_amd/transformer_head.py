"""TransformerHead of the LSM branch on the gfx950 kernels.

Mirrors ovr/modeling/mmss_heads/transformer_head.py:22-307 (classes, constructor arguments, config keys, submodule and parameter
names -- a reference checkpoint loads with strict=True --, `_init_weights`, the decoder tying, the requires_grad switches, forward
signature, returned dictionaries and their key strings): the BERT encoder over [caption tokens; regions] of all B^2 (caption, image)
pairs with the masked-language-modelling and image-caption-matching losses, and the `trans` cost matrix the distillation losses read.
`transformers` is not imported: the encoder layers are the small modules below.

HOW it computes differs, WHAT it computes does not:
  * every linear layer is ops.linear_autograd (f32 MFMA GEMMs), weights read at call time (`v2l_projection` is tied to the grounding
    head's by the meta-architecture); Q, K and V are ONE GEMM against the concatenated weight and land as the three column blocks of
    one matrix;
  * the attention core is ops.mha_packed (csrc/mha.hip): one launch forward, two backward, no [.., S, S] tensor.  Its key bias is the
    concatenated [caption_mask, region_mask] as 0 / 1 floats EXACTLY as the reference hands them to BertEncoder (:167-172): the value
    is ADDED to the scores, so a padded key is down-weighted by e^-1 and NOT excluded.  That is the reference's behaviour (perturbing
    a padded caption token changes `trans`), pinned by tests/golden/g10_transformer_head.npz, and kept.  In training the attention
    dropout's keep mask is drawn here with torch.rand from the global generator and handed to the kernel;
  * LayerNorm, erf-GELU, tanh, the hidden dropouts and the residual adds are torch elementwise ops (plumbing; fusing them is listed
    as a follow-up in docs/experiments.md);
  * the LM head (768 -> 30 522 at configs/coco_lsm.yaml) runs on the B * T tokens of the B matching pairs only -- the reference runs
    it on all B^2 * T and then keeps the diagonal (:187-194).  Loss and accuracy are torch's cross_entropy(ignore_index=-1) and an
    argmax comparison on the device: no nonzero, no count read to the host.  (Not ops.cls_loss: its statistics are the ROI head's
    foreground / background counts, not the masked-token accuracy, and an all-ignored batch must give the reference's NaN.)
  * heads.imagePredictions is NOT evaluated: the reference's forward never uses its output (:195-201 are dead values) and with
    MVM_LOSS "" its parameters are frozen.  It stays in the module for the checkpoint keys;
  * the image-caption-matching tail (:208-215, :235-245) is torch ops on the [B, B] cost.  (Not ops.grounding_ce: that tail replaces
    the cost of pairs without words and regions by max + 100, which this head does not do.)
  * `log_info` is filled lazily with the device tensors, without host syncs, as GroundingHead does.

LOCOV_FUSED_ATTENTION=0 selects a composed torch path for the attention core (matmul, softmax, matmul on the same Q / K / V) for
A/B runs and tests only.
"""
from __future__ import annotations

import copy
import math
import os
from typing import Dict, Optional

import torch
from torch import nn
import torch.nn.functional as F

from . import ops

__all__ = ["TransformerHead", "VisualEmbedding", "MMPreTrainingHeads", "BertImagePredictionHead", "build_transformer_head",
           "attention_core"]

BertLayerNorm = nn.LayerNorm


def _lin(x: torch.Tensor, m: nn.Linear) -> torch.Tensor:
    """m(x) for x [..., K] on the GEMM kernel, weights read at call time."""
    y = ops.linear_autograd(x.reshape(-1, x.shape[-1]), m.weight, m.bias)
    return y.view(*x.shape[:-1], y.shape[-1])


def _fused() -> bool:
    return os.environ.get("LOCOV_FUSED_ATTENTION", "1") != "0"


def _composed(q, k, v, key_bias, H, scale, keep, p_drop):
    nseq, S = key_bias.shape
    d = q.shape[1] // H
    heads = lambda t: t.reshape(nseq, S, H, d).permute(0, 2, 1, 3)
    p = torch.softmax(torch.matmul(heads(q), heads(k).transpose(-1, -2)) * scale + key_bias[:, None, None, :], dim=-1)
    if keep is not None:
        p = p * keep * (1.0 / (1.0 - p_drop))
    return torch.matmul(p, heads(v)).permute(0, 2, 1, 3).reshape(nseq * S, H * d)


def attention_core(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_bias: torch.Tensor, num_heads: int, *,
                   scale: Optional[float] = None, keep: Optional[torch.Tensor] = None, p_drop: float = 0.0) -> torch.Tensor:
    """dropout(softmax(q k^T * scale + key_bias)) v per (sequence, head): ops.mha, or with LOCOV_FUSED_ATTENTION=0 the composed torch
    chain on the same operands (A/B runs and tests only)."""
    if _fused():
        return ops.mha(q, k, v, key_bias, num_heads, scale=scale, keep=keep, p_drop=p_drop)
    scale = 1.0 / math.sqrt(q.shape[1] // num_heads) if scale is None else scale
    return _composed(q, k, v, key_bias, num_heads, scale, keep, p_drop)


class BertConfig:
    """The keys of MODEL.MMSS_HEAD.TRANSFORMER.BERT_CONFIG as attributes."""

    def __init__(self, **kw):
        self.vocab_size, self.hidden_size, self.num_hidden_layers, self.num_attention_heads = 30522, 768, 12, 12
        self.intermediate_size, self.hidden_act, self.hidden_dropout_prob, self.attention_probs_dropout_prob = 3072, "gelu", 0.1, 0.1
        self.initializer_range, self.layer_norm_eps = 0.02, 1e-12
        self.__dict__.update(kw)
        if self.hidden_size % self.num_attention_heads != 0:
            raise ValueError(f"hidden_size {self.hidden_size} is not a multiple of num_attention_heads {self.num_attention_heads}")
        if self.hidden_act != "gelu":
            raise NotImplementedError(f"hidden_act {self.hidden_act!r}: only the erf 'gelu' of the reference's configuration")


class BertSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = config.hidden_size // config.num_attention_heads
        self.query = nn.Linear(config.hidden_size, config.hidden_size)
        self.key = nn.Linear(config.hidden_size, config.hidden_size)
        self.value = nn.Linear(config.hidden_size, config.hidden_size)
        self.dropout = nn.Dropout(config.attention_probs_dropout_prob)

    def forward(self, x, key_bias):
        """x [Nseq * S, hidden], key_bias [Nseq, S] -> context [Nseq * S, hidden]."""
        H, E = self.num_attention_heads, x.shape[1]
        qkv = ops.linear_autograd(x, torch.cat([self.query.weight, self.key.weight, self.value.weight], dim=0),
                                  torch.cat([self.query.bias, self.key.bias, self.value.bias], dim=0))
        nseq, S = key_bias.shape
        keep, p = None, self.dropout.p
        if self.training and p > 0.0:
            keep = (torch.rand((nseq, H, S, S), device=x.device) >= p).to(torch.uint8)
        scale = 1.0 / math.sqrt(self.attention_head_size)
        if _fused():
            return ops.mha_packed(qkv, key_bias, H, scale=scale, keep=keep, p_drop=p)
        return _composed(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], key_bias, H, scale, keep, p)


class BertSelfOutput(nn.Module):
    def __init__(self, config, in_features=None):
        super().__init__()
        self.dense = nn.Linear(in_features or config.hidden_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, hidden_states, input_tensor):
        return self.LayerNorm(self.dropout(_lin(hidden_states, self.dense)) + input_tensor)


class BertAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self = BertSelfAttention(config)
        self.output = BertSelfOutput(config)

    def forward(self, x, key_bias):
        return self.output(self.self(x, key_bias), x)


class BertIntermediate(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.intermediate_size)

    def forward(self, x):
        return F.gelu(_lin(x, self.dense))


class BertLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = BertAttention(config)
        self.intermediate = BertIntermediate(config)
        self.output = BertSelfOutput(config, config.intermediate_size)

    def forward(self, x, key_bias):
        a = self.attention(x, key_bias)
        return self.output(self.intermediate(a), a)


class BertEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(config) for _ in range(config.num_hidden_layers)])

    def forward(self, x, key_bias):
        for layer in self.layer:
            x = layer(x, key_bias)
        return x


class BertPooler(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)

    def forward(self, first_token):
        return torch.tanh(_lin(first_token, self.dense))


class BertPredictionHeadTransform(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def forward(self, x):
        return self.LayerNorm(F.gelu(_lin(x, self.dense)))


class BertLMPredictionHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(config.hidden_size, config.vocab_size, bias=True)
        self.bias = nn.Parameter(torch.zeros(config.vocab_size))
        self.decoder.bias = self.bias                       # one parameter under both names, as the reference's library ties them

    def forward(self, x):
        return _lin(self.transform(x), self.decoder)


class BertImagePredictionHead(nn.Module):
    def __init__(self, config, v_feature_size):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(config.hidden_size, v_feature_size)

    def forward(self, hidden_states):
        return _lin(self.transform(hidden_states), self.decoder)


class MMPreTrainingHeads(nn.Module):
    def __init__(self, config, v_feature_size):
        super().__init__()
        self.predictions = BertLMPredictionHead(config)
        self.bi_seq_relationship = nn.Linear(config.hidden_size, 2)
        self.imagePredictions = BertImagePredictionHead(config, v_feature_size)

    def forward(self, sequence_output_t, pooled_output):
        """(LM scores of the given tokens, sequence-relationship scores); imagePredictions is not evaluated (module docstring)."""
        return self.predictions(sequence_output_t), _lin(pooled_output, self.bi_seq_relationship)


class VisualEmbedding(nn.Module):
    """Construct the embeddings from image and spatial location embeddings (:284-303)."""

    def __init__(self, config, v_feature_size, v_loc_size):
        super().__init__()
        self.image_embeddings = nn.Linear(v_feature_size, config.hidden_size)
        self.image_location_embeddings = nn.Linear(v_loc_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, input_features, input_loc):
        return self.dropout(self.LayerNorm(_lin(input_features, self.image_embeddings) + _lin(input_loc, self.image_location_embeddings)))


class TransformerHead(nn.Module):
    def __init__(self, config, v_dim, l_dim, loc_dim, backbone, *args, **kwargs):
        super().__init__()
        self.config = config.MODEL.MMSS_HEAD.TRANSFORMER
        self.v_dim, self.l_dim, self.loc_dim = v_dim, l_dim, loc_dim
        self.backbone = backbone
        self.mvm_loss = self.config.MVM_LOSS
        self.mmm_loss = self.config.MMM_LOSS
        self.num_negative = self.config.MVM_LOSS_NUM_NEGATIVE

        bc = self.config.BERT_CONFIG
        self.bert_config = BertConfig(**(dict(bc) if isinstance(bc, dict) else vars(bc)))
        self.v2l_projection = nn.Linear(self.v_dim, self.l_dim)
        self.visual_emb = VisualEmbedding(self.bert_config, self.l_dim, self.loc_dim)
        self.encoder = BertEncoder(self.bert_config)
        self.pooler = BertPooler(self.bert_config)
        self.heads = MMPreTrainingHeads(self.bert_config, self.v_dim)

        self.encoder.apply(self._init_weights)
        self.pooler.apply(self._init_weights)
        self.heads.apply(self._init_weights)
        self._tie_weights()

        if self.mvm_loss in ("reconstruction_error", "contrastive_cross_entropy"):
            pass                                            # (:49-52 build a criterion the forward never calls)
        elif self.mvm_loss == "":
            for p in self.heads.imagePredictions.parameters():
                p.requires_grad = False
        else:
            raise NotImplementedError
        if self.mmm_loss == "":
            for p in self.pooler.parameters():
                p.requires_grad = False
            for p in self.heads.bi_seq_relationship.parameters():
                p.requires_grad = False
        self.return_dist = config.MODEL.MMSS_HEAD.DISTILLATION_LOSS
        self.log_info: Dict[str, object] = {}               # LoggedModule.log_info (filled lazily, no host syncs)

    def _tie_weights(self):
        assert self.heads.predictions.decoder.weight.shape[0] == self.backbone.embeddings.shape[0]
        assert self.heads.predictions.decoder.weight.shape[1] == self.backbone.embeddings.shape[1]
        self.heads.predictions.decoder.weight = self.backbone.embeddings

    def _init_weights(self, module):
        """Initialize the weights (:80-103)."""
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.bert_config.initializer_range)
        elif isinstance(module, BertLayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()
        if self.config.pretrained_weights and isinstance(module, BertEncoder):
            pretrained_weights = copy.deepcopy(self.backbone.state_dict())
            actual_weights = module.state_dict()
            for name, val in actual_weights.items():
                src = pretrained_weights.get("bert_model.encoder." + name)
                if src is not None and src.shape == val.shape:
                    actual_weights[name] = src.to(val.device)
            module.load_state_dict(actual_weights)

    def forward(self, input_image, input_caption):
        caption_emb = input_caption["encoded_tokens"]
        caption_mask = input_caption["attention_mask"]
        mlm_mask = input_caption["mlm_mask"]
        target_caption_ids = input_caption["target_ids"]
        region_features = input_image["region_features"]
        region_mask = input_image["region_mask"]
        region_loc = input_image["region_loc"]
        if self.mmm_loss not in ("cross_entropy", ""):
            raise NotImplementedError                                                # :216-219

        target_caption_ids = torch.where(mlm_mask > 0, target_caption_ids, torch.full_like(target_caption_ids, -1))
        caption_mask = caption_mask.to(torch.float32)
        region_mask = region_mask.to(torch.float32)
        T = caption_mask.shape[1]
        B, NR, _ = region_features.shape
        L, V = self.l_dim, self.bert_config.vocab_size

        image_emb = _lin(region_features.float(), self.v2l_projection)               # :142, weights read at call time
        image_emb = self.visual_emb(image_emb, region_loc.float())                   # [B, NR, L]
        caption_emb = caption_emb.float()
        if self.mmm_loss == "cross_entropy":                                         # :145-165: pair i * B + j = (caption i, image j)
            P = B * B
            image_emb = image_emb[None].expand(B, B, NR, L).reshape(P, NR, L)
            caption_emb = caption_emb[:, None].expand(B, B, T, L).reshape(P, T, L)
            region_mask = region_mask[None].expand(B, B, NR).reshape(P, NR)
            caption_mask = caption_mask[:, None].expand(B, B, T).reshape(P, T)
        else:
            P = B
        S = T + NR
        embedded_tokens = torch.cat([caption_emb, image_emb], dim=1).reshape(P * S, L)
        attention_mask = torch.cat([caption_mask, region_mask], dim=1).contiguous()  # the raw 0 / 1 floats: ADDED to the scores

        sequence_output = self.encoder(embedded_tokens, attention_mask).view(P, S, L)
        # the LM head on the tokens of the matching pairs (pairs i * (B + 1)) only
        diagonal = sequence_output[::B + 1] if self.mmm_loss == "cross_entropy" else sequence_output
        tokens = diagonal[:, :T].reshape(B * T, L)
        if self.mmm_loss == "cross_entropy":
            pooled_output = self.pooler(sequence_output[:, 0])
            prediction_scores_t, seq_relationship_score = self.heads(tokens, pooled_output)
        else:                                                                        # (pooler and bi_seq_relationship are frozen and unused)
            prediction_scores_t = self.heads.predictions(tokens)
        targets = target_caption_ids.reshape(-1)
        masked_lm_loss = F.cross_entropy(prediction_scores_t, targets, ignore_index=-1)   # :203-206 (NaN when nothing is masked)

        eye = torch.arange(B, device=prediction_scores_t.device)
        if self.mmm_loss == "cross_entropy":                                         # :208-215
            pw_cost = seq_relationship_score[:, 0].reshape(B, B)
            next_sentence_loss = torch.diag(-torch.log_softmax(-pw_cost, dim=0)).mean() + \
                torch.diag(-torch.log_softmax(-pw_cost, dim=1)).mean()
        else:
            next_sentence_loss = torch.zeros((), dtype=torch.float32, device=prediction_scores_t.device)
        losses = {"Masked Language Modeling Loss": masked_lm_loss, "Image Caption Matching Loss": next_sentence_loss}
        acc_num = (prediction_scores_t.argmax(dim=-1) == targets).to(torch.float32).sum()
        acc_denom = (targets >= 0).to(torch.float32).sum()
        other_info = {"Masked Language Modeling Accuracy": torch.where(acc_denom > 0, acc_num / acc_denom, acc_denom)}
        if self.mmm_loss == "cross_entropy":
            other_info["Batch Accuracy (Choose Caption)"] = (pw_cost.argmin(dim=0) == eye).to(torch.float32).mean()
            other_info["Batch Accuracy (Choose Image)"] = (pw_cost.argmin(dim=1) == eye).to(torch.float32).mean()
        self.log_info = {**losses, **other_info}
        if self.return_dist:
            if self.mmm_loss != "cross_entropy":                                     # :250-251 reads a name that was never bound
                raise UnboundLocalError("local variable 'pw_cost' referenced before assignment")
            return other_info, losses, {"trans": pw_cost}
        return other_info, losses


def build_transformer_head(name, cfg, v_dim, l_dim, loc_dim, backbone, *args, **kwargs):
    if name != "TransformerHead":
        raise KeyError(f"No object named '{name}' found in 'MMSS_HEADS' registry!")
    return TransformerHead(cfg, v_dim, l_dim, loc_dim, backbone)
