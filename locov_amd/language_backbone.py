"""The language backbone of the LSM model: `BertEmbedding`, the one configs/coco_lsm.yaml selects, with its caption path on the device.

Mirrors ovr/modeling/language/transf_models.py:83-167 (class, `bert_model` / `embeddings` names, `freeze`, the returned dictionary
and its key strings) and ovr/modeling/language/backbone.py (`build_backbone`, here `build_language_backbone`, the name the
reference imports it under; the `nn.Sequential(OrderedDict([("body", body)]))` wrapper with `.out_channels`).  A checkpoint's keys
read `body.embeddings`, `body.bert_model.word_embeddings.weight`, `...position_embeddings.weight`,
`...token_type_embeddings.weight`, `...LayerNorm.{weight,bias}`; the `...bert_model.position_ids` / `token_type_ids` buffers that
older `transformers` releases saved are accepted and dropped.

HOW it computes differs, WHAT it computes does not:
  * `transformers` is not imported and nothing is downloaded.  The tokenizer is a constructor argument (any object with
    `__call__(text_list, max_length)` returning the four lists, `mask_token_id` and `__len__`) or the `WordPieceTokenizer` below
    built from MODEL.LANGUAGE_BACKBONE.VOCAB_FILE.  PRETRAINED True means "the weights come with the checkpoint": the module
    initialises as PRETRAINED False does (normal, std 0.02) and warns once; weights arrive through load_state_dict.
  * the reference hard-codes bert-base-uncased's dimensions; here vocab_size, hidden_size, max_position_embeddings,
    type_vocab_size, layer_norm_eps and hidden_dropout_prob are read from MODEL.MMSS_HEAD.TRANSFORMER.BERT_CONFIG, whose defaults
    are bert-base's (TransformerHead._tie_weights asserts that the two agree).
  * the reference's caption path is a Python loop over B * T tokens calling np.random.rand() (:114-137), one
    torch.tensor(v).cuda() per dictionary key from pageable memory (:139) and index ops.  Here the four tokenizer lists are
    validated on the host, written into one reused pinned int32 [4, N] block, uploaded with one non_blocking copy, and ONE launch
    (ops.caption_embed, csrc/caption.hip) applies the masked-language-modelling rule, writes the six int64 tensors, gathers
    input_embeddings and -- with ADD_POSITION_EMBEDDING -- forms dropout(LayerNorm((W[id] + Tt[type]) + P[j])).  The rule's random
    numbers are `draws` [2, B, T] float64 (default torch.rand from the device generator): draws[0] is :125's np.random.rand(),
    draws[1] stands in for :134's np.random.randint(len(tokenizer)) as min(int(draws[1] * len), len - 1) -- a deterministic
    function of the draws, as mmss_regions and the proposal samplers do it.  The dropout keep mask is drawn here with torch.rand.
  * on CPU tensors, with LOCOV_FUSED_CAPTION=0 (A/B runs and tests, like LOCOV_FUSED_ATTENTION) or beyond the kernel's limits
    (ops.CAPTION_MAX_TOKENS, ops.CAPTION_MAX_HIDDEN) the torch expression `caption_rule` / `_torch_embed` runs; it is the definition.
  * the library's nn.Embedding(padding_idx=0) zeroes row 0 at construction and drops the encoded_tokens gradient of [PAD] rows;
    here row 0 is an ordinary row (it is overwritten by the checkpoint, and with FREEZE True, the shipped setting, has no gradient).

Not built: `build_bert_backbone` (the full 12-layer `BERT` class, :7-80) is not registered.
"""
from __future__ import annotations

import os
import unicodedata
import warnings
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .registry import Registry

__all__ = ["BertEmbedding", "BertEmbeddings", "WordPieceTokenizer", "LANGUAGE_BACKBONES_REGISTRY", "build_bertemb_backbone",
           "build_language_backbone", "caption_rule"]

LANGUAGE_BACKBONES_REGISTRY = Registry("LANGUAGE_BACKBONES")
TOKEN_KEYS = ("input_ids", "token_type_ids", "attention_mask", "special_tokens_mask")
MAX_LENGTH = 70                                            # :110


# ---------------------------------------------------------------------------------------------------------------- tokenizer

def _is_punctuation(ch: str) -> bool:
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


class WordPieceTokenizer:
    """bert-base-uncased's tokenization from a local vocab.txt (one token per line, the line number is the id): lower-case, NFD
    accent strip, whitespace and punctuation split, greedy longest-match WordPiece with "##", [UNK] for a word with no match or
    over 100 characters, [CLS] ... [SEP], truncation to max_length, [PAD] up to it, special_tokens_mask 1 on [CLS], [SEP] and
    the padding (what BertTokenizer returns)."""

    def __init__(self, vocab_file: str, max_chars_per_word: int = 100):
        with open(vocab_file, "r", encoding="utf-8") as f:
            tokens = [line.rstrip("\n") for line in f]
        while tokens and tokens[-1] == "":
            tokens.pop()
        self.vocab: Dict[str, int] = OrderedDict((t, i) for i, t in enumerate(tokens))
        for name in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"):
            if name not in self.vocab:
                raise ValueError(f"{vocab_file}: the vocabulary lacks {name}")
        self.pad_token_id, self.unk_token_id = self.vocab["[PAD]"], self.vocab["[UNK]"]
        self.cls_token_id, self.sep_token_id, self.mask_token_id = self.vocab["[CLS]"], self.vocab["[SEP]"], self.vocab["[MASK]"]
        self.max_chars_per_word = max_chars_per_word

    def __len__(self) -> int:
        return len(self.vocab)

    def basic_tokens(self, text: str) -> List[str]:
        text = unicodedata.normalize("NFD", text.lower())
        out, word = [], []
        for ch in text:
            cat = unicodedata.category(ch)
            if cat == "Mn" or ord(ch) == 0 or ord(ch) == 0xFFFD or (cat.startswith("C") and ch not in "\t\n\r"):
                continue                                   # accents and control characters
            if ch.isspace() or _is_punctuation(ch):
                if word:
                    out.append("".join(word))
                    word = []
                if not ch.isspace():
                    out.append(ch)
            else:
                word.append(ch)
        if word:
            out.append("".join(word))
        return out

    def wordpiece(self, word: str) -> List[int]:
        if len(word) > self.max_chars_per_word:
            return [self.unk_token_id]
        ids, start = [], 0
        while start < len(word):
            end, cur = len(word), None
            while start < end:
                piece = ("##" if start > 0 else "") + word[start:end]
                if piece in self.vocab:
                    cur = self.vocab[piece]
                    break
                end -= 1
            if cur is None:
                return [self.unk_token_id]
            ids.append(cur)
            start = end
        return ids

    def encode(self, text: str) -> List[int]:
        return [i for w in self.basic_tokens(text) for i in self.wordpiece(w)]

    def __call__(self, text_list: Sequence[str], max_length: int = MAX_LENGTH) -> Dict[str, List[List[int]]]:
        if max_length < 2:
            raise ValueError("WordPieceTokenizer: max_length must hold [CLS] and [SEP]")
        out = {k: [] for k in TOKEN_KEYS}
        for text in text_list:
            ids = [self.cls_token_id] + self.encode(text)[:max_length - 2] + [self.sep_token_id]
            n, pad = len(ids), max_length - len(ids)
            out["input_ids"].append(ids + [self.pad_token_id] * pad)
            out["token_type_ids"].append([0] * max_length)
            out["attention_mask"].append([1] * n + [0] * pad)
            out["special_tokens_mask"].append([1] + [0] * (n - 2) + [1] + [1] * pad)
        return out


# ---------------------------------------------------------------------------------------------------------------- the rule

def caption_rule(ids, types, attn, special, draws, mlm: Optional[ops.CaptionMlm]):
    """transf_models.py:114-137 on integer tensors of one shape, every comparison in double: (input_ids, special_tokens_mask,
    target_ids, mlm_mask).  draws [2, ...] float64 or None (masked language modelling inactive: nothing changes, mlm_mask 0)."""
    target = ids
    if draws is None:
        return ids, special, target, torch.zeros_like(ids)
    u, r = draws[0], draws[1]
    selected = (special == 0) & (attn != 0) & (u < mlm.p)
    q = u / mlm.p
    to_mask = selected & (q < mlm.p_mask)
    to_noise = selected & ~to_mask & (q < mlm.p_mask_noise)
    noise = torch.clamp((r * float(mlm.len_tok)).to(torch.int64), max=mlm.len_tok - 1)
    new_ids = torch.where(to_mask, torch.full_like(ids, mlm.mask_id), torch.where(to_noise, noise, ids))
    return new_ids, torch.where(to_mask, torch.ones_like(special), special), target, selected.to(torch.int64)


class BertEmbeddings(nn.Module):
    """The library's BertEmbeddings: parameter names and state-dict order of `BertModel(config).embeddings`."""

    def __init__(self, bert_config):
        super().__init__()
        c = bert_config
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden_size)
        self.position_embeddings = nn.Embedding(c.max_position_embeddings, c.hidden_size)
        self.token_type_embeddings = nn.Embedding(c.type_vocab_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)
        for m in (self.word_embeddings, self.position_embeddings, self.token_type_embeddings):
            m.weight.data.normal_(mean=0.0, std=c.initializer_range)
        self._register_load_state_dict_pre_hook(self._drop_index_buffers)

    @staticmethod
    def _drop_index_buffers(state_dict, prefix, *_):
        for name in ("position_ids", "token_type_ids"):       # buffers older `transformers` releases saved
            state_dict.pop(prefix + name, None)

    def forward(self, input_ids, token_type_ids, keep=None):
        """dropout(LayerNorm((W[id] + Tt[type]) + P[:T])) in torch ops; keep: the caller's keep mask instead of a fresh draw."""
        T = input_ids.shape[1]
        x = (self.word_embeddings.weight[input_ids] + self.token_type_embeddings.weight[token_type_ids]) + self.position_embeddings.weight[:T]
        y = F.layer_norm(x, (x.shape[-1],), self.LayerNorm.weight, self.LayerNorm.bias, self.LayerNorm.eps)
        if keep is not None:
            y = y * keep.to(y.dtype) * (1.0 / (1.0 - self.dropout.p))
        return y


class _BertDims:
    def __init__(self, bc):
        d = dict(bc) if isinstance(bc, dict) else vars(bc)
        self.vocab_size, self.hidden_size = int(d.get("vocab_size", 30522)), int(d.get("hidden_size", 768))
        self.max_position_embeddings, self.type_vocab_size = int(d.get("max_position_embeddings", 512)), int(d.get("type_vocab_size", 2))
        self.layer_norm_eps, self.hidden_dropout_prob = float(d.get("layer_norm_eps", 1e-12)), float(d.get("hidden_dropout_prob", 0.1))
        self.initializer_range = float(d.get("initializer_range", 0.02))


_WARNED_PRETRAINED = False


class BertEmbedding(nn.Module):
    def __init__(self, config, tokenizer=None):
        super().__init__()
        global _WARNED_PRETRAINED
        self.config = config
        lb = config.MODEL.LANGUAGE_BACKBONE
        head_config = config.MODEL.MMSS_HEAD.TRANSFORMER
        self.bert_config = _BertDims(head_config.BERT_CONFIG)
        if tokenizer is None:
            vocab_file = getattr(lb, "VOCAB_FILE", "")
            if not vocab_file:
                raise ValueError("BertEmbedding: pass a tokenizer or set MODEL.LANGUAGE_BACKBONE.VOCAB_FILE (nothing is downloaded)")
            tokenizer = WordPieceTokenizer(vocab_file)
        self.tokenizer = tokenizer
        if len(tokenizer) > self.bert_config.vocab_size or not 0 <= int(tokenizer.mask_token_id) < self.bert_config.vocab_size:
            raise ValueError(f"BertEmbedding: the tokenizer ({len(tokenizer)} tokens, [MASK] = {tokenizer.mask_token_id}) does not fit "
                             f"the {self.bert_config.vocab_size}-row word table")
        if lb.PRETRAINED and not _WARNED_PRETRAINED:
            _WARNED_PRETRAINED = True
            warnings.warn("MODEL.LANGUAGE_BACKBONE.PRETRAINED: nothing is downloaded; the weights are initialised as with PRETRAINED False "
                          "and are expected to come with the checkpoint (load_state_dict)")
        self.bert_model = BertEmbeddings(self.bert_config)
        self.freeze()
        self.out_channels = self.bert_config.hidden_size
        self.add_position_embedding = bool(lb.ADD_POSITION_EMBEDDING)
        self.mlm = head_config.MASKED_LANGUAGE_MODELING
        self.mlm_prob = head_config.MASKED_LANGUAGE_MODELING_PROB
        self.mlm_prob_mask = head_config.MASKED_LANGUAGE_MODELING_PROB_MASK
        self.mlm_prob_noise = head_config.MASKED_LANGUAGE_MODELING_PROB_NOISE
        self.mlm_during_validation = head_config.MASKED_LANGUAGE_MODELING_VALIDATION
        self.embeddings = self.bert_model.word_embeddings.weight          # the same Parameter under a second name (:103)
        self._staging = None                                              # (pinned int32 [4, N] block, the event behind its last upload)

    def freeze(self):
        if self.config.MODEL.LANGUAGE_BACKBONE.FREEZE:
            for p in self.parameters():
                p.requires_grad = False
        else:
            for name, param in self.named_parameters():
                if param.requires_grad and name != "bert_model.word_embeddings.weight":
                    param.requires_grad = False

    # ------------------------------------------------------------------------------------------------------------- the calls

    def forward(self, text_list):
        return self.forward_tokenized(self.tokenizer(text_list, max_length=MAX_LENGTH))

    def _mlm_numbers(self) -> ops.CaptionMlm:
        return ops.CaptionMlm(float(self.mlm_prob), float(self.mlm_prob_mask), float(self.mlm_prob_mask) + float(self.mlm_prob_noise),
                              int(self.tokenizer.mask_token_id), len(self.tokenizer))

    def _host_block(self, tokenized) -> np.ndarray:
        """The four lists as one int64 [4, B, T] array, validated against the tables (the ids are host integers here)."""
        try:
            block = np.stack([np.asarray(tokenized[k], dtype=np.int64) for k in TOKEN_KEYS])
        except ValueError as e:
            raise ValueError(f"forward_tokenized: the four token lists must be rectangular and of one shape ({e})") from None
        if block.ndim != 3:
            raise ValueError(f"forward_tokenized: the token lists must be [B, T], got {block.shape[1:]}")
        c = self.bert_config
        if block.size:
            if block[0].min() < 0 or block[0].max() >= c.vocab_size:
                raise ValueError(f"forward_tokenized: an input id lies outside the word table [0, {c.vocab_size})")
            if block[1].min() < 0 or block[1].max() >= c.type_vocab_size:
                raise ValueError(f"forward_tokenized: a token type id lies outside [0, {c.type_vocab_size})")
            if self.add_position_embedding and block.shape[2] > c.max_position_embeddings:
                raise ValueError(f"forward_tokenized: T = {block.shape[2]} exceeds the {c.max_position_embeddings} position embeddings")
        return block

    def _upload(self, block: np.ndarray, device) -> torch.Tensor:
        """One pinned, reused staging block and one non_blocking copy."""
        n = block.shape[1] * block.shape[2]
        if self._staging is None or self._staging[0].shape[1] != n:      # (torch's pinned allocator keeps a dropped block until its copy is done)
            self._staging = [torch.empty((4, n), dtype=torch.int32).pin_memory(), None]
        pinned, event = self._staging
        if event is not None:
            event.synchronize()                               # the previous call's copy, long finished: no wait in practice
        pinned.numpy()[...] = block.reshape(4, n)
        packed = pinned.to(device, non_blocking=True)
        self._staging[1] = torch.cuda.Event()
        self._staging[1].record(torch.cuda.current_stream(device))
        return packed

    def forward_tokenized(self, tokenized, draws: Optional[torch.Tensor] = None):
        """The reference's dictionary from the four token lists / arrays [B, T].  draws: float64 [2, B, T] on the parameters' device
        (default: torch.rand from that device's generator), read only when masked language modelling is active."""
        block = self._host_block(tokenized)
        _, B, T = block.shape
        W = self.embeddings
        device = W.device
        active = bool(self.mlm) and (self.training or bool(self.mlm_during_validation)) and float(self.mlm_prob) > 0.0
        mlm = self._mlm_numbers() if self.mlm else None
        if active:
            if draws is None:
                draws = torch.rand((2, B, T), dtype=torch.float64, device=device)
            elif tuple(draws.shape) != (2, B, T) or draws.dtype != torch.float64:
                raise ValueError(f"forward_tokenized: draws must be float64 [2, {B}, {T}], got {draws.dtype} {tuple(draws.shape)}")
            draws = draws.to(device)
        else:
            draws = None
        bm = self.bert_model
        keep = None
        if self.add_position_embedding and self.training and bm.dropout.p > 0.0:
            keep = (torch.rand((B, T, W.shape[1]), device=device) >= bm.dropout.p).to(torch.uint8)
        fused = (device.type == "cuda" and os.environ.get("LOCOV_FUSED_CAPTION", "1") != "0" and W.dtype == torch.float32
                 and 0 < B * T <= ops.CAPTION_MAX_TOKENS and W.shape[1] <= ops.CAPTION_MAX_HIDDEN)
        if fused:
            packed = self._upload(block, device)
            ln = dict(position=bm.position_embeddings.weight, token_type=bm.token_type_embeddings.weight, ln_weight=bm.LayerNorm.weight,
                      ln_bias=bm.LayerNorm.bias, eps=bm.LayerNorm.eps, keep=keep, p_drop=bm.dropout.p) if self.add_position_embedding else {}
            ints, emb, enc = ops.caption_embed(packed, draws.reshape(2, B * T) if draws is not None else None, T, W, mlm=mlm,
                                               with_targets=bool(self.mlm), **ln)
            out = {k: ints[i].view(B, T) for i, k in enumerate(TOKEN_KEYS)}
            if self.mlm:
                out["target_ids"], out["mlm_mask"] = ints[4].view(B, T), ints[5].view(B, T)
            emb = emb.view(B, T, -1)
            out["encoded_tokens"] = enc.view(B, T, -1) if enc is not None else emb
            out["input_embeddings"] = emb
            return out
        return self._torch_embed(torch.from_numpy(block).to(device), draws, mlm, keep)

    def _torch_embed(self, block: torch.Tensor, draws, mlm, keep):
        """The definition: :114-154 as torch ops on the tensors' device."""
        ids, types, attn, special = block[0], block[1], block[2], block[3]
        out = {"input_ids": ids, "token_type_ids": types, "attention_mask": attn, "special_tokens_mask": special}
        if self.mlm:
            out["input_ids"], out["special_tokens_mask"], out["target_ids"], out["mlm_mask"] = caption_rule(ids, types, attn, special, draws, mlm)
        emb = self.embeddings[out["input_ids"]]
        out["encoded_tokens"] = self.bert_model(out["input_ids"], types, keep) if self.add_position_embedding else emb
        out["input_embeddings"] = emb
        return out


@LANGUAGE_BACKBONES_REGISTRY.register()
def build_bertemb_backbone(cfg, tokenizer=None):
    body = BertEmbedding(cfg, tokenizer)
    model = nn.Sequential(OrderedDict([("body", body)]))
    model.out_channels = body.out_channels
    return model


def build_language_backbone(cfg, tokenizer=None):
    """ovr/modeling/language/backbone.py:build_backbone: the builder MODEL.LANGUAGE_BACKBONE.TYPE names."""
    name = cfg.MODEL.LANGUAGE_BACKBONE.TYPE
    assert name in LANGUAGE_BACKBONES_REGISTRY, \
        f"cfg.MODEL.LANGUAGE_BACKBONE.TYPE: {name} is not registered in registry"
    model = LANGUAGE_BACKBONES_REGISTRY.get(name)(cfg, tokenizer)
    model.to(torch.device(cfg.MODEL.DEVICE))
    return model
