"""Shared by tests/test_lsm_model_host.py and tests/test_gpu_lsm_model.py: the toy LSM configuration (R50-C4, five classes,
BERT_CONFIG vocab 50 / hidden 64 / 1 layer), a tokenizer object over that vocabulary, and the two-image batch with captions."""
import numpy as np
import torch

STD = [57.375, 57.12, 58.395]
VOCAB, HIDDEN, T = 50, 64, 12
PAD, UNK, CLS, SEP, MASK = 0, 1, 2, 3, 4


class ToyTokenizer:
    """Any object with __call__(text_list, max_length), mask_token_id and __len__: words are 'w<id>'."""
    mask_token_id = MASK

    def __len__(self):
        return VOCAB

    def __call__(self, text_list, max_length=70):
        out = {k: [] for k in ("input_ids", "token_type_ids", "attention_mask", "special_tokens_mask")}
        for text in text_list:
            ids = [CLS] + [int(w[1:]) for w in text.split()][:max_length - 2] + [SEP]
            n, pad = len(ids), max_length - len(ids)
            out["input_ids"].append(ids + [PAD] * pad)
            out["token_type_ids"].append([0] * max_length)
            out["attention_mask"].append([1] * n + [0] * pad)
            out["special_tokens_mask"].append([1] + [0] * (n - 2) + [1] + [1] * pad)
        return out


class SizedTokenizer(ToyTokenizer):
    """The same with a given len() and [MASK] id (the caption kernels' tests)."""

    def __init__(self, n, mask_id=MASK):
        self.n, self.mask_token_id = n, mask_id

    def __len__(self):
        return self.n


def toy_cfg(pkg, device, arch="DistillProposalMMSSRCNN", **over):
    cfg = pkg.config.get_cfg()
    m = cfg.MODEL
    m.META_ARCHITECTURE, m.DEVICE, m.PIXEL_STD = arch, device, STD
    m.LOAD_EMB_PRED_FROM_MMSS_HEAD = True
    m.BACKBONE.TRAIN_ON_DEVICE = device != "cpu"
    m.RPN.PRE_NMS_TOPK_TEST, m.RPN.POST_NMS_TOPK_TEST = 200, 50
    m.RPN.PRE_NMS_TOPK_TRAIN, m.RPN.POST_NMS_TOPK_TRAIN = 200, 50
    m.ROI_HEADS.NAME, m.ROI_HEADS.NUM_CLASSES, m.ROI_HEADS.BATCH_SIZE_PER_IMAGE, m.ROI_HEADS.SCORE_THRESH_TEST = \
        "EmbeddingProposalsRes5ROIHeads", 5, 32, 0.0
    m.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG, m.ROI_BOX_HEAD.EMBEDDING_BASED, m.ROI_BOX_HEAD.EMB_DIM = True, True, HIDDEN
    m.LANGUAGE_BACKBONE.TYPE, m.LANGUAGE_BACKBONE.PRETRAINED = "build_bertemb_backbone", False
    h = m.MMSS_HEAD
    h.TYPES, h.DEFAULT_HEAD, h.TIE_VL_PROJECTION_WEIGHTS = ("GroundingHead", "TransformerHead"), "GroundingHead", True
    h.SPATIAL_DROPOUT, h.DISTILLATION_LOSS = 16, True
    t = h.TRANSFORMER
    t.MASKED_LANGUAGE_MODELING, t.MMM_LOSS = True, "cross_entropy"
    t.BERT_CONFIG.update(vocab_size=VOCAB, hidden_size=HIDDEN, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                         max_position_embeddings=32)
    for k, v in over.items():
        node = cfg
        *parents, leaf = k.split(".")
        for p in parents:
            node = node[p]
        node[leaf] = v
    return cfg


def captions():
    return ["w10 w11 w12 w13 w14 w15 w16", "w20 w21 w10 w22"]


def inputs(pkg, with_gt=True, tokens=False):
    g = torch.Generator().manual_seed(5)
    out = []
    tok = ToyTokenizer()(captions(), max_length=T)
    # (Res5 grids of 5 x 6 and 4 x 5 valid cells: both hold SPATIAL_DROPOUT = 16 regions)
    for n, ((h, w), (oh, ow)) in enumerate((((160, 192), (240, 427)), ((128, 160), (61, 75)))):
        d = {"image": torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g), "height": oh, "width": ow}
        if with_gt:
            boxes = torch.tensor([[8.0, 10.0, 60.0, 70.0], [50.0, 20.0, w - 6.0, h - 9.0], [30.0, 30.0, 62.0, 58.0]])
            d["instances"] = pkg.structures.Instances((h, w), gt_boxes=pkg.structures.Boxes(boxes), gt_classes=torch.tensor([0, 3, 4]))
        if tokens:
            d["tokens"] = {k: v[n] for k, v in tok.items()}
        else:
            d["caption"] = captions()[n]
        out.append(d)
    return out


def mlm_draws(seed=3):
    """float64 [2, 2, T] draws that select and mask at least one word of each caption (tests/test_lsm_model_host.py asserts it)."""
    d = np.random.default_rng(seed).random((2, 2, T))
    d[0, 0, 2], d[0, 1, 1] = 0.01, 0.02                      # u < 0.15 and u / 0.15 < 0.9: [MASK]
    return d
