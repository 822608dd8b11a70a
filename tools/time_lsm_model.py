"""The LSM model's caption path and one whole training step, timed in a fresh process.

    timeout -k 10 900 python tools/time_lsm_model.py [--iters 50] [--warmup 10] [--skip-step] [--out records.json]

  (a) language backbone  BertEmbedding.forward_tokenized at the per-GPU LSM shape (B = 4 captions, T = 70 tokens, H = 768,
                         V = 30 522, masked language modelling on, training mode): host wall time per call, the call followed by
                         a device synchronisation, on the kernel path (ops.caption_embed, one launch) and with
                         LOCOV_FUSED_CAPTION=0 (the torch expression on the device), for both ADD_POSITION_EMBEDDING values; with
                         FREEZE False also forward plus backward (the weight gradient of the [V, H] word table).  The two sides
                         alternate in one process and swap order every iteration.
  (b) training step      DistillProposalMMSSRCNN (R50-C4, GroundingHead + TransformerHead, KD, SPATIAL_DROPOUT 100) forward and
                         backward on --step-images images of --step-size pixels, BERT_CONFIG at --step-layers layers.
Protocol: >= 10 warm-up and >= 50 timed iterations per side; median and 10th / 90th percentile.  Needs a ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, T, H, V = 4, 70, 768, 30522


class Tokenizer:
    """A stand-in of bert-base-uncased's size: the timing does not depend on which words the ids name."""
    mask_token_id = 103

    def __len__(self):
        return V


def spread(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "n": len(ms)}


def alternate_wall(sides, iters, warmup):
    """Host wall time of each side's call plus a device synchronisation, the sides alternating and swapping order."""
    names = list(sides)
    ms = {k: [] for k in names}
    for it in range(warmup + iters):
        for k in (names if it % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sides[k]()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in ms.items()}


def language_backbone(add_pos, freeze, dev):
    from locov_amd.config import get_cfg
    from locov_amd.language_backbone import build_language_backbone
    cfg = get_cfg()
    cfg.MODEL.DEVICE = str(dev)
    lb, tr = cfg.MODEL.LANGUAGE_BACKBONE, cfg.MODEL.MMSS_HEAD.TRANSFORMER
    lb.TYPE, lb.PRETRAINED, lb.ADD_POSITION_EMBEDDING, lb.FREEZE = "build_bertemb_backbone", False, add_pos, freeze
    tr.MASKED_LANGUAGE_MODELING = True
    return build_language_backbone(cfg, Tokenizer()).train()


def tokens(rng):
    ids = rng.integers(1000, V, size=(B, T))
    lengths = rng.integers(8, 20, size=B)
    attn = (np.arange(T)[None] < lengths[:, None]).astype(np.int64)
    ids = ids * attn
    special = 1 - attn
    ids[:, 0], special[:, 0] = 101, 1
    for i, n in enumerate(lengths):
        ids[i, n - 1], special[i, n - 1] = 102, 1
    return {"input_ids": ids.tolist(), "token_type_ids": np.zeros((B, T), np.int64).tolist(), "attention_mask": attn.tolist(),
            "special_tokens_mask": special.tolist()}


def time_backbone(args, dev):
    rng = np.random.default_rng(0)
    tok = tokens(rng)
    rec = {}
    for add_pos in (False, True):
        for freeze in (True, False):
            m = language_backbone(add_pos, freeze, dev).body

            def call(fused, backward=not freeze):
                os.environ["LOCOV_FUSED_CAPTION"] = fused
                out = m.forward_tokenized(tok)
                if backward:
                    m.embeddings.grad = None
                    (out["encoded_tokens"].sum() + out["input_embeddings"].sum()).backward()
            try:
                t = alternate_wall({"kernel": lambda: call("1"), "torch": lambda: call("0")}, args.iters, args.warmup)
            finally:
                os.environ.pop("LOCOV_FUSED_CAPTION", None)
            key = f"add_position_embedding={add_pos} freeze={freeze} ({'forward' if freeze else 'forward+backward'})"
            rec[key] = dict(t, kernel_faster=t["kernel"]["median_ms"] < t["torch"]["median_ms"])
            print(json.dumps({key: rec[key]}), flush=True)
    return rec


def time_step(args, dev):
    import locov_amd
    from locov_amd.structures import Boxes, Instances
    torch.manual_seed(0)
    cfg = locov_amd.config.get_cfg()
    m = cfg.MODEL
    m.META_ARCHITECTURE, m.DEVICE, m.PIXEL_STD, m.LOAD_EMB_PRED_FROM_MMSS_HEAD = "DistillProposalMMSSRCNN", str(dev), [57.375, 57.12, 58.395], True
    m.BACKBONE.TRAIN_ON_DEVICE = True
    m.ROI_HEADS.NAME, m.ROI_HEADS.BATCH_SIZE_PER_IMAGE, m.ROI_HEADS.POSITIVE_FRACTION = "EmbeddingProposalsRes5ROIHeads", 200, 1.0
    m.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG, m.ROI_BOX_HEAD.EMBEDDING_BASED = True, True
    m.LANGUAGE_BACKBONE.TYPE, m.LANGUAGE_BACKBONE.PRETRAINED = "build_bertemb_backbone", False
    h = m.MMSS_HEAD
    h.TYPES, h.TIE_VL_PROJECTION_WEIGHTS, h.SPATIAL_DROPOUT, h.DISTILLATION_LOSS = ("GroundingHead", "TransformerHead"), True, 100, True
    h.TRANSFORMER.MASKED_LANGUAGE_MODELING, h.TRANSFORMER.MMM_LOSS = True, "cross_entropy"
    h.TRANSFORMER.BERT_CONFIG.num_hidden_layers, h.TRANSFORMER.BERT_CONFIG.num_attention_heads = args.step_layers, 8      # coco_lsm.yaml: 6, 8
    model = locov_amd.build_model(cfg, tokenizer=Tokenizer()).train()
    model.roi_heads.box_predictor.set_class_embeddings(torch.randn(81, m.ROI_BOX_HEAD.EMB_DIM) * 0.05)
    model.roi_heads.num_classes = model.roi_heads.box_predictor.num_classes
    hh, ww = args.step_size
    rng = np.random.default_rng(1)
    g = torch.Generator().manual_seed(2)
    tok = tokens(rng)
    inputs = []
    for i in range(args.step_images):
        xy = torch.rand(6, 2, generator=g) * torch.tensor([ww * 0.6, hh * 0.6])
        boxes = torch.cat([xy, xy + 40.0 + torch.rand(6, 2, generator=g) * torch.tensor([ww * 0.35, hh * 0.35])], dim=1)
        inputs.append({"image": torch.randint(0, 256, (3, hh, ww), dtype=torch.uint8, generator=g).to(dev),
                       "instances": Instances((hh, ww), gt_boxes=Boxes(boxes), gt_classes=torch.randint(0, 80, (6,), generator=g)),
                       "tokens": {k: v[i % B] for k, v in tok.items()}})

    def step():
        model.zero_grad(set_to_none=True)
        _, losses = model(inputs)
        sum(losses.values()).backward()
        return losses
    t = alternate_wall({"step": step}, args.iters, args.warmup)["step"]
    rec = dict(t, images=args.step_images, size=[hh, ww], bert_layers=args.step_layers, losses=sorted(step()))
    print(json.dumps({"training step": rec}), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true", help="only (a)")
    ap.add_argument("--step-images", type=int, default=4)
    ap.add_argument("--step-size", type=int, nargs=2, default=[800, 1333])
    ap.add_argument("--step-layers", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the record as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_lsm_model: needs a ROCm GPU")
    if args.iters < 50 or args.warmup < 10:
        raise SystemExit("time_lsm_model: the protocol asks for >= 10 warm-up and >= 50 timed iterations")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rec = {"device": torch.cuda.get_device_name(dev), "shape": {"B": B, "T": T, "H": H, "V": V}, "language_backbone": time_backbone(args, dev)}
    if not args.skip_step:
        rec["training_step"] = time_step(args, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
