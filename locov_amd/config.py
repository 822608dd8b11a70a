"""The configuration keys the LSM ROI-head path reads, with the reference's defaults.

The reference uses a yacs CfgNode (detectron2.config.get_cfg + ovr/config/config.py:4-174
add_ovr_config).  yacs / Detectron2 are not installed here, so this is a minimal attribute
tree holding exactly the keys of SURVEY.md section 5.6 -- same names, same defaults
([D2-upstream] defaults marked) -- and it can read the reference's own yaml files
(configs/coco_lsm.yaml, configs/coco_stt.yaml): unknown keys are kept, not rejected, so the
rest of those files passes through untouched.  A real Detectron2 CfgNode works just as well
with every from_config in this package (only attribute access is used).
"""
from __future__ import annotations

import copy
from ast import literal_eval
from typing import Any, Dict


class CfgNode(dict):
    def __init__(self, init: Dict[str, Any] = None):
        super().__init__()
        for k, v in (init or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) and not isinstance(v, CfgNode) else v

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value

    def clone(self) -> "CfgNode":
        return copy.deepcopy(self)

    def merge_from_dict(self, other: Dict[str, Any]) -> None:
        for k, v in other.items():
            if isinstance(v, dict):
                if k not in self or not isinstance(self[k], CfgNode):
                    self[k] = CfgNode()
                self[k].merge_from_dict(v)
            else:
                if isinstance(v, str):
                    try:    # yaml keeps python tuples such as ("backbone.body.",) as strings
                        lit = literal_eval(v)
                        if isinstance(lit, (tuple, list)):
                            v = lit
                    except (ValueError, SyntaxError):
                        pass
                self[k] = v

    def merge_from_file(self, path: str) -> None:
        import yaml
        with open(path, "r") as f:
            self.merge_from_dict(yaml.safe_load(f) or {})

    def merge_from_list(self, opts) -> None:
        """["MODEL.ROI_HEADS.NUM_CLASSES", 80, ...] as in train_ovnet.py:49-56."""
        assert len(opts) % 2 == 0
        for full_key, v in zip(opts[0::2], opts[1::2]):
            node = self
            *parents, leaf = full_key.split(".")
            for p in parents:
                node = node.setdefault(p, CfgNode())
            if isinstance(v, str):
                try:
                    v = literal_eval(v)
                except (ValueError, SyntaxError):
                    pass
            node[leaf] = v


def get_cfg() -> CfgNode:
    """Defaults for the keys the hot path reads."""
    return CfgNode({
        "MODEL": {
            "DEVICE": "cuda",
            "META_ARCHITECTURE": "GeneralizedRCNN",                # [D2-upstream]; coco_stt.yaml -> "OvrRCNN" (meta_arch.py)
            "PIXEL_MEAN": [103.530, 116.280, 123.675],             # [D2-upstream] (BGR)
            "PIXEL_STD": [1.0, 1.0, 1.0],                          # [D2-upstream]
            "MASK_ON": False,
            "KEYPOINT_ON": False,
            "LOAD_EMB_PRED_FROM_MMSS_HEAD": False,                # config.py:13
            "LOAD_OBJ_PROPOSALS": False,                          # config.py:14; coco_lsm.yaml -> True (data.py: the OLN pseudo-GT)
            # NAME, FREEZE_AT: [D2-upstream]; coco_lsm.yaml -> FREEZE_AT 0.  TRAIN_ON_DEVICE (this port): a backbone with trainable
            # weights runs forward AND backward on the gfx950 kernels instead of the torch path (backbone.py; opt-in)
            "BACKBONE": {"NAME": "build_resnet_backbone", "FREEZE_AT": 2, "TRAIN_ON_DEVICE": False},
            "PROPOSAL_GENERATOR": {"NAME": "RPN", "MIN_SIZE": 0},     # [D2-upstream]
            "ANCHOR_GENERATOR": {                                  # [D2-upstream]
                "NAME": "DefaultAnchorGenerator",
                "SIZES": [[32, 64, 128, 256, 512]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]], "OFFSET": 0.0,
            },
            "RPN": {                                               # [D2-upstream]; coco_lsm.yaml -> PRE_NMS_TOPK_TEST 6000
                "HEAD_NAME": "StandardRPNHead",
                "IN_FEATURES": ["res4"],
                "BBOX_REG_WEIGHTS": (1.0, 1.0, 1.0, 1.0),
                "PRE_NMS_TOPK_TRAIN": 12000, "PRE_NMS_TOPK_TEST": 6000,
                "POST_NMS_TOPK_TRAIN": 2000, "POST_NMS_TOPK_TEST": 1000,
                "NMS_THRESH": 0.7,
                "CONV_DIMS": [-1],
                # the training half: anchor labelling, the sample draw and the two losses
                "IOU_THRESHOLDS": [0.3, 0.7], "IOU_LABELS": [0, -1, 1],
                "BATCH_SIZE_PER_IMAGE": 256, "POSITIVE_FRACTION": 0.5,
                "BOUNDARY_THRESH": -1,
                "LOSS_WEIGHT": 1.0, "BBOX_REG_LOSS_WEIGHT": 1.0,
                "BBOX_REG_LOSS_TYPE": "smooth_l1", "SMOOTH_L1_BETA": 0.0,
            },
            "ROI_HEADS": {
                "NAME": "EmbeddingRes5ROIHeads",
                "IN_FEATURES": ["res4"],                           # [D2-upstream]
                "NUM_CLASSES": 80,
                "BATCH_SIZE_PER_IMAGE": 512,                       # [D2-upstream]; coco_lsm.yaml:32 -> 200
                "POSITIVE_FRACTION": 0.25,                         # [D2-upstream]; coco_lsm.yaml:30 -> 1.0
                "IOU_THRESHOLDS": [0.5],                           # [D2-upstream]
                "IOU_LABELS": [0, 1],                              # [D2-upstream]
                "PROPOSAL_APPEND_GT": True,                        # [D2-upstream]
                "SCORE_THRESH_TEST": 0.05,                         # [D2-upstream]
                "NMS_THRESH_TEST": 0.5,                            # [D2-upstream]
                "DETACH_CLASS_PREDICTOR": False,                   # config.py:136
                # read by EmbeddingGroundingFastRCNNOutputLayers.from_config (box_emb_grounding_head.py:355) but
                # never defined in ovr/config/config.py; defined here so that the predictor can be built
                "MAX_TOKENS": 8,
            },
            # config.py:23-28 (language_backbone.py).  coco_lsm.yaml -> TYPE "build_bertemb_backbone"; the default names the full BERT
            # class, which is not built here.  VOCAB_FILE (this port): the vocab.txt the default WordPieceTokenizer is built from
            "LANGUAGE_BACKBONE": {"TYPE": "build_bert_backbone", "FREEZE": True, "EMBEDDING_PATH": "", "ADD_POSITION_EMBEDDING": False,
                                  "PRETRAINED": True, "VOCAB_FILE": ""},
            "MMSS_HEAD": {
                "TYPES": ("GroundingHead",), "DEFAULT_HEAD": "GroundingHead",          # config.py:36-41
                "TIE_VL_PROJECTION_WEIGHTS": False, "IN_FEATURES": "res5",
                "SPATIAL_DROPOUT": -1,                             # coco_lsm.yaml -> 100
                "GROUNDING": {                                     # config.py:51-63
                    "LOCAL_METRIC": "dot", "GLOBAL_METRIC": "aligned_local", "ALIGNMENT": "softmax",
                    "ALIGNMENT_TEMPERATURE": 10.0,
                    "LOSS": "cross_entropy", "NEGATIVE_MINING": "random", "TRIPLET_MARGIN": 1.0,
                    "ALIGN_WORDS_TO_REGIONS": True, "ALIGN_REGIONS_TO_WORDS": True,
                    "TEXT_INPUT": "input_embeddings",
                },
                "DISTILLATION_LOSS": False,                        # config.py:43; coco_lsm.yaml -> True
                "DISTILLATION_LOSS_TYPE": "KD", "DISTILLATION_TEMPERATURE": 1.0, "DISTILLATION_LOSS_WEIGHT": 1.0,      # config.py:44-48
                "DISTILLATION_DETACH_TEACHER": False, "DISTILLATION_TEACHER_TRANSFORMER": True,
                "TRANSFORMER": {                                   # config.py:66-102 (keys TransformerHead reads)
                    "MASKED_LANGUAGE_MODELING": False,             # config.py:67-79 (language_backbone.py, meta_arch.py)
                    "MASKED_LANGUAGE_MODELING_PROB": 0.15, "MASKED_LANGUAGE_MODELING_PROB_MASK": 0.9,
                    "MASKED_LANGUAGE_MODELING_PROB_NOISE": 0.0, "MASKED_LANGUAGE_MODELING_VALIDATION": True,
                    "MASKED_VISUAL_MODELING": False,
                    "MVM_LOSS": "",                                # "", "reconstruction_error" or "contrastive_cross_entropy"
                    "MVM_LOSS_NUM_NEGATIVE": 128,
                    "MMM_LOSS": "",                                # "" or "cross_entropy"; coco_lsm.yaml -> "cross_entropy"
                    "BERT_CONFIG": {
                        "vocab_size": 30522, "hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12,
                        "intermediate_size": 3072, "hidden_act": "gelu", "hidden_dropout_prob": 0.1,
                        "attention_probs_dropout_prob": 0.1, "max_position_embeddings": 512, "type_vocab_size": 2,
                        "initializer_range": 0.02, "layer_norm_eps": 1e-12, "pad_token_id": 0, "gradient_checkpointing": False,
                    },
                    "pretrained_weights": False,
                },
            },
            "ROI_BOX_HEAD": {
                "NAME": "EmbeddingFastRCNNOutputLayers",
                "POOLER_RESOLUTION": 14,                           # [D2-upstream]
                "POOLER_TYPE": "ROIAlignV2",                       # [D2-upstream]
                "POOLER_SAMPLING_RATIO": 0,                        # [D2-upstream]
                "CLS_AGNOSTIC_BBOX_REG": False,                    # coco_lsm.yaml:36 -> True
                "BBOX_REG_WEIGHTS": (10.0, 10.0, 5.0, 5.0),        # [D2-upstream]
                "BBOX_REG_LOSS_TYPE": "smooth_l1",                 # [D2-upstream] "smooth_l1", "giou", "diou" or "ciou"
                "BBOX_REG_LOSS_WEIGHT": 1.0,                       # [D2-upstream]
                "SMOOTH_L1_BETA": 0.0,                             # [D2-upstream]
                "USE_SIGMOID_CE": False,                           # [D2-upstream] per-class sigmoid cross-entropy instead of the softmax
                "USE_FED_LOSS": False,                             # [D2-upstream] ... over a federated class set (needs USE_SIGMOID_CE)
                "FED_LOSS_FREQ_WEIGHT_POWER": 0.5,                 # [D2-upstream] sampling weight = image count ** this
                "FED_LOSS_NUM_CLASSES": 50,                        # [D2-upstream] size the class set is filled up to
                "EMBEDDING_BASED": False,                          # config.py:124
                "EMB_DIM": 768,                                    # config.py:126
                "FREEZE_EMB_PRED": False,                          # config.py:129
                "NORMALIZE_EMB_PRED": False,                       # config.py:131
                "STANDARDIZE_EMB_PRED": False,                     # config.py:133
                # extension (not in the reference): dtype of the similarity GEMM operands
                "SIM_GEMM_DTYPE": "fp32",
                # extension: "hip" = hand-written channels-last MFMA GEMM Res5, "miopen" = torch conv2d
                "RES5_BACKEND": "hip",
                "RES5_CONV3X3": "winograd",
                # extension: arithmetic of the Res5 GEMMs on the HIP backend.  "f16x2": fp32 in / fp32 out, products formed
                # from split (hi, lo) f16 operand pairs on the f16 matrix pipe, fp32 accumulate -- error vs fp64 no larger
                # than the f32 MFMA's, ~2x its speed (activations must stay below 4094 in magnitude); "fp32": the f32 MFMA;
                # "bf16": bf16 operands (reduced precision, opt-in, not a parity configuration)
                "RES5_DTYPE": "f16x2",
                # extension: with "f16x2" every split launch ORs a range-guard word when an activation left fp16's range; the
                # heads read it once per call and repeat the call on the f32 MFMA (with a warning) if it is set
                "RES5_OVERFLOW_CHECK": True,
                # training forwards: "sync" = the guard word is looked at at the end of the ROI heads' forward (an event wait behind
                # the Res5 calls that leaves the predictor's launches queued) and an out-of-range forward is repeated on the f32
                # MFMA; "deferred" = never read inside the step, acted on on the device (a skipped step), read with the next labelling
                "RES5_TRAIN_GUARD": "sync",
                # extension: memory layout of EmbeddingProposalsRes5ROIHeads' visual_grid_features.  "nchw": contiguous NCHW (one
                # transpose of Res5's pixel rows each way); "channels_last": the same logical [N, C5, H/2, W/2] tensor as a view of
                # those rows, no transpose -- for callers that only gather regions from it (mmss_regions.grid_regions)
                "GRID_FEATURES_LAYOUT": "nchw",
            },
            "RESNETS": {
                "NUM_GROUPS": 1, "WIDTH_PER_GROUP": 64, "RES2_OUT_CHANNELS": 256,
                "STRIDE_IN_1X1": True, "NORM": "FrozenBN",
                "DEFORM_ON_PER_STAGE": [False, False, False, False],
                "DEPTH": 50, "OUT_FEATURES": ["res4"], "STEM_OUT_CHANNELS": 64, "RES5_DILATION": 1,     # [D2-upstream] (backbone.py)
            },
        },
        "INPUT": {                                                 # [D2-upstream] (data.py: build_augmentation, DatasetMapper)
            "FORMAT": "BGR",
            "MIN_SIZE_TRAIN": (800,), "MIN_SIZE_TRAIN_SAMPLING": "choice", "MAX_SIZE_TRAIN": 1333,
            "MIN_SIZE_TEST": 800, "MAX_SIZE_TEST": 1333,
            "RANDOM_FLIP": "horizontal",                           # "horizontal", "vertical" or "none" (config.py:166)
            "CROP": {"ENABLED": False},                            # True is refused: RandomCrop is not built
            # config.py:168-174, the strong augmentations: off in both yaml files; anything else is refused (not built)
            "COLOR_JITTER": 0.0, "RANDOM_GRAY_SCALE": False, "GAUSSIAN_BLUR": False, "RANDOM_ERASE": False,
        },
        "VIS_PERIOD": 0,                                           # [D2-upstream]; > 0 is refused (meta_arch.py)
        "TEST": {"DETECTIONS_PER_IMAGE": 100},                     # [D2-upstream]
        # [D2-upstream] (TRAIN: USE_FED_LOSS reads its class_image_count; ..._TOPK_*: the mapper's cut under MODEL.LOAD_OBJ_PROPOSALS)
        "DATASETS": {"TRAIN": (), "PRECOMPUTED_PROPOSAL_TOPK_TRAIN": 2000, "PRECOMPUTED_PROPOSAL_TOPK_TEST": 1000},
        "SOLVER": {                                                # [D2-upstream] (solver.py); the yaml files set BASE_LR, STEPS, MAX_ITER, ...
            "BASE_LR": 0.001, "MOMENTUM": 0.9, "NESTEROV": False,
            "WEIGHT_DECAY": 0.0001, "WEIGHT_DECAY_NORM": 0.0, "BIAS_LR_FACTOR": 1.0, "WEIGHT_DECAY_BIAS": 0.0001,
            "GAMMA": 0.1, "STEPS": (30000,), "MAX_ITER": 40000,
            "WARMUP_FACTOR": 0.001, "WARMUP_ITERS": 1000, "WARMUP_METHOD": "linear", "LR_SCHEDULER_NAME": "WarmupMultiStepLR",
            # ENABLED False: coco_lsm.yaml, which sets only CLIP_VALUE, does not clip
            "CLIP_GRADIENTS": {"ENABLED": False, "CLIP_TYPE": "value", "CLIP_VALUE": 1.0, "NORM_TYPE": 2.0},
            # extension (this port): the update as ONE launch of the gfx950 kernel (solver.FusedSGD) instead of torch.optim.SGD.
            # True: 3.0x - 11.9x faster than torch's best variant on both models' parameter sets (docs/experiments.md, "Solver")
            "FUSED_ON_DEVICE": True,
        },
    })
