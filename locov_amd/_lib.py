"""ctypes binding of liblocov_hip.so (the C ABI of include/locov_hip.h).

The library is loaded on first use and the import fails loudly if it is missing or lacks a
symbol: there is no PyTorch / CPU fallback for the hot path.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float,c_int, c_int64, c_uint, c_void_p, POINTER

HERE = os.path.dirname(os.path.abspath(__file__))
# LOCOV_HIP_LIB: developer override to A/B an experimental build of the same ABI (tools/)
LIB_PATH = os.environ.get("LOCOV_HIP_LIB") or os.path.join(HERE, "liblocov_hip.so")

OK = 0
F32, BF16 = 0, 1
NORM_NONE, NORM_L2, NORM_STANDARDIZE = 0, 1, 2
EPI_RELU = 1
WINO_OUT_ROI_MAJOR = 0x100
WINO_IN_ROI_MAJOR = 0x200
SEGMEAN_RES_ROI_MAJOR = 0x400
GEMM_A_SPLIT = 0x1000
EPI_OUT_SPLIT = 0x2000
EPI_RES_SPLIT = 0x4000
MAX_LEVELS = 8
ZERO_LIST_MAX = 24
LABEL_MAX_IMAGES, LABEL_MAX_THRESHOLDS, SAMPLE_MAX_PROPOSALS = 64, 6, 4096
ABI_VERSION = 8
DETECT_MAX_CANDIDATES, DETECT_FLAG_NONFINITE, DETECT_FLAG_OVERFLOW = 8192, 1, 2
RPN_FLAG_NONFINITE, RPN_MAX_PRE_NMS_TOPK, RPN_MAX_ANCHORS = 1, 16384, (1 << 22) - 1
RPN_LOSS_FLAG_DEGENERATE = 1
FED_LOSS_MAX_CLASSES = 32767
DISTILL_KD, DISTILL_JS, DISTILL_MSE, DISTILL_MAX_B = 0, 1, 2, 64
GROUNDING_ALIGN_SOFTMAX, GROUNDING_ALIGN_HARDMAX = 0, 1
TRIPLET_HARDEST, TRIPLET_EASIEST, TRIPLET_GIVEN = 0, 1, 2
BOX_IOU_GIOU, BOX_IOU_DIOU, BOX_IOU_CIOU = 0, 1, 2
REGIONS_MAX_B, REGIONS_MAX_CANDIDATES = 64, 4096
REGIONS_GRID, REGIONS_GRID_ALL, REGIONS_BOXES = 0, 1, 2
REGIONS_ROWS, REGIONS_NCHW = 0, 1
IMAGE_U8, IMAGE_F32, IMAGE_MAX_CHANNELS = 0, 1, 4
MHA_MAX_S, MHA_MAX_GRID, MHA_HEAD_DIMS = 4096, 65535, (32, 64, 96, 128)
CAPTION_MAX_TOKENS, CAPTION_MAX_HIDDEN = 8192, 4096
SGD_MAX_CLASSES, SGD_CHUNK, SGD_RECORD_BYTES = 8, 4096, 48
SGD_CLIP_NONE, SGD_CLIP_VALUE, SGD_CLIP_NORM = 0, 1, 2
COCO_MAX_AREAS, COCO_MAX_THRESHOLDS, COCO_MAX_CAPS, COCO_MAX_RECALL_THRESHOLDS = 4, 16, 3, 256
COCO_MAX_DET, COCO_MAX_BLOCKS = 4096, 8388608
LVIS_CELL_NEG, LVIS_CELL_NOT_EXHAUSTIVE = 1, 2
PROPOSAL_RECALL_MAX_LIMIT, PROPOSAL_RECALL_MAX_GT, PROPOSAL_RECALL_MAX_LIMITS = 2048, 1024, 4
RESIZE_MAX_TAPS, FLIP_NONE, FLIP_HORIZONTAL, FLIP_VERTICAL = 17, 0, 1, 2
PROPOSAL_F32, PROPOSAL_F64 = 0, 1
AUG_OP_BRIGHTNESS, AUG_OP_CONTRAST, AUG_OP_SATURATION, AUG_OP_HUE, AUG_MAX_ERASERS = 1, 2, 3, 4, 3

_p = c_void_p  # device pointer

WEIGHT_PREP_MAX_JOBS = 32
AMAX_BOUND_MAX = 4
PREP_PLAIN, PREP_TRANSPOSE, PREP_IM2COL, PREP_IM2COL_FLIP, PREP_WINO, PREP_WINO_FLIP = range(6)


class WeightPrepJob(ctypes.Structure):
    """locov_weight_prep_job of include/locov_hip.h"""
    _fields_ = [("w", c_void_p), ("row_scale", c_void_p), ("out", c_void_p), ("scale", c_float), ("kind", c_int), ("N", c_int), ("K", c_int)]


class AugmentDesc(ctypes.Structure):
    """locov_augment_desc of include/locov_hip.h"""
    _fields_ = [("height", ctypes.c_int32), ("width", ctypes.c_int32), ("n_ops", ctypes.c_int32), ("ops", ctypes.c_int32 * 4),
                ("brightness", c_float), ("contrast", c_float), ("saturation", c_float), ("hue_shift", ctypes.c_int32),
                ("gray", ctypes.c_int32), ("sigma", c_float), ("n_erase", ctypes.c_int32),
                ("erase", (ctypes.c_int32 * 4) * AUG_MAX_ERASERS), ("noise_offset", c_int64)]


# name -> (restype, argtypes); mirrors include/locov_hip.h declaration by declaration
SIGNATURES = {
    "locov_abi_version": (c_int, []),
    "locov_last_error": (c_char_p, []),
    "locov_launch_count": (c_int64, []),
    "locov_device_info": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "locov_level_assign": (c_int, [_p, c_int64, c_int, c_int, c_int, c_int, _p, _p]),
    "locov_roi_align_fwd": (c_int, [_p, c_int, c_int, c_int, c_int, _p, c_int64, c_int, c_int, c_float,
                                    c_int, c_int, _p, _p]),
    "locov_roi_align_bwd": (c_int, [_p, c_int, c_int, c_int, c_int, _p, c_int64, c_int, c_int, c_float,
                                    c_int, c_int, _p, _p]),
    "locov_roi_align_levels_fwd": (c_int, [POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_float),
                                           c_int, c_int, c_int, _p, _p, c_int64, c_int, c_int, c_int, c_int,
                                           _p, _p]),
    "locov_nchw_to_nhwc": (c_int, [_p, c_int, c_int, c_int, c_int, _p, c_int, _p]),
    "locov_roi_align_nhwc_fwd": (c_int, [_p, c_int, c_int, c_int, c_int, c_int, _p, c_int64, c_int, c_int,
                                         c_float, c_int, c_int, c_int, c_int, _p, c_int, _p]),
    "locov_roi_align_nhwc_ld_fwd": (c_int, [_p, c_int, c_int, c_int, c_int, c_int, _p, c_int64, c_int, c_int,
                                            c_float, c_int, c_int, c_int, c_int, _p, c_int64, c_int, _p]),
    "locov_roi_align_nhwc_affine_fwd": (c_int, [_p, c_int, c_int, c_int, c_int, c_int, c_int64, _p, c_int64, c_int, c_int,
                                                c_float, c_int, c_int, c_int, c_int, _p, _p, c_int, _p, c_int64, c_int, _p]),
    "locov_roi_align_from_nhwc_fwd": (c_int, [_p, c_int, c_int, c_int, c_int, _p, c_int64, c_int, c_int, c_float,
                                              c_int, c_int, _p, _p]),
    "locov_roi_align_plan_bytes": (c_int64, [c_int64]),
    "locov_roi_align_from_nhwc_fwd_ex": (c_int, [_p, c_int, c_int, c_int, c_int, _p, c_int64, c_int, c_int, c_float,
                                                 c_int, c_int, c_int, _p, c_int64, _p, _p]),
    "locov_spatial_mean_fwd": (c_int, [_p, c_int64, c_int, c_int, c_int, _p, _p]),
    "locov_gemm_nt_f32": (c_int, [_p, c_int64, _p, _p, _p, _p, _p, c_int64, c_int64, c_int, c_int, c_uint, _p]),
    "locov_conv3x3_nhwc_f32": (c_int, [_p, c_int64, c_int, c_int, c_int, c_int, _p, _p, _p, _p, _p, c_int, c_uint,
                                       _p]),
    "locov_pack_conv3x3_weight": (c_int, [_p, c_int, c_int, _p, c_int, _p]),
    "locov_winograd_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "locov_winograd_pack_weight": (c_int, [_p, c_int, c_int, _p, _p]),
    "locov_winograd_conv3x3_f32": (c_int, [_p, c_int64, c_int, _p, _p, _p, _p, c_int64, c_int, c_uint, _p, c_int64, _p]),
    "locov_winograd_conv3x3_f32_split": (c_int, [_p, c_int64, c_int, _p, c_float, c_float, _p, _p, _p, c_int64, c_int, c_uint,
                                                 _p, c_int64, _p, _p]),
    "locov_gemm_nt_batched_f32": (c_int, [_p, c_int64, c_int64, _p, c_int64, _p, c_int64, c_int64, c_int64, c_int,
                                          c_int, c_int, _p]),
    "locov_gemm_timing_enable": (c_int, [c_int]),
    "locov_gemm_timing_read": (c_int, [c_int, _p, _p, _p]),
    "locov_gemm_timing_read_ex": (c_int, [c_int, _p, _p, _p, _p]),
    "locov_frozen_bn_fold": (c_int, [_p, _p, _p, _p, c_float, c_int, _p, _p, _p]),
    "locov_label_proposals": (c_int, [_p, POINTER(c_int), _p, _p, POINTER(c_int), c_int, POINTER(c_float), POINTER(c_float),
                                      POINTER(c_int), c_int, c_int64, _p, _p, _p, _p, _p, _p, _p]),
    "locov_sample_proposals": (c_int, [_p, _p, _p, _p, _p, _p, _p, _p, POINTER(c_int), POINTER(c_int), c_int, c_int, c_int, c_int64,
                                       _p, _p, _p, _p, _p, _p, _p, _p]),
    "locov_box_reg_loss": (c_int, [_p, _p, _p, c_int64, _p, c_int64, c_int64, c_float, c_float, c_float, c_float, c_float, _p, _p, _p]),
    "locov_box_iou_loss": (c_int, [_p, _p, _p, c_int64, _p, c_int64, c_int64, c_float, c_float, c_float, c_float, c_double, c_int, _p, _p,
                                   _p]),
    "locov_cls_loss_workspace_bytes": (c_int64, [c_int64]),
    "locov_cls_loss": (c_int, [_p, c_int64, _p, c_int64, c_int, c_int64, _p, c_int64, _p, _p, _p, _p]),
    "locov_fed_loss_classes": (c_int, [_p, c_int64, _p, _p, c_int, c_int, _p, _p, _p]),
    "locov_sigmoid_cls_loss_workspace_bytes": (c_int64, [c_int64]),
    "locov_sigmoid_cls_loss": (c_int, [_p, c_int64, _p, _p, c_int64, c_int, _p, c_int64, _p, _p, _p, _p]),
    "locov_grounding_ce_fwd": (c_int, [_p, _p, _p, _p, c_int, c_int, c_int, _p, _p]),
    "locov_grounding_ce_bwd": (c_int, [_p, _p, _p, _p, c_int, c_int, c_int, _p, _p, _p, _p, _p, _p, _p]),
    "locov_grounding_ce_dist_fwd": (c_int, [_p, _p, _p, _p, c_int, c_int, c_int, _p, _p, _p, _p]),
    "locov_grounding_ce_dist_bwd": (c_int, [_p, _p, _p, _p, c_int, c_int, c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "locov_grounding_triplet_fwd": (c_int, [_p, _p, _p, _p, c_int, c_int, c_int, c_int, c_float, _p, _p, _p, _p, _p]),
    "locov_grounding_triplet_bwd": (c_int, [_p, _p, _p, _p, c_int, c_int, c_int, c_int, c_float, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                            _p]),
    "locov_distill_loss_fwd": (c_int, [_p, _p, _p, c_int, c_int, c_int, c_float, c_float, _p, _p]),
    "locov_distill_loss_bwd": (c_int, [_p, _p, _p, c_int, c_int, c_int, c_float, c_float, _p, _p, _p, _p, _p]),
    "locov_nms_workspace_bytes": (c_int64, [c_int64]),
    "locov_nms_sorted": (c_int, [_p, c_int64, c_float, _p, _p, _p, _p]),
    "locov_detect_postprocess_workspace_bytes": (c_int64, [c_int64, c_int]),
    "locov_detect_postprocess": (c_int, [_p, c_int64, c_int, _p, _p, POINTER(c_int), POINTER(c_float), c_int, c_float, c_float, c_float,
                                         c_float, c_float, c_float, c_float, c_int, _p, c_int64, _p, _p, _p, _p, _p, _p]),
    "locov_detect_postprocess_wide_workspace_bytes": (c_int64, [POINTER(c_int), c_int, c_int, c_int]),
    "locov_detect_postprocess_wide": (c_int, [_p, c_int64, c_int, _p, _p, POINTER(c_int), POINTER(c_float), c_int, c_float, c_float, c_float,
                                              c_float, c_float, c_float, c_float, c_int, c_int, _p, c_int64, _p, _p, _p, _p, _p, _p]),
    "locov_detect_postprocess_cs_workspace_bytes": (c_int64, [c_int64, c_int, c_int, c_int64, c_int]),
    "locov_detect_postprocess_cs": (c_int, [_p, c_int64, c_int, _p, c_int64, c_int, _p, POINTER(c_int), POINTER(c_float), c_int, c_float, c_float,
                                            c_float, c_float, c_float, c_float, c_float, c_int, _p, c_int64, _p, _p, _p, _p, _p, _p]),
    "locov_detect_postprocess_wide_cs_workspace_bytes": (c_int64, [POINTER(c_int), c_int, c_int, c_int, c_int64, c_int]),
    "locov_detect_postprocess_wide_cs": (c_int, [_p, c_int64, c_int, _p, c_int64, c_int, _p, POINTER(c_int), POINTER(c_float), c_int, c_float,
                                                 c_float, c_float, c_float, c_float, c_float, c_float, c_int, c_int, _p, c_int64, _p, _p, _p,
                                                 _p, _p, _p]),
    "locov_rpn_proposals_workspace_bytes": (c_int64, [c_int, c_int64, c_int]),
    "locov_rpn_proposals": (c_int, [_p, _p, _p, c_int64, POINTER(c_float), c_int, c_float, c_float, c_float, c_float, c_float, c_int, c_int,
                                    c_float, c_float, _p, c_int64, _p, _p, _p, _p, _p]),
    "locov_rpn_label_anchors_workspace_bytes": (c_int64, [c_int, c_int64, c_int64]),
    "locov_rpn_label_anchors": (c_int, [_p, c_int64, _p, POINTER(c_int), POINTER(c_float), c_int, POINTER(c_float), POINTER(c_float),
                                        POINTER(c_int), c_int, c_int, c_float, _p, c_int64, _p, _p, _p, _p]),
    "locov_rpn_sample_anchors": (c_int, [_p, _p, c_int64, c_int, c_int, c_int, _p, _p, _p]),
    "locov_rpn_loss_workspace_bytes": (c_int64, [c_int, c_int64]),
    "locov_rpn_loss": (c_int, [_p, _p, _p, _p, _p, c_int64, c_int, c_float, c_float, c_float, c_float, c_float, c_float, c_float, _p,
                               c_int64, _p, _p, _p, _p, _p]),
    "locov_grounding_fwd": (c_int, [_p, c_int, c_int, c_int, _p, _p, c_float, _p, _p, _p]),
    "locov_grounding_bwd": (c_int, [_p, c_int, c_int, c_int, _p, _p, c_float, _p, _p, _p, _p]),
    "locov_grounding_align_fwd": (c_int, [_p, c_int, c_int, c_int, _p, _p, c_float, c_int, _p, _p, _p]),
    "locov_grounding_align_bwd": (c_int, [_p, c_int, c_int, c_int, _p, _p, c_float, c_int, _p, _p, _p, _p]),
    "locov_token_attention_fwd": (c_int, [_p, c_int64, c_int, _p, _p, c_int, c_int, c_float, c_int, c_int, _p, _p, _p, _p]),
    "locov_token_attention_bwd": (c_int, [_p, c_int64, c_int, _p, _p, c_int, c_int, c_float, c_int, c_int, _p, _p, _p, _p, _p]),
    "locov_rownorm_fwd": (c_int, [_p, c_int64, c_int, c_int, c_float, _p, _p]),
    "locov_rownorm_bwd": (c_int, [_p, _p, c_int64, c_int, c_int, c_float, _p, _p]),
    "locov_pool_fc_bwd_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "locov_pool_fc_bwd": (c_int, [_p, c_int64, c_int, _p, c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p, c_int64, _p]),
    "locov_sim_gemm_bwd_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "locov_sim_gemm_bwd": (c_int, [_p, _p, _p, c_int64, c_int, c_int, _p, _p, _p, c_int64, _p]),
    "locov_f32_to_bf16": (c_int, [_p, c_int64, _p, _p]),
    "locov_gemm_nt_bf16": (c_int, [_p, c_int64, _p, _p, _p, _p, _p, c_int64, c_int64, c_int, c_int, c_uint, _p]),
    "locov_conv3x3_nhwc_bf16": (c_int, [_p, c_int64, c_int, c_int, c_int, c_int, _p, _p, _p, _p, _p, c_int, c_uint, _p]),
    "locov_split_f16x2_pack": (c_int, [_p, c_int64, c_int, c_int64, c_float, _p, _p, _p]),
    "locov_gemm_nt_f32_split": (c_int, [_p, c_int64, _p, _p, _p, _p, _p, c_int64, c_int64, c_int, c_int, c_uint, c_float,
                                        c_float, _p, _p]),
    "locov_gemm_segmean_supported": (c_int, [c_int64, c_int64, c_int, c_int, c_int, c_uint]),
    "locov_gemm_segmean_workspace_bytes": (c_int64, [c_int64, c_int]),
    "locov_gemm_nt_f32_split_segmean": (c_int, [_p, c_int64, _p, _p, _p, _p, _p, c_int64, c_int, c_int, c_int, c_uint, c_float,
                                                c_float, _p, c_int64, _p, _p]),
    "locov_gemm_nt_batched_f32_split": (c_int, [_p, c_int64, c_int64, _p, c_int64, _p, c_int64, c_int64, c_int64, c_int,
                                                c_int, c_int, c_float, c_float, _p, _p]),
    "locov_sim_gemm_bf16": (c_int, [_p, _p, c_int64, c_int, c_int, _p, c_int64, _p]),
    "locov_gemm_nt_f32_ex": (c_int, [_p, c_int64, _p, c_int64, _p, _p, _p, _p, _p, c_int64, c_int64, c_int, c_int, c_uint, _p]),
    "locov_conv3x3_nhwc_f32_ex": (c_int, [_p, c_int64, c_int, c_int, c_int, c_int, _p, _p, _p, _p, _p, _p, c_int, c_uint, _p]),
    "locov_winograd_conv3x3_f32_ex": (c_int, [_p, c_int64, c_int, _p, _p, _p, _p, _p, c_int64, c_int, c_uint, _p, c_int64, _p]),
    "locov_gemm_tn_workspace_bytes": (c_int64, [c_int64, c_int, c_int, c_int]),
    "locov_gemm_tn_f32": (c_int, [_p, c_int64, c_int64, _p, c_int64, c_int64, _p, c_int64, c_int64, c_int64, c_int, c_int, c_int,
                                  _p, _p, c_int64, _p]),
    "locov_split_scale_from_amax": (c_int, [_p, c_int64, c_float, _p, _p]),
    "locov_amax_bound": (c_int, [POINTER(c_void_p), POINTER(c_int64), POINTER(c_float), c_int, _p, _p]),
    "locov_split_scale_from_amax_zeroed": (c_int, [_p, c_int64, c_float, _p, _p]),
    "locov_gemm_nt_f32_split_ex": (c_int, [_p, c_int64, _p, _p, _p, _p, _p, _p, c_int64, c_int64, c_int, c_int, c_uint, c_float, _p,
                                           c_float, _p, _p, _p]),
    "locov_gemm_tn_f32_split": (c_int, [_p, c_int64, c_int64, _p, c_int64, c_int64, _p, c_int64, c_int64, c_int64, c_int, c_int, c_int,
                                        _p, _p, c_float, _p, _p, c_int64, _p]),
    "locov_gemm_tn_f32_split_b": (c_int, [_p, c_int64, c_int64, _p, c_int64, c_int64, _p, c_int64, c_int64, c_int64, c_int, c_int, c_int,
                                        _p, _p, c_float, _p, _p, c_int64, _p]),
    "locov_winograd_conv3x3_f32_split_ex": (c_int, [_p, c_int64, c_int, _p, c_float, c_float, c_int, _p, _p, _p, _p, c_int64, c_int,
                                                    c_uint, c_float, _p, c_int64, _p, _p, _p]),
    "locov_winograd_wgrad_f32_split": (c_int, [_p, _p, c_int64, c_int, c_int, c_uint, _p, _p, _p, _p, c_int64, _p]),
    "locov_winograd_wgrad_f32_split_v": (c_int, [_p, _p, c_int64, c_int, c_int, c_uint, _p, _p, _p, _p, c_int64, _p]),
    "locov_conv1x1_winograd_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "locov_conv1x1_winograd_workspace_bytes_for": (c_int64, [c_int64, c_int, c_int, c_int, c_int64]),
    "locov_roi_align_winograd_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "locov_roi_align_winograd_conv3x3_f32_split": (c_int, [_p, c_int, c_int, c_int, c_int, c_int64, _p, c_int64, c_int, c_float, c_int, c_int,
                                                           _p, _p, _p, c_float, c_float, _p, _p, _p, c_int64, c_int, c_uint, c_float, _p, c_int64,
                                                           _p, _p]),
    "locov_conv1x1_winograd_conv3x3_f32_split": (c_int, [_p, c_int64, c_int, c_float, _p, c_float, _p, _p, c_int64, c_int, _p, c_float, c_float,
                                                         _p, _p, _p, c_int64, c_int, c_uint, c_float, _p, c_int64, _p, _p]),
    "locov_winograd_wgrad_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "locov_winograd_wgrad_f32": (c_int, [_p, _p, c_int64, c_int, c_int, c_uint, _p, _p, _p, c_int64, _p]),
    "locov_res5_weight_prep": (c_int, [POINTER(WeightPrepJob), c_int, _p, _p]),
    "locov_weight_transpose_scale": (c_int, [_p, c_int, c_int, _p, _p, _p]),
    "locov_conv3x3_weight_flip": (c_int, [_p, c_int, c_int, _p, _p, _p]),
    "locov_im2col3x3_nhwc": (c_int, [_p, c_int64, c_int, c_int, c_int, _p, _p]),
    "locov_conv3x3_wgrad_unpack": (c_int, [_p, c_int, c_int, _p, _p, _p]),
    "locov_relu_mask": (c_int, [_p, _p, c_int64, _p, _p, _p]),
    "locov_zero_if_raised": (c_int, [POINTER(c_void_p), POINTER(c_int64), c_int, _p, _p]),
    "locov_spatial_mean_bwd": (c_int, [_p, _p, c_int64, c_int, c_int, _p, _p, _p]),
    "locov_rows_stride2": (c_int, [_p, c_int, c_int, c_int, c_int, c_int, _p, _p]),
    "locov_roi_align_nhwc_bwd": (c_int, [_p, c_int64, c_int, c_int, c_int, c_int, _p, c_int64, c_int, c_int, c_float, c_int, c_int,
                                         c_int, c_int, _p, _p]),
    "locov_box_head_fwd": (c_int, [_p, c_int64, c_int, c_int, c_int, _p, _p, _p, _p, _p, _p, c_int, c_int,
                                   c_int, c_int, _p, _p, _p, _p, _p, _p]),
    "locov_regions_select": (c_int, [_p, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, POINTER(c_void_p), c_int, c_int,
                                     c_int, c_int, _p, _p, _p, _p, _p, _p, _p]),
    "locov_regions_gather_fwd": (c_int, [_p, c_int, c_int64, c_int, c_int, c_int, c_int64, _p, _p, _p]),
    "locov_regions_gather_bwd": (c_int, [_p, c_int, c_int64, c_int64, c_int, c_int64, _p, _p, _p]),
    "locov_mha_fwd": (c_int, [_p, c_int64, _p, c_int64, _p, c_int64, _p, _p, c_float, c_float, c_int, c_int, c_int, c_int, _p, c_int64,
                              _p, _p]),
    "locov_mha_bwd": (c_int, [_p, c_int64, _p, c_int64, _p, c_int64, _p, _p, c_float, c_float, c_int, c_int, c_int, c_int, _p,
                              c_int64, _p, _p, _p, c_int64, _p, c_int64, _p, c_int64, _p]),
    "locov_resnet_stem_fwd": (c_int, [_p, c_int, c_int, c_int, _p, _p, _p, c_int, _p, _p]),
    "locov_resnet_stem_fwd_sel": (c_int, [_p, c_int, c_int, c_int, _p, _p, _p, c_int, _p, _p, _p]),
    "locov_resnet_stem_wgrad_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "locov_resnet_stem_wgrad": (c_int, [_p, c_int, c_int, c_int, _p, _p, _p, c_int, _p, _p, c_int64, _p]),
    "locov_preprocess_images": (c_int, [POINTER(c_void_p), POINTER(c_int), POINTER(c_int), c_int, c_int, c_int, POINTER(c_float),
                                        POINTER(c_float), c_float, _p, c_int, c_int, _p]),
    "locov_detector_rescale": (c_int, [_p, POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_int), c_int,
                                       _p, _p, _p, _p]),
    "locov_caption_embed_fwd": (c_int, [_p, _p, c_int, c_int, c_int, c_int, _p, _p, c_int, _p, c_int, _p, _p, c_float, _p, c_float, c_double,
                                        c_double, c_double, c_int, c_int, c_int, _p, _p, _p, _p, _p, _p]),
    "locov_caption_embed_bwd_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "locov_caption_embed_bwd": (c_int, [_p, c_int, c_int, c_int, c_int, _p, _p, _p, _p, _p, _p, _p, c_float, _p, _p, _p, _p, c_int64, _p]),
    "locov_sgd_workspace_bytes": (c_int64, [c_int, c_int64]),
    "locov_sgd_step": (c_int, [_p, c_int, c_int64, POINTER(c_float), POINTER(c_float), c_int, c_float, c_double, c_int, c_int, c_float,
                               _p, c_int64, _p]),
    "locov_coco_match_workspace_bytes": (c_int64, [c_int, c_int]),
    "locov_coco_match": (c_int, [_p, _p, c_int64, c_int, c_int, c_int, _p, _p, _p, _p, POINTER(c_double), c_int, POINTER(c_double), c_int,
                                 _p, _p, _p, c_int64, _p]),
    "locov_coco_accumulate": (c_int, [_p, c_int, _p, _p, _p, c_int, _p, _p, c_int, c_int, POINTER(c_int), c_int, POINTER(c_double), c_int,
                                      _p, _p, _p, _p]),
    "locov_lvis_match": (c_int, [_p, _p, _p, c_int64, c_int, c_int, c_int, _p, _p, _p, _p, POINTER(c_double), c_int, POINTER(c_double), c_int,
                                 _p, _p, _p, c_int64, _p]),
    "locov_resize_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "locov_resize_flip_images": (c_int, [POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_void_p), POINTER(c_int),
                                         POINTER(c_int), POINTER(c_int), c_int, c_int, _p]),
    "locov_map_proposals": (c_int, [_p, c_int64, c_int, POINTER(c_int64), POINTER(c_int), POINTER(c_double), POINTER(c_double),
                                    POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, c_int, c_float, _p, _p, _p, _p, _p, _p, _p,
                                    _p, _p]),
    "locov_proposal_recall": (c_int, [_p, _p, c_int, c_int, c_int, c_int, _p, _p, _p, _p, POINTER(c_float), c_int, POINTER(c_int), c_int,
                                      POINTER(c_float), c_int, _p, _p, _p]),
    "locov_augment_supported": (c_int, [c_float]),
    "locov_augment_images_workspace_bytes": (c_int64, [POINTER(AugmentDesc), c_int]),
    "locov_augment_images": (c_int, [POINTER(c_void_p), POINTER(c_void_p), POINTER(AugmentDesc), c_int, _p, c_int64, _p, c_int64, _p]),
}

# include/locov_jpeg.h: the JPEG decoder's entry points, in the same library, bound next to SIGNATURES by load()
JPEG_RGB, JPEG_BGR, JPEG_L, JPEG_MAX_DEQUANTISED = 0, 1, 2, 1096


class JpegHeader(ctypes.Structure):
    """locov_jpeg_header of include/locov_jpeg.h"""
    _fields_ = [("supported", ctypes.c_int32), ("reason", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("ncomp", ctypes.c_int32), ("comp_id", ctypes.c_int32 * 3), ("comp_h", ctypes.c_int32 * 3), ("comp_v", ctypes.c_int32 * 3),
                ("comp_tq", ctypes.c_int32 * 3), ("comp_td", ctypes.c_int32 * 3), ("comp_ta", ctypes.c_int32 * 3),
                ("restart_interval", ctypes.c_int32), ("scan_start", c_int64), ("qt_present", ctypes.c_uint8 * 4),
                ("qt", (ctypes.c_uint16 * 64) * 4), ("dc_present", ctypes.c_uint8 * 4), ("ac_present", ctypes.c_uint8 * 4),
                ("dc_counts", (ctypes.c_uint8 * 16) * 4), ("ac_counts", (ctypes.c_uint8 * 16) * 4),
                ("dc_symbols", (ctypes.c_uint8 * 256) * 4), ("ac_symbols", (ctypes.c_uint8 * 256) * 4)]


class JpegDesc(ctypes.Structure):
    """locov_jpeg_desc of include/locov_jpeg.h"""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("hs", ctypes.c_int32), ("vs", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("record_offset", c_int64), ("record_bytes", c_int64), ("qt_offset", c_int64)]


# name -> (restype, argtypes); mirrors include/locov_jpeg.h declaration by declaration
JPEG_SIGNATURES = {
    "locov_jpeg_parse": (c_int, [c_void_p, c_int64, POINTER(JpegHeader)]),
    "locov_jpeg_entropy_bytes": (c_int64, [POINTER(JpegHeader), c_int64]),
    "locov_jpeg_entropy_decode": (c_int, [POINTER(c_void_p), POINTER(c_int64), POINTER(JpegHeader), POINTER(c_void_p), POINTER(c_int64), c_int,
                                          POINTER(ctypes.c_int32), POINTER(c_int64)]),
    "locov_jpeg_entropy_pack": (c_int, [POINTER(JpegHeader), POINTER(c_void_p), POINTER(c_int64), POINTER(c_void_p), c_int]),
    "locov_jpeg_decode_workspace_bytes": (c_int64, [POINTER(JpegDesc), c_int]),
    "locov_jpeg_decode": (c_int, [_p, c_int64, POINTER(JpegDesc), c_int, c_int, POINTER(c_void_p), _p, c_int64, _p]),
}

_lib = None


class LocovError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load liblocov_hip.so and bind every symbol of the header; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LocovError(
            f"{LIB_PATH} not found: build it with `python -m locov_amd.build` "
            "(or __graft_entry__.build()).  The LSM ROI-head path has no fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in list(SIGNATURES.items()) + list(JPEG_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise LocovError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.locov_abi_version() != ABI_VERSION:
        raise LocovError(f"ABI version mismatch: library {lib.locov_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        msg = load().locov_last_error()
        raise LocovError(f"{what or 'liblocov_hip'} failed (code {rc}): {msg.decode() if msg else ''}")
