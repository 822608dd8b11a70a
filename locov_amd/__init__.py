"""locov_amd -- MI355X (gfx950) implementation of LocOV's Localized-Semantic-Matching ROI head.

Only what the hot path needs: hand-written HIP kernels behind a C ABI
(csrc/, include/locov_hip.h), their ctypes binding (_lib, ops), and the host-side mirror of the
reference's Detectron2 plugin surface (poolers, res5, roi_heads).
"""
__version__ = "0.1.0"

from . import backbone, config, mmss_regions, ops, poolers, proposal_generator, res5, structures, transformer_head  # noqa: F401
from .mmss_regions import box_regions, grid_regions  # noqa: F401
from .transformer_head import TransformerHead, build_transformer_head  # noqa: F401
from .roi_heads import (EmbeddingFastRCNNOutputLayers, EmbeddingProposalsRes5ROIHeads,  # noqa: F401
                        EmbeddingRes5ROIHeads, build_box_predictor, build_roi_heads)
from .proposal_generator import RPN, DefaultAnchorGenerator, StandardRPNHead, build_proposal_generator  # noqa: F401
from .backbone import BasicStem, ResNet, build_backbone, build_resnet_backbone  # noqa: F401
from . import meta_arch  # noqa: F401,E402
from .meta_arch import (META_ARCH_REGISTRY, DistillOnlyProposalMMSSRCNN, DistillProposalMMSSRCNN, GeneralizedRCNN,  # noqa: F401
                        OvrRCNN, ProposalNetwork, build_model, detector_postprocess)
from . import language_backbone, mmss_heads  # noqa: F401,E402
from .language_backbone import (LANGUAGE_BACKBONES_REGISTRY, BertEmbedding, WordPieceTokenizer,  # noqa: F401,E402
                                build_bertemb_backbone, build_language_backbone)
from .mmss_heads import build_mmss_heads  # noqa: F401,E402
from . import engine, solver  # noqa: F401,E402
from .engine import SimpleTrainerMMSS  # noqa: F401,E402
from .solver import (FusedSGD, WarmupCosineLR, WarmupMultiStepLR, build_lr_scheduler, build_optimizer,  # noqa: F401,E402
                     get_default_optimizer_params)
from . import evaluation  # noqa: F401,E402
from .evaluation import COCOEvaluator, LVISEvaluator, build_evaluator, inference_on_dataset  # noqa: F401,E402
from . import data  # noqa: F401,E402
from .data import DatasetMapper, build_augmentation, iterate_batches, resize_bilinear_host  # noqa: F401,E402
from .strong_augment import StrongAugmentation, build_complete_augmentation  # noqa: F401,E402
