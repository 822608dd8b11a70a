"""The multimedia self-supervision heads of the LSM model as one ModuleDict.

Mirrors ovr/modeling/mmss_heads/mmss_heads.py:14-41: one head per name in MODEL.MMSS_HEAD.TYPES, and with
TIE_VL_PROJECTION_WEIGHTS the `v2l_projection` of every other head IS the default head's (the same Parameter objects, :29-40).
"MLPHead" is not built here.
"""
from __future__ import annotations

from torch import nn

from .grounding_head import build_grounding_head
from .transformer_head import build_transformer_head

__all__ = ["build_mmss_heads", "MMSS_HEAD_BUILDERS"]

MMSS_HEAD_BUILDERS = {"GroundingHead": build_grounding_head, "TransformerHead": build_transformer_head}


def build_mmss_heads(cfg, *, v_dim, l_dim, loc_dim, backbone) -> nn.ModuleDict:
    heads = {}
    for head_type in cfg.MODEL.MMSS_HEAD.TYPES:
        assert head_type in MMSS_HEAD_BUILDERS, \
            "cfg.MODEL.MMSS_HEAD.TYPE: {} is not registered in Registry".format(head_type)
        heads[head_type] = MMSS_HEAD_BUILDERS[head_type](head_type, cfg, v_dim=v_dim, l_dim=l_dim, loc_dim=loc_dim, backbone=backbone)
    if cfg.MODEL.MMSS_HEAD.TIE_VL_PROJECTION_WEIGHTS:
        default = cfg.MODEL.MMSS_HEAD.DEFAULT_HEAD
        weight, bias = heads[default].v2l_projection.weight, heads[default].v2l_projection.bias
        for head_type in cfg.MODEL.MMSS_HEAD.TYPES:
            if head_type == default or not hasattr(heads[head_type], "v2l_projection"):
                continue
            assert weight.shape[0] == heads[head_type].v2l_projection.weight.shape[0]
            assert weight.shape[1] == heads[head_type].v2l_projection.weight.shape[1]
            heads[head_type].v2l_projection.weight = weight
            heads[head_type].v2l_projection.bias = bias
    return nn.ModuleDict(heads)
