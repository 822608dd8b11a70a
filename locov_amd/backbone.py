"""The ResNet C4 backbone in front of the RPN and the ROI heads: stem, res2-res4 (res5 on request), on the gfx950 kernels.

The reference has no backbone source of its own: both shipped configs build Detectron2's ([D2-upstream] detectron2.modeling.
backbone: BasicStem, BottleneckBlock, ResNet, build_resnet_backbone, build_backbone), reached as self.backbone(images.tensor) from
OvrRCNN (ovr/modeling/meta_arch/ovr_rcnn.py) and the STT fine-tune.  This module restates that surface from public sources -- class
names, constructor arguments, config keys, attributes and state-dict keys -- so that a Detectron2 checkpoint's
backbone.{stem.conv1,res2.0.conv1,...}.{weight,norm.*} load unchanged.

forward(x) -> {"res4": [N,1024,H/16,W/16]}, contiguous NCHW as upstream, takes one of three paths:

  device path   x fp32 on a ROCm device, every norm FrozenBN, STRIDE_IN_1X1, ungrouped convolutions, a 64-channel stem, and no
                gradient wanted (grad disabled, or nothing in the module requires grad).  The stem is ONE launch
                (ops.resnet_stem: conv 7x7 / 2, FrozenBN, ReLU and the max-pool fused, channels-last out); every stage runs on
                channels-last pixel rows through Res5Stage.forward_rows (fp32 MFMA GEMMs with FrozenBN / ReLU / residual in the
                epilogue, the implicit 3x3) behind ops.rows_stride2 where it strides; ops.nhwc_to_nchw once per requested feature.
                fp32 throughout.
  device training path   opt-in (MODEL.BACKBONE.TRAIN_ON_DEVICE / ResNet.train_on_device, default off): the same input and
                structural conditions, a gradient wanted for some weight, none for x.  The frozen prefix (FREEZE_AT: the stem
                and / or leading stages without a trainable parameter) runs the inference kernels above under no_grad; a
                trainable stem is ops.resnet_stem_train / ops.resnet_stem_wgrad under autograd (the forward saves which conv
                position every pooled element came from, the backward is the weight gradient alone: images carry no
                gradient); every stage from the first trainable one on is res5_train.res5_rows (f32 MFMA GEMMs forward, masked
                NT / TN GEMMs backward, im2col for the 3x3) behind res5_train.grid_rows where it strides -- also a frozen stage
                behind a trainable one, whose input carries the graph; res5_train.to_nchw per requested feature.  fp32, no
                range guard, no host wait in forward or backward.
  torch path    everything else (CPU tensors, BN, grouped or STRIDE_IN_1X1=False blocks, x.requires_grad, and trainable weights
                with grad enabled unless the training path was asked for): the plain differentiable torch expression of the
                same modules.  Silent; it is the definition of the result.

Not here: split-f16 arithmetic for the backbone, trainable BN, a data gradient for the images, pixel normalisation and ImageList
padding (the caller's, as upstream: they happen in the meta-architecture).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import ops, res5_train
from .registry import Registry
from .res5 import BottleneckBlock, Conv2d, FrozenBatchNorm2d, Res5Stage, get_norm
from .res5_operands import conv_version
from .structures import ShapeSpec

__all__ = ["BasicStem", "ResNet", "build_resnet_backbone", "build_backbone", "BACKBONE_REGISTRY"]

BACKBONE_REGISTRY = Registry("BACKBONE")


def _freeze(module: nn.Module) -> nn.Module:
    """[D2-upstream] CNNBlockBase.freeze: no parameter trains, BatchNorm becomes FrozenBatchNorm with the same statistics."""
    for p in module.parameters():
        p.requires_grad = False
    for name, child in list(module.named_children()):
        if isinstance(child, nn.modules.batchnorm._BatchNorm):
            frozen = FrozenBatchNorm2d(child.num_features, eps=child.eps)
            with torch.no_grad():
                for k in ("weight", "bias", "running_mean", "running_var"):
                    getattr(frozen, k).copy_(getattr(child, k))
            setattr(module, name, frozen.to(child.running_mean.device))
        else:
            _freeze(child)
    return module


class _StemTrainFn(torch.autograd.Function):
    """The stem under autograd on the device: y = ops.resnet_stem_train(images, weight, scale, shift), differentiable in the
    weight alone (FrozenBN is buffers, images carry no gradient).  saved_tensors: (images, sel, scale)."""

    @staticmethod
    def forward(ctx, images, weight, scale, shift):
        y, sel = ops.resnet_stem_train(images, weight.detach(), scale, shift)
        ctx.save_for_backward(images, sel, scale)
        return y

    @staticmethod
    def backward(ctx, g):
        images, sel, scale = ctx.saved_tensors
        return None, ops.resnet_stem_wgrad(images, g, sel, scale), None, None


class BasicStem(nn.Module):
    """[D2-upstream] the standard ResNet stem: conv1 7x7 / 2 (+ norm), ReLU, max-pool 3x3 / 2."""

    def __init__(self, in_channels: int = 3, out_channels: int = 64, norm: str = "BN"):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, 4
        self.conv1 = Conv2d(in_channels, out_channels, kernel_size=7, stride=2, padding=3, bias=False, norm=get_norm(norm, out_channels))
        nn.init.kaiming_normal_(self.conv1.weight, mode="fan_out", nonlinearity="relu")      # [D2-upstream] c2_msra_fill
        self._fold = None           # (FrozenBN version, (scale, shift))

    def freeze(self):
        return _freeze(self)

    def forward(self, x):
        x = F.relu_(self.conv1(x))
        return F.max_pool2d(x, kernel_size=3, stride=2, padding=1)

    def supports_rows_path(self) -> bool:
        return self.in_channels == 3 and self.out_channels == 64 and isinstance(self.conv1.norm, FrozenBatchNorm2d)

    @torch.no_grad()
    def _folded(self):
        version = conv_version(self.conv1, weight=False)
        if self._fold is None or self._fold[0] != version:
            n = self.conv1.norm
            self._fold = (version, ops.frozen_bn_fold(n.weight, n.bias, n.running_mean, n.running_var, n.eps))
        return self._fold[1]

    @torch.no_grad()
    def forward_rows(self, x: torch.Tensor) -> torch.Tensor:
        """x [N,3,H,W] on the device -> the pooled map, channels-last [N,PH,PW,64], in one launch."""
        scale, shift = self._folded()
        return ops.resnet_stem(x, self.conv1.weight.detach(), scale, shift)

    def forward_rows_train(self, x: torch.Tensor) -> torch.Tensor:
        """forward_rows under autograd: the same values, differentiable in conv1.weight (one more launch pair in backward)."""
        scale, shift = self._folded()
        return _StemTrainFn.apply(x.detach(), self.conv1.weight, scale, shift)


class ResNet(nn.Module):
    """[D2-upstream] detectron2.modeling.backbone.ResNet: `stem`, then the stages as sub-modules res2, res3, ... (each an
    nn.Sequential of blocks -- here a Res5Stage, which also owns the stage's folded GEMM operands)."""

    def __init__(self, stem: BasicStem, stages: List[List[nn.Module]], num_classes: Optional[int] = None,
                 out_features: Optional[List[str]] = None, freeze_at: int = 0, train_on_device: bool = False):
        super().__init__()
        self.train_on_device = bool(train_on_device)      # MODEL.BACKBONE.TRAIN_ON_DEVICE: may be set afterwards
        if num_classes is not None:
            raise NotImplementedError("ResNet(num_classes=...): the classification head (avgpool + linear) is not part of the C4 backbone")
        self.stem = stem
        current_stride = stem.stride
        self._out_feature_strides = {"stem": current_stride}
        self._out_feature_channels = {"stem": stem.out_channels}
        self.stage_names, self.stages = [], []
        if out_features is not None:      # [D2-upstream] stages behind the last requested one are not built
            num_stages = max({"res2": 1, "res3": 2, "res4": 3, "res5": 4}.get(f, 0) for f in out_features)
            stages = stages[:num_stages]
        for i, blocks in enumerate(stages):
            assert len(blocks) > 0, len(blocks)
            name = "res" + str(i + 2)
            stage = blocks if isinstance(blocks, Res5Stage) else Res5Stage(*blocks)
            self.add_module(name, stage)
            self.stage_names.append(name)
            self.stages.append(stage)
            current_stride = current_stride * math.prod(blk.stride for blk in stage)
            self._out_feature_strides[name] = current_stride
            self._out_feature_channels[name] = stage[-1].out_channels
        self.stage_names = tuple(self.stage_names)
        if out_features is None:
            out_features = [self.stage_names[-1]] if self.stage_names else ["stem"]
        self._out_features = list(out_features)
        assert len(self._out_features)
        children = [n for n, _ in self.named_children()]
        for f in self._out_features:
            assert f in children, f"Available children: {', '.join(children)}"
        self.freeze(freeze_at)

    # -- [D2-upstream] Backbone ------------------------------------------------------------------------------------------------
    @property
    def size_divisibility(self) -> int:
        return 0

    @property
    def padding_constraints(self) -> Dict[str, int]:
        return {}

    def output_shape(self) -> Dict[str, ShapeSpec]:
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name])
                for name in self._out_features}

    def freeze(self, freeze_at: int = 0):
        """[D2-upstream] 1 freezes the stem, k the stem and the stages below res{k+1}."""
        if freeze_at >= 1:
            self.stem.freeze()
        for idx, stage in enumerate(self.stages, start=2):
            if freeze_at >= idx:
                for block in stage.children():
                    _freeze(block)
        return self

    # -- forward ---------------------------------------------------------------------------------------------------------------
    def device_path_ok(self, x: torch.Tensor) -> bool:
        """The hand-written path computes forward(x): device fp32 input, FrozenBN / STRIDE_IN_1X1 / ungrouped everywhere, a
        64-channel stem, 32-aligned 3x3 widths, and nobody waiting for a gradient."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] > 0):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return self._rows_structure_ok()

    def train_path_ok(self, x: torch.Tensor) -> bool:
        """The device training path computes forward(x) and its weight gradients: asked for (train_on_device), the input and
        structure of device_path_ok, a gradient wanted for some weight and none for x."""
        if not (self.train_on_device and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and x.shape[0] > 0):
            return False
        if not torch.is_grad_enabled() or x.requires_grad or not any(p.requires_grad for p in self.parameters()):
            return False
        return self._rows_structure_ok()

    def _rows_structure_ok(self) -> bool:
        return self.stem.supports_rows_path() and all(
            stage.supports_rows_path() and all(blk.stride in (1, 2) and blk.conv2.in_channels % 32 == 0 and
                                               (blk.shortcut is None or isinstance(blk.shortcut.norm, FrozenBatchNorm2d)) and
                                               (bi == 0 or blk.stride == 1) for bi, blk in enumerate(stage))
            for stage in self.stages)

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        assert x.dim() == 4, f"ResNet takes an input of shape (N, C, H, W). Got {x.shape} instead!"
        if self.device_path_ok(x):
            return self._forward_device(x)
        return self._forward_device_train(x) if self.train_path_ok(x) else self._forward_torch(x)

    def _forward_torch(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        outputs = {}
        x = self.stem(x)
        if "stem" in self._out_features:
            outputs["stem"] = x
        for name, stage in zip(self.stage_names, self.stages):
            x = nn.Sequential.forward(stage, x)
            if name in self._out_features:
                outputs[name] = x
        return outputs

    @torch.no_grad()
    def _forward_device(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        outputs = {}
        N = x.shape[0]
        nhwc = self.stem.forward_rows(x)
        H, W, C = nhwc.shape[1:]
        if "stem" in self._out_features:
            outputs["stem"] = ops.nhwc_to_nchw(nhwc)
        rows = nhwc.view(N * H * W, C)
        for name, stage in zip(self.stage_names, self.stages):
            if stage[0].stride == 2:       # STRIDE_IN_1X1: block 0's 1x1 convolutions see the even pixels only
                rows = ops.rows_stride2(rows.view(N, H, W, C), N, H, W, True)
                H, W = (H + 1) // 2, (W + 1) // 2
            rows = stage.forward_rows(rows, H, W, pos_major=False, winograd=False, split=False)
            C = rows.shape[1]
            if name in self._out_features:
                outputs[name] = ops.nhwc_to_nchw(rows.view(N, H, W, C))
        return outputs

    def _forward_device_train(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        outputs = {}
        N = x.shape[0]
        graph = any(p.requires_grad for p in self.stem.parameters())       # does `rows` carry a graph yet?
        nhwc = self.stem.forward_rows_train(x) if graph else self.stem.forward_rows(x)
        H, W, C = nhwc.shape[1:]
        if "stem" in self._out_features:
            outputs["stem"] = res5_train.to_nchw(nhwc.view(N * H * W, C), N, H, W) if graph else ops.nhwc_to_nchw(nhwc)
        rows = nhwc.view(N * H * W, C)
        for name, stage in zip(self.stage_names, self.stages):
            if not graph and not any(p.requires_grad for p in stage.parameters()):      # the frozen prefix: the inference kernels
                with torch.no_grad():
                    if stage[0].stride == 2:
                        rows = ops.rows_stride2(rows.view(N, H, W, C), N, H, W, True)
                        H, W = (H + 1) // 2, (W + 1) // 2
                    rows = stage.forward_rows(rows, H, W, pos_major=False, winograd=False, split=False)
            else:
                if stage[0].stride == 2:
                    rows = res5_train.grid_rows(rows.view(N, H, W, C))
                    H, W = (H + 1) // 2, (W + 1) // 2
                rows = res5_train.res5_rows(stage, rows, N, H, W, pooled=False, split=False, overflow_check=False)
                graph = True
            C = rows.shape[1]
            if name in self._out_features:
                outputs[name] = res5_train.to_nchw(rows, N, H, W) if graph else ops.nhwc_to_nchw(rows.view(N, H, W, C))
        return outputs

    def saved_training_state(self, out: torch.Tensor) -> Dict[str, object]:
        """What the device training path kept for the backward of `out` (one of its outputs): {"stem": the stem's sel (uint8
        [N,PH,PW,64]; absent when the stem is frozen), "res2": [(x, y1, y2, out) per block], ...} -- the post-ReLU activations
        over the stage's pixel rows, i.e. the device's own active sets (stages of the frozen prefix keep nothing).  To be read
        before out's backward, which frees what the nodes saved."""
        state: Dict[str, object] = {}
        stack, seen = [out.grad_fn], set()                  # (seen holds the nodes themselves: the id of a released wrapper is reused)
        while stack:
            n = stack.pop()
            if n is None or n in seen:
                continue
            seen.add(n)
            if "_StemTrainFn" in type(n).__name__:
                state["stem"] = n.saved_tensors[1]
            stack += [f for f, _ in n.next_functions]
        for step, saved in res5_train.saved_activations_per_step(out):
            for name, stage in zip(self.stage_names, self.stages):
                if step.stage is stage:
                    state[name] = [tuple(saved[4 * b:4 * b + 4]) for b in range(len(saved) // 4)]
        return state


@BACKBONE_REGISTRY.register()
def build_resnet_backbone(cfg, input_shape: ShapeSpec) -> ResNet:
    """[D2-upstream] the ResNet named by MODEL.RESNETS.* (bottleneck depths: 50, 101, 152)."""
    R = cfg.MODEL.RESNETS
    norm = R.NORM
    stem = BasicStem(in_channels=input_shape.channels, out_channels=R.STEM_OUT_CHANNELS, norm=norm)
    freeze_at = cfg.MODEL.BACKBONE.FREEZE_AT
    out_features = list(R.OUT_FEATURES)
    depth = R.DEPTH
    if depth in (18, 34):
        raise NotImplementedError(f"MODEL.RESNETS.DEPTH = {depth}: the BasicBlock depths (18, 34) are not implemented, only the "
                                  "bottleneck depths 50, 101 and 152")
    if depth not in (50, 101, 152):
        raise KeyError(f"MODEL.RESNETS.DEPTH = {depth} is not a ResNet depth")
    if R.RES5_DILATION != 1:
        raise NotImplementedError(f"MODEL.RESNETS.RES5_DILATION = {R.RES5_DILATION}: a dilated res5 is not implemented")
    if any(R.DEFORM_ON_PER_STAGE):
        raise NotImplementedError(f"MODEL.RESNETS.DEFORM_ON_PER_STAGE = {list(R.DEFORM_ON_PER_STAGE)}: deformable stages are not implemented")
    num_blocks_per_stage = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3], 152: [3, 8, 36, 3]}[depth]
    num_groups, width_per_group = R.NUM_GROUPS, R.WIDTH_PER_GROUP
    bottleneck_channels = num_groups * width_per_group
    in_channels, out_channels = R.STEM_OUT_CHANNELS, R.RES2_OUT_CHANNELS
    out_stage_idx = [{"res2": 2, "res3": 3, "res4": 4, "res5": 5}[f] for f in out_features if f != "stem"]
    max_stage_idx = max(out_stage_idx) if out_stage_idx else 1
    stages = []
    for idx, stage_idx in enumerate(range(2, max_stage_idx + 1)):
        first_stride = 1 if idx == 0 else 2
        blocks = []
        for b in range(num_blocks_per_stage[idx]):
            blocks.append(BottleneckBlock(in_channels, out_channels, bottleneck_channels=bottleneck_channels,
                                          stride=first_stride if b == 0 else 1, num_groups=num_groups, norm=norm,
                                          stride_in_1x1=R.STRIDE_IN_1X1))
            in_channels = out_channels
        out_channels *= 2
        bottleneck_channels *= 2
        stages.append(blocks)
    return ResNet(stem, stages, out_features=out_features, freeze_at=freeze_at,
                  train_on_device=bool(cfg.MODEL.BACKBONE.get("TRAIN_ON_DEVICE", False)))


def build_backbone(cfg, input_shape: Optional[ShapeSpec] = None) -> ResNet:
    """[D2-upstream] the backbone named by MODEL.BACKBONE.NAME, for an input of len(MODEL.PIXEL_MEAN) channels."""
    if input_shape is None:
        input_shape = ShapeSpec(channels=len(getattr(cfg.MODEL, "PIXEL_MEAN", (0.0, 0.0, 0.0))))
    backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, input_shape)
    assert isinstance(backbone, ResNet)
    return backbone
