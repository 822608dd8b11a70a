"""The region proposal network in front of the ROI heads: anchors, the RPN head and the proposal generation, on the gfx950 kernels.

The reference has no RPN source of its own: both shipped configs run Detectron2's ([D2-upstream] detectron2.modeling.
proposal_generator: DefaultAnchorGenerator, StandardRPNHead, RPN, find_top_rpn_proposals; detectron2.modeling.anchor_generator),
reached from OvrRCNN.inference (ovr/modeling/meta_arch/ovr_rcnn.py:76-124) and from the STT fine-tune
(ovr/modeling/meta_arch/distill_prop_mmss_gcnn.py:243-246,508-509).  This module restates that surface from public sources -- class
names, constructor arguments, config keys and state-dict keys -- so that a Detectron2 checkpoint's
proposal_generator.rpn_head.{conv,objectness_logits,anchor_deltas}.{weight,bias} load unchanged.

Proposal generation of a single feature level (what the reference uses: RPN.IN_FEATURES ["res4"]) is ONE device operation,
ops.rpn_proposals (csrc/rpn.hip).  In predict_proposals several levels, CPU tensors, LOCOV_FUSED_RPN=0 and non-finite predictions
take the torch chain of this file, which computes the same proposals.  The head itself (and so RPN.forward) needs device tensors:
it has no torch fallback.

Training ([D2-upstream] RPN.label_and_sample_anchors, RPN.losses): RPN.forward with targets labels the anchors (Matcher with
low-quality matches, the boundary test), draws the 256-anchor sample and forms loss_rpn_cls / loss_rpn_loc.  One feature level on
device tensors is three device operations (ops.rpn_label_anchors, ops.rpn_sample_anchors, ops.rpn_loss: csrc/rpn_train.hip) that
read nothing back; several levels, CPU tensors, LOCOV_FUSED_RPN=0 and sizes beyond the kernels' limits take the torch chain of this
file, which returns the same labels and matched boxes for the same `rnd` (the uniforms of the draw, [2, N, HWA] float64: the
num_pos positives of smallest rnd[0], then the negatives of smallest rnd[1], equal keys in anchor order).  With grad enabled the
head builds a graph over the same kernels (the 3x3 layer: _Conv3x3ReluFn; the 1x1 pair: ops.linear_autograd).
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import ops
from .registry import Registry, configurable
from .res5_train import _wino_ok
from .roi_heads.box_emb_head import Box2BoxTransform, batched_nms
from .roi_heads.labelling import Matcher, get_event_storage
from .structures import Boxes, Instances, ShapeSpec, pairwise_iou

__all__ = ["DefaultAnchorGenerator", "StandardRPNHead", "RPN", "build_proposal_generator", "build_anchor_generator", "build_rpn_head",
           "find_top_rpn_proposals", "PROPOSAL_GENERATOR_REGISTRY", "ANCHOR_GENERATOR_REGISTRY", "RPN_HEAD_REGISTRY"]

PROPOSAL_GENERATOR_REGISTRY = Registry("PROPOSAL_GENERATOR")
ANCHOR_GENERATOR_REGISTRY = Registry("ANCHOR_GENERATOR")
RPN_HEAD_REGISTRY = Registry("RPN_HEAD")


def _fused_rpn() -> bool:               # (developer A/B / tests: 0 = the torch chain)
    return os.environ.get("LOCOV_FUSED_RPN", "1") != "0"


def _broadcast_params(params, num_features: int, name: str):
    assert isinstance(params, (list, tuple)), f"{name} in anchor generator has to be a list! Got {params}."
    assert len(params), f"{name} in anchor generator cannot be empty!"
    if not isinstance(params[0], (list, tuple)):
        return [list(params)] * num_features
    if len(params) == 1:
        return [list(params[0])] * num_features
    assert len(params) == num_features, f"Got {name} of length {len(params)} in anchor generator, but the number of input features is {num_features}!"
    return [list(p) for p in params]


@ANCHOR_GENERATOR_REGISTRY.register()
class DefaultAnchorGenerator(nn.Module):
    """[D2-upstream] the anchors of every feature map: per cell len(sizes) x len(aspect_ratios) boxes (sizes the outer loop),
    shifted over the grid; ordered (y, x, a), the flattening of an NHWC head output."""

    box_dim = 4

    @configurable
    def __init__(self, sizes, aspect_ratios, strides, offset: float = 0.0):
        super().__init__()
        self.strides = [int(s) for s in strides]
        self.num_features = len(self.strides)
        sizes = _broadcast_params(sizes, self.num_features, "sizes")
        aspect_ratios = _broadcast_params(aspect_ratios, self.num_features, "aspect_ratios")
        self._num_cell = [len(s) * len(a) for s, a in zip(sizes, aspect_ratios)]
        for i, (s, a) in enumerate(zip(sizes, aspect_ratios)):           # non-persistent: not part of the state dict
            self.register_buffer(f"cell_anchors_{i}", self.generate_cell_anchors(s, a), persistent=False)
        self.offset = float(offset)
        assert 0.0 <= self.offset < 1.0, self.offset
        self._cache: Dict[Tuple, torch.Tensor] = {}

    @classmethod
    def from_config(cls, cfg, input_shape: List[ShapeSpec]):
        return {"sizes": cfg.MODEL.ANCHOR_GENERATOR.SIZES, "aspect_ratios": cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS,
                "strides": [x.stride for x in input_shape], "offset": cfg.MODEL.ANCHOR_GENERATOR.OFFSET}

    @property
    def cell_anchors(self) -> List[torch.Tensor]:
        return [getattr(self, f"cell_anchors_{i}") for i in range(self.num_features)]

    @property
    def num_cell_anchors(self) -> List[int]:
        return list(self._num_cell)

    num_anchors = num_cell_anchors

    @staticmethod
    def generate_cell_anchors(sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1, 2)) -> torch.Tensor:
        anchors = []
        for size in sizes:
            area = size ** 2.0
            for aspect_ratio in aspect_ratios:
                w = math.sqrt(area / aspect_ratio)
                h = aspect_ratio * w
                anchors.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
        return torch.tensor(anchors, dtype=torch.float32)

    def _grid_anchors(self, level: int, size: Tuple[int, int]) -> torch.Tensor:
        base = self.cell_anchors[level]
        key = (level, int(size[0]), int(size[1]), base.device)
        got = self._cache.get(key)
        if got is None:
            stride = self.strides[level]
            sx = torch.arange(self.offset * stride, size[1] * stride, step=stride, dtype=torch.float32, device=base.device)
            sy = torch.arange(self.offset * stride, size[0] * stride, step=stride, dtype=torch.float32, device=base.device)
            yy, xx = torch.meshgrid(sy, sx, indexing="ij")
            shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), dim=1)
            got = self._cache[key] = (shifts.view(-1, 1, 4) + base.view(1, -1, 4)).reshape(-1, 4).contiguous()
        return got

    def forward(self, features: Sequence[torch.Tensor]) -> List[Boxes]:
        """features: the NCHW maps, one per level -> per level the Boxes [H W A, 4] of its anchors."""
        return [Boxes(self._grid_anchors(i, f.shape[-2:])) for i, f in enumerate(features)]


class _Conv3x3ReluFn(torch.autograd.Function):
    """relu(conv3x3(rows) + bias) over N channels-last H x W maps, differentiable in rows, weight and bias.  Forward: the implicit-GEMM
    kernel on the packed weight (what the no_grad path runs: the same bits).  Backward, from kernels the Res5 stage already uses:
    the ReLU mask on the incoming gradient; the data gradient as the same convolution with the flipped filter; the weight gradient in
    the Winograd domain on 7 x 7 maps, else g^T . im2col(rows) on the TN GEMM; the bias gradient a column sum."""

    @staticmethod
    def forward(ctx, rows, weight, bias, w_packed, shift, H, W):
        y = ops.conv3x3_nhwc_ex(rows, w_packed, H, W, shift=shift, relu=True)
        ctx.save_for_backward(rows, weight, y)
        ctx.hw = (H, W)
        return y

    @staticmethod
    def backward(ctx, g):
        rows, weight, y = ctx.saved_tensors
        H, W = ctx.hw
        cout, cin = weight.shape[:2]
        g = ops.relu_mask(g.contiguous(), y)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            flipped = ops.conv3x3_weight_flip(weight.detach().float().contiguous())
            gx = ops.conv3x3_nhwc_ex(g, ops.pack_conv3x3_weight(flipped), H, W)
        if ctx.needs_input_grad[1]:
            if _wino_ok(H, W, cin, cout):
                gw = ops.winograd_wgrad(rows, g, roi_major=True)
            else:
                gw = ops.conv3x3_wgrad_unpack(ops.gemm_tn(g, ops.im2col3x3(rows, H, W)))
        if ctx.needs_input_grad[2]:
            gb = g.sum(dim=0)
        return gx, gw, gb, None, None, None, None


@RPN_HEAD_REGISTRY.register()
class StandardRPNHead(nn.Module):
    """[D2-upstream] 3x3 conv + ReLU, then two 1x1 layers: an objectness logit and box_dim deltas per anchor.  The 3x3 runs on the
    implicit-GEMM f32 kernel with its bias / ReLU epilogue; the two 1x1 layers are ONE NT GEMM against their concatenated
    [A + A box_dim, C] weight, whose channels-last rows are already the (y, x, a) order the proposal generation reads."""

    @configurable
    def __init__(self, in_channels: int, num_anchors: int, box_dim: int = 4, conv_dims: Sequence[int] = (-1,)):
        super().__init__()
        if len(conv_dims) != 1:
            raise NotImplementedError("StandardRPNHead: one 3x3 layer (MODEL.RPN.CONV_DIMS of length 1)")
        out = in_channels if conv_dims[0] == -1 else int(conv_dims[0])
        self.conv = nn.Conv2d(in_channels, out, kernel_size=3, stride=1, padding=1)
        self.objectness_logits = nn.Conv2d(out, num_anchors, kernel_size=1, stride=1)
        self.anchor_deltas = nn.Conv2d(out, num_anchors * box_dim, kernel_size=1, stride=1)
        self.num_anchors, self.box_dim = int(num_anchors), int(box_dim)
        for layer in (self.conv, self.objectness_logits, self.anchor_deltas):
            nn.init.normal_(layer.weight, std=0.01)
            nn.init.constant_(layer.bias, 0)

    @classmethod
    def from_config(cls, cfg, input_shape: List[ShapeSpec]):
        in_channels = [s.channels for s in input_shape]
        assert len(set(in_channels)) == 1, "Each level must have the same channel!"
        anchor_generator = build_anchor_generator(cfg, input_shape)
        num_anchors, box_dim = anchor_generator.num_anchors, anchor_generator.box_dim
        assert len(set(num_anchors)) == 1, "Each level must have the same number of anchors per spatial position"
        return {"in_channels": in_channels[0], "num_anchors": num_anchors[0], "box_dim": box_dim, "conv_dims": cfg.MODEL.RPN.CONV_DIMS}

    def _operands(self):
        """The packed 3x3 weight and the concatenated 1x1 weight / bias, rebuilt only when a parameter was written or moved."""
        params = (self.conv.weight, self.conv.bias, self.objectness_logits.weight, self.objectness_logits.bias,
                  self.anchor_deltas.weight, self.anchor_deltas.bias)
        key = tuple((p.data_ptr(), p._version, p.device) for p in params)
        if getattr(self, "_operands_key", None) != key:
            cw, cb, lw, lb, dw, db = (p.detach().float() for p in params)
            self._operands_val = (ops.pack_conv3x3_weight(cw.contiguous()), cb.contiguous(),
                                  torch.cat([lw.flatten(1), dw.flatten(1)]).contiguous(), torch.cat([lb, db]).contiguous())
            self._operands_key = key
        return self._operands_val

    def _rows(self, x: torch.Tensor) -> torch.Tensor:
        """One NCHW device map -> [N H W, A + A box_dim] channels-last rows: the A logits, then the deltas of anchor a at columns
        A + a box_dim ...  The head runs on the kernels only: a CPU map is an error (ops raises LocovError), not a torch fallback."""
        N, C, H, W = x.shape
        w3, b3, w1, b1 = self._operands()
        if torch.is_grad_enabled() and (x.requires_grad or (self.training and any(p.requires_grad for p in self.parameters()))):
            # training (or an input that carries a graph; evaluation and no_grad keep the detached path below): the same two kernels with a graph behind them; torch.cat hands the 1x1 pair's weight gradient back in slices
            rows = x.float().permute(0, 2, 3, 1).reshape(N * H * W, C).contiguous()
            t = _Conv3x3ReluFn.apply(rows, self.conv.weight, self.conv.bias, w3, b3, H, W)
            lw, dw = self.objectness_logits.weight, self.anchor_deltas.weight
            return ops.linear_autograd(t, torch.cat([lw.flatten(1), dw.flatten(1)]).float(),
                                       torch.cat([self.objectness_logits.bias, self.anchor_deltas.bias]).float())
        rows = x.detach().float().permute(0, 2, 3, 1).reshape(N * H * W, C).contiguous()
        return ops.linear(ops.conv3x3_nhwc_ex(rows, w3, H, W, shift=b3, relu=True), w1, b1)

    def flat_predictions(self, features: Sequence[torch.Tensor]):
        """Per level: logits [N, H W A] and deltas [N, H W A, box_dim], flattened (y, x, a) -- what RPN hands to the selection."""
        A, D = self.num_anchors, self.box_dim
        logits, deltas = [], []
        for x in features:
            N = x.shape[0]
            y = self._rows(x)
            logits.append(y[:, :A].reshape(N, -1))
            deltas.append(y[:, A:].reshape(N, -1, D))
        return logits, deltas

    def forward(self, features: Sequence[torch.Tensor]):
        """Detectron2's lists: per level objectness logits [N, A, H, W] and anchor deltas [N, A box_dim, H, W] (views)."""
        A = self.num_anchors
        logits, deltas = [], []
        for x in features:
            N, _, H, W = x.shape
            y = self._rows(x).view(N, H, W, -1).permute(0, 3, 1, 2)
            logits.append(y[:, :A])
            deltas.append(y[:, A:])
        return logits, deltas


def find_top_rpn_proposals(logits: Sequence[torch.Tensor], deltas: Sequence[torch.Tensor], anchors: Sequence[torch.Tensor], image_sizes,
                           box2box_transform: Box2BoxTransform, nms_thresh: float, pre_nms_topk: int, post_nms_topk: int,
                           min_box_size: float, training: bool):
    """[D2-upstream] find_top_rpn_proposals as a torch chain: per level the pre_nms_topk best anchors (stable descending sort: ties
    in anchor order), apply_deltas, the finite test, Boxes.clip, nonempty(min_box_size), batched_nms with the level ids, slice.
    logits [N, Hi Wi A] / deltas [N, Hi Wi A, 4] / anchors [Hi Wi A, 4] per level.
    Returns per image (boxes [k, 4], logits [k], index [k] int64: the anchor's flat index inside its level, level [k] int64)."""
    N = logits[0].shape[0]
    top_l, top_d, top_a, top_i, top_lvl = [], [], [], [], []
    for lvl, (lg, dl, an) in enumerate(zip(logits, deltas, anchors)):
        k = min(lg.shape[1], int(pre_nms_topk))
        order = torch.sort(lg, dim=1, descending=True, stable=True)[1][:, :k]
        top_l.append(torch.gather(lg, 1, order))
        top_d.append(torch.gather(dl, 1, order[:, :, None].expand(-1, -1, 4)))
        top_a.append(an[order])
        top_i.append(order)
        top_lvl.append(torch.full((k,), lvl, dtype=torch.int64, device=lg.device))
    top_l, top_d, top_a, top_i = (torch.cat(t, dim=1) for t in (top_l, top_d, top_a, top_i))
    top_lvl = torch.cat(top_lvl)
    results = []
    for n in range(N):
        boxes = Boxes(box2box_transform.apply_deltas(top_d[n], top_a[n]))
        scores, index, lvl = top_l[n], top_i[n], top_lvl
        valid = torch.isfinite(boxes.tensor).all(dim=1) & torch.isfinite(scores)
        if not bool(valid.all()):
            if training:
                raise FloatingPointError("Predicted boxes or scores contain Inf/NaN. Training has diverged.")
            boxes, scores, index, lvl = boxes[valid], scores[valid], index[valid], lvl[valid]
        boxes.clip(image_sizes[n])
        keep = boxes.nonempty(threshold=min_box_size)
        boxes, scores, index, lvl = boxes[keep], scores[keep], index[keep], lvl[keep]
        keep = batched_nms(boxes.tensor, scores, lvl, nms_thresh)[:int(post_nms_topk)]
        results.append((boxes.tensor[keep], scores[keep], index[keep], lvl[keep]))
    return results


@PROPOSAL_GENERATOR_REGISTRY.register()
class RPN(nn.Module):
    """[D2-upstream] Region Proposal Network: head -> anchors -> proposals.  `forward` returns the proposals of the batch as
    Instances with proposal_boxes and objectness_logits, in descending objectness order."""

    @configurable
    def __init__(self, *, in_features: List[str], head: nn.Module, anchor_generator: nn.Module, box2box_transform: Box2BoxTransform,
                 pre_nms_topk: Tuple[int, int], post_nms_topk: Tuple[int, int], nms_thresh: float = 0.7, min_box_size: float = 0.0,
                 anchor_matcher: Optional[Matcher] = None, batch_size_per_image: int = 256, positive_fraction: float = 0.5,
                 anchor_boundary_thresh: float = -1.0, loss_weight=1.0, box_reg_loss_type: str = "smooth_l1", smooth_l1_beta: float = 0.0):
        super().__init__()
        self.in_features = list(in_features)
        self.rpn_head = head
        self.anchor_generator = anchor_generator
        self.box2box_transform = box2box_transform
        self.pre_nms_topk = {True: int(pre_nms_topk[0]), False: int(pre_nms_topk[1])}
        self.post_nms_topk = {True: int(post_nms_topk[0]), False: int(post_nms_topk[1])}
        self.nms_thresh = float(nms_thresh)
        self.min_box_size = float(min_box_size)
        self.anchor_matcher = anchor_matcher if anchor_matcher is not None else Matcher([0.3, 0.7], [0, -1, 1], allow_low_quality_matches=True)
        self.batch_size_per_image = int(batch_size_per_image)
        self.positive_fraction = float(positive_fraction)
        self.anchor_boundary_thresh = anchor_boundary_thresh
        if isinstance(loss_weight, (int, float)):
            loss_weight = {"loss_rpn_cls": float(loss_weight), "loss_rpn_loc": float(loss_weight)}
        self.loss_weight = dict(loss_weight)
        self.box_reg_loss_type = box_reg_loss_type
        self.smooth_l1_beta = float(smooth_l1_beta)
        self._fused_batch = None            # the batch tensors behind the lists label_and_sample_anchors last returned
        self._pending_log = None            # (pinned counters, event, images) of a fused losses call not yet logged
        self._defer_log = False

    @classmethod
    def from_config(cls, cfg, input_shape: Dict[str, ShapeSpec]):
        in_features = cfg.MODEL.RPN.IN_FEATURES
        shapes = [input_shape[f] for f in in_features]
        return {"in_features": in_features, "min_box_size": cfg.MODEL.PROPOSAL_GENERATOR.MIN_SIZE, "nms_thresh": cfg.MODEL.RPN.NMS_THRESH,
                "box2box_transform": Box2BoxTransform(weights=cfg.MODEL.RPN.BBOX_REG_WEIGHTS),
                "pre_nms_topk": (cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, cfg.MODEL.RPN.PRE_NMS_TOPK_TEST),
                "post_nms_topk": (cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN, cfg.MODEL.RPN.POST_NMS_TOPK_TEST),
                "anchor_generator": build_anchor_generator(cfg, shapes), "head": build_rpn_head(cfg, shapes),
                "anchor_matcher": Matcher(cfg.MODEL.RPN.IOU_THRESHOLDS, cfg.MODEL.RPN.IOU_LABELS, allow_low_quality_matches=True),
                "batch_size_per_image": cfg.MODEL.RPN.BATCH_SIZE_PER_IMAGE, "positive_fraction": cfg.MODEL.RPN.POSITIVE_FRACTION,
                "anchor_boundary_thresh": cfg.MODEL.RPN.BOUNDARY_THRESH,
                "loss_weight": {"loss_rpn_cls": cfg.MODEL.RPN.LOSS_WEIGHT,
                                "loss_rpn_loc": cfg.MODEL.RPN.BBOX_REG_LOSS_WEIGHT * cfg.MODEL.RPN.LOSS_WEIGHT},
                "box_reg_loss_type": cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE, "smooth_l1_beta": cfg.MODEL.RPN.SMOOTH_L1_BETA}

    def forward(self, images, features: Dict[str, torch.Tensor], gt_instances: Optional[List[Instances]] = None):
        """images: an ImageList (its image_sizes are read); features: name -> NCHW map.  Returns (proposals, losses): in training
        with gt_instances the losses are {"loss_rpn_cls", "loss_rpn_loc"}, otherwise {}."""
        feats = [features[f] for f in self.in_features]
        if not (self.training and gt_instances is not None):
            anchors = self.anchor_generator(feats)
            logits, deltas = self.rpn_head.flat_predictions(feats)
            return self.predict_proposals(anchors, logits, deltas, images.image_sizes), {}
        if not all(f.is_cuda for f in feats):
            raise NotImplementedError("RPN: the training losses need device tensors (feature maps on a ROCm GPU): the RPN head runs on "
                                      "the kernels only and has no torch path")
        anchors = self.anchor_generator(feats)
        logits, deltas = self.rpn_head.flat_predictions(feats)
        gt_labels, gt_boxes = self.label_and_sample_anchors(anchors, gt_instances)
        self._defer_log = True              # the counters are handed to the event storage behind predict_proposals' own read
        try:
            losses = self.losses(anchors, logits, gt_labels, deltas, gt_boxes)
        finally:
            self._defer_log = False
        proposals = self.predict_proposals(anchors, [l.detach() for l in logits], [d.detach() for d in deltas], images.image_sizes)
        self._flush_log()
        return proposals, losses

    # ------------------------------------------------------------------------------------------------ training: labels and sample

    def _fused_train_ok(self, tensors, n_levels: int, n_images: int, hwa: int) -> bool:
        m = self.anchor_matcher
        return (_fused_rpn() and n_levels == 1 and type(m) is Matcher and len(m.labels) <= ops.LABEL_MAX_THRESHOLDS
                and 0 < n_images <= ops.RPN_MAX_IMAGES and 0 < hwa <= ops.RPN_MAX_ANCHORS
                and all(t.is_cuda and t.device == tensors[0].device for t in tensors))

    @torch.no_grad()
    def label_and_sample_anchors(self, anchors: List[Boxes], gt_instances: List[Instances], rnd: Optional[torch.Tensor] = None):
        """[D2-upstream] per image: pairwise_iou(gt, anchors) -> the matcher (low-quality matches promoted) -> the boundary test ->
        subsample_labels with background label 0, everything not drawn -1.  rnd: the draw's [2, N, HWA] float64 uniforms (drawn here
        when None): the min(#positive, int(B f)) positives of smallest rnd[0], then the min(#negative, B - num_pos) negatives of
        smallest rnd[1], equal keys in anchor order -- a uniformly random subset, as upstream's randperm[:k].
        Returns (gt_labels: per image [HWA] int8 in {-1, 0, 1}, matched_gt_boxes: per image [HWA, 4]; zeros without ground truth)."""
        n_levels = len(anchors)
        anchors_t = Boxes.cat(list(anchors)).tensor
        N, HWA = len(gt_instances), anchors_t.shape[0]
        gt = [x.gt_boxes.tensor.float() if x.has("gt_boxes") else anchors_t.new_zeros((0, 4)) for x in gt_instances]
        sizes = [x.image_size for x in gt_instances]
        if rnd is None:
            rnd = torch.rand((2, N, HWA), dtype=torch.float64, device=anchors_t.device)
        if tuple(rnd.shape) != (2, N, HWA) or rnd.dtype != torch.float64:
            raise ValueError(f"label_and_sample_anchors: rnd must be float64 [2, {N}, {HWA}]")
        B, max_pos = self.batch_size_per_image, int(self.batch_size_per_image * self.positive_fraction)
        m = self.anchor_matcher
        if self._fused_train_ok([anchors_t, rnd] + gt, n_levels, N, HWA):
            n_gt = [g.shape[0] for g in gt]
            gtb = torch.cat([g for g in gt if g.shape[0]]) if sum(n_gt) else None
            pre, matched, counts = ops.rpn_label_anchors(anchors_t, gtb, n_gt, sizes, m.thresholds, m.labels, m.allow_low_quality_matches,
                                                         float(self.anchor_boundary_thresh))
            labels = ops.rpn_sample_anchors(pre, counts, rnd, B, max_pos)
            gt_labels, gt_boxes = list(labels.unbind(0)), list(matched.unbind(0))
            self._fused_batch = (gt_labels, gt_boxes, labels, matched, counts)
            return gt_labels, gt_boxes
        self._fused_batch = None
        gt_labels, gt_boxes = [], []
        for n in range(N):
            if gt[n].shape[0]:
                was, m.check_quality = getattr(m, "check_quality", True), False
                try:
                    matched_idxs, lab = m(pairwise_iou(Boxes(gt[n]), Boxes(anchors_t)))
                finally:
                    m.check_quality = was
                lab = lab.to(torch.int8)
                boxes = gt[n][matched_idxs]
            else:
                lab = torch.zeros(HWA, dtype=torch.int8, device=anchors_t.device)
                boxes = torch.zeros_like(anchors_t)
            if self.anchor_boundary_thresh >= 0:
                lab[~Boxes(anchors_t).inside_box(sizes[n], self.anchor_boundary_thresh)] = -1
            pos, neg = lab == 1, lab == 0
            num_pos = min(int(pos.sum()), max_pos)
            num_neg = min(int(neg.sum()), B - num_pos)
            pos_idx = torch.argsort(rnd[0, n] + (~pos).to(rnd.dtype) * 2.0, stable=True)[:num_pos]
            neg_idx = torch.argsort(rnd[1, n] + (~neg).to(rnd.dtype) * 2.0, stable=True)[:num_neg]
            out = torch.full_like(lab, -1)
            out[pos_idx] = 1
            out[neg_idx] = 0
            gt_labels.append(out)
            gt_boxes.append(boxes)
        return gt_labels, gt_boxes

    # ------------------------------------------------------------------------------------------------ training: losses

    def losses(self, anchors: List[Boxes], pred_objectness_logits: List[torch.Tensor], gt_labels: List[torch.Tensor],
               pred_anchor_deltas: List[torch.Tensor], gt_boxes: List[torch.Tensor]) -> Dict[str, torch.Tensor]:
        """[D2-upstream] RPN.losses: loss_rpn_cls = the sum of binary_cross_entropy_with_logits over the anchors of label >= 0,
        loss_rpn_loc = the sum over label == 1 of smooth-L1 between the predicted deltas and get_deltas(anchor, matched box) (beta
        < 1e-5: L1), both divided by batch_size_per_image x N and multiplied by their loss weights.  Logs rpn/num_pos_anchors and
        rpn/num_neg_anchors.  pred_objectness_logits [N, Hi Wi A] and pred_anchor_deltas [N, Hi Wi A, 4] per level."""
        if self.box_reg_loss_type != "smooth_l1":
            raise NotImplementedError(f"RPN: MODEL.RPN.BBOX_REG_LOSS_TYPE {self.box_reg_loss_type!r} (box_reg_loss_type) is not implemented; "
                                      "only \"smooth_l1\"")
        N = len(gt_labels)
        normalizer = self.batch_size_per_image * N
        w_cls, w_loc = self.loss_weight.get("loss_rpn_cls", 1.0), self.loss_weight.get("loss_rpn_loc", 1.0)
        anchors_t = Boxes.cat(list(anchors)).tensor
        logits0 = pred_objectness_logits[0]
        if self._fused_train_ok([anchors_t, logits0, pred_anchor_deltas[0]] + list(gt_labels) + list(gt_boxes), len(pred_objectness_logits),
                                N, anchors_t.shape[0]):
            fb = self._fused_batch
            if fb is not None and fb[0] is gt_labels and fb[1] is gt_boxes:
                labels, matched, counts = fb[2], fb[3], fb[4]
            else:
                labels, matched = torch.stack(list(gt_labels)).to(torch.int8), torch.stack(list(gt_boxes)).float()
                n_pos, n_neg = (labels == 1).sum(dim=1), (labels == 0).sum(dim=1)
                counts = torch.stack([n_pos, n_neg, n_pos, n_neg], dim=1).to(torch.int32)      # (the kernels' [N, 4] layout)
            loss, flags = ops.rpn_loss(logits0, pred_anchor_deltas[0], labels, anchors_t, matched, self.box2box_transform.weights,
                                       self.smooth_l1_beta, w_cls / normalizer, w_loc / normalizer)
            # the two logged counters and the degenerate-anchor bit: to pinned memory, read behind an event (no wait here)
            host = self.__dict__.get("_log_pinned")
            if host is None or host.numel() < 4 * N + 1:
                host = self.__dict__["_log_pinned"] = torch.empty(4 * max(N, ops.RPN_MAX_IMAGES) + 1, dtype=torch.int32).pin_memory()
            host[:4 * N].copy_(counts.view(-1), non_blocking=True)
            host[4 * N:4 * N + 1].copy_(flags, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(logits0.device))
            self._pending_log = (host, event, N)
            if not self._defer_log:
                self._flush_log()
            return {"loss_rpn_cls": loss[0], "loss_rpn_loc": loss[1]}
        labels = torch.stack(list(gt_labels))
        pos_mask, valid_mask = labels == 1, labels >= 0
        storage = get_event_storage()
        storage.put_scalar("rpn/num_pos_anchors", int(pos_mask.sum()) / N)
        storage.put_scalar("rpn/num_neg_anchors", int((labels == 0).sum()) / N)
        degenerate = ~(((anchors_t[:, 2] - anchors_t[:, 0]) > 0) & ((anchors_t[:, 3] - anchors_t[:, 1]) > 0))
        assert not bool((degenerate[None, :] & pos_mask).any()), "Input boxes to Box2BoxTransform are not valid!"
        target = torch.stack([self.box2box_transform.get_deltas(anchors_t, b, check=False) for b in gt_boxes])
        diff = (torch.cat(list(pred_anchor_deltas), dim=1)[pos_mask] - target[pos_mask]).abs()
        if self.smooth_l1_beta < 1e-5:
            loss_loc = diff.sum()
        else:
            beta = self.smooth_l1_beta
            loss_loc = torch.where(diff < beta, 0.5 * diff ** 2 / beta, diff - 0.5 * beta).sum()
        loss_cls = torch.nn.functional.binary_cross_entropy_with_logits(torch.cat(list(pred_objectness_logits), dim=1)[valid_mask],
                                                                        labels[valid_mask].to(torch.float32), reduction="sum")
        return {"loss_rpn_cls": loss_cls / normalizer * w_cls, "loss_rpn_loc": loss_loc / normalizer * w_loc}

    def _flush_log(self) -> None:
        """Hand the counters of the last fused losses call to the event storage (one event wait; none when a later read of the same
        stream -- predict_proposals' -- has already returned)."""
        pending, self._pending_log = self._pending_log, None
        if pending is None:
            return
        host, event, N = pending
        event.synchronize()
        vals = host[:4 * N + 1].tolist()
        assert not vals[4 * N] & ops.RPN_LOSS_FLAG_DEGENERATE, "Input boxes to Box2BoxTransform are not valid!"
        storage = get_event_storage()
        storage.put_scalar("rpn/num_pos_anchors", sum(vals[2:4 * N:4]) / N)
        storage.put_scalar("rpn/num_neg_anchors", sum(vals[3:4 * N:4]) / N)

    @torch.no_grad()
    def predict_proposals(self, anchors: List[Boxes], logits: List[torch.Tensor], deltas: List[torch.Tensor], image_sizes) -> List[Instances]:
        """anchors per level; logits [N, Hi Wi A] and deltas [N, Hi Wi A, 4] per level, flattened (y, x, a)."""
        pre, post = self.pre_nms_topk[self.training], self.post_nms_topk[self.training]
        anchors = [a.tensor for a in anchors]
        out = None
        if self._fused_ok(logits, pre, post):
            got = ops.rpn_proposals(logits[0].float(), deltas[0].float(), anchors[0], image_sizes, self.box2box_transform.weights,
                                    self.box2box_transform.scale_clamp, pre, post, self.min_box_size, self.nms_thresh)
            if got is not None:             # (None: non-finite predictions -- the chain drops them, or raises in training)
                boxes, scores, _, counts = got
                out = [(boxes[n, :c], scores[n, :c]) for n, c in enumerate(counts)]
        if out is None:
            out = [r[:2] for r in find_top_rpn_proposals(logits, deltas, anchors, image_sizes, self.box2box_transform, self.nms_thresh, pre,
                                                         post, self.min_box_size, self.training)]
        results = []
        for size, (boxes, scores) in zip(image_sizes, out):
            res = Instances(tuple(size))
            res.proposal_boxes = Boxes(boxes)
            res.objectness_logits = scores
            results.append(res)
        return results

    def _fused_ok(self, logits, pre: int, post: int) -> bool:
        return (_fused_rpn() and len(logits) == 1 and logits[0].is_cuda and logits[0].shape[0] <= ops.RPN_MAX_IMAGES
                and logits[0].shape[1] <= ops.RPN_MAX_ANCHORS and 1 <= post <= pre <= ops.RPN_MAX_PRE_NMS_TOPK)


def build_anchor_generator(cfg, input_shape):
    name = getattr(cfg.MODEL.ANCHOR_GENERATOR, "NAME", "DefaultAnchorGenerator")
    return ANCHOR_GENERATOR_REGISTRY.get(name)(cfg, input_shape)


def build_rpn_head(cfg, input_shape):
    return RPN_HEAD_REGISTRY.get(cfg.MODEL.RPN.HEAD_NAME)(cfg, input_shape)


def build_proposal_generator(cfg, input_shape):
    """[D2-upstream] the module named by MODEL.PROPOSAL_GENERATOR.NAME; "PrecomputedProposals" -> None."""
    name = cfg.MODEL.PROPOSAL_GENERATOR.NAME
    if name == "PrecomputedProposals":
        return None
    return PROPOSAL_GENERATOR_REGISTRY.get(name)(cfg, input_shape)
