"""The detector end to end: a list of {"image", "height", "width"[, "instances" | "proposals"]} dicts in, per-image results in.

[D2-upstream] detectron2.modeling.meta_arch.rcnn.GeneralizedRCNN and the reference's subclass of it
(ovr/modeling/meta_arch/ovr_rcnn.py:20-124): preprocess_image -> backbone -> proposal generator -> ROI heads -> _postprocess, the
surface restated here on this package's builders (backbone.py, proposal_generator.py, roi_heads/).  The two ends that are not one
of those modules run as ONE launch each for the whole batch (csrc/image_batch.hip):
  * preprocess_image: (x - pixel_mean) / pixel_std and ImageList.from_tensors' padding (ops.preprocess_images), bit-identical
    to the torch expression, which stays as the definition and as the path for whatever the kernel does not take;
  * _postprocess: detector_postprocess' scale / clip / nonempty for every image (ops.detector_rescale) and one host read of the
    N counts, instead of a boolean-mask index (a host wait) per image.
Visualisation, masks and keypoints are not part of this path.  The classes are registered in THIS package's META_ARCH_REGISTRY
only: under Detectron2 the reference registers `OvrRCNN` itself, under the same name.
"""
from __future__ import annotations

import numbers
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import ops
from .backbone import build_backbone
from .proposal_generator import build_proposal_generator
from .registry import Registry, configurable
from .roi_heads import build_roi_heads
from .structures import ImageList, boxes_class_of, cat_rows

META_ARCH_REGISTRY = Registry("META_ARCH")

__all__ = ["META_ARCH_REGISTRY", "GeneralizedRCNN", "ProposalNetwork", "OvrRCNN", "DistillProposalMMSSRCNN", "DistillOnlyProposalMMSSRCNN",
           "build_model", "detector_postprocess"]


def build_model(cfg, **kwargs) -> nn.Module:
    """[D2-upstream] build_model: the meta-architecture named by MODEL.META_ARCHITECTURE, on MODEL.DEVICE.  kwargs go to its
    from_config (the LSM models take tokenizer=...)."""
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg, **kwargs)
    model.to(torch.device(cfg.MODEL.DEVICE))
    return model


def detector_postprocess(results, output_height: int, output_width: int):
    """[D2-upstream] detector_postprocess, box part, for ONE image in plain torch ops: the boxes predicted at results.image_size
    scaled to (output_height, output_width), clipped to it, and the instances whose box became empty dropped.  The result is a new
    object of the classes of `results`; unlike upstream, the boxes of `results` are left as they were."""
    scale_x, scale_y = output_width / results.image_size[1], output_height / results.image_size[0]
    name = "pred_boxes" if results.has("pred_boxes") else "proposal_boxes" if results.has("proposal_boxes") else None
    assert name is not None, "Predictions must contain boxes!"
    fields = dict(results.get_fields())
    fields[name] = output_boxes = fields[name].clone()
    results = type(results)((output_height, output_width), **fields)
    output_boxes.scale(scale_x, scale_y)
    output_boxes.clip(results.image_size)
    return results[output_boxes.nonempty()]


@META_ARCH_REGISTRY.register()
class GeneralizedRCNN(nn.Module):
    """Backbone, proposal generator and ROI heads behind one call.  state_dict() holds backbone.*, proposal_generator.* and
    roi_heads.* only (the reference's checkpoint keys): the pixel statistics are non-persistent buffers."""

    @configurable
    def __init__(self, *, backbone: nn.Module, proposal_generator: Optional[nn.Module], roi_heads: nn.Module, pixel_mean: Sequence[float],
                 pixel_std: Sequence[float], input_format: Optional[str] = None, vis_period: int = 0):
        super().__init__()
        if vis_period > 0:
            raise NotImplementedError(f"vis_period = {vis_period}: training visualisation is not part of this port (VIS_PERIOD must be 0)")
        self.backbone = backbone
        self.proposal_generator = proposal_generator
        self.roi_heads = roi_heads
        self.input_format = input_format
        self.vis_period = vis_period
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        assert self.pixel_mean.shape == self.pixel_std.shape, f"{self.pixel_mean} and {self.pixel_std} have different shapes!"
        self._pixel_stats = ([float(v) for v in pixel_mean], [float(v) for v in pixel_std])    # (host copies: the kernel's arguments)

    @classmethod
    def from_config(cls, cfg) -> Dict[str, Any]:
        backbone = build_backbone(cfg)
        return {"backbone": backbone, "proposal_generator": build_proposal_generator(cfg, backbone.output_shape()),
                "roi_heads": build_roi_heads(cfg, backbone.output_shape()),
                "input_format": getattr(getattr(cfg, "INPUT", None), "FORMAT", None), "vis_period": getattr(cfg, "VIS_PERIOD", 0),
                "pixel_mean": cfg.MODEL.PIXEL_MEAN, "pixel_std": cfg.MODEL.PIXEL_STD}

    @property
    def device(self) -> torch.device:
        return self.pixel_mean.device

    # ------------------------------------------------------------------------------------------------------------------- the call

    def _proposals(self, batched_inputs, images, features, gt_instances):
        if self.proposal_generator is not None:
            return self.proposal_generator(images, features, gt_instances)
        assert "proposals" in batched_inputs[0], "without a proposal generator every input needs its 'proposals'"
        return [x["proposals"].to(self.device) for x in batched_inputs], {}

    def _losses(self, batched_inputs):
        """The training forward: the detector's losses, then the proposal generator's, in one dict."""
        images = self.preprocess_image(batched_inputs)
        gt_instances = [x["instances"].to(self.device) for x in batched_inputs] if "instances" in batched_inputs[0] else None
        features = self.backbone(images.tensor)
        proposals, proposal_losses = self._proposals(batched_inputs, images, features, gt_instances)
        _, detector_losses = self.roi_heads(images, features, proposals, gt_instances)
        losses = {}
        losses.update(detector_losses)
        losses.update(proposal_losses)
        return losses

    def forward(self, batched_inputs: List[Dict[str, Any]]):
        """Training: the dict of losses.  Evaluation: inference(batched_inputs)."""
        if not self.training:
            return self.inference(batched_inputs)
        return self._losses(batched_inputs)

    def inference(self, batched_inputs: List[Dict[str, Any]], detected_instances: Optional[List[Any]] = None, do_postprocess: bool = True):
        """[{"instances": Instances}] per image at the input dict's "height" / "width" (do_postprocess), or the ROI heads' raw
        Instances at the network's image size.  detected_instances: known pred_boxes / pred_classes per image; box detection is
        then skipped (roi_heads.forward_with_given_boxes)."""
        assert not self.training
        images = self.preprocess_image(batched_inputs)
        features = self.backbone(images.tensor)
        if detected_instances is None:
            proposals, _ = self._proposals(batched_inputs, images, features, None)
            results, _ = self.roi_heads(images, features, proposals, None)
        else:
            detected_instances = [x.to(self.device) for x in detected_instances]
            results = self.roi_heads.forward_with_given_boxes(features, detected_instances)
        if do_postprocess:
            return self._postprocess(results, batched_inputs, images.image_sizes)
        return results

    # ------------------------------------------------------------------------------------------------------------------ both ends

    def _kernel_preprocess_ok(self, images: Sequence[torch.Tensor]) -> bool:
        C = len(self._pixel_stats[0])
        return (0 < len(images) <= ops.IMAGE_BATCH_MAX_IMAGES and C <= ops.IMAGE_BATCH_MAX_CHANNELS
                and images[0].dtype in (torch.uint8, torch.float32)
                and all(x.is_cuda and x.device == images[0].device and x.dtype == images[0].dtype and x.dim() == 3 and x.shape[0] == C
                        for x in images))

    def preprocess_image(self, batched_inputs: List[Dict[str, Any]]) -> ImageList:
        """Normalise, pad and batch the inputs' images.  Device images of one dtype (uint8 or fp32), at most 64 of them with at
        most 4 channels, go through one launch; anything else through the torch expression, which gives the same bits."""
        images = [x["image"].to(self.device) for x in batched_inputs]
        divisibility = getattr(self.backbone, "size_divisibility", 0)
        constraints = getattr(self.backbone, "padding_constraints", None)
        if self._kernel_preprocess_ok(images):
            tensor, sizes = ops.preprocess_images(images, *self._pixel_stats, size_divisibility=divisibility, padding_constraints=constraints)
            return ImageList(tensor, sizes)
        images = [(x - self.pixel_mean) / self.pixel_std for x in images]
        return ImageList.from_tensors(images, divisibility, padding_constraints=constraints)

    @staticmethod
    def _postprocess(instances, batched_inputs: List[Dict[str, Any]], image_sizes: Sequence[Tuple[int, int]], *,
                     box_field: str = "pred_boxes", output_key: str = "instances"):
        """The results rescaled to each input's "height" / "width" (default: the image's own size).  fp32 device pred_boxes of at
        most 64 images: one launch and one read of the counts for the batch; an image that loses no box keeps its other fields
        untouched, the others gather theirs by the kept rows (in their order: the compaction keeps it).  Otherwise the per-image
        torch function.  box_field / output_key: the Instances field that holds the boxes and the key of the result dicts
        (ProposalNetwork: "proposal_boxes" under "proposals")."""
        instances = list(instances)
        out_sizes = [(inp.get("height", size[0]), inp.get("width", size[1])) for inp, size in zip(batched_inputs, image_sizes)]
        if not _kernel_postprocess_ok(instances, out_sizes, box_field):
            return [{output_key: detector_postprocess(r, h, w)} for r, (h, w) in zip(instances, out_sizes)]
        inst_cls, box_cls = boxes_class_of(instances)
        sizes = [len(r) for r in instances]
        boxes = cat_rows([r.get(box_field).tensor for r in instances])
        out_boxes, src, counts = ops.detector_rescale(boxes, sizes, [r.image_size for r in instances], out_sizes)
        processed, lo = [], 0
        for r, n, kept, size in zip(instances, sizes, counts, out_sizes):
            fields = dict(r.get_fields())
            if kept != n:
                rows = src[lo:lo + kept]
                fields = {k: v[rows] for k, v in fields.items() if k != box_field}
            fields[box_field] = box_cls(out_boxes[lo:lo + kept])
            processed.append({output_key: inst_cls(size, **fields)})
            lo += n
        return processed


def _kernel_postprocess_ok(instances, out_sizes, box_field: str = "pred_boxes") -> bool:
    if not (0 < len(instances) <= ops.IMAGE_BATCH_MAX_IMAGES):
        return False
    for r, (h, w) in zip(instances, out_sizes):
        if not r.has(box_field) or not isinstance(h, numbers.Integral) or not isinstance(w, numbers.Integral):
            return False
        t = getattr(r.get(box_field), "tensor", None)
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.device == instances[0].get(box_field).tensor.device):
            return False
    return True


@META_ARCH_REGISTRY.register()
class ProposalNetwork(nn.Module):
    """[D2-upstream] ProposalNetwork, the RPN-only meta-architecture: backbone -> proposal generator.  Training returns the
    proposal losses; evaluation [{"proposals": Instances(proposal_boxes, objectness_logits)}] per image, rescaled to the input's
    "height" / "width", in descending objectness -- what the evaluators score as "box_proposals".  state_dict() holds backbone.*
    and proposal_generator.* only.  Both ends are GeneralizedRCNN's: one launch for the batch's preprocessing, one launch and one
    read of the counts for the rescaling."""

    @configurable
    def __init__(self, *, backbone: nn.Module, proposal_generator: nn.Module, pixel_mean: Sequence[float], pixel_std: Sequence[float]):
        super().__init__()
        self.backbone = backbone
        self.proposal_generator = proposal_generator
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        assert self.pixel_mean.shape == self.pixel_std.shape, f"{self.pixel_mean} and {self.pixel_std} have different shapes!"
        self._pixel_stats = ([float(v) for v in pixel_mean], [float(v) for v in pixel_std])    # (host copies: the kernel's arguments)

    @classmethod
    def from_config(cls, cfg) -> Dict[str, Any]:
        backbone = build_backbone(cfg)
        return {"backbone": backbone, "proposal_generator": build_proposal_generator(cfg, backbone.output_shape()),
                "pixel_mean": cfg.MODEL.PIXEL_MEAN, "pixel_std": cfg.MODEL.PIXEL_STD}

    @property
    def device(self) -> torch.device:
        return self.pixel_mean.device

    _kernel_preprocess_ok = GeneralizedRCNN._kernel_preprocess_ok
    preprocess_image = GeneralizedRCNN.preprocess_image

    def forward(self, batched_inputs: List[Dict[str, Any]]):
        """Training: the proposal generator's losses.  Evaluation: [{"proposals": Instances}] per image."""
        images = self.preprocess_image(batched_inputs)
        features = self.backbone(images.tensor)
        gt_instances = None
        if self.training and "instances" in batched_inputs[0]:
            gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
        proposals, proposal_losses = self.proposal_generator(images, features, gt_instances)
        if self.training:
            return proposal_losses
        return GeneralizedRCNN._postprocess(proposals, batched_inputs, images.image_sizes, box_field="proposal_boxes", output_key="proposals")


@META_ARCH_REGISTRY.register()
class OvrRCNN(GeneralizedRCNN):
    """The reference's STT detector (ovr_rcnn.py:20): GeneralizedRCNN whose training forward returns ({}, losses) -- an empty
    first dict where its sibling meta-architectures report their outputs -- with the detector losses first."""

    def forward(self, batched_inputs: List[Dict[str, Any]]):
        if not self.training:
            return self.inference(batched_inputs)
        return {}, self._losses(batched_inputs)


@META_ARCH_REGISTRY.register()
class DistillProposalMMSSRCNN(GeneralizedRCNN):
    """The LSM training model (ovr/modeling/meta_arch/distill_prop_mmss_gcnn.py:30-559, what configs/coco_lsm.yaml names): the
    detector, the language backbone, the grounding / transformer heads on the whole-image grid and on the sampled boxes, and the
    distillation losses between them.  Inference, preprocess_image and _postprocess are GeneralizedRCNN's kernel paths.

    The training forward follows :210-477 statement by statement; the region dictionaries are mmss_regions.grid_regions /
    box_regions, the caption dictionary language_backbone.BertEmbedding's one launch.  Differences, all on the host side:
      * a caption is x["caption"] (a string, tokenized by the language backbone) or, when every input carries x["tokens"] -- a dict
        of the four token lists [T] --, the tokens themselves;
      * forward(batched_inputs, sample=None): `sample` may hold "mlm_draws" [2, B, T] float64, "grid_keys" [B, gh * gw] and "box_keys"
        [sum of the sampled proposals] to replay the step's random choices; a missing entry is drawn from torch's device generator;
      * the per-loss torch.isnan loop (:444-449, one host wait per loss) is ONE stacked test and one host read at the end of the
        forward (ValueError, as the reference raises);
      * self.log(...) statistics are not computed (each is a host sync); the heads' log_info stays lazy."""

    @configurable
    def __init__(self, *, language_backbone: nn.Module, mmss_heads: nn.Module, distill_loss: Optional[nn.Module] = None,
                 vis_in_features: str = "res5", mvm: Optional[bool] = False, spatial_dropout: int = 100, **kwargs):
        super().__init__(**kwargs)
        self.language_backbone = language_backbone
        self.vis_in_features = vis_in_features
        self.mmss_heads = mmss_heads
        self.mvm = mvm
        self.spatial_dropout = spatial_dropout
        self.distill_loss = distill_loss

    @classmethod
    def from_config(cls, cfg, tokenizer=None) -> Dict[str, Any]:
        from .distill_losses import MultiDistillLoss, MultiDistillLossJS, MultiDistillLossL2
        from .language_backbone import build_language_backbone
        from .mmss_heads import build_mmss_heads
        ret = super().from_config(cfg)
        roi_heads, head_cfg = ret["roi_heads"], cfg.MODEL.MMSS_HEAD
        language_backbone = build_language_backbone(cfg, tokenizer)
        mmss_heads = build_mmss_heads(cfg, v_dim=roi_heads.output_shape, l_dim=language_backbone.out_channels, loc_dim=2,
                                      backbone=language_backbone.body)
        if cfg.MODEL.LOAD_EMB_PRED_FROM_MMSS_HEAD:            # :116-125 the detector's embedding layer IS the default head's projection
            weight = mmss_heads[head_cfg.DEFAULT_HEAD].v2l_projection.weight
            bias = mmss_heads[head_cfg.DEFAULT_HEAD].v2l_projection.bias
            assert hasattr(roi_heads.box_predictor, "emb_pred")
            assert weight.shape[0] == roi_heads.box_predictor.emb_pred.weight.shape[0]
            assert weight.shape[1] == roi_heads.box_predictor.emb_pred.weight.shape[1]
            roi_heads.box_predictor.emb_pred.weight = weight
            roi_heads.box_predictor.emb_pred.bias = bias
        distill_loss = None
        if head_cfg.DISTILLATION_LOSS:                        # :127-150 (an unknown type leaves the name unbound there: an error here too)
            kinds = {"KD": MultiDistillLoss, "JS": MultiDistillLossJS, "MSE": MultiDistillLossL2}
            if head_cfg.DISTILLATION_LOSS_TYPE not in kinds:
                raise UnboundLocalError(f"DISTILLATION_LOSS_TYPE {head_cfg.DISTILLATION_LOSS_TYPE!r}: one of {sorted(kinds)}")
            distill_loss = kinds[head_cfg.DISTILLATION_LOSS_TYPE](head_cfg.DISTILLATION_TEMPERATURE, head_cfg.DISTILLATION_LOSS_WEIGHT,
                                                                  head_cfg.DISTILLATION_DETACH_TEACHER,
                                                                  head_cfg.DISTILLATION_TEACHER_TRANSFORMER)
        ret.update(language_backbone=language_backbone, vis_in_features=head_cfg.IN_FEATURES, mmss_heads=mmss_heads,
                   mvm=head_cfg.TRANSFORMER.MASKED_VISUAL_MODELING, spatial_dropout=head_cfg.SPATIAL_DROPOUT, distill_loss=distill_loss)
        return ret

    # ------------------------------------------------------------------------------------------------------------------- the call

    grid_branch = True                                        # (DistillOnlyProposalMMSSRCNN: the sampled boxes only)

    def preprocess_text(self, batched_inputs):
        return [x["caption"] for x in batched_inputs]

    def _caption(self, batched_inputs, draws):
        body = self.language_backbone.body
        if all("tokens" in x for x in batched_inputs):
            keys = ("input_ids", "token_type_ids", "attention_mask", "special_tokens_mask")
            return body.forward_tokenized({k: [x["tokens"][k] for x in batched_inputs] for k in keys}, draws)
        from .language_backbone import MAX_LENGTH
        return body.forward_tokenized(body.tokenizer(self.preprocess_text(batched_inputs), max_length=MAX_LENGTH), draws)

    def _heads(self, regions, input_caption, prefix_out: str, prefix_dist: str, outputs, losses, distributions):
        """:337-346 / :403-417: every head on one region dictionary, the results under the branch's prefixes."""
        for head in self.mmss_heads:
            if self.distill_loss is not None:
                o, l, d = self.mmss_heads[head](regions, input_caption)
                distributions.update({prefix_dist + k: v for k, v in d.items()})
            else:
                o, l = self.mmss_heads[head](regions, input_caption)
            outputs.update({prefix_out + k: v for k, v in o.items()})
            losses.update({prefix_out + k: v for k, v in l.items()})

    def forward(self, batched_inputs: List[Dict[str, Any]], sample: Optional[Dict[str, torch.Tensor]] = None):
        from .mmss_regions import box_regions, grid_regions
        if not self.training:
            return self.inference(batched_inputs)
        if self.mvm:                                          # :330-331 / :400-401, before anything is enqueued
            raise NotImplementedError("MASKED_VISUAL_MODELING is not implemented (nor is it in the reference)")
        sample = sample or {}
        input_caption = self._caption(batched_inputs, sample.get("mlm_draws"))                       # :229-230
        images = self.preprocess_image(batched_inputs)
        gt_instances = [x["instances"].to(self.device) for x in batched_inputs] if "instances" in batched_inputs[0] else None
        features = self.backbone(images.tensor)
        proposals, proposal_losses = self._proposals(batched_inputs, images, features, gt_instances)
        visual_grid_features, box_features, box_proposals, detector_losses = self.roi_heads(images, features, proposals, gt_instances)
        losses = {}
        losses.update(detector_losses)
        losses.update(proposal_losses)

        mmss_outputs, mmss_losses, mmss_distributions = {}, {}, {}
        if self.grid_branch:                                                                         # :273-346
            input_image = grid_regions(visual_grid_features, images.image_sizes, images.tensor.shape[-2:], self.spatial_dropout,
                                       self.training, keys=sample.get("grid_keys"))
            self._heads(input_image, input_caption, "", "", mmss_outputs, mmss_losses, mmss_distributions)
        input_boxes, _ = box_regions(box_features, box_proposals, self.spatial_dropout, self.training, keys=sample.get("box_keys"))   # :348-399
        self._heads(input_boxes, input_caption, "Box ", "box_", mmss_outputs, mmss_losses, mmss_distributions)

        if self.distill_loss is not None or not self.grid_branch:                                    # :424-442 / :692-699
            d = mmss_distributions
            if self.grid_branch:
                mmss_losses["kd_loss"] = self.distill_loss(d["trans"], d["w2r"], d["r2w"])
            mmss_losses["box_kd_loss"] = self.distill_loss(d["box_trans"], d["box_w2r"], d["box_r2w"])
            if self.grid_branch:
                mmss_losses["mixbox_kd_loss"] = self.distill_loss(d["trans"], d["box_w2r"], d["box_r2w"])

        if mmss_losses:                                                                              # :444-449, one host read
            if bool(torch.isnan(torch.stack([v.detach().reshape(()) for v in mmss_losses.values()])).any()):
                for head in self.mmss_heads:
                    print(head, self.mmss_heads[head].log_info)
                print(images.image_sizes)
                raise ValueError()
        losses.update(mmss_losses)
        return mmss_outputs, losses


@META_ARCH_REGISTRY.register()
class DistillOnlyProposalMMSSRCNN(DistillProposalMMSSRCNN):
    """distill_prop_mmss_gcnn.py:561-: the same model without the whole-image grid branch -- the heads run on the sampled boxes
    only, always with their distributions (the reference unpacks three results whatever DISTILLATION_LOSS says), and box_kd_loss is
    the one distillation loss."""
    grid_branch = False
