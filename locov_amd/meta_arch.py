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

__all__ = ["META_ARCH_REGISTRY", "GeneralizedRCNN", "OvrRCNN", "build_model", "detector_postprocess"]


def build_model(cfg) -> nn.Module:
    """[D2-upstream] build_model: the meta-architecture named by MODEL.META_ARCHITECTURE, on MODEL.DEVICE."""
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
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
    def _postprocess(instances, batched_inputs: List[Dict[str, Any]], image_sizes: Sequence[Tuple[int, int]]):
        """The results rescaled to each input's "height" / "width" (default: the image's own size).  fp32 device pred_boxes of at
        most 64 images: one launch and one read of the counts for the batch; an image that loses no box keeps its other fields
        untouched, the others gather theirs by the kept rows.  Otherwise the per-image torch function."""
        instances = list(instances)
        out_sizes = [(inp.get("height", size[0]), inp.get("width", size[1])) for inp, size in zip(batched_inputs, image_sizes)]
        if not _kernel_postprocess_ok(instances, out_sizes):
            return [{"instances": detector_postprocess(r, h, w)} for r, (h, w) in zip(instances, out_sizes)]
        inst_cls, box_cls = boxes_class_of(instances)
        sizes = [len(r) for r in instances]
        boxes = cat_rows([r.pred_boxes.tensor for r in instances])
        out_boxes, src, counts = ops.detector_rescale(boxes, sizes, [r.image_size for r in instances], out_sizes)
        processed, lo = [], 0
        for r, n, kept, size in zip(instances, sizes, counts, out_sizes):
            fields = dict(r.get_fields())
            if kept != n:
                rows = src[lo:lo + kept]
                fields = {k: v[rows] for k, v in fields.items() if k != "pred_boxes"}
            fields["pred_boxes"] = box_cls(out_boxes[lo:lo + kept])
            processed.append({"instances": inst_cls(size, **fields)})
            lo += n
        return processed


def _kernel_postprocess_ok(instances, out_sizes) -> bool:
    if not (0 < len(instances) <= ops.IMAGE_BATCH_MAX_IMAGES):
        return False
    for r, (h, w) in zip(instances, out_sizes):
        if not r.has("pred_boxes") or not isinstance(h, numbers.Integral) or not isinstance(w, numbers.Integral):
            return False
        t = getattr(r.pred_boxes, "tensor", None)
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.device == instances[0].pred_boxes.tensor.device):
            return False
    return True


@META_ARCH_REGISTRY.register()
class OvrRCNN(GeneralizedRCNN):
    """The reference's STT detector (ovr_rcnn.py:20): GeneralizedRCNN whose training forward returns ({}, losses) -- an empty
    first dict where its sibling meta-architectures report their outputs -- with the detector losses first."""

    def forward(self, batched_inputs: List[Dict[str, Any]]):
        if not self.training:
            return self.inference(batched_inputs)
        return {}, self._losses(batched_inputs)
