"""From a decoded image to the dict the models take: the reference's dataset mapper, its image side on the device.

The reference's BasicTextImageDatasetMapper.__call__ (ovr/data/mappers/basic_mappers.py:90-192) reduces, for every shipped config, to
Detectron2's build_augmentation -- ResizeShortestEdge plus, in training, RandomFlip -- because the strong augmentations of
ovr/data/detection_utils.py:60-100 are off by default and in coco_lsm.yaml / coco_stt.yaml.  ResizeTransform.apply_image resizes
uint8 images with Pillow: Image.fromarray(img).resize((new_w, new_h), Image.BILINEAR).

As in evaluation.py the numpy path of this module is the DEFINITION:

  * resize_bilinear_host restates Pillow's ImagingResample (public Resample.c) for 8-bit channels and the bilinear filter, byte for
    byte.  Per axis, in float64: scale = in / out, fs = max(scale, 1), support = fs, and for output index xx
        center = (xx + 0.5) * scale;  xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), in) - xmin
        w[x] = f((x + xmin - center + 0.5) * (1 / fs)), f(t) = 1 - |t| below 1, else 0;  w /= sum(w) (summed in order, if != 0)
        k[x] = int(w[x] * 2^22 + 0.5)     (- 0.5 for a negative weight; int() truncates)
    and a pass is clamp((2^21 + sum k[x] * pixel[xmin + x]) >> 22, 0, 255) in int32.  The horizontal pass comes first and writes
    uint8; the vertical pass reads those rounded bytes.  A pass between equal sizes is skipped (it is the identity anyway).
  * the device path (ops.resize_flip_images: csrc/image_resize.hip) does resize, flip and the HWC -> CHW transposition of a whole
    batch in one launch and gives the same bytes.  The host path serves CPU tensors, LOCOV_FUSED_RESIZE=0 and the sizes outside
    ops.resize_supported.
  * a "file_name" that is a baseline JPEG is decoded without Pillow on a cuda mapper, to Pillow's bytes: jpeg.py is the definition,
    the scans of the batch are Huffman-decoded on host threads inside the library and the pixels made in two launches
    (ops.jpeg_entropy_stage / jpeg_pack / jpeg_decode_records: csrc/jpeg_entropy.h, csrc/jpeg.hip).  Pillow serves everything else:
    CPU mappers, LOCOV_FUSED_JPEG=0, other files, streams the decoder does not take, any anomaly in a scan.
  * transform_proposals and change_proposals_as_gt are the definition of the proposal side (MODEL.LOAD_OBJ_PROPOSALS, as in
    coco_lsm.yaml: CocoImageDatasetMapper turns the image's precomputed OLN proposals with objectness > 0.7 into its "instances",
    gt_classes 1, and moves the annotated boxes to "gt_obj").  The boxes go through apply_box in the ARRAY'S dtype -- numpy rounds
    the Python factor new_w * 1.0 / w (formed in double) and the Python size to it, so fp32 rows are multiplied and mirrored in
    fp32 --, are rounded once to fp32, clipped, the empty ones dropped, the first topk kept; the threshold is compared in fp32.
    The device path (ops.map_proposals: csrc/proposal_map.hip) does both steps for a whole batch in one launch, on rows that
    ProposalStore put on the device once, and gives the same values.  The host path serves CPU tensors, LOCOV_FUSED_PROPOSALS=0
    and row dtypes outside ops.PROPOSAL_DTYPES.

[D2-upstream] (restated from Detectron2's public sources, unverified here: Detectron2 is not installed): ResizeShortestEdge,
RandomFlip, build_augmentation, the transforms' apply_coords / apply_box, BoxMode.convert, transform_instance_annotations,
filter_empty_instances, transform_proposals.  annotations_to_instances and check_image_size are the reference's own
(ovr/data/detection_utils.py:21-58, 272-352), as are CocoImageDatasetMapper, change_proposals_as_gt and get_mapper
(ovr/data/mappers/coco_mappers.py:24-106, __init__.py:11-35).  The annotated boxes stay on the host, in float64 numpy as upstream: a
handful of boxes per image.

The strong augmentations (INPUT.COLOR_JITTER, RANDOM_GRAY_SCALE, GAUSSIAN_BLUR, RANDOM_ERASE; basic_mappers.py:171-180) are opt-in
through the reference's own constructor parameter: DatasetMapper(cfg, is_train, device, seed, train_aug =
strong_augment.build_complete_augmentation(cfg, is_train)).  strong_augment.apply_host is their definition (Pillow's and
torchvision's bytes); on a cuda device the batch goes through ops.augment_images (csrc/image_augment.hip) in at most two launches
after the resize's one.  The host path serves CPU tensors, LOCOV_FUSED_AUGMENT=0 and a sigma outside ops.augment_supported.
Without train_aug the four keys are refused as before, and build_augmentation refuses them always.

Not built: INPUT.CROP, masks, keypoints, VawImageDatasetMapper, TextImageDatasetMapperNoise and its NOISE_* options, dataset
registration and reading the proposal file -- the crop and the two mappers are refused with an error, never ignored.
"""
from __future__ import annotations

import copy
import math
import os
import random
from dataclasses import dataclass
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .structures import Boxes, Instances

PRECISION_BITS = 22                      # Pillow's PRECISION_BITS for 8-bit channels: 32 - 8 - 2
XYXY_ABS, XYWH_ABS = 0, 1                # [D2-upstream] BoxMode
FLIP_NONE, FLIP_HORIZONTAL, FLIP_VERTICAL = 0, 1, 2
# a JPEG file larger than this is Pillow's to answer on every mapper: libjpeg refuses more than 65 500 pixels a side, and Pillow
# warns above Image.MAX_IMAGE_PIXELS (89 478 485) and raises DecompressionBombError -- the black image -- above twice that
JPEG_MAX_SIDE, JPEG_MAX_PIXELS = 65500, 89478485


# ---- Pillow's resampling -------------------------------------------------------------------------------------------------------

def bilinear_coefficients(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter: (xmin [out], count [out], k [out, ksize] int32), the
    row of k behind count zero."""
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                  # (astype truncates, as C's (int))
    count = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        t = np.abs(((x + xmin).astype(np.float64) - center + 0.5) * ss)
        w[:, x] = np.where((x < count) & (t < 1.0), 1.0 - t, 0.0)
        ww = ww + w[:, x]                                                            # in order; the zeros behind count change nothing
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz, None]
    k = np.where(w < 0.0, -0.5 + w * float(1 << PRECISION_BITS), 0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
    return xmin, count, k


def _resample_axis0(img: np.ndarray, out_size: int) -> np.ndarray:
    """One pass along axis 0 of a uint8 array [in, ...]."""
    xmin, _, k = bilinear_coefficients(img.shape[0], out_size)
    acc = np.full((out_size,) + img.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
    tail = (slice(None),) + (None,) * (img.ndim - 1)
    for x in range(k.shape[1]):
        rows = np.minimum(xmin + x, img.shape[0] - 1)                                # (behind count the tap is 0)
        acc += k[:, x][tail] * img[rows].astype(np.int32)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_bilinear_host(img, new_h: int, new_w: int) -> np.ndarray:
    """np.asarray(Image.fromarray(img).resize((new_w, new_h), Image.BILINEAR)) for uint8 [H, W, C] (or [H, W]), without Pillow."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise TypeError(f"resize_bilinear_host: a uint8 [H, W, C] image, got {img.dtype} {img.shape}")
    new_h, new_w = int(new_h), int(new_w)
    if min(img.shape[:2]) < 1 or new_h < 1 or new_w < 1:
        raise ValueError(f"resize_bilinear_host: sizes must be positive, got {img.shape[:2]} -> {(new_h, new_w)}")
    if new_w != img.shape[1]:
        img = np.swapaxes(_resample_axis0(np.swapaxes(img, 0, 1), new_w), 0, 1)
    if new_h != img.shape[0]:
        img = _resample_axis0(img, new_h)
    return np.ascontiguousarray(img)


# ---- [D2-upstream] transforms: what they do to an image and to coordinates -----------------------------------------------------

class NoOpTransform:
    flip = FLIP_NONE

    def output_shape(self, h: int, w: int) -> Tuple[int, int]:
        return h, w

    def apply_image(self, img: np.ndarray) -> np.ndarray:
        return img

    def apply_coords(self, coords: np.ndarray) -> np.ndarray:
        return coords

    def apply_box(self, box: np.ndarray) -> np.ndarray:
        """Transform.apply_box: the four corners through apply_coords, then their min / max."""
        idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
        coords = np.asarray(box).reshape(-1, 4)[:, idxs].reshape(-1, 2)
        coords = self.apply_coords(coords).reshape((-1, 4, 2))
        return np.concatenate((coords.min(axis=1), coords.max(axis=1)), axis=1)


class ResizeTransform(NoOpTransform):
    def __init__(self, h: int, w: int, new_h: int, new_w: int):
        self.h, self.w, self.new_h, self.new_w = int(h), int(w), int(new_h), int(new_w)

    def output_shape(self, h, w):
        return self.new_h, self.new_w

    def apply_image(self, img):
        assert img.shape[:2] == (self.h, self.w)
        return resize_bilinear_host(img, self.new_h, self.new_w)

    def apply_coords(self, coords):
        coords[:, 0] = coords[:, 0] * (self.new_w * 1.0 / self.w)
        coords[:, 1] = coords[:, 1] * (self.new_h * 1.0 / self.h)
        return coords


class HFlipTransform(NoOpTransform):
    flip = FLIP_HORIZONTAL

    def __init__(self, width: int):
        self.width = int(width)

    def apply_image(self, img):
        return np.flip(img, axis=1)

    def apply_coords(self, coords):
        coords[:, 0] = self.width - coords[:, 0]
        return coords


class VFlipTransform(NoOpTransform):
    flip = FLIP_VERTICAL

    def __init__(self, height: int):
        self.height = int(height)

    def apply_image(self, img):
        return np.flip(img, axis=0)

    def apply_coords(self, coords):
        coords[:, 1] = self.height - coords[:, 1]
        return coords


class TransformList:
    def __init__(self, transforms: Sequence[NoOpTransform]):
        self.transforms = list(transforms)

    def apply_image(self, img):
        for t in self.transforms:
            img = t.apply_image(img)
        return img

    def apply_coords(self, coords):
        for t in self.transforms:
            coords = t.apply_coords(coords)
        return coords

    def apply_box(self, box):
        for t in self.transforms:
            box = t.apply_box(box)
        return box


class ResizeShortestEdge:
    """short_edge_length: the choices ("choice") or the [min, max] range ("range"); a drawn size of 0 is a no-op."""

    def __init__(self, short_edge_length, max_size: int = 2 ** 31 - 1, sample_style: str = "range"):
        assert sample_style in ("range", "choice"), sample_style
        self.is_range = sample_style == "range"
        if isinstance(short_edge_length, int):
            short_edge_length = (short_edge_length, short_edge_length)
        if self.is_range:
            assert len(short_edge_length) == 2, f"short_edge_length must be two values using 'range' sample style. Got {short_edge_length}!"
        self.short_edge_length, self.max_size = tuple(int(v) for v in short_edge_length), int(max_size)

    def draw(self, rng: random.Random) -> int:
        if self.is_range:
            return rng.randint(self.short_edge_length[0], self.short_edge_length[1])
        return rng.choice(self.short_edge_length)

    @staticmethod
    def get_output_shape(oldh: int, oldw: int, short_edge_length: int, max_size: int) -> Tuple[int, int]:
        h, w = oldh, oldw
        size = short_edge_length * 1.0
        scale = size / min(h, w)
        if h < w:
            newh, neww = size, scale * w
        else:
            newh, neww = scale * h, size
        if max(newh, neww) > max_size:
            scale = max_size * 1.0 / max(newh, neww)
            newh = newh * scale
            neww = neww * scale
        return int(newh + 0.5), int(neww + 0.5)

    def get_transform(self, h: int, w: int, size: int) -> NoOpTransform:
        if size == 0:
            return NoOpTransform()
        newh, neww = self.get_output_shape(h, w, size, self.max_size)
        return ResizeTransform(h, w, newh, neww)


class RandomFlip:
    def __init__(self, prob: float = 0.5, *, horizontal: bool = True, vertical: bool = False):
        if horizontal and vertical:
            raise ValueError("Cannot do both horiz and vert. Please use two Flip instead.")
        if not horizontal and not vertical:
            raise ValueError("At least one of horiz or vert has to be True!")
        self.prob, self.horizontal, self.vertical = float(prob), bool(horizontal), bool(vertical)

    def draw(self, rng: random.Random) -> bool:
        return rng.random() < self.prob

    def get_transform(self, h: int, w: int, do: bool) -> NoOpTransform:
        if not do:
            return NoOpTransform()
        return HFlipTransform(w) if self.horizontal else VFlipTransform(h)


def _refuse_unbuilt(cfg, strong_given: bool = False) -> None:
    """strong_given: the caller holds a StrongAugmentation (DatasetMapper's train_aug), which lifts the four strong keys only."""
    inp = cfg.INPUT
    crop = getattr(inp, "CROP", None)
    if crop is not None and getattr(crop, "ENABLED", False):
        raise NotImplementedError("INPUT.CROP.ENABLED: RandomCrop is not built (locov_amd.data)")
    if strong_given:
        return
    for key, off in (("COLOR_JITTER", 0.0), ("RANDOM_GRAY_SCALE", False), ("GAUSSIAN_BLUR", False), ("RANDOM_ERASE", False)):
        v = getattr(inp, key, off)
        if (v > 0) if key == "COLOR_JITTER" else bool(v):
            raise NotImplementedError(f"INPUT.{key}: the strong augmentations are not built (locov_amd.data)")


def build_augmentation(cfg, is_train: bool) -> list:
    """[ResizeShortestEdge] plus, in training and unless INPUT.RANDOM_FLIP is "none", [RandomFlip].  The strong keys are refused
    here, always: they are served by DatasetMapper(..., train_aug=strong_augment.build_complete_augmentation(cfg, is_train))."""
    _refuse_unbuilt(cfg)
    return _resize_and_flip(cfg, is_train)


def _resize_and_flip(cfg, is_train: bool) -> list:
    if is_train:
        min_size, max_size, sample_style = cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING
    else:
        min_size, max_size, sample_style = cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, "choice"
    if isinstance(min_size, (list, tuple)):
        min_size = tuple(min_size)
    augmentation = [ResizeShortestEdge(min_size, max_size, sample_style)]
    if is_train and cfg.INPUT.RANDOM_FLIP != "none":
        augmentation.append(RandomFlip(horizontal=cfg.INPUT.RANDOM_FLIP == "horizontal", vertical=cfg.INPUT.RANDOM_FLIP == "vertical"))
    return augmentation


# ---- the box side --------------------------------------------------------------------------------------------------------------

def convert_to_xyxy(box, from_mode: int) -> list:
    """BoxMode.convert(box, from_mode, XYXY_ABS) of one box given as a list.  Upstream forms torch.tensor(box) -- fp32 for Python
    floats, int64 for ints -- adds x + w, y + h in that type and returns a list of Python numbers; so does this."""
    if int(from_mode) == XYXY_ABS:
        return list(box)
    if int(from_mode) != XYWH_ABS:
        raise NotImplementedError(f"bbox_mode {from_mode}: only XYXY_ABS (0) and XYWH_ABS (1) are built")
    assert len(box) == 4, "BoxMode.convert takes either a k-tuple/list or an Nxk array/tensor, where k == 4 or 5"
    arr = torch.tensor(list(box))[None, :]
    arr[:, 2] += arr[:, 0]
    arr[:, 3] += arr[:, 1]
    return arr.flatten().tolist()


def transform_instance_annotations(annotation: dict, transforms: TransformList, image_size: Tuple[int, int]) -> dict:
    """The box part: XYXY, the corners through the transforms, clipped at 0 and at the image, in float64."""
    bbox = convert_to_xyxy(annotation["bbox"], annotation["bbox_mode"])
    bbox = transforms.apply_box(np.array([bbox]))[0].clip(min=0)
    annotation["bbox"] = np.minimum(bbox, list(image_size + image_size)[::-1])
    annotation["bbox_mode"] = XYXY_ABS
    return annotation


def annotations_to_instances(annos: List[dict], image_size: Tuple[int, int]) -> Instances:
    """ovr/data/detection_utils.py:272-352 without masks and keypoints: gt_boxes (fp32), gt_classes (int64) and, as there, every
    other annotation field whose values are ints or arrays."""
    boxes = [convert_to_xyxy(obj["bbox"], obj["bbox_mode"]) for obj in annos]
    target = Instances(tuple(image_size))
    target.gt_boxes = Boxes(torch.as_tensor(np.asarray(boxes, dtype=np.float64).reshape(-1, 4), dtype=torch.float32))
    target.gt_classes = torch.tensor([int(obj["category_id"]) for obj in annos], dtype=torch.int64)
    if len(annos):
        for name in set(annos[0].keys()).difference({"iscrowd", "bbox", "category_id", "area", "bbox_mode"}):
            v = [ann[name] for ann in annos]
            if isinstance(v[0], int):
                v = torch.tensor(v, dtype=torch.int64)
            elif isinstance(v[0], np.ndarray):
                v = torch.stack([torch.from_numpy(np.ascontiguousarray(x)) for x in v])
            if torch.is_tensor(v):
                target.set(name, v)
    return target


def filter_empty_instances(instances: Instances, box_threshold: float = 1e-5) -> Instances:
    return instances[instances.gt_boxes.nonempty(threshold=box_threshold)]


def check_image_size(dataset_dict: dict, image_hw: Tuple[int, int]) -> None:
    """ovr/data/detection_utils.py:21-58: a transposed size in the dict is swapped, any other mismatch is overwritten with the
    image's size (with a message), and a missing entry is filled in."""
    h, w = int(image_hw[0]), int(image_hw[1])
    if "width" in dataset_dict or "height" in dataset_dict:
        image_wh, expected_wh = (w, h), (dataset_dict["width"], dataset_dict["height"])
        if image_wh != expected_wh:
            if image_wh == (expected_wh[1], expected_wh[0]):
                dataset_dict["width"], dataset_dict["height"] = expected_wh[1], expected_wh[0]
            else:
                print("Mismatched image shape{}, got {}, expect {}.".format(
                    " for image " + dataset_dict["file_name"] if "file_name" in dataset_dict else "", image_wh, expected_wh)
                    + " Please check the width/height in your annotation.")
                dataset_dict["width"], dataset_dict["height"] = w, h
    dataset_dict.setdefault("width", w)
    dataset_dict.setdefault("height", h)


# ---- precomputed proposals and the pseudo ground truth ---------------------------------------------------------------------------

OBJECTNESS_THR = 0.7                     # change_proposals_as_gt's default (ovr/data/mappers/coco_mappers.py:88)


def transform_proposals(dataset_dict: dict, image_shape: Tuple[int, int], transforms: TransformList, proposal_topk: int,
                        min_box_size: float = 0) -> None:
    """[D2-upstream] detection_utils.transform_proposals, in place: a dict with "proposal_boxes" ([n, 4] array), "proposal_bbox_mode"
    and "proposal_objectness_logits" loses the three and gains "proposals" = Instances(image_shape, proposal_boxes,
    objectness_logits).  The boxes go through transforms.apply_box in the ARRAY'S OWN dtype (numpy rounds the Python factor and
    the Python size to it), are rounded once to fp32 (Boxes), clipped, the empty ones dropped, the first proposal_topk kept."""
    if "proposal_boxes" not in dataset_dict:
        return
    mode = dataset_dict.pop("proposal_bbox_mode")
    if int(mode) != XYXY_ABS:
        raise NotImplementedError(f"proposal_bbox_mode {mode}: only XYXY_ABS (0) is built")
    boxes = Boxes(torch.as_tensor(transforms.apply_box(np.asarray(dataset_dict.pop("proposal_boxes"))).astype("float32")))
    logits = torch.as_tensor(np.asarray(dataset_dict.pop("proposal_objectness_logits")).astype("float32"))
    boxes.clip(image_shape)
    keep = boxes.nonempty(threshold=min_box_size)
    dataset_dict["proposals"] = Instances(tuple(image_shape), proposal_boxes=boxes[keep][:proposal_topk],
                                          objectness_logits=logits[keep][:proposal_topk])


def change_proposals_as_gt(dataset_dict: dict, objectness_thr: float = OBJECTNESS_THR) -> dict:
    """ovr/data/mappers/coco_mappers.py:88-106: a new dict whose "instances" are the proposals with objectness_logits >
    objectness_thr (compared in the logits' fp32, as torch compares a tensor with a Python number) under the fields
    objectness_logits, gt_classes (ones: "an object") and gt_boxes; the former "instances" are "gt_obj"; "proposals" is gone.
    Without "proposals" or "instances": KeyError, as there."""
    out = dict(dataset_dict)
    proposals, annotated = out.pop("proposals"), out.pop("instances")
    picked = proposals[proposals.objectness_logits > objectness_thr]
    out["gt_obj"] = annotated
    out["instances"] = Instances(picked.image_size, objectness_logits=picked.objectness_logits,
                                 gt_classes=torch.ones(len(picked), dtype=torch.int64, device=picked.objectness_logits.device),
                                 gt_boxes=picked.proposal_boxes)
    return out


class ProposalStore:
    """The precomputed proposals of a dataset, packed ONCE: proposals_by_image_id is the reference's metadata entry
    "object_proposals", {image_id: array [n, >= 5] or a list whose element 0 is that array}, rows of XYXY + objectness logit; only
    the first five columns are used.

    All arrays of one dtype keep it.  MIXED dtypes across images are promoted to float64 -- on every device, so that an image's
    boxes do not depend on where the store lives; the transform then runs in float64 for all of them.
    On a cuda device the rows of all images stand in one [R, 5] tensor (`rows`) and `table` maps image_id -> (first row, n): a
    step then uploads a descriptor, not rows.  `rows` is None on the CPU, and for a dtype outside ops.PROPOSAL_DTYPES, where the
    store is a thin view over the arrays (store[image_id] -> [n, >= 5] array, KeyError for an unknown id) and the host
    definition does the work."""

    def __init__(self, proposals_by_image_id: dict, device="cpu"):
        self.device = torch.device(device)
        arrays = {}
        for image_id, rows in proposals_by_image_id.items():
            rows = np.asarray(rows[0] if isinstance(rows, list) else rows)
            if rows.ndim != 2 or rows.shape[1] < 5:
                raise ValueError(f"ProposalStore: image {image_id!r}: rows must be [n, >= 5] (XYXY + logit), got {rows.shape}")
            arrays[image_id] = rows
        dtypes = {a.dtype for a in arrays.values()}
        self.dtype = next(iter(dtypes)) if len(dtypes) == 1 else np.dtype(np.float64)
        if len(dtypes) > 1:                                        # (mixed: one dtype for the whole dataset)
            arrays = {k: a.astype(np.float64) for k, a in arrays.items()}
        self.arrays = arrays
        self.table: Dict[object, Tuple[int, int]] = {}
        self.rows: Optional[torch.Tensor] = None
        if self.device.type == "cuda" and self.dtype in (np.float32, np.float64):
            start = 0
            for image_id, a in arrays.items():
                self.table[image_id] = (start, a.shape[0])
                start += a.shape[0]
            packed = np.empty((start, 5), dtype=self.dtype)
            for image_id, a in arrays.items():
                s, n = self.table[image_id]
                packed[s:s + n] = a[:, :5]
            self.rows = torch.from_numpy(packed).to(self.device)

    def __contains__(self, image_id) -> bool:
        return image_id in self.arrays

    def __len__(self) -> int:
        return len(self.arrays)

    def __getitem__(self, image_id) -> np.ndarray:
        return self.arrays[image_id]


# ---- the mapper ----------------------------------------------------------------------------------------------------------------

@dataclass
class _Prepared:
    """One image between _prepare and _finish: the dict being built, the raw HWC image, its drawn transforms, their (new_h, new_w)."""
    d: dict
    raw: Union[np.ndarray, torch.Tensor]
    transforms: TransformList
    size: Tuple[int, int]

    @property
    def flip(self) -> int:
        return max((t.flip for t in self.transforms.transforms), default=FLIP_NONE)

    @property
    def factors(self) -> Tuple[float, float]:                      # (fx, fy) as ResizeTransform.apply_coords forms them, in double
        resize, (nh, nw) = self.transforms.transforms[0], self.size
        return (nw * 1.0 / resize.w, nh * 1.0 / resize.h) if isinstance(resize, ResizeTransform) else (1.0, 1.0)


def _slices(idx: List[int]) -> Iterator[List[int]]:               # the images a kernel takes, as many at a time as one call holds
    for lo in range(0, len(idx), ops.IMAGE_BATCH_MAX_IMAGES):
        yield idx[lo:lo + ops.IMAGE_BATCH_MAX_IMAGES]


def _read_file(path: str, fmt: str) -> np.ndarray:
    """[D2-upstream] detection_utils.read_image for the formats "RGB", "BGR" and "L" (EXIF orientation is not applied)."""
    from PIL import Image
    with open(path, "rb") as f:
        image = Image.open(f)
        image = np.asarray(image.convert("L" if fmt == "L" else "RGB"))
    if fmt == "L":
        return image[:, :, None]
    return np.ascontiguousarray(image[:, :, ::-1]) if fmt == "BGR" else image


class DatasetMapper:
    """The reference's BasicTextImageDatasetMapper for the shipped configs.  __call__(dataset_dict) maps one image, map_batch a
    list; both return the dicts the models take: "image" uint8 [C, new_h, new_w], "height" / "width" of the original
    (check_image_size's rules), "instances" (when the dict has "annotations"), "caption" (one string when the dict has a list).

    The raw image is dataset_dict["image_raw"], HWC uint8 (numpy or tensor) already in INPUT.FORMAT order; without it "file_name"
    is read with Pillow, and when that fails the reference's fallback applies: a black image and the caption "A black image.".
    On a cuda device a baseline JPEG file is decoded without Pillow, to Pillow's bytes (jpeg.py is the definition): the batch's
    scans on host threads, one pinned upload, two launches (ops.jpeg_entropy_stage / jpeg_pack / jpeg_decode_records).  "cpu",
    LOCOV_FUSED_JPEG=0, a file that is no JPEG, a header the decoder does not take (progressive, other sampling layouts, ...: jpeg.py)
    and any anomaly in the scan take Pillow as before, with its error semantics -- the truncated file is still the black image.

    device: where "image" is produced.  A cuda device resizes, flips and transposes the whole batch in one launch
    (ops.resize_flip_images); "cpu" -- and LOCOV_FUSED_RESIZE=0, and any image outside ops.resize_supported -- takes the numpy
    definition (and is then moved to `device`).  None: cfg.MODEL.DEVICE when a GPU is present, else the CPU.

    MODEL.LOAD_OBJ_PROPOSALS: a dict carrying "proposal_boxes" ([n, 4] array, XYXY_ABS), "proposal_bbox_mode" and
    "proposal_objectness_logits" gets "proposals" (transform_proposals, cut at DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN / _TEST), on
    `device`.  On a cuda device the batch's rows are packed into one pinned buffer, uploaded once and mapped in one launch
    (ops.map_proposals); LOCOV_FUSED_PROPOSALS=0, a CPU device and rows that are not fp32 / fp64 take the host definition.

    train_aug: None, or strong_augment.build_complete_augmentation(cfg, is_train).  Given, it lifts the refusal of the four strong
    keys (INPUT.CROP stays refused) and is applied in training to "image" after the resize and flip; boxes, captions and proposals
    are untouched.  draw_sample then also returns "strong" (StrongAugmentation.draw's dict per image, drawn for the resized size)
    and "erase_seed"; the erasers' noise is torch.randn on `device` from a torch.Generator seeded with it (erase_noise), or
    sample["erase_noise"] when the caller carries noise from one device to another.

    Every random draw comes from draw_sample(dataset_dicts) (the edge length, the flip and the caption index per image, from
    self.rng); map_batch(dataset_dicts, sample=...) replays one."""

    def __init__(self, cfg, is_train: bool = True, device=None, seed: Optional[int] = None, train_aug=None):
        self.is_train = bool(is_train)
        _refuse_unbuilt(cfg, strong_given=train_aug is not None)
        self.augmentations = _resize_and_flip(cfg, is_train)
        # files by name until _raw takes them: what draw_sample decoded for its size (train_aug only; None: it failed there), and on
        # the JPEG device path the staged scan (ops.JpegStaged), then the decoded device tensor
        self._decoded: Dict[str, object] = {}
        self.train_aug = train_aug if self.is_train else None      # (basic_mappers.py:171: applied in training only)
        if getattr(cfg.MODEL, "MASK_ON", False) or getattr(cfg.MODEL, "KEYPOINT_ON", False):
            raise NotImplementedError("MODEL.MASK_ON / KEYPOINT_ON: only the box side of the mapper is built")
        self.proposal_topk: Optional[int] = None                   # (basic_mappers.py:82-87)
        if getattr(cfg.MODEL, "LOAD_OBJ_PROPOSALS", False):
            self.proposal_topk = int(cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TRAIN if is_train else cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST)
        self.image_format = cfg.INPUT.FORMAT
        if device is None:
            device = cfg.MODEL.DEVICE if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.rng = random.Random(seed)

    def _on_device(self, stage: str) -> bool:                      # the stage's kernel serves a cuda mapper unless LOCOV_FUSED_<stage>=0
        return self.device.type == "cuda" and os.environ.get(f"LOCOV_FUSED_{stage}", "1") != "0"

    # -- the draws
    def _caption_choices(self, d: dict):
        return d.get("caption")

    def draw_sample(self, dataset_dicts: Sequence[dict]) -> Dict[str, list]:
        resize = self.augmentations[0]
        flip = self.augmentations[1] if len(self.augmentations) > 1 else None
        sample = {"short_edge": [], "flip": [], "caption": []}
        self._decoded.clear()
        if self.train_aug is not None:
            self._jpeg_stage(dataset_dicts)                        # (the sizes below come from the entropy stage's verdict)
        for d in dataset_dicts:
            sample["short_edge"].append(int(resize.draw(self.rng)))
            sample["flip"].append(bool(flip.draw(self.rng)) if flip is not None else False)
            cap = self._caption_choices(d)
            sample["caption"].append(self.rng.randrange(len(cap)) if self.is_train and isinstance(cap, list) and len(cap) else 0)
            if self.train_aug is not None:
                h, w = self._raw_size(d)
                nh, nw = resize.get_transform(h, w, sample["short_edge"][-1]).output_shape(h, w)
                sample.setdefault("strong", []).append(self.train_aug.draw(self.rng, nh, nw))
        if self.train_aug is not None:
            sample.setdefault("strong", [])
            sample["erase_seed"] = self.rng.getrandbits(62)
        return sample

    def _raw_size(self, d: dict) -> Tuple[int, int]:
        """(h, w) of the image _raw will return: the erasers are drawn for the resized image's size.  A file is DECODED here, once,
        and kept for _raw: whether the black-image fallback applies is known only after the decode (a truncated file has a header),
        and the draws must be for the image the batch will really hold."""
        raw = d.get("image_raw")
        if raw is not None:
            return int(raw.shape[0]), int(raw.shape[1])
        staged = self._decoded.get(d.get("file_name"))
        if isinstance(staged, ops.JpegStaged):                     # (_jpeg_stage: the scan decoded without an anomaly; the record waits for _raw)
            return int(staged.header.height), int(staged.header.width)
        try:
            image = _read_file(d["file_name"], self.image_format)
        except Exception:
            image = None
        if "file_name" in d:
            self._decoded[d["file_name"]] = image
        if image is None:
            return int(d["height"]), int(d["width"])               # (the black image of _raw)
        return int(image.shape[0]), int(image.shape[1])

    # -- JPEG files on a cuda mapper: the scans on host threads, the pixels on the device (ops.decode_jpeg_images' two halves)
    def _jpeg_stage(self, dataset_dicts: Sequence[dict]) -> None:
        """Reads the files of the dicts without "image_raw" that start with FF D8 and are not in self._decoded yet, and
        Huffman-decodes those whose header the device decoder takes, all in one call.  A stream that came through without an
        anomaly is kept in self._decoded as its ops.JpegStaged; every other file is left to _read_file, with Pillow's error
        semantics.  Does nothing unless the mapper is on a cuda device and LOCOV_FUSED_JPEG is not "0"."""
        if not self._on_device("JPEG") or self.image_format not in ops.JPEG_FORMATS:
            return
        names, datas = [], []
        for d in dataset_dicts:
            name = d.get("file_name")
            if d.get("image_raw") is not None or not isinstance(name, str) or name in self._decoded or name in names:
                continue
            try:
                with open(name, "rb") as f:
                    data = f.read(2)
                    if data != b"\xff\xd8":
                        continue
                    data += f.read()
            except OSError:
                continue
            names.append(name)
            datas.append(data)
        headers = [ops.jpeg_parse(data) for data in datas]
        # (sizes at which Pillow itself refuses or warns -- libjpeg's 65 500 a side, Image.MAX_IMAGE_PIXELS -- stay Pillow's to answer)
        take = [i for i, h in enumerate(headers) if h.supported and (self.image_format != "L" or h.ncomp == 1)
                and max(h.width, h.height) <= JPEG_MAX_SIDE and h.width * h.height <= JPEG_MAX_PIXELS]
        staged = ops.jpeg_entropy_stage([datas[i] for i in take], [headers[i] for i in take])
        for i, s in zip(take, staged):
            if s.status == 0:
                self._decoded[names[i]] = s

    def _jpeg_decode(self, dataset_dicts: Sequence[dict]) -> None:
        """The staged streams of the batch's files become HWC uint8 device tensors: one pinned buffer, one upload and one
        ops.jpeg_decode_records call per IMAGE_BATCH_MAX_IMAGES images.  What an earlier draw_sample staged for other dicts is dropped."""
        wanted = {d.get("file_name") for d in dataset_dicts}
        for name in [n for n, v in self._decoded.items() if isinstance(v, ops.JpegStaged) and n not in wanted]:
            del self._decoded[name]
        names = [name for name, v in self._decoded.items() if isinstance(v, ops.JpegStaged)]
        for part in _slices(names):
            batch = ops.jpeg_pack([self._decoded[name] for name in part], pin_memory=True)
            images = ops.jpeg_decode_records(batch.records.to(self.device, non_blocking=True), batch.descs, self.image_format)
            self._decoded.update(zip(part, images))

    # -- one image's host-side part: the raw image, the transforms, the boxes, the caption
    def _raw(self, d: dict):
        raw = d.pop("image_raw", None)
        if raw is not None:
            if not isinstance(raw, torch.Tensor):
                raw = np.asarray(raw)
            if raw.dtype not in (np.uint8, torch.uint8) or raw.ndim != 3:
                raise TypeError(f"image_raw must be uint8 [H, W, C], got {raw.dtype} {tuple(raw.shape)}")
            return raw, True
        try:
            if d.get("file_name") in self._decoded:                                  # (draw_sample read it for its size; None: it failed there)
                image = self._decoded.pop(d["file_name"])
                if image is None:
                    raise OSError("not decoded")
                return image, True
            return _read_file(d["file_name"], self.image_format), True
        except Exception:
            print("Image not loaded {}, replaced by black image".format(d.get("file_name")))
            return np.zeros((d["height"], d["width"], 3), dtype=np.uint8), False

    def _prepare(self, dataset_dict: dict, i: int, sample: Dict[str, list]):
        d = copy.copy(dataset_dict)                                # (the raw image is not copied; the annotations are, below)
        raw, loaded = self._raw(d)
        h, w = int(raw.shape[0]), int(raw.shape[1])
        check_image_size(d, (h, w))
        tfms = [self.augmentations[0].get_transform(h, w, int(sample["short_edge"][i]))]
        nh, nw = tfms[0].output_shape(h, w)
        if len(self.augmentations) > 1:
            tfms.append(self.augmentations[1].get_transform(nh, nw, bool(sample["flip"][i])))
        transforms = TransformList(tfms)
        if "annotations" in d:
            annos = [transform_instance_annotations(copy.deepcopy(obj), transforms, (nh, nw))
                     for obj in d.pop("annotations") if obj.get("iscrowd", 0) == 0]
            for obj in annos:
                obj.pop("segmentation", None)
                obj.pop("keypoints", None)
            d["instances"] = filter_empty_instances(annotations_to_instances(annos, (nh, nw)))
        if isinstance(d.get("caption"), list):
            d["caption"] = d["caption"][int(sample["caption"][i])] if self.is_train else d["caption"][0]
            if not loaded:
                d["caption"] = "A black image."
        return _Prepared(d, raw, transforms, (nh, nw))

    def _chw(self, hwc: np.ndarray) -> torch.Tensor:               # a host HWC image as the CHW tensor on the mapper's device
        return torch.as_tensor(np.ascontiguousarray(hwc.transpose(2, 0, 1))).to(self.device)

    def _host_image(self, p: _Prepared) -> torch.Tensor:
        return self._chw(p.transforms.apply_image(p.raw.cpu().numpy() if isinstance(p.raw, torch.Tensor) else p.raw))

    def map_batch(self, dataset_dicts: Sequence[dict], sample: Optional[Dict[str, list]] = None) -> List[dict]:
        dataset_dicts = list(dataset_dicts)
        sample = self.draw_sample(dataset_dicts) if sample is None else sample
        self._jpeg_stage(dataset_dicts)
        self._jpeg_decode(dataset_dicts)
        prepared = [self._prepare(d, i, sample) for i, d in enumerate(dataset_dicts)]
        self._decoded.clear()
        fused: Dict[int, List[int]] = {}                           # channel count -> the images the kernel takes
        if self._on_device("RESIZE"):
            for i, p in enumerate(prepared):
                C = int(p.raw.shape[2])
                if 1 <= C <= ops.IMAGE_BATCH_MAX_CHANNELS and ops.resize_supported(p.raw.shape[:2], p.size, C):
                    fused.setdefault(C, []).append(i)
        images: Dict[int, torch.Tensor] = {}                       # what the kernel made, by the image's place in the batch
        for idx in fused.values():
            for part in _slices(idx):
                raws = [torch.as_tensor(prepared[i].raw).to(self.device, non_blocking=True) for i in part]
                images.update(zip(part, ops.resize_flip_images(raws, [prepared[i].size for i in part], [prepared[i].flip for i in part])))
        for i, p in enumerate(prepared):
            p.d["image"] = images[i] if i in images else self._host_image(p)
        if self.train_aug is not None:
            self._strong(prepared, sample)
        return self._finish(prepared)

    def erase_noise(self, sample: Dict[str, list]) -> torch.Tensor:
        """The erasers' normal draws of a sample, fp32 [sum of the images' noise_count] on the mapper's device, image after image:
        sample["erase_noise"] when the caller gives it (e.g. copied from another device), else torch.randn from a torch.Generator
        on the device seeded with sample["erase_seed"]."""
        from .strong_augment import noise_count
        total = sum(noise_count(s) for s in sample["strong"])
        given = sample.get("erase_noise")
        if given is not None:
            if given.dtype != torch.float32 or given.dim() != 1 or given.numel() < total:
                raise ValueError(f"sample['erase_noise'] must be fp32 [>= {total}], got {given.dtype} {tuple(given.shape)}")
            return given.to(self.device)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(sample["erase_seed"]))
        return torch.randn(total, generator=gen, device=self.device, dtype=torch.float32)

    def _strong(self, prepared, sample: Dict[str, list]) -> None:
        """The strong augmentation of the batch's "image" entries, after the resize and flip (basic_mappers.py:171-180)."""
        from . import strong_augment as sa
        draws = list(sample["strong"])
        if len(draws) != len(prepared):
            raise ValueError(f"sample['strong'] holds {len(draws)} entries for {len(prepared)} images")
        for s, p in zip(draws, prepared):
            nh, nw = p.size
            if tuple(p.d["image"].shape[1:]) != (nh, nw) or any(e is not None and (e[0] + e[2] > nh or e[1] + e[3] > nw) for e in s["erase"]):
                raise ValueError(f"sample['strong']: an eraser was drawn for another size than the image's {(nh, nw)}")
        noise = self.erase_noise(sample)
        counts = [sa.noise_count(s) for s in draws]
        offsets = [0] + list(np.cumsum(counts)[:-1])
        takes = lambda s, p: p.d["image"].shape[0] == 3 and (not s["blur"] or ops.augment_supported(s["sigma"]))
        fused = [i for i, (s, p) in enumerate(zip(draws, prepared)) if takes(s, p)] if self._on_device("AUGMENT") else []
        images: Dict[int, torch.Tensor] = {}
        for part in _slices(fused):
            images.update(zip(part, ops.augment_images([prepared[i].d["image"] for i in part], [draws[i] for i in part], noise,
                                                       [int(offsets[i]) for i in part])))
        host_noise = None
        for i, p in enumerate(prepared):
            if i not in images:
                host_noise = noise.cpu().numpy() if host_noise is None else host_noise
                hwc = p.d["image"].permute(1, 2, 0).cpu().numpy()
                images[i] = self._chw(sa.apply_host(hwc, draws[i], host_noise[offsets[i]:offsets[i] + counts[i]]))
            p.d["image"] = images[i]

    def __call__(self, dataset_dict: dict, sample: Optional[Dict[str, list]] = None) -> dict:
        return self.map_batch([dataset_dict], sample)[0]

    # -- the proposal side (MODEL.LOAD_OBJ_PROPOSALS)
    def _finish(self, prepared: List[_Prepared]) -> List[dict]:
        if self.proposal_topk is not None:
            self._map_proposals(prepared, as_gt=False)
        return [p.d for p in prepared]

    def _proposal_rows(self, dicts: List[dict]):
        """(rows [R, 5] on the device, first row per image, rows per image) for the dicts, which all carry "proposal_boxes": their
        rows packed into ONE pinned buffer and uploaded once.  None where only the host definition applies."""
        boxes = [np.asarray(d["proposal_boxes"]) for d in dicts]
        logits = [np.asarray(d["proposal_objectness_logits"]) for d in dicts]
        dtypes = {a.dtype for a in boxes + logits}
        if (any(int(d["proposal_bbox_mode"]) != XYXY_ABS for d in dicts) or len(dtypes) != 1
                or getattr(torch, str(next(iter(dtypes))), None) not in ops.PROPOSAL_DTYPES
                or any(b.ndim != 2 or b.shape[1] != 4 or l.shape != b.shape[:1] for b, l in zip(boxes, logits))):
            return None
        counts = [b.shape[0] for b in boxes]
        starts = [0] + list(np.cumsum(counts)[:-1])
        pinned = torch.empty((sum(counts), 5), dtype=getattr(torch, str(boxes[0].dtype)), pin_memory=True)
        view = pinned.numpy()
        for s, n, b, l in zip(starts, counts, boxes, logits):
            view[s:s + n, :4], view[s:s + n, 4] = b, l
        return pinned.to(self.device, non_blocking=True), starts, counts

    def _map_proposals(self, prepared: List[_Prepared], as_gt: bool) -> None:
        """transform_proposals, and with as_gt change_proposals_as_gt behind it, for the dicts that carry proposals; the others are
        left as they are.  On a cuda device both are one launch (ops.map_proposals).  Otherwise -- LOCOV_FUSED_PROPOSALS=0, a CPU
        device, a dtype or box mode the kernel does not take -- the host definition, its result moved to the device."""
        carrying = [p for p in prepared if "proposal_boxes" in p.d]
        if not carrying:
            return
        source = self._proposal_rows([p.d for p in carrying]) if self._on_device("PROPOSALS") else None
        if source is None:
            for p in carrying:
                transform_proposals(p.d, p.size, p.transforms, self.proposal_topk)
                p.d["proposals"] = p.d["proposals"].to(self.device)
                if as_gt:
                    p.d = change_proposals_as_gt(p.d)
            return
        mapped = ops.map_proposals(*source, [p.factors for p in carrying], [p.flip for p in carrying], [p.size for p in carrying],
                                   self.proposal_topk, OBJECTNESS_THR)
        for p, m in zip(carrying, mapped):
            d, size = p.d, tuple(p.size)
            for key in ("proposal_boxes", "proposal_bbox_mode", "proposal_objectness_logits"):
                d.pop(key)
            if as_gt:
                d["gt_obj"] = d.pop("instances")
                d["instances"] = Instances(size, objectness_logits=m.gt_logits, gt_classes=m.gt_classes, gt_boxes=Boxes(m.gt_boxes))
            else:
                d["proposals"] = Instances(size, proposal_boxes=Boxes(m.prop_boxes), objectness_logits=m.prop_logits)


class CocoImageDatasetMapper(DatasetMapper):
    """The reference's CocoImageDatasetMapper (ovr/data/mappers/coco_mappers.py:24-85).  metadata: anything with .get(name) and
    .thing_classes; no catalog is involved.

      * metadata.get("captions_dict"), {image_id: [caption, ...]}: "caption" is a drawn one in training (the draw is part of
        draw_sample, so `sample` replays it) and the first one otherwise; every annotation gains "category" =
        thing_classes[category_id], and "nouns" / "nouns_id" list them.  An image without an entry: "" and two empty lists.
      * metadata.get("object_proposals"), the reference's dict or a ProposalStore built from it: the image's rows become its
        proposals (KeyError for an image without an entry, as there), transform_proposals cuts them at the config's topk and
        change_proposals_as_gt makes the ones above OBJECTNESS_THR the "instances" (gt_classes 1), the annotated boxes "gt_obj",
        and removes "proposals".  With the store on a cuda device both steps are ops.map_proposals' one launch on rows that never
        leave the device; "instances" is on the device, "gt_obj" on the host."""

    def __init__(self, cfg, metadata, is_train: bool = True, device=None, seed: Optional[int] = None, train_aug=None):
        super().__init__(cfg, is_train, device, seed, train_aug)
        self.metadata = metadata
        store = metadata.get("object_proposals")
        if store is not None and not isinstance(store, ProposalStore):
            store = ProposalStore(store, self.device) if len(store) else None
        self.store: Optional[ProposalStore] = store

    def _caption_choices(self, d: dict):
        captions = self.metadata.get("captions_dict")
        return captions.get(d["image_id"]) if captions else d.get("caption")

    def _prepare(self, dataset_dict: dict, i: int, sample: Dict[str, list]):
        d = copy.copy(dataset_dict)
        captions = self.metadata.get("captions_dict")
        if captions:
            if d["image_id"] in captions:
                choices = captions[d["image_id"]]
                d["caption"] = choices[int(sample["caption"][i])] if self.is_train else choices[0]
                d["annotations"] = [dict(ann, category=self.metadata.thing_classes[ann["category_id"]]) for ann in d["annotations"]]
                d["nouns"] = [ann["category"] for ann in d["annotations"]]
                d["nouns_id"] = [ann["category_id"] for ann in d["annotations"]]
            else:
                d["caption"], d["nouns"], d["nouns_id"] = "", [], []
        if self.store is not None and d["image_id"] in self.store:
            rows = self.store[d["image_id"]]
            d["proposal_boxes"], d["proposal_objectness_logits"], d["proposal_bbox_mode"] = rows[:, :4], rows[:, 4], XYXY_ABS
        return super()._prepare(d, i, sample)

    def _proposal_rows(self, dicts: List[dict]):
        store = self.store
        if store is None or store.rows is None or store.rows.device.type != self.device.type or any(d["image_id"] not in store.table for d in dicts):
            return super()._proposal_rows(dicts)
        where = [store.table[d["image_id"]] for d in dicts]
        return store.rows, [s for s, _ in where], [n for _, n in where]

    def _finish(self, prepared: List[_Prepared]) -> List[dict]:
        if self.store is None:
            return super()._finish(prepared)
        rest = [p for p in prepared if self.proposal_topk is None or "proposal_boxes" not in p.d]
        if self.proposal_topk is not None:
            self._map_proposals(prepared, as_gt=True)
        for p in rest:                                             # (nobody made their "proposals": the reference's KeyError)
            p.d = change_proposals_as_gt(p.d)
        return [p.d for p in prepared]


def get_mapper(dataset_name: str, cfg, is_train: bool, metadata=None, device=None, train_aug=None) -> DatasetMapper:
    """ovr/data/mappers/__init__.py:11-35 with the metadata given by the caller: "coco" -> CocoImageDatasetMapper, "lvis" ->
    DatasetMapper; the "vaw" mapper and the noise mapper of every other name are not built.  train_aug: the mappers' argument."""
    if "coco" in dataset_name:
        return CocoImageDatasetMapper(cfg, metadata, is_train, device=device, train_aug=train_aug)
    if "vaw" in dataset_name:
        raise NotImplementedError(f"{dataset_name}: VawImageDatasetMapper is not built (locov_amd.data)")
    if "lvis" in dataset_name:
        return DatasetMapper(cfg, is_train, device=device, train_aug=train_aug)
    raise NotImplementedError(f"{dataset_name}: TextImageDatasetMapperNoise is not built (locov_amd.data)")


def iterate_batches(dataset_dicts: Iterable[dict], mapper: DatasetMapper, batch_size: int) -> Iterator[List[dict]]:
    """The mapped batches of a dataset, in order: inference_on_dataset(model, iterate_batches(dicts, mapper, n), evaluator) runs from
    raw images."""
    batch: List[dict] = []
    for d in dataset_dicts:
        batch.append(d)
        if len(batch) == int(batch_size):
            yield mapper.map_batch(batch)
            batch = []
    if batch:
        yield mapper.map_batch(batch)
