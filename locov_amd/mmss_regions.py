"""The grounding branches' inputs: the whole-image grid and the sampled boxes as region dictionaries, assembled on the device.

Mirrors the two inline blocks of ovr/modeling/meta_arch/distill_prop_mmss_gcnn.py that turn the ROI heads' 4-tuple
(`EmbeddingProposalsRes5ROIHeads.forward`, :249-258) into what `GroundingHead` / `TransformerHead` consume:

    :273-328   input_image   grid_regions(visual_grid_features, images.image_sizes, images.tensor.shape[-2:], SPATIAL_DROPOUT, training)
    :348-399   input_boxes   box_regions(box_features, box_proposals, SPATIAL_DROPOUT, training)

Both return the reference's dictionary -- `region_features`, `region_mask` (uint8), `region_loc`, `mvm_mask` (zeros),
`target_region_features` (the same tensor object as `region_features`) -- with its shapes and dtypes, on the features' device.

The reference builds the masks and cell centres in numpy loops, shuffles with numpy's host RNG, indexes once per image,
pad_sequences and copies three arrays from pageable memory.  Here each branch is one selection launch and one gather launch
(csrc/regions.hip), one scatter launch in backward, and no host wait: everything the host contributes -- the valid extents of
:281-284, the output length, the images' sizes -- is a handful of integers that travel as launch arguments.

Selection.  numpy's shuffle cannot be reproduced draw for draw on the device; as in roi_heads/labelling.py the permutation is
replaced by random keys with the same distribution over subsets: `keys` holds one float per candidate (grid [B, gh*gw], boxes
[R_total]; default torch.rand(..., dtype=float64) under torch's device generator), and slot r of image i receives the valid
candidate with the r-th smallest (key, candidate index) pair.  The result is a deterministic function of `keys`; passing them
explicitly replays a sample.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

__all__ = ["grid_regions", "box_regions", "grid_extents", "grid_output_length", "box_output_length"]


def grid_extents(image_sizes, padded_hw, grid_h: int, grid_w: int) -> np.ndarray:
    """:281-284 verbatim in meaning: the valid (rows, columns) of every image's grid, int32 [B, 2] -- ceil(size * grid / padded) as
    numpy evaluates it on a float32 array."""
    image_h, image_w = int(padded_hw[0]), int(padded_hw[1])
    sizes = np.asarray(image_sizes, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(sizes.shape, dtype=np.int32)
    out[:, 0] = np.ceil(sizes[:, 0] * grid_h / image_h)
    out[:, 1] = np.ceil(sizes[:, 1] * grid_w / image_w)
    return out


def grid_output_length(extents: np.ndarray, spatial_dropout: int) -> int:
    """The length pad_sequence gives the subsampled grid (:309-316): max_i min(SPATIAL_DROPOUT, valid cells of image i)."""
    return int(max(min(int(spatial_dropout), int(h) * int(w)) for h, w in extents))


def box_output_length(lengths: Sequence[int], spatial_dropout: int, training: bool = True) -> int:
    """:349-352: min_i len(box_i), capped at SPATIAL_DROPOUT when that is on and the model trains."""
    n = min(int(x) for x in lengths)
    if spatial_dropout > 0 and training:
        n = min(n, int(spatial_dropout))
    return n


def _dict(features, mask, loc, mvm) -> Dict[str, torch.Tensor]:
    return {"region_features": features, "region_mask": mask, "region_loc": loc, "mvm_mask": mvm, "target_region_features": features}


def grid_regions(visual_grid_features: torch.Tensor, image_sizes, padded_hw, spatial_dropout: int, training: bool = True,
                 keys: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """`input_image` of distill_prop_mmss_gcnn.py:273-328.

    visual_grid_features: logical [B, C, gh, gw] fp32 on the device, NCHW-contiguous (a strided read) or in channels-last memory
    (MODEL.ROI_BOX_HEAD.GRID_FEATURES_LAYOUT "channels_last": contiguous 4 C-byte rows, and a backward whose gradient has the same
    strides).  image_sizes: `ImageList.image_sizes` [(h, w)]; padded_hw: the padded batch's (H, W) (:273).

    spatial_dropout == 0 or not training (:302 not taken): region_features is the flattened [B, gh*gw, C] view of all cells (no
    kernel), region_mask [B, gh*gw] the valid extent (:285-288), region_loc [B, gh*gw, 2] the cell centres ((x + 0.5) / gw_i,
    (y + 0.5) / gh_i), zero outside the extent (:290-299).
    Subsampled (:302-320): region_mask is `new_mask` [B, spatial_dropout]; region_features [B, n, C] / region_loc [B, n, 2] have the
    length pad_sequence yields, n = max_i min(spatial_dropout, valid_i), zero in the padding slots.  n == spatial_dropout whenever
    one image has that many valid cells (every shipped configuration); with smaller grids the mask stays wider than the features,
    exactly as in the reference.  mvm_mask is zeros [B, gh*gw] in both cases (:326).
    keys: [B, gh*gw] (any float dtype, finite), see the module docstring."""
    x = visual_grid_features
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("grid_regions: visual_grid_features must be a [B, C, gh, gw] tensor")
    B, C, gh, gw = x.shape
    if len(image_sizes) != B:
        raise ValueError(f"grid_regions: {len(image_sizes)} image sizes for a batch of {B}")
    ops._dev(x[:0], "visual_grid_features")                                     # device / dtype ("no CPU fallback")
    hw = gh * gw
    ext = grid_extents(image_sizes, padded_hw, gh, gw)
    if (ext[:, 0] > gh).any() or (ext[:, 1] > gw).any() or (ext < 0).any():
        raise ValueError(f"grid_regions: an image size exceeds the padded size {tuple(padded_hw)}")
    if not (spatial_dropout > 0 and training):
        sel = ops.regions_select("grid_all", None, [hw] * B, ext[:, 0], ext[:, 1], hw, hw, hw, hw, grid_w=gw, device=x.device)
        return _dict(x.reshape(B, C, hw).permute(0, 2, 1), sel.mask, sel.loc, sel.mvm)           # :277-279
    if keys is None:
        keys = torch.rand((B, hw), dtype=torch.float64, device=x.device)
    elif tuple(keys.shape) != (B, hw):
        raise ValueError(f"grid_regions: keys must be [{B}, {hw}], got {tuple(keys.shape)}")
    n = grid_output_length(ext, spatial_dropout)
    sel = ops.regions_select("grid", keys.to(torch.float64), [hw] * B, ext[:, 0], ext[:, 1], n, int(spatial_dropout), int(spatial_dropout), hw,
                             grid_w=gw)
    return _dict(ops.regions_gather(x, sel), sel.mask, sel.loc, sel.mvm)


def _one_matrix(box_features, lengths: List[int]) -> torch.Tensor:
    """The [R, C] matrix behind the heads' per-image list: the tensor the list was split from when its entries are consecutive
    views of it (roi_emb_heads.py:529 -- no copy), their concatenation otherwise."""
    if isinstance(box_features, torch.Tensor):
        if box_features.dim() != 2 or box_features.shape[0] != sum(lengths):
            raise ValueError(f"box_regions: box_features must be [{sum(lengths)}, C] for these proposals, got {tuple(box_features.shape)}")
        return box_features
    if len(box_features) != len(lengths) or any(t.dim() != 2 or t.shape[0] != n for t, n in zip(box_features, lengths)):
        raise ValueError("box_regions: box_features must hold one [len(proposals_i), C] tensor per image")
    base = box_features[0]._base
    if base is not None and base.dim() == 2 and base.shape[0] == sum(lengths) and all(t._base is base for t in box_features):
        row = 0
        for t, n in zip(box_features, lengths):
            if t.shape[1] != base.shape[1] or t.stride() != base.stride() or t.storage_offset() != base.storage_offset() + row * base.stride(0):
                break
            row += n
        else:
            return base
    return torch.cat(list(box_features), dim=0)


def box_regions(box_features: Union[torch.Tensor, Sequence[torch.Tensor]], box_proposals, spatial_dropout: int, training: bool = True,
                keys: Optional[torch.Tensor] = None) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """`input_boxes` of distill_prop_mmss_gcnn.py:348-399.

    box_features: the heads' list of [Ri, C] tensors, or one [R, C] tensor whose rows follow the proposals image after image.
    box_proposals: the sampled `Instances` (`proposal_boxes`, `image_size`); their len() is a host integer.
    Every image contributes n = min_i Ri random rows, capped at spatial_dropout when that is on and `training` (:349-352); the rows
    are shuffled in either case (:357-359).  region_mask is ones [B, n] (:391), region_loc the box centres over the image size,
    ((x0 + x1) / 2 / image_w, (y0 + y1) / 2 / image_h) (:368-383), mvm_mask zeros [B, n] (:397).
    Returns (dictionary, indices): indices [B, n] int64 on the device are the rows chosen within each image, so that a caller can
    subsample its Instances the way :360 does (`box[idx]`).  keys: [R_total], see the module docstring."""
    lengths = [len(p) for p in box_proposals]
    B = len(lengths)
    if B == 0:
        raise ValueError("box_regions: no images")
    feats = _one_matrix(box_features, lengths)
    ops._dev(feats[:0], "box_features")
    total = sum(lengths)
    n = box_output_length(lengths, spatial_dropout, training)
    if keys is None:
        keys = torch.rand((total,), dtype=torch.float64, device=feats.device)
    elif keys.numel() != total:
        raise ValueError(f"box_regions: keys must hold {total} values, got {tuple(keys.shape)}")
    sizes = [p.image_size for p in box_proposals]
    boxes = [p.proposal_boxes.tensor for p in box_proposals]
    sel = ops.regions_select("boxes", keys.reshape(-1).to(torch.float64), lengths, [s[0] for s in sizes], [s[1] for s in sizes], n, n, n, n,
                             boxes=boxes)
    return _dict(ops.regions_gather(feats, sel), sel.mask, sel.loc, sel.mvm), sel.indices
