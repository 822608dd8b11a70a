"""Reference for locov_amd.mmss_regions: the two assembly blocks of ovr/modeling/meta_arch/distill_prop_mmss_gcnn.py -- :273-328
(`input_image`, the whole-image grid) and :348-399 (`input_boxes`, the sampled boxes) -- restated in numpy / torch from their
semantics, with the per-image permutation an ARGUMENT instead of np.random.shuffle's draw.

Unlike the vectors of G4-G9 these cannot come from running the reference's own code: the assembly is inline in the 270-line
`forward` of a Detectron2 meta-architecture, and Detectron2 is not installed here.  Nothing below is copied text.

The functions run on whatever device the feature tensors live on (index / pad_sequence / torch.tensor(numpy).to(device), as the
reference's statements do), so the same code is the CPU reference of the bit-identity tests and, on device tensors, the
"torch statement chain" baseline of tools/lsm_region_tail.py and of the end-to-end test.
"""
import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence


def grid_extents(image_sizes, padded_hw, grid_h, grid_w):
    """:281-284: valid (rows, columns) per image, int32 [B, 2], through numpy's float32 array statement."""
    image_h, image_w = padded_hw
    sizes = np.asarray(image_sizes, dtype=np.float32)
    out = np.zeros(sizes.shape, dtype=np.int32)
    out[:, 0] = np.ceil(sizes[:, 0] * grid_h / image_h)
    out[:, 1] = np.ceil(sizes[:, 1] * grid_w / image_w)
    return out


def grid_mask_loc(ext, grid_h, grid_w):
    """:285-299: the uint8 valid-extent mask [B, gh*gw] and the float32 cell centres [B, gh*gw, 2] (zero outside the extent)."""
    B = ext.shape[0]
    mask = np.zeros([B, grid_h, grid_w], dtype=np.uint8)
    loc_x = np.zeros([B, grid_h, grid_w], dtype=np.float32)
    loc_y = np.zeros([B, grid_h, grid_w], dtype=np.float32)
    for i in range(B):
        h, w = ext[i]
        mask[i, :h, :w] = 1
        loc_x[i, :h, :w] = ((np.arange(w, dtype=np.float32) + 0.5) / w)[None, :]
        loc_y[i, :h, :w] = ((np.arange(h, dtype=np.float32) + 0.5) / h)[:, None]
    return mask.reshape(B, -1), np.stack([loc_x, loc_y], axis=-1).reshape(B, grid_h * grid_w, 2)


def grid_perms(keys, ext, grid_w):
    """The permutation the keys stand for: per image the valid cells in the order of a stable argsort of their keys."""
    keys = np.asarray(keys)
    perms = []
    for i in range(keys.shape[0]):
        cells = np.arange(keys.shape[1])
        valid = cells[(cells // grid_w < ext[i, 0]) & (cells % grid_w < ext[i, 1])]
        perms.append(valid[np.argsort(keys[i, valid], kind="stable")])
    return perms


def grid_regions(features, image_sizes, padded_hw, spatial_dropout, training, perms=None):
    """:273-328.  features [B, C, gh, gw] (any device); perms: per image the shuffled valid cells (what np.random.shuffle leaves in
    `idx`, :307-308).  Returns the `input_image` dictionary."""
    B, C, gh, gw = features.shape
    dev = features.device
    flat = features.reshape(B, C, gh * gw).permute(0, 2, 1)
    ext = grid_extents(image_sizes, padded_hw, gh, gw)
    mask, loc = grid_mask_loc(ext, gh, gw)
    loc = torch.tensor(loc).to(dev)
    if spatial_dropout > 0 and training:
        sub_f, sub_l = [], []
        new_mask = np.zeros([B, spatial_dropout], dtype=np.uint8)
        for i in range(B):
            idx = np.asarray(perms[i])
            assert sorted(idx.tolist()) == np.where(mask[i])[0].tolist(), "perms[i] must permute the valid cells"
            idx = idx[:min(spatial_dropout, idx.shape[0])]
            sub_f.append(flat[i, idx])
            sub_l.append(loc[i, idx])
            new_mask[i, :len(idx)] = 1
        flat, loc, mask = pad_sequence(sub_f, batch_first=True), pad_sequence(sub_l, batch_first=True), new_mask
    return {"region_features": flat, "region_mask": torch.tensor(mask).to(dev), "region_loc": loc,
            "mvm_mask": torch.zeros(B, gh * gw).to(dev), "target_region_features": flat}


def box_perms(keys, lengths):
    keys = np.asarray(keys).reshape(-1)
    perms, row = [], 0
    for n in lengths:
        perms.append(np.argsort(keys[row:row + n], kind="stable"))
        row += n
    return perms


def box_regions(box_features, boxes, image_sizes, spatial_dropout, training, perms):
    """:348-399.  box_features: list of [Ri, C]; boxes: list of [Ri, 4] XYXY tensors; image_sizes: each Instances' (h, w); perms:
    per image a permutation of range(Ri) (:357-358).  Returns (`input_boxes`, the chosen rows per image)."""
    B = len(box_features)
    dev = box_features[0].device
    n = min(len(b) for b in boxes)
    if spatial_dropout > 0 and training:
        n = min(n, spatial_dropout)
    feats, locs, chosen = [], [], []
    for f, b, (h, w), p in zip(box_features, boxes, image_sizes, perms):
        assert sorted(np.asarray(p).tolist()) == list(range(len(b)))
        idx = np.asarray(p)[:n]
        chosen.append(idx)
        feats.append(f[idx])
        bb = b[idx]
        centers = (bb[:, :2] + bb[:, 2:]) / 2
        locs.append(torch.stack([centers[:, 0] / w, centers[:, 1] / h], dim=-1))
    flat, loc = pad_sequence(feats, batch_first=True), pad_sequence(locs, batch_first=True)
    return {"region_features": flat, "region_mask": torch.tensor(np.ones([B, n], dtype=np.uint8)).to(dev), "region_loc": loc,
            "mvm_mask": torch.zeros(B, n).to(dev), "target_region_features": flat}, chosen
