"""An independent restatement of the proposal side of the dataset mapper, for tests/test_proposals_host.py: [D2-upstream]
transform_proposals and the reference's change_proposals_as_gt (ovr/data/mappers/coco_mappers.py:88-106) over the Detectron2 stub
tests/stubs/detectron2/structures.py (Boxes.clip, Boxes.nonempty, Instances.__getitem__), loaded by path so that no `detectron2`
enters sys.modules.

Unlike locov_amd/data.py it does not go through Transform objects and corner lists: per axis, with every scalar converted to the
rows' dtype BY HAND (what numpy's promotion does with a Python number beside an array), it multiplies the two ends, orders them with
np.minimum / np.maximum (NaN-propagating, as ndarray.min is) and mirrors them.

Upstream's Boxes.clip asserts that every coordinate is finite, and so does the stub.  The project's definition lets non-finite rows
through as its own Boxes does; for those this module restates the four clamps of the stub's clip without the assertion."""
import importlib.util
import os

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location(
    "proposal_ref_d2_structures", os.path.join(os.path.dirname(os.path.abspath(__file__)), "stubs", "detectron2", "structures.py"))
structures = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(structures)
Boxes, Instances = structures.Boxes, structures.Instances


def _axis(lo_in: np.ndarray, hi_in: np.ndarray, factor: float, mirror_size):
    t = lo_in.dtype.type
    a, b = lo_in * t(factor), hi_in * t(factor)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    if mirror_size is not None:
        a, b = t(mirror_size) - lo, t(mirror_size) - hi
        lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo, hi


def transform_proposals(rows: np.ndarray, hw, new_hw, flip: int, topk: int):
    """rows [n, 5] -> (Instances with proposal_boxes / objectness_logits, the kept rows' numbers)."""
    (h, w), (nh, nw) = hw, (hw if new_hw is None else new_hw)
    fx, fy = (1.0, 1.0) if new_hw is None else (nw * 1.0 / w, nh * 1.0 / h)
    x1, x2 = _axis(rows[:, 0], rows[:, 2], fx, nw if flip == 1 else None)
    y1, y2 = _axis(rows[:, 1], rows[:, 3], fy, nh if flip == 2 else None)
    boxes = Boxes(torch.from_numpy(np.stack([x1, y1, x2, y2], axis=1).astype(np.float32)))
    logits = torch.from_numpy(rows[:, 4].astype(np.float32))
    if bool(torch.isfinite(boxes.tensor).all()):
        boxes.clip((nh, nw))
    else:
        t = boxes.tensor
        boxes = Boxes(torch.stack((t[:, 0].clamp(min=0, max=nw), t[:, 1].clamp(min=0, max=nh), t[:, 2].clamp(min=0, max=nw),
                                   t[:, 3].clamp(min=0, max=nh)), dim=-1))
    keep = boxes.nonempty(threshold=0)
    out = Instances((nh, nw))
    out.proposal_boxes = boxes[keep][:topk]
    out.objectness_logits = logits[keep][:topk]
    return out, torch.nonzero(keep)[:, 0][:topk]


def change_proposals_as_gt(dataset_dict: dict, objectness_thr: float = 0.7) -> dict:
    d = dict(dataset_dict)
    proposals = d.pop("proposals")
    annotated = d.pop("instances")
    chosen = proposals[proposals.get("objectness_logits") > objectness_thr]
    chosen.set("gt_classes", torch.ones(len(chosen), dtype=torch.long))
    chosen.set("gt_boxes", chosen.get("proposal_boxes"))
    chosen.remove("proposal_boxes")
    d["gt_obj"], d["instances"] = annotated, chosen
    return d
