"""COCO-protocol bounding-box AP with seen / unseen AP50 (the reference's CustomCOCOEvaluator, ovr/evaluation/custom_coco_eval.py,
and the public COCOeval with iouType="bbox", useCats=1 it sits on), without pycocotools.

The protocol, as every path below computes it (float64 and integers only, so the paths agree bit for bit):

  * Parameters: iouThrs = linspace(.5, .95, 10), recThrs = linspace(0, 1, 101), maxDets = (1, 10, 100) (any ascending tuple of
    1-3 caps), areaRng = [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10].  Images in ascending image id, categories in ascending
    category id; contiguous class c is the c-th smallest category id.
  * Ground truth: bbox XYWH as float64, area = the annotation's own field, ignore = iscrowd.
  * Detections: fp32 XYXY boxes; XYWH is formed in fp32 (w = x2 - x1, as BoxMode.convert does on the fp32 array), then widened;
    area = w * h in double; scores widened to double.
  * Per (image, category) cell with a gt or a det: the dets stable-sorted by descending score, the first maxDets[-1] kept; IoU in
    double, each step rounded on its own: w = min(dx + dw, gx + gw) - max(dx, gx), h likewise, 0 if w <= 0 or h <= 0, else
    i = w * h, u = crowd ? dw * dh : dw * dh + gw * gh - i, IoU = i / u.
  * Per area range a gt is ignored if it is crowd or its area is outside [lo, hi]; gts are visited non-ignored first (stable).
  * Per threshold t, the dets in order: best = min(t, 1 - 1e-10), m = none; a gt already matched at t and not crowd is skipped; the
    walk stops when m is a non-ignored gt and the next is ignored; a gt with iou >= best becomes m and raises best (equal IoU moves
    to the later gt).  A matched det takes m's ignore flag and marks m; an unmatched det whose own area is outside the range is
    ignored.  (Done here as two passes: the non-ignored gts, then the ignored ones only if the first pass found nothing.)
  * Per (category, range, cap m): each cell's first m dets, concatenated in image order and stable-sorted by descending score;
    npig = the category's non-ignored gts in the range (0: precision, recall and scores stay -1); tp / fp = cumulative counts of
    the non-ignored matched / unmatched dets; rc = tp / npig; pr = tp / (fp + tp + spacing(1)); recall = the last rc (0 with no
    det); pr made non-increasing from the right; for each recThrs[r] the first index with rc >= recThrs[r] gives precision and
    score, 0 for this and every later r once the index runs off the end.
  * The twelve stats (means over the entries > -1, -1 with none, taken with numpy on the host): AP, AP at iouThrs[0] and [5], AP
    small / medium / large, AR at each cap (-1 for a cap that is not configured), AR small / medium / large.
  * Results: the six AP metrics x 100 (nan for -1), AP-<name> per category, and AP50-seen / AP50-unseen: plain means of the
    per-category AP50 x 100 over `seen_names` / `unseen_names` (the reference imports those lists from a file it does not ship;
    nan for an empty list).

Paths (one for both protocols; what LVIS switches is stated under its rules below): the numpy functions of this file are the
definition; they serve CPU tensors, LOCOV_FUSED_COCOEVAL=0 (A/B runs, like LOCOV_FUSED_ATTENTION) and sizes beyond the kernels'
limits.  Device tensors take _evaluate_device: ops.coco_order / coco_match / coco_accumulate (csrc/coco_eval.hip) with one
device-to-host copy, of the result arrays.  COCOEvaluator.evaluate() chooses between the two; a protocol is three hooks of the
evaluator (its host function, its device function, its derive_results).  The evaluator scores what its own process saw.

LVIS-protocol box AP with APr / APc / APf (the public lvis-api's LVISEval and LVISResults, and Detectron2's LVISEvaluator, which
the reference's select_and_build_evaluator returns for every dataset whose name contains "lvis": ovr/evaluation/evaluator.py:39-50),
without lvis-api.  LVIS is federated: an image is annotated exhaustively for a few categories only.  The protocol, float64 and
integers again:

  * Parameters: iou_thrs, rec_thrs and the four area ranges as above; one cap, max_dets_per_image = 300.  Images and categories in
    ascending id; contiguous class c is the c-th smallest category id.
  * Ground truth: bbox XYWH as float64, area = the annotation's own field, ignore = its `ignore` field (0 when absent); there is
    no crowd notion and iscrowd is not read.  Per image neg_category_ids and not_exhaustive_category_ids (empty when absent); per
    category frequency "r" / "c" / "f" (a category without the field belongs to no group).
  * Detections: as above.  A det whose class is outside [0, K) is left out before anything else.
  * The cap (LVISResults.limit_dets_per_image): an image with more than max_dets_per_image dets keeps the first max_dets_per_image
    of a stable sort by descending score (ties in input order), over all its categories together.
  * The federated filter: a det of (image i, category k) takes part only if k has a gt in i or k is in i's neg_category_ids; any
    other det is dropped, neither a true nor a false positive.
  * Per cell and area range: a gt is ignored if its ignore is set or its area is outside [lo, hi]; gts are visited non-ignored
    first (stable); IoU is the non-crowd formula for every gt.  Per threshold t, the dets in descending score (ties in the order the
    cap left, which is input order): best = min(t, 1 - 1e-10); a gt already matched at t is skipped, so an ignored gt is taken once
    only; the walk stops when the match is a non-ignored gt and the next is ignored; a gt with iou >= best becomes the match and
    raises best (equal IoU moves to the later gt).  A matched det takes its gt's ignore flag; an unmatched det is ignored if its
    own area is outside the range or its category is in the image's not_exhaustive_category_ids.
  * Accumulate: the COCO one above with the one cap and no scores; num_gt = the category's non-ignored gts over all images.
    -> precision [T, R, K, A], recall [T, K, A], -1 where num_gt == 0.
  * The thirteen stats: AP, AP50 (iou_thrs[0]), AP75 (iou_thrs[5]), APs, APm, APl; APr, APc, APf = precision[:, :, group, 0] over
    the category ranks of each frequency group; AR@cap, ARs, ARm, ARl.  Each the mean over the entries > -1, -1 with none.
  * Results: the nine AP metrics x 100 with no special case, as Detectron2 does (-1 becomes -100.0); all nan when nothing was
    processed.
  * Stated differences (COCO's too): a gt with id 0 counts as a match like any other (LVISEval reads a stored id 0 as
    "unmatched"); an image id absent from the ground truth raises in process().

Paths: the same two, switched as the kernel's template parameter is.  On the host _match_host is the one matching loop; under LVIS
it takes the gt's `ignore` as the flag of the ignore test, an all-false crowd (so no crowd union and no second taking of a matched
gt) and the cells' flags; evaluate_host_lvis drops the unlisted dets literally before it.  On the device _evaluate_device first
runs ops.lvis_limit (the cap: two stable integer-key sorts and the in-image position; a det past the cap goes to the trailing
cell), calls ops.lvis_match in place of ops.coco_match (the match kernel's other instantiation, which writes the dets of an unlisted
cell as ignored: the accumulation passes over an ignored det, so precision and recall do not move) and ops.coco_accumulate without
scores, and summarises precision [T, R, K, A] with the thirteen stats.

Class-agnostic proposal recall, AR@100 / AR@1000 with ARs / ARm / ARl (the public Detectron2's _evaluate_box_proposals and
COCOEvaluator._eval_box_proposals, which both evaluators above report as "box_proposals" for outputs that hold
{"proposals": Instances(proposal_boxes, objectness_logits)}; the reference has none of it).  The protocol, fp32 rounded step by
step and integers:

  * Parameters: limits (100, 1000); the four area ranges above; thresholds = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=fp32),
    formed once on the CPU: its ten fp32 values are what every path compares against.
  * Ground truth of an image: every annotation of the image, whatever its category, in the order of the annotation file; COCO
    takes those with iscrowd == 0, LVIS all of them.  Box = fp32(x), fp32(y), fp32(x + w), fp32(y + h), the sums taken in double
    (BoxMode.convert on Python floats, then torch.as_tensor); area = the annotation's own field rounded to fp32.  A gt is in a
    range if lo <= area <= hi in fp32 (an area of exactly 1024 is small and medium).
  * Proposals of an image: stable-sorted by descending objectness_logits, ties in input order (upstream's sort is unstable: a
    stated difference), the first `limit` kept.  The boxes are finite.
  * Per (image, range, limit): an image with no gt before the area filter, or with no proposal, is skipped entirely.  Otherwise
    num_pos += the gts in the range (so an image with gts and no proposal adds nothing: upstream's behaviour).  IoU in fp32 =
    structures.pairwise_iou = csrc/select_common.h's box_pairwise_iou, each step rounded on its own.  min(P, G) times: among the
    unused proposals x unused gts the largest IoU, ties to the lowest gt, then to the lowest proposal rank; that IoU is the step's
    overlap and both are used from then on.  The maxima never rise, so from the first step whose maximum is 0 every overlap is 0;
    the remaining entries of the image's G overlaps are 0.  (Upstream's literal overlaps.max(dim=0) / max_overlaps.max(dim=0) /
    -1 marking loop gives the same overlaps: tests/proposal_recall_ref.py restates it.)
  * Totals: count[a, l, t] = the overlaps >= thresholds[t], an integer; recalls = count.float() / float(num_pos) and ar =
    recalls.mean(), formed on the host with the same torch CPU expressions on every path; NaN when num_pos == 0.
  * Results: "AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", ... in that order, each float(ar.item() * 100).

Paths: proposal_recall_host is the definition (CPU tensors, LOCOV_FUSED_COCOEVAL=0, sizes beyond the kernel's limits).  Device
tensors take proposal_recall_device: ops.proposal_recall (two stable integer sorts, csrc/proposal_recall.hip's one launch, an
integer sum over the images) with one device-to-host copy, of the totals.  evaluate() adds "box_proposals" behind "bbox" if, and
only if, process() saw a "proposals" output; evaluator.proposal_eval keeps counts, num_pos, recalls and ar.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

__all__ = ["COCOEvaluator", "LVISEvaluator", "build_evaluator", "inference_on_dataset", "IOU_THRS", "REC_THRS", "AREA_RNG",
           "proposal_recall_host", "PROPOSAL_LIMITS", "PROPOSAL_THRS"]

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0., 1., 101)
AREA_RNG = np.array([[0., 1e10], [0., 32. ** 2], [32. ** 2, 96. ** 2], [96. ** 2, 1e10]], dtype=np.float64)
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")


def _fused() -> bool:
    return os.environ.get("LOCOV_FUSED_COCOEVAL", "1") != "0"


class _GroundTruth:
    """The annotations in cell order (cell = category rank * n_images + image rank; inside a cell, dataset order)."""

    def __init__(self, gt):
        if isinstance(gt, (str, os.PathLike)):
            with open(gt) as f:
                gt = json.load(f)
        cats = sorted(gt["categories"], key=lambda c: c["id"])
        self.cat_ids = [c["id"] for c in cats]
        self.cat_names = [c.get("name", str(c["id"])) for c in cats]
        self.image_ids = sorted({im["id"] for im in gt["images"]})
        self.image_rank = {iid: r for r, iid in enumerate(self.image_ids)}
        cat_rank = {cid: r for r, cid in enumerate(self.cat_ids)}
        I, K = len(self.image_ids), len(self.cat_ids)
        anns = [a for a in gt.get("annotations", ()) if a["image_id"] in self.image_rank and a["category_id"] in cat_rank]
        cell = np.array([cat_rank[a["category_id"]] * I + self.image_rank[a["image_id"]] for a in anns], dtype=np.int64)
        order = np.argsort(cell, kind="stable")
        anns, cell = [anns[i] for i in order], cell[order]
        self.n_images, self.n_categories, self.n_cells = I, K, I * K
        self.box = np.array([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        self.area = np.array([a["area"] for a in anns], dtype=np.float64)
        self.crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in anns], dtype=np.uint8)
        self.offsets = np.searchsorted(cell, np.arange(I * K + 1, dtype=np.int64), side="left").astype(np.int32)
        self.cat_offsets = self.offsets[::I].astype(np.int64) if I else np.zeros(K + 1, dtype=np.int64)   # [K + 1]
        self._read_more(gt, cats, cat_rank, anns)
        self._device = {}
        self._annotations = gt.get("annotations", ())                                          # (the loaded list itself: image_index reads it)
        self._image_index = None

    _uploaded = ("box", "area", "crowd", "offsets", "cat_offsets")                             # what on() copies to the device
    _uploaded_by_image = ("image_offsets", "image_box", "image_area", "image_skip")            # ... and with by_image, once asked for
    proposals_skip_crowd = True                                                                # COCO's proposal recall leaves crowd gts out

    def _read_more(self, gt, cats, cat_rank, anns):
        """What a protocol reads beyond the arrays above, from the loaded dict, its categories in ascending id, their ranks and the
        annotations in cell order (_LVISGroundTruth's fields)."""

    def image_index(self):
        """The annotations by image, for the proposal recall (module docstring): every annotation of an image of the ground truth,
        whatever its category, in the order of the annotation file.  Built on the first call, so a user who never feeds proposals
        pays nothing.  -> dict(offsets int32 [I + 1] (CSR by image rank), box fp32 [G, 4] XYXY (x + w and y + h summed in double,
        then rounded once), area fp32 [G] (the annotation's own field), crowd uint8 [G], skip uint8 [G] or None (the gts the
        protocol leaves out: crowd under COCO, none under LVIS), max_per_image)."""
        if self._image_index is None:
            anns = [a for a in self._annotations if a["image_id"] in self.image_rank]
            rank = np.array([self.image_rank[a["image_id"]] for a in anns], dtype=np.int64)
            order = np.argsort(rank, kind="stable")
            anns, rank = [anns[i] for i in order], rank[order]
            xywh = np.array([[float(v) for v in a["bbox"]] for a in anns], dtype=np.float64).reshape(-1, 4)
            box = np.stack([xywh[:, 0], xywh[:, 1], xywh[:, 0] + xywh[:, 2], xywh[:, 1] + xywh[:, 3]], axis=1).astype(np.float32)
            crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in anns], dtype=np.uint8)
            offsets = np.searchsorted(rank, np.arange(self.n_images + 1, dtype=np.int64), side="left").astype(np.int32)
            self._image_index = dict(offsets=offsets, box=box, area=np.array([a["area"] for a in anns], dtype=np.float64).astype(np.float32),
                                     crowd=crowd, skip=crowd if self.proposals_skip_crowd else None,
                                     max_per_image=int(np.diff(offsets.astype(np.int64)).max()) if self.n_images else 0)
        return self._image_index

    def on(self, device, by_image: bool = False):
        """The device copies of the arrays, made once per device; by_image: image_index()'s arrays too, as image_offsets, image_box,
        image_area and image_skip (None where the protocol leaves no gt out)."""
        d = self._device.get(device)
        if d is None:
            d = self._device[device] = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device) for k in self._uploaded}
        if by_image and "image_offsets" not in d:
            index = self.image_index()
            for k in self._uploaded_by_image:
                v = index[k[len("image_"):]]
                d[k] = torch.from_numpy(np.ascontiguousarray(v)).to(device) if v is not None else None
        return d


# ---- the host path: numpy, float64; the definition ------------------------------------------------------------------------------
def order_host(img_rank, cls, score, n_images, n_categories):
    """The two orderings of the dets.  Cell order: (cell, descending score, input order); accumulate order: (category, descending
    score, image rank, in-cell rank).  A class outside [0, K) goes to a trailing cell nothing reads.
    -> perm (input index per cell-order slot), det_offsets int32 [C + 1], rank (in-cell), acc_index (cell-order slot per
    accumulate-order slot), cat_offsets int32 [K + 1]."""
    I, K = n_images, n_categories
    C = I * K
    cell = np.where((cls >= 0) & (cls < K), cls * I + img_rank, C).astype(np.int64)
    p1 = np.argsort(-score, kind="stable")
    perm = p1[np.argsort(cell[p1], kind="stable")]
    cell = cell[perm]
    det_offsets = np.searchsorted(cell, np.arange(C + 1, dtype=np.int64), side="left").astype(np.int32)
    rank = (np.arange(len(cell), dtype=np.int64) - det_offsets[cell]).astype(np.int32)
    pa = np.argsort(-score[perm], kind="stable")
    cat = np.minimum(cell // max(I, 1), K)
    acc_index = pa[np.argsort(cat[pa], kind="stable")].astype(np.int32)
    cat_offsets = np.searchsorted(cat[acc_index], np.arange(K + 1, dtype=np.int64), side="left").astype(np.int32)
    return perm, det_offsets, rank, acc_index, cat_offsets


def _match_host(gt: _GroundTruth, flag, flag_is_crowd, cell_flags, det_offsets, boxes, max_det, area_rng, iou_thrs):
    """The matching of both protocols, with the switches csrc/coco_eval.hip's header lists.  flag uint8 [G]: the gt's own ignore
    flag (iscrowd, or LVIS's ignore).  flag_is_crowd: the flag also selects the crowd union and lets a matched gt be taken again.
    cell_flags uint8 [C] or None: the federated lists; None: every det is listed and no cell is not-exhaustive.
    -> det_bits uint8 [N, A * T] (bit 0 matched, bit 1 ignored), gt_ignore uint8 [A, G], listed bool [N]."""
    A, T = len(area_rng), len(iou_thrs)
    lo, hi = area_rng[:, 0], area_rng[:, 1]
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    dw = (boxes[:, 2] - boxes[:, 0]).astype(np.float64)                       # fp32 differences, then widened
    dh = (boxes[:, 3] - boxes[:, 1]).astype(np.float64)
    dx, dy = boxes[:, 0].astype(np.float64), boxes[:, 1].astype(np.float64)
    darea = dw * dh
    gt_ignore = ((flag[None, :] != 0) | (gt.area[None, :] < lo[:, None]) | (gt.area[None, :] > hi[:, None]))
    all_crowd = flag != 0 if flag_is_crowd else np.zeros(len(flag), dtype=bool)
    counts = np.diff(det_offsets.astype(np.int64))
    gcount = np.diff(gt.offsets.astype(np.int64))
    n_listed = int(det_offsets[-1])                                                            # (the rest: classes outside the bank)
    in_cell = np.arange(n_listed, dtype=np.int64) - np.repeat(det_offsets[:-1].astype(np.int64), counts)
    listed, nel = np.ones(len(boxes), dtype=bool), np.zeros(len(boxes), dtype=bool)
    if cell_flags is not None:
        cell_of = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
        listed[:n_listed] = (gcount[cell_of] > 0) | ((cell_flags[cell_of] & _lib.LVIS_CELL_NEG) != 0)
        listed[n_listed:] = False
        nel[:n_listed] = (cell_flags[cell_of] & _lib.LVIS_CELL_NOT_EXHAUSTIVE) != 0
    det_out = (darea[:, None] < lo[None, :]) | (darea[:, None] > hi[None, :]) | nel[:, None]   # [N, A]: an unmatched det is ignored
    bits = np.repeat(det_out.astype(np.uint8) * 2, T, axis=1)
    bits[~listed] = 0                                                                          # unlisted: no part, bits 0
    bits[:n_listed][in_cell >= max_det] = 0                                                    # past the cap: no part, bits 0
    start = np.minimum(iou_thrs, 1 - 1e-10)
    for c in np.nonzero((counts > 0) & (gcount > 0))[0]:
        d0, g0, G = int(det_offsets[c]), int(gt.offsets[c]), int(gcount[c])
        D = min(int(counts[c]), max_det)
        gb, crowd = gt.box[g0:g0 + G], all_crowd[g0:g0 + G]
        sl = slice(d0, d0 + D)
        w = np.minimum((dx[sl] + dw[sl])[:, None], (gb[:, 0] + gb[:, 2])[None, :]) - np.maximum(dx[sl][:, None], gb[None, :, 0])
        h = np.minimum((dy[sl] + dh[sl])[:, None], (gb[:, 1] + gb[:, 3])[None, :]) - np.maximum(dy[sl][:, None], gb[None, :, 1])
        inter = w * h
        da = np.broadcast_to(darea[sl][:, None], inter.shape)
        union = np.where(crowd[None, :], da, da + (gb[:, 2] * gb[:, 3])[None, :] - inter)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = np.where((w > 0) & (h > 0), inter / union, 0.0)
        gig = gt_ignore[:, g0:g0 + G]                                                          # [A, G]
        gtm = np.zeros((A, T, G), dtype=bool)
        ai, ti = np.meshgrid(np.arange(A), np.arange(T), indexing="ij")
        for d in range(D):
            best = np.broadcast_to(start[None, :], (A, T)).copy()
            m = np.full((A, T), -1, dtype=np.int64)
            for g in range(G):                                                                 # the gts not ignored in the range
                ok = ~gig[:, g, None] & ~gtm[:, :, g] & (iou[d, g] >= best)
                best[ok] = iou[d, g]
                m[ok] = g
            second = m < 0
            for g in range(G):                                                                 # nothing there: the ignored gts (a
                ok = second & gig[:, g, None] & ~(gtm[:, :, g] & ~crowd[g]) & (iou[d, g] >= best)   # crowd one again and again)
                best[ok] = iou[d, g]
                m[ok] = g
            matched = m >= 0
            gtm[ai[matched], ti[matched], m[matched]] = True
            ign = np.where(matched, second, det_out[d0 + d][:, None])
            bits[d0 + d] = (matched.astype(np.uint8) | (ign.astype(np.uint8) << 1)).reshape(-1)
    return bits, gt_ignore.astype(np.uint8), listed


def match_host(gt: _GroundTruth, det_offsets, boxes, max_det, area_rng=AREA_RNG, iou_thrs=IOU_THRS):
    """boxes: fp32 XYXY in cell order.  -> det_bits uint8 [N, A * T] (bit 0 matched, bit 1 ignored), gt_ignore uint8 [A, G]."""
    return _match_host(gt, gt.crowd, True, None, det_offsets, boxes, max_det, area_rng, iou_thrs)[:2]


def npig_host(gt: _GroundTruth, gt_ignore):
    """int32 [K, A]: the category's gts that are not ignored in the range."""
    c = np.concatenate([np.zeros((gt_ignore.shape[0], 1), dtype=np.int64), np.cumsum(gt_ignore == 0, axis=1)], axis=1)
    return (c[:, gt.cat_offsets[1:]] - c[:, gt.cat_offsets[:-1]]).T.astype(np.int32)


def npig_device(cat_offsets: torch.Tensor, gt_ignore: torch.Tensor) -> torch.Tensor:
    """npig_host on device tensors (cat_offsets: _GroundTruth.on()'s int64 [K + 1]), without a host read."""
    c = torch.cat([torch.zeros((gt_ignore.shape[0], 1), dtype=torch.int64, device=gt_ignore.device), torch.cumsum(gt_ignore == 0, dim=1)],
                  dim=1)
    return (c[:, cat_offsets[1:]] - c[:, cat_offsets[:-1]]).t().contiguous().to(torch.int32)


def accumulate_host(cat_offsets, acc_index, acc_rank, acc_score, det_bits, npig, max_dets, n_thresholds, rec_thrs=REC_THRS):
    """-> precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M]; acc_rank / acc_score in accumulate order."""
    K, A = npig.shape
    T, R, M = n_thresholds, len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        n0, n1 = int(cat_offsets[k]), int(cat_offsets[k + 1])
        if not npig[k].any():
            continue
        for m, cap in enumerate(max_dets):
            sel = np.nonzero(acc_rank[n0:n1] < cap)[0] + n0
            b = det_bits[acc_index[sel]].reshape(len(sel), A, T)
            sc = acc_score[sel]
            tps = np.cumsum(b == 1, axis=0).astype(np.float64)
            fps = np.cumsum(b == 0, axis=0).astype(np.float64)
            nd = len(sel)
            for a in range(A):
                if npig[k, a] == 0:
                    continue
                rc = tps[:, a] / int(npig[k, a])
                pr = tps[:, a] / (fps[:, a] + tps[:, a] + np.spacing(1))
                recall[:, k, a, m] = rc[-1] if nd else 0
                pr = np.maximum.accumulate(pr[::-1], axis=0)[::-1]
                for t in range(T):
                    inds = np.searchsorted(rc[:, t], rec_thrs, side="left")
                    ok = inds < nd
                    q, ss = np.zeros(R), np.zeros(R)
                    q[ok] = pr[inds[ok], t]
                    ss[ok] = sc[inds[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return precision, recall, scores


def _mean(s):
    """The mean over the entries > -1, -1 with none."""
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def summarize(precision, recall):
    """COCOeval.summarize's twelve numbers.  AP and the area ARs use the last cap; a cap that is not configured gives -1."""
    M = precision.shape[-1]
    stats = np.full(12, -1.0)
    stats[0] = _mean(precision[:, :, :, 0, M - 1])
    stats[1] = _mean(precision[0, :, :, 0, M - 1])
    if precision.shape[0] > 5:
        stats[2] = _mean(precision[5, :, :, 0, M - 1])
    for i in range(1, min(4, precision.shape[3])):
        stats[2 + i] = _mean(precision[:, :, :, i, M - 1])
        stats[8 + i] = _mean(recall[:, :, i, M - 1])
    for m in range(M):
        stats[6 + m] = _mean(recall[:, :, 0, m])
    return stats


def derive_results(ev, class_names, seen_names=(), unseen_names=()):
    """CustomCOCOEvaluator._derive_coco_results (custom_coco_eval.py:30-137) on {"precision", "stats"}; ev None: nothing was processed."""
    if ev is None:
        return {metric: float("nan") for metric in METRICS}
    stats = ev["stats"]
    results = {metric: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, metric in enumerate(METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    precisions = ev["precision"]
    assert len(class_names) == precisions.shape[2], "one class name per category"
    seen, unseen = set(seen_names), set(unseen_names)
    per_cat, ap50_seen, ap50_unseen = [], [], []
    for idx, name in enumerate(class_names):
        p = precisions[:, :, idx, 0, -1]
        p = p[p > -1]
        per_cat.append((str(name), float(np.mean(p) * 100) if p.size else float("nan")))
        p50 = precisions[0, :, idx, 0, -1]
        p50 = p50[p50 > -1]
        ap50 = float(np.mean(p50) * 100) if p50.size else float("nan")
        if name in seen:
            ap50_seen.append(ap50)
        if name in unseen:
            ap50_unseen.append(ap50)
    results.update({"AP-" + name: ap for name, ap in per_cat})
    results["AP50-seen"] = sum(ap50_seen) / len(ap50_seen) if ap50_seen else float("nan")
    results["AP50-unseen"] = sum(ap50_unseen) / len(ap50_unseen) if ap50_unseen else float("nan")
    return results


def evaluate_host(gt: _GroundTruth, img_rank, cls, score, boxes, max_dets):
    """The whole protocol on numpy arrays -> {"precision", "recall", "scores", "stats"}."""
    img_rank, cls = np.asarray(img_rank, dtype=np.int64), np.asarray(cls, dtype=np.int64)
    score = np.asarray(score).astype(np.float64)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    perm, det_offsets, rank, acc_index, cat_offsets = order_host(img_rank, cls, score, gt.n_images, gt.n_categories)
    bits, gt_ignore = match_host(gt, det_offsets, boxes[perm], max_dets[-1])
    score_c = score[perm]
    precision, recall, scores = accumulate_host(cat_offsets, acc_index, rank[acc_index], score_c[acc_index], bits,
                                                npig_host(gt, gt_ignore), max_dets, len(IOU_THRS))
    return dict(precision=precision, recall=recall, scores=scores, stats=summarize(precision, recall))


# ---- the device path ------------------------------------------------------------------------------------------------------------
def device_supported(gt: _GroundTruth, n_det: int, max_dets) -> bool:
    """Sizes inside the kernels' stated limits (beyond them locov_coco_* answer LOCOV_ERR_UNSUPPORTED: the host path is taken)."""
    blocks = gt.n_categories * len(AREA_RNG) * len(max_dets) * len(IOU_THRS)
    return (max_dets[-1] <= _lib.COCO_MAX_DET and gt.n_cells <= 4 * _lib.COCO_MAX_BLOCKS and blocks <= _lib.COCO_MAX_BLOCKS
            and n_det < 2 ** 31 - 1 and len(gt.area) < 2 ** 31 - 1 and gt.n_cells > 0)


def _evaluate_device(gt: _GroundTruth, img_rank, cls, score, boxes, max_dets, lvis, mark=None):
    """The device path of both protocols; `lvis` switches the cap step, the match wrapper, the scores and the result's shape.
    mark: called with each step's name after the step (tools/time_evaluation.py synchronises there); None: nothing extra."""
    from . import ops
    step = mark if mark is not None else (lambda name: None)
    g = gt.on(boxes.device)
    K, A, T, R, M = gt.n_categories, len(AREA_RNG), len(IOU_THRS), len(REC_THRS), len(max_dets)
    if lvis:
        cls = ops.lvis_limit(img_rank, cls, score, gt.n_images, K, max_dets[-1])
        step("cap")
    o = ops.coco_order(img_rank, cls, score, boxes, gt.n_images, K)
    step("orderings")
    if lvis:
        bits, gt_ignore = ops.lvis_match(o.det_offsets, g["offsets"], g["cell_flags"], o.boxes, g["box"], g["area"], g["ignore"], AREA_RNG,
                                         IOU_THRS, max_dets[-1])
    else:
        bits, gt_ignore = ops.coco_match(o.det_offsets, g["offsets"], o.boxes, g["box"], g["area"], g["crowd"], AREA_RNG, IOU_THRS,
                                         max_dets[-1])
    step("match")
    npig = npig_device(g["cat_offsets"], gt_ignore)
    step("npig")
    flat = ops.coco_accumulate(o.cat_offsets, o.acc_index, o.acc_rank, o.acc_score, bits, npig, T, max_dets, REC_THRS, with_scores=not lvis)
    step("accumulate")
    host = flat.cpu().numpy()                                                  # the one device-to-host copy
    n = T * R * K * A * M
    if lvis:
        step("copy")
        precision, recall = host[:n].reshape(T, R, K, A), host[n:].reshape(T, K, A)
        ev = dict(precision=precision, recall=recall, stats=summarize_lvis(precision, recall, gt.freq_groups))
        step("means")
    else:
        precision, scores = host[:n].reshape(T, R, K, A, M), host[n:2 * n].reshape(T, R, K, A, M)
        recall = host[2 * n:].reshape(T, K, A, M)
        ev = dict(precision=precision, recall=recall, scores=scores, stats=summarize(precision, recall))
        step("copy_and_means")
    return ev


def evaluate_device(gt: _GroundTruth, img_rank, cls, score, boxes, max_dets, mark=None):
    """The same on device tensors: orderings by stable integer sorts, two kernel launches, one copy to the host."""
    return _evaluate_device(gt, img_rank, cls, score, boxes, max_dets, False, mark)


# ---- class-agnostic proposal recall (module docstring) ------------------------------------------------------------------------------
PROPOSAL_LIMITS = (100, 1000)
PROPOSAL_AREA_NAMES = ("", "s", "m", "l")                                                      # AR, ARs, ARm, ARl: AREA_RNG's rows
PROPOSAL_AREA_RNG = AREA_RNG.astype(np.float32)
PROPOSAL_THRS = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32).numpy()              # formed once, on the CPU


def proposal_order_host(img_rank, logits):
    """int64 [N]: the proposals by image rank, inside an image by descending objectness, ties in input order."""
    p = np.argsort(-np.asarray(logits, dtype=np.float64), kind="stable")
    return p[np.argsort(np.asarray(img_rank, dtype=np.int64)[p], kind="stable")]


def proposal_recall_host(index, img_rank, logits, boxes, limits=PROPOSAL_LIMITS, area_rng=PROPOSAL_AREA_RNG, thrs=PROPOSAL_THRS):
    """The definition of the proposal recall.  index: _GroundTruth.image_index(); img_rank int64 [N], logits [N], boxes fp32 [N, 4]
    XYXY: the proposals of every processed image, in any order.
    -> dict(counts int64 [A, L, T], num_pos int64 [A, L], gt_overlaps fp32 [A * L, G]: per (range, limit) row, in each image's gt
    segment, the steps' overlaps in match order, then zeros)."""
    from .structures import Boxes, pairwise_iou
    img_rank = np.asarray(img_rank, dtype=np.int64)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    area_rng, thrs = np.asarray(area_rng, dtype=np.float32).reshape(-1, 2), np.asarray(thrs, dtype=np.float32)
    A, L, T = len(area_rng), len(limits), len(thrs)
    perm = proposal_order_host(img_rank, logits)
    img_rank, boxes = img_rank[perm], boxes[perm]
    offsets, gt_box, gt_area, skip = index["offsets"], index["box"], index["area"], index["skip"]
    counted = np.ones(len(gt_area), dtype=bool) if skip is None else skip == 0
    overlaps = np.zeros((A * L, len(gt_area)), dtype=np.float32)
    counts, num_pos = np.zeros((A, L, T), dtype=np.int64), np.zeros((A, L), dtype=np.int64)
    images, first = np.unique(img_rank, return_index=True)
    last = np.append(first[1:], len(img_rank))
    for i, p0, p1 in zip(images, first, last):                                                 # (an image with no proposal is not here)
        g0, g1 = int(offsets[i]), int(offsets[i + 1])
        if not counted[g0:g1].any():
            continue                                                                           # no gt before the area filter: skipped
        for a in range(A):
            cols = np.nonzero(counted[g0:g1] & (gt_area[g0:g1] >= area_rng[a, 0]) & (gt_area[g0:g1] <= area_rng[a, 1]))[0]
            num_pos[a] += len(cols)
            if len(cols) == 0:
                continue
            full = pairwise_iou(Boxes(torch.from_numpy(gt_box[g0:g1][cols])), Boxes(torch.from_numpy(boxes[p0:p1]))).numpy()
            for l, limit in enumerate(limits):
                iou = full[:, :limit].copy()                                                   # [gts in the range, first `limit` proposals]
                row = overlaps[a * L + l]
                for step in range(min(iou.shape)):
                    g, p = np.unravel_index(np.argmax(iou), iou.shape)                         # (the first maximum: lowest gt, then lowest proposal)
                    v = iou[g, p]
                    if not v > 0:
                        break                                                                  # the maxima never rise: the rest stay 0
                    row[g0 + step] = v
                    iou[g, :] = -1
                    iou[:, p] = -1
                counts[a, l] += (row[g0:g1, None] >= thrs[None, :]).sum(axis=0)
    return dict(counts=counts, num_pos=num_pos, gt_overlaps=overlaps)


def proposal_totals(counts, num_pos):
    """recalls and AR from the integer totals, with the torch CPU expressions every path shares: recalls = counts.float() /
    float(num_pos), ar = recalls.mean(); NaN where num_pos == 0.
    -> dict(counts int64 [A, L, T], num_pos int64 [A, L], recalls fp32 [A, L, T], ar fp32 [A, L])."""
    counts, num_pos = np.asarray(counts, dtype=np.int64), np.asarray(num_pos, dtype=np.int64)
    A, L, T = counts.shape
    recalls, ar = np.zeros((A, L, T), dtype=np.float32), np.zeros((A, L), dtype=np.float32)
    for a in range(A):
        for l in range(L):
            r = torch.from_numpy(counts[a, l]).float() / float(num_pos[a, l]) if num_pos[a, l] else torch.full((T,), float("nan"))
            recalls[a, l], ar[a, l] = r.numpy(), r.mean().item()
    return dict(counts=counts, num_pos=num_pos, recalls=recalls, ar=ar)


def derive_proposal_results(ev, limits=PROPOSAL_LIMITS):
    """AR@100, ARs@100, ARm@100, ARl@100, AR@1000, ... from proposal_totals' dict."""
    return OrderedDict((f"AR{name}@{limit}", float(ev["ar"][a, l].item() * 100)) for l, limit in enumerate(limits)
                       for a, name in enumerate(PROPOSAL_AREA_NAMES))


def proposal_device_supported(gt: _GroundTruth, n_prop: int, limits) -> bool:
    """Sizes inside locov_proposal_recall's stated limits (beyond them it answers LOCOV_ERR_UNSUPPORTED: the host path is taken)."""
    index = gt.image_index()
    return (len(limits) <= _lib.PROPOSAL_RECALL_MAX_LIMITS and limits[-1] <= _lib.PROPOSAL_RECALL_MAX_LIMIT
            and index["max_per_image"] <= _lib.PROPOSAL_RECALL_MAX_GT and 0 < n_prop < 2 ** 31 - 1 and len(index["area"]) < 2 ** 31 - 1
            and 0 < gt.n_images * len(PROPOSAL_AREA_RNG) * len(limits) <= _lib.COCO_MAX_BLOCKS)


def proposal_recall_device(gt: _GroundTruth, img_rank, logits, boxes, limits=PROPOSAL_LIMITS, mark=None):
    """The same totals from device tensors: two stable integer sorts, one launch, an integer sum over the images and ONE copy to
    the host, of the A * L * (T + 1) totals.  mark: as in _evaluate_device.  -> (counts int64 [A, L, T], num_pos int64 [A, L])."""
    from . import ops
    g = gt.on(boxes.device, by_image=True)
    A, L, T = len(PROPOSAL_AREA_RNG), len(limits), len(PROPOSAL_THRS)
    totals, _ = ops.proposal_recall(img_rank, logits, boxes, g["image_offsets"], g["image_box"], g["image_area"], g["image_skip"],
                                    gt.image_index()["max_per_image"], PROPOSAL_AREA_RNG, limits, PROPOSAL_THRS, mark=mark)
    host = totals.cpu().numpy().reshape(A, L, T + 1)                          # the one device-to-host copy
    if mark is not None:
        mark("copy")
    return host[:, :, :T], host[:, :, T]


class COCOEvaluator:
    """Box AP under the COCO protocol (module docstring), with the reference's AP50-seen / AP50-unseen.

    gt: a COCO-format dict or the path of its JSON (images, annotations, categories).  class_names: one name per category in
    ascending category id (default: the categories' own names).  seen_names / unseen_names: the two lists the reference imports
    from its dataset file.  max_dets: an ascending tuple of 1-3 caps.  device: where evaluate() runs (default: where the
    processed tensors are).  Outputs that hold "proposals" are scored too, as "box_proposals" (the proposal recall of the module
    docstring, at proposal_limits); .proposal_eval holds its totals."""

    def __init__(self, gt, class_names: Optional[Sequence[str]] = None, seen_names: Sequence[str] = (), unseen_names: Sequence[str] = (),
                 max_dets: Sequence[int] = (1, 10, 100), device=None):
        max_dets = tuple(int(m) for m in max_dets)
        if not 1 <= len(max_dets) <= 3 or max_dets[0] < 1 or any(b <= a for a, b in zip(max_dets, max_dets[1:])):
            raise ValueError(f"max_dets must be an ascending tuple of 1-3 positive caps, got {max_dets}")
        self._gt = gt if isinstance(gt, _GroundTruth) else _GroundTruth(gt)
        self._class_names = list(class_names) if class_names is not None else list(self._gt.cat_names)
        if len(self._class_names) != self._gt.n_categories:
            raise ValueError(f"{len(self._class_names)} class names for {self._gt.n_categories} categories")
        self._seen, self._unseen = tuple(seen_names), tuple(unseen_names)
        self.max_dets = max_dets
        self._device = torch.device(device) if device is not None else None
        self.eval = None
        self.reset()

    proposal_limits = PROPOSAL_LIMITS                  # (an ascending tuple; an instance may set its own before evaluate())

    def reset(self) -> None:
        self._ranks, self._counts, self._boxes, self._scores, self._classes = [], [], [], [], []
        self._prop_ranks, self._prop_counts, self._prop_boxes, self._prop_logits = [], [], [], []
        self.eval = None
        self.proposal_eval = None

    def process(self, inputs, outputs) -> None:
        """inputs[i]["image_id"], outputs[i]["instances"] (pred_boxes XYXY, scores, pred_classes) and / or outputs[i]["proposals"]
        (proposal_boxes XYXY, objectness_logits).  The tensors are kept where they are; nothing is read to the host (the image id
        is host data)."""
        for inp, out in zip(inputs, outputs):
            if "instances" not in out and "proposals" not in out:
                continue
            iid = inp["image_id"]
            if iid not in self._gt.image_rank:
                raise KeyError(f"image id {iid!r} is not in the ground truth")
            if "proposals" in out:
                prop = out["proposals"]
                boxes = prop.proposal_boxes
                boxes = boxes.tensor if hasattr(boxes, "tensor") else boxes
                self._prop_ranks.append(self._gt.image_rank[iid])
                self._prop_counts.append(int(boxes.shape[0]))
                self._prop_boxes.append(boxes.detach().reshape(-1, 4))
                self._prop_logits.append(prop.objectness_logits.detach().reshape(-1))
            if "instances" not in out:
                continue
            inst = out["instances"]
            boxes = inst.pred_boxes
            boxes = boxes.tensor if hasattr(boxes, "tensor") else boxes
            self._ranks.append(self._gt.image_rank[iid])
            self._counts.append(int(boxes.shape[0]))
            self._boxes.append(boxes.detach().reshape(-1, 4))
            self._scores.append(inst.scores.detach().reshape(-1))
            self._classes.append(inst.pred_classes.detach().reshape(-1))

    @staticmethod
    def _cat(parts, device, dtype):
        if len({(p.device, p.dtype) for p in parts}) == 1:                 # one concatenation, then one move / conversion
            return torch.cat(parts).to(device=device, dtype=dtype)
        return torch.cat([p.to(device=device, dtype=dtype) for p in parts])

    def _gathered(self, device):
        cat = self._cat
        boxes, score, cls = cat(self._boxes, device, torch.float32), cat(self._scores, device, torch.float64), cat(self._classes, device, torch.int64)
        img_rank = torch.from_numpy(np.repeat(np.asarray(self._ranks, dtype=np.int64), self._counts)).to(device)
        return img_rank, cls, score, boxes

    def _gathered_proposals(self, device):
        boxes, logits = self._cat(self._prop_boxes, device, torch.float32), self._cat(self._prop_logits, device, torch.float64)
        img_rank = torch.from_numpy(np.repeat(np.asarray(self._prop_ranks, dtype=np.int64), self._prop_counts)).to(device)
        return img_rank, logits, boxes

    def _evaluate_proposals(self, mark=None):
        """The proposal recall of what process() saw -> "box_proposals"' dict; the totals stay on self.proposal_eval (counts,
        num_pos, recalls, ar).  The path is chosen as evaluate() chooses the AP's."""
        limits = tuple(int(v) for v in self.proposal_limits)
        if not limits or limits[0] < 1 or any(b <= a for a, b in zip(limits, limits[1:])):
            raise ValueError(f"proposal_limits must be an ascending tuple of positive limits, got {limits}")
        n = sum(self._prop_counts)
        device = self._device or self._prop_boxes[0].device
        on_device = device.type == "cuda" and _fused() and proposal_device_supported(self._gt, n, limits)
        img_rank, logits, boxes = self._gathered_proposals(device if on_device else torch.device("cpu"))
        if mark is not None:
            mark("gather")
        if on_device:
            counts, num_pos = proposal_recall_device(self._gt, img_rank, logits, boxes, limits, mark)
        else:
            host = proposal_recall_host(self._gt.image_index(), img_rank.numpy(), logits.numpy(), boxes.numpy(), limits)
            counts, num_pos = host["counts"], host["num_pos"]
        self.proposal_eval = proposal_totals(counts, num_pos)
        return derive_proposal_results(self.proposal_eval, limits)

    # the three places where a protocol differs; LVISEvaluator overrides them
    def _evaluate_host(self, img_rank, cls, score, boxes):
        return evaluate_host(self._gt, img_rank, cls, score, boxes, self.max_dets)

    def _evaluate_device(self, img_rank, cls, score, boxes, mark=None):
        return evaluate_device(self._gt, img_rank, cls, score, boxes, self.max_dets, mark)

    def _derive_results(self, ev):
        return derive_results(ev, self._class_names, self._seen, self._unseen)

    def _evaluate_bbox(self):
        n = sum(self._counts)
        if n == 0:
            self.eval = None
            return self._derive_results(None)
        device = self._device or self._boxes[0].device
        on_device = device.type == "cuda" and _fused() and device_supported(self._gt, n, self.max_dets)
        tensors = self._gathered(device if on_device else torch.device("cpu"))
        self.eval = self._evaluate_device(*tensors) if on_device else self._evaluate_host(*(t.numpy() for t in tensors))
        return self._derive_results(self.eval)

    def evaluate(self):
        """"bbox" always; "box_proposals" behind it if, and only if, process() saw at least one "proposals" output."""
        results = OrderedDict(bbox=self._evaluate_bbox())
        if self._prop_counts:
            results["box_proposals"] = self._evaluate_proposals()
        else:
            self.proposal_eval = None
        return results


def inference_on_dataset(model, data_loader, evaluator):
    """model.eval() under no_grad over the loader, evaluator.process per batch, then evaluator.evaluate(); the model's training
    mode is restored on exit."""
    was_training = model.training
    evaluator.reset()
    model.eval()
    try:
        with torch.no_grad():
            for inputs in data_loader:
                evaluator.process(inputs, model(inputs))
    finally:
        model.train(was_training)
    results = evaluator.evaluate()
    return results if results is not None else {}


# ---- the LVIS protocol (module docstring) ------------------------------------------------------------------------------------------
LVIS_METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf")
LVIS_FREQUENCIES = ("r", "c", "f")


class _LVISGroundTruth(_GroundTruth):
    """_GroundTruth plus what the federated protocol reads: each gt's `ignore` field (cell order), a byte per cell with the image's
    neg / not-exhaustive lists, and the frequency groups as arrays of category ranks.  `crowd` is kept but never read."""

    _uploaded = _GroundTruth._uploaded + ("ignore", "cell_flags")
    proposals_skip_crowd = False                                                               # LVIS's proposal recall takes every annotation

    def _read_more(self, gt, cats, cat_rank, anns):
        I, K = self.n_images, self.n_categories
        self.ignore = np.array([1 if a.get("ignore", 0) else 0 for a in anns], dtype=np.uint8)
        self.cell_flags = np.zeros(I * K, dtype=np.uint8)
        for field, bit in (("neg_category_ids", _lib.LVIS_CELL_NEG), ("not_exhaustive_category_ids", _lib.LVIS_CELL_NOT_EXHAUSTIVE)):
            cells = np.array([cat_rank[c] * I + self.image_rank[im["id"]] for im in gt["images"] for c in im.get(field, ())
                              if c in cat_rank], dtype=np.int64)
            self.cell_flags[cells] |= np.uint8(bit)                                            # (a scatter of one constant)
        freq = [c.get("frequency") for c in cats]
        self.freq_groups = [np.array([r for r, f in enumerate(freq) if f == name], dtype=np.int64) for name in LVIS_FREQUENCIES]


def limit_host(img_rank, cls, score, n_categories, max_dets_per_image):
    """LVISResults.limit_dets_per_image -> bool [N]: the dets that stay.  A class outside [0, K) is left out first; of the others
    each image keeps the first max_dets_per_image of a stable sort by descending score, over all categories together."""
    keep = (cls >= 0) & (cls < n_categories)
    idx = np.nonzero(keep)[0]
    p = idx[np.argsort(-score[idx], kind="stable")]
    p = p[np.argsort(img_rank[p], kind="stable")]
    image = img_rank[p]
    first = np.searchsorted(image, image, side="left")
    keep[p[np.arange(len(p)) - first >= max_dets_per_image]] = False
    return keep


def listed_host(gt: _LVISGroundTruth, img_rank, cls):
    """bool [N] for dets with a class in [0, K): the category has a gt in the image or is in its neg_category_ids."""
    cell = cls * gt.n_images + img_rank
    return (np.diff(gt.offsets.astype(np.int64))[cell] > 0) | ((gt.cell_flags[cell] & _lib.LVIS_CELL_NEG) != 0)


def match_host_lvis(gt: _LVISGroundTruth, det_offsets, boxes, max_det, area_rng=AREA_RNG, iou_thrs=IOU_THRS):
    """match_host under the LVIS rules.  boxes: fp32 XYXY in cell order.  -> det_bits uint8 [N, A * T], gt_ignore uint8 [A, G],
    listed bool [N]: False for the dets of unlisted cells (and of the trailing cell), which take no part; their bits are 0."""
    return _match_host(gt, gt.ignore, False, gt.cell_flags, det_offsets, boxes, max_det, area_rng, iou_thrs)


def summarize_lvis(precision, recall, freq_groups):
    """LVISEval._summarize's thirteen numbers on precision [T, R, K, A] and recall [T, K, A]: AP, AP50, AP75, APs, APm, APl, APr,
    APc, APf, AR@cap, ARs, ARm, ARl."""
    stats = np.full(13, -1.0)
    stats[0] = _mean(precision[:, :, :, 0])
    stats[1] = _mean(precision[0, :, :, 0])
    stats[2] = _mean(precision[5, :, :, 0])
    for i in range(1, 4):
        stats[2 + i] = _mean(precision[:, :, :, i])
        stats[9 + i] = _mean(recall[:, :, i])
    for i, group in enumerate(freq_groups):
        stats[6 + i] = _mean(precision[:, :, group, 0])
    stats[9] = _mean(recall[:, :, 0])
    return stats


def derive_results_lvis(ev):
    """Detectron2's LVISEvaluator: the nine AP metrics x 100 with no special case (-1 becomes -100.0); ev None: all nan."""
    if ev is None:
        return {metric: float("nan") for metric in LVIS_METRICS}
    return {metric: float(ev["stats"][i] * 100) for i, metric in enumerate(LVIS_METRICS)}


def evaluate_host_lvis(gt: _LVISGroundTruth, img_rank, cls, score, boxes, max_dets_per_image):
    """The whole LVIS protocol on numpy arrays -> {"precision" [T, R, K, A], "recall" [T, K, A], "stats" [13]}."""
    img_rank, cls = np.asarray(img_rank, dtype=np.int64), np.asarray(cls, dtype=np.int64)
    score = np.asarray(score).astype(np.float64)
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    keep = np.nonzero(limit_host(img_rank, cls, score, gt.n_categories, max_dets_per_image))[0]
    keep = keep[listed_host(gt, img_rank[keep], cls[keep])]                                    # the federated filter
    img_rank, cls, score, boxes = img_rank[keep], cls[keep], score[keep], boxes[keep]
    perm, det_offsets, rank, acc_index, cat_offsets = order_host(img_rank, cls, score, gt.n_images, gt.n_categories)
    bits, gt_ignore, _ = match_host_lvis(gt, det_offsets, boxes[perm], max_dets_per_image)
    precision, recall, _ = accumulate_host(cat_offsets, acc_index, rank[acc_index], score[perm][acc_index], bits,
                                           npig_host(gt, gt_ignore), (max_dets_per_image,), len(IOU_THRS))
    precision, recall = np.ascontiguousarray(precision[..., 0]), np.ascontiguousarray(recall[..., 0])
    return dict(precision=precision, recall=recall, stats=summarize_lvis(precision, recall, gt.freq_groups))


def evaluate_device_lvis(gt: _LVISGroundTruth, img_rank, cls, score, boxes, max_dets_per_image, mark=None):
    """The same on device tensors: the cap and the orderings by stable integer sorts, two launches, one copy to the host.  The
    unlisted dets stay in their cells; locov_lvis_match marks them ignored, which leaves precision and recall unchanged."""
    return _evaluate_device(gt, img_rank, cls, score, boxes, (max_dets_per_image,), True, mark)


class LVISEvaluator(COCOEvaluator):
    """Box AP under the LVIS protocol (module docstring), as Detectron2's LVISEvaluator reports it: AP, AP50, AP75, APs, APm, APl
    and APr / APc / APf over the rare / common / frequent categories.

    gt: an LVIS-format dict or the path of its JSON (images with neg_category_ids / not_exhaustive_category_ids, annotations,
    categories with frequency).  class_names: one name per category in ascending category id (checked for length; LVIS reports no
    per-category rows).  max_dets_per_image: the cap over all categories of an image.  device: where evaluate() runs.
    process(), reset() and evaluate() are COCOEvaluator's; .eval holds {"precision" [T, R, K, A], "recall" [T, K, A], "stats" [13]}."""

    def __init__(self, gt, class_names: Optional[Sequence[str]] = None, max_dets_per_image: int = 300, device=None):
        if int(max_dets_per_image) != max_dets_per_image or max_dets_per_image < 1:
            raise ValueError(f"max_dets_per_image must be a positive integer, got {max_dets_per_image!r}")
        super().__init__(gt if isinstance(gt, _LVISGroundTruth) else _LVISGroundTruth(gt), class_names=class_names,
                         max_dets=(int(max_dets_per_image),), device=device)
        self.max_dets_per_image = int(max_dets_per_image)

    def _evaluate_host(self, img_rank, cls, score, boxes):
        return evaluate_host_lvis(self._gt, img_rank, cls, score, boxes, self.max_dets_per_image)

    def _evaluate_device(self, img_rank, cls, score, boxes, mark=None):
        return evaluate_device_lvis(self._gt, img_rank, cls, score, boxes, self.max_dets_per_image, mark)

    def _derive_results(self, ev):
        return derive_results_lvis(ev)


def build_evaluator(dataset_name: str, gt, **kwargs):
    """The box branch of the reference's select_and_build_evaluator (ovr/evaluation/evaluator.py:39-50): a dataset whose name
    contains "lvis" is scored under the LVIS protocol, any other under COCO's."""
    return LVISEvaluator(gt, **kwargs) if "lvis" in dataset_name else COCOEvaluator(gt, **kwargs)
