"""The box-regression tail of a training step for BBOX_REG_LOSS_TYPE "giou" / "diou" / "ciou" -- fused against the torch chain.

FastRCNNOutputLayers.losses + the backward to the logits and deltas: as torch ops `loss_box_reg` is Box2BoxTransform.apply_deltas, the
fvcore loss (about 40 element-wise launches) and as many again in autograd; as ops.box_iou_loss (csrc/box_iou_loss.hip) one launch that
also makes the gradient, and backward's one multiplication by the incoming gradient.  Shapes: deltas [1536, 4] (class-agnostic, the
reference's configurations: 3 x 512 sampled proposals) and [1536, 4 * 1203] (class-specific at LVIS size); logits [1536, K + 1],
boxes up to 900 px, ground truth = box + N(0, 6), a quarter of the rows foreground.

    python tools/box_iou_loss_tail.py [--kinds giou diou ciou] [--shapes 1536x1 1536x1203] [--iters 100] [--warmup 10] [--queue-steps 4]
                                     [--queue-iters 20] [--out FILE]

(--shapes: rows x classes; classes 1 = class-agnostic deltas over an 80-class head.)  Prints one JSON record per (kind, shape) with, for
the fused path and for the torch chain (LOCOV_FUSED_LOSSES=0's path, switched in the same process) alternating:
  "losses":   median and 10th-90th percentile of device-event times of losses() + backward, one call per event bracket;
  "box_tail": the same for box_reg_loss + its backward alone;
  "box_tail_queued": --queue-steps such calls per bracket, enqueued while a long kernel keeps the device busy, divided by their number
              -- the device's time per call when the host runs ahead, as it does in the training step;
  "launches": device kernels of one losses() + backward (torch.profiler device events, as tools/count_launches.py counts them);
  "waits":    host waits of one call (torch's sync-debug mode + event waits, as tools/find_syncs.py counts them).
Needs a ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(1536, 1), (1536, 1203)]
KINDS = ("giou", "diou", "ciou")


class Tail:
    def __init__(self, R: int, classes: int, kind: str, device, seed: int = 0):
        from locov_amd.roi_heads import box_emb_head as beh
        from locov_amd.structures import Boxes, Instances
        self.beh = beh
        agnostic = classes == 1
        K = 80 if agnostic else classes
        g = torch.Generator().manual_seed(seed)
        boxes = torch.rand(R, 4, generator=g) * 600
        boxes[:, 2:] = boxes[:, :2] + 4 + torch.rand(R, 2, generator=g) * 300
        gt = boxes + torch.randn(R, 4, generator=g) * 6
        gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
        labels = torch.randint(0, K, (R,), generator=g)
        labels[torch.rand(R, generator=g) < 0.75] = K
        p = Instances((1000, 1000))
        p.proposal_boxes, p.gt_boxes, p.gt_classes = Boxes(boxes.to(device)), Boxes(gt.to(device)), labels.to(device)
        self.props = [p]
        self.scores = (torch.randn(R, K + 1, generator=g) * 3.0).to(device).requires_grad_(True)
        self.deltas = (torch.randn(R, 4 if agnostic else 4 * K, generator=g) * 0.3).to(device).requires_grad_(True)
        self.bp = beh.FastRCNNOutputLayers(64, box2box_transform=beh.Box2BoxTransform((10.0, 10.0, 5.0, 5.0)), num_classes=K,
                                           cls_agnostic_bbox_reg=agnostic, box_reg_loss_type=kind).to(device).train()

    def losses(self, fused: bool):
        """losses() + backward; returns (loss_box_reg, d / d deltas)."""
        self.beh._FUSED_BOX_LOSS = fused
        try:
            losses = self.bp.losses((self.scores, self.deltas), self.props, boxes_validated=True)
            grads = torch.autograd.grad(sum(losses.values()), [self.scores, self.deltas])
        finally:
            self.beh._FUSED_BOX_LOSS = True
        return losses["loss_box_reg"].detach(), grads[1]

    def box_tail(self, fused: bool):
        self.beh._FUSED_BOX_LOSS = fused
        try:
            p = self.props[0]
            loss = self.bp.box_reg_loss(p.proposal_boxes.tensor, p.gt_boxes.tensor, self.deltas, p.gt_classes, boxes_validated=True)
            grad = torch.autograd.grad(loss, self.deltas)[0]
        finally:
            self.beh._FUSED_BOX_LOSS = True
        return loss.detach(), grad


def timings(step, iters: int, warmup: int):
    ms = {True: [], False: []}
    for it in range(warmup + iters):
        for fused in ((True, False) if it % 2 == 0 else (False, True)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(fused)
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[fused].append(a.elapsed_time(b))
    return {("fused" if fused else "torch"): {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                                              "p90_ms": float(np.percentile(v, 90))} for fused, v in ms.items()}


def timings_queued(step, iters: int, warmup: int, steps: int):
    """`steps` calls per bracket, enqueued while a long kernel keeps the device busy, divided by their number: the device's time per
    call when the host runs ahead, as it does in the training step ("ahead": the host had finished before the device got there)."""
    import time
    blocker = torch.randn(8192, 8192, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        a.record()
        blocker @ blocker
        b.record()
        b.synchronize()
    blocker_ms = a.elapsed_time(b)
    ms, host = {True: [], False: []}, {True: [], False: []}
    for it in range(warmup + iters):
        for fused in ((True, False) if it % 2 == 0 else (False, True)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            blocker @ blocker
            t0 = time.perf_counter()
            a.record()
            for _ in range(steps):
                step(fused)
            b.record()
            t1 = time.perf_counter()
            b.synchronize()
            if it >= warmup:
                ms[fused].append(a.elapsed_time(b) / steps)
                host[fused].append((t1 - t0) * 1e3)
    return {("fused" if fused else "torch"): {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                                              "p90_ms": float(np.percentile(v, 90)),
                                              "ahead": bool(np.percentile(host[fused], 90) < blocker_ms)} for fused, v in ms.items()}


def launches(fn) -> int:
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def host_waits(fn) -> int:
    waits = []
    orig = torch.cuda.Event.synchronize

    def counted(self):
        waits.append(1)
        return orig(self)

    torch.cuda.Event.synchronize = counted
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.Event.synchronize = orig
    return len(waits) + sum(1 for x in w if "synchroniz" in str(x.message))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=KINDS)
    ap.add_argument("--shapes", nargs="+", default=[f"{r}x{k}" for r, k in SHAPES], help="ROWSxCLASSES ... (classes 1: class-agnostic)")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--queue-steps", type=int, default=4)
    ap.add_argument("--queue-iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the records as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("box_iou_loss_tail: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    recs = []
    for shape in args.shapes:
        R, classes = (int(x) for x in shape.lower().split("x"))
        for kind in args.kinds:
            tail = Tail(R, classes, kind, dev)
            (lf, gf), (lt, gt) = tail.losses(True), tail.losses(False)
            rec = {"kind": kind, "R": R, "deltas": list(tail.deltas.shape), "logits": list(tail.scores.shape),
                   "device": torch.cuda.get_device_name(dev), "loss_fused": float(lf), "loss_torch": float(lt),
                   "grad_max_abs_diff": float((gf - gt).abs().max())}
            rec["losses"] = timings(tail.losses, args.iters, args.warmup)
            rec["box_tail"] = timings(tail.box_tail, args.iters, args.warmup)
            rec["box_tail_queued"] = timings_queued(tail.box_tail, args.queue_iters, 3, args.queue_steps)
            rec["launches"] = {name: launches(lambda f=f: tail.losses(f)) for name, f in (("fused", True), ("torch", False))}
            rec["waits"] = {name: host_waits(lambda f=f: tail.losses(f)) for name, f in (("fused", True), ("torch", False))}
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
