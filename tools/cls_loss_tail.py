"""The classification tail of a training step -- loss_cls forward + backward on the logits -- fused against the torch chain.

FastRCNNOutputLayers.losses' `cross_entropy(scores, gt_classes, reduction="mean")` and its backward: as torch ops a chain of small
launches (log-softmax, NLL, their two backwards, the reduction and the gradient scaling); as ops.cls_loss (csrc/cls_loss.hip) a row
kernel that also makes the gradient and the classification statistics, a small finishing launch, and backward's one multiplication by
the incoming gradient.  Shapes: [1536, 49] (configs/coco_stt.yaml: 3 x 512 sampled proposals, 48 + 1 bank), [1536, 81], [800, 1204]
and [1536, 1204] (LVIS size).  Logits of sigma 3 with the background column exactly 0, every 7th label ignored.

    python tools/cls_loss_tail.py [--shapes 1536x49 ...] [--iters 200] [--warmup 20] [--queue-steps 20] [--queue-iters 40] [--out FILE]

Prints, per shape, for both paths alternating in one process (median and the 10th-90th percentile spread of device-event times):
  "fused" / "torch":                 one forward + backward per event bracket on an idle device -- the host paces it, so this is mostly
                                     the interpreter's and the dispatcher's time per call;
  "fused_queued" / "torch_queued":   --queue-steps calls per bracket, enqueued while a long kernel keeps the device busy, divided by
                                     their number -- the device's time per call when the host runs ahead, as it does in the training
                                     step, whose losses are enqueued before its one host wait ("host_ms" is the enqueueing time per
                                     call, "ahead" says whether the host had finished before the device started on the bracket);
and the device kernels one call enqueues in each (torch.profiler, as tools/count_launches.py counts them).  Needs a ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(1536, 49), (1536, 81), (800, 1204), (1536, 1204)]


class Tail:
    def __init__(self, R: int, C: int, device, seed: int = 0):
        g = torch.Generator().manual_seed(seed)
        scores = torch.randn(R, C, generator=g) * 3.0
        scores[:, -1] = 0.0
        labels = torch.randint(0, C, (R,), generator=g)
        labels[6::7] = -100
        self.scores = scores.to(device).requires_grad_(True)
        self.labels = labels.to(device)

    def step(self, fused: bool):
        """forward + backward; returns (loss, d loss / d scores)."""
        from locov_amd import ops
        if fused:
            loss, _ = ops.cls_loss(self.scores, self.labels)
        else:
            loss = F.cross_entropy(self.scores, self.labels, reduction="mean")
        return loss.detach(), torch.autograd.grad(loss, self.scores)[0]


def kernel_counts(tail: Tail, fused: bool):
    from count_launches import count
    n, names = count(lambda: tail.step(fused))
    return {"device_kernels": n, "locov_kernels": sum(v for k, v in names.items() if "locov" in k), "names": names}


def timings(tail: Tail, iters: int, warmup: int):
    ms = {True: [], False: []}
    for it in range(warmup + iters):
        for fused in ((True, False) if it % 2 == 0 else (False, True)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tail.step(fused)
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[fused].append(a.elapsed_time(b))
    out = {}
    for fused, v in ms.items():
        v = np.array(v)
        out["fused" if fused else "torch"] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                                              "p90_ms": float(np.percentile(v, 90))}
    return out


def timings_queued(tail: Tail, iters: int, warmup: int, steps: int):
    import time
    dev = tail.scores.device
    blocker = torch.randn(8192, 8192, device=dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    blocker @ blocker
    b.record()
    b.synchronize()
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
            blocker @ blocker                                 # the device is busy while the host enqueues the bracket
            t0 = time.perf_counter()
            a.record()
            for _ in range(steps):
                tail.step(fused)
            b.record()
            t1 = time.perf_counter()
            b.synchronize()
            if it >= warmup:
                ms[fused].append(a.elapsed_time(b) / steps)
                host[fused].append((t1 - t0) * 1e3)
    out = {}
    for fused, v in ms.items():
        v, h = np.array(v), np.array(host[fused])
        out[("fused" if fused else "torch") + "_queued"] = {
            "median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)),
            "host_ms": float(np.median(h) / steps), "ahead": bool(np.percentile(h, 90) < blocker_ms)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=[f"{r}x{c}" for r, c in SHAPES], help="RxC ...")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--queue-steps", type=int, default=20)
    ap.add_argument("--queue-iters", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the records as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cls_loss_tail: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    recs = []
    for shape in args.shapes:
        R, C = (int(x) for x in shape.lower().split("x"))
        tail = Tail(R, C, dev)
        (lf, gf), (lt, gt) = tail.step(True), tail.step(False)
        rec = {"R": R, "C": C, "device": torch.cuda.get_device_name(dev), "loss_fused": float(lf), "loss_torch": float(lt),
               "grad_max_abs_diff": float((gf - gt).abs().max())}
        for fused in (True, False):
            rec["kernels_" + ("fused" if fused else "torch")] = kernel_counts(tail, fused)
        rec.update(timings(tail, args.iters, args.warmup))
        rec.update(timings_queued(tail, args.queue_iters, 5, args.queue_steps))
        rec["saved_ms"] = rec["torch"]["median_ms"] - rec["fused"]["median_ms"]
        rec["saved_queued_ms"] = rec["torch_queued"]["median_ms"] - rec["fused_queued"]["median_ms"]
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
