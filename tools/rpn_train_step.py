"""The RPN's training half at the reference's shape: anchor labelling + the sample draw + the two losses, forward and backward to the
logits and deltas (without the head), fused (ops.rpn_label_anchors / rpn_sample_anchors / rpn_loss, csrc/rpn_train.hip) against the
torch chain of locov_amd/proposal_generator.py (LOCOV_FUSED_RPN=0) on the same device tensors and the same draw.

    timeout -k 10 600 python tools/rpn_train_step.py [--iters 30] [--warmup 5] [--out records.json]

  reference    4 images, a 50 x 84 map, 15 anchors per cell (63 000 anchors of the default generator), 0-15 ground-truth boxes each,
               BATCH_SIZE_PER_IMAGE 256, images 800 x 1333
  small        2 images, a 12 x 20 map (3 600 anchors), 0-5 boxes each
The two sides alternate (and swap order) in one process; device-event time of each call, median and the 10th / 90th percentile.  Also
printed, from a torch.profiler run of its own per side: the device kernels one call enqueues and its host waits (torch's
synchronisation debug mode plus the package's event waits; the fused side defers its logged counters as RPN.forward does, so it
should make none).  Labels and matched boxes of both sides are compared bit for bit before anything is timed.  Needs a ROCm GPU.
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

import torch  # noqa: E402

from rpn_proposals_step import alternate, host_reads  # noqa: E402

SHAPES = {"reference": (4, 50, 84, 15, (800, 1333)), "small": (2, 12, 20, 5, (192, 320))}


def make_sides(n_img, H, W, max_gt, image, dev):
    from torch import nn
    from locov_amd.proposal_generator import RPN, DefaultAnchorGenerator
    from locov_amd.roi_heads.box_emb_head import Box2BoxTransform
    from locov_amd.structures import Boxes, Instances
    gen = DefaultAnchorGenerator([[32, 64, 128, 256, 512]], [[0.5, 1.0, 2.0]], [16]).to(dev)
    anchors = gen([torch.zeros(n_img, 1, H, W, device=dev)])
    n = anchors[0].tensor.shape[0]
    rpn = RPN(in_features=["res4"], head=nn.Identity(), anchor_generator=gen, box2box_transform=Box2BoxTransform((1.0, 1.0, 1.0, 1.0)),
              pre_nms_topk=(12000, 6000), post_nms_topk=(2000, 1000)).train()
    g = torch.Generator().manual_seed(n_img)
    gt = []
    for i in range(n_img):                                       # 0 .. max_gt boxes, the first image none
        k = 0 if i == 0 else int(torch.randint(1, max_gt + 1, (1,), generator=g))
        xy = torch.rand(k, 2, generator=g) * torch.tensor([image[1] * 0.7, image[0] * 0.7])
        wh = 16 + torch.rand(k, 2, generator=g) * torch.tensor([image[1] * 0.3, image[0] * 0.3])
        gt.append(Instances(image, gt_boxes=Boxes(torch.cat([xy, xy + wh], dim=1).to(dev))))
    sets = [(torch.randn(n_img, n, generator=g).to(dev).requires_grad_(), (0.2 * torch.randn(n_img, n, 4, generator=g)).to(dev).requires_grad_())
            for _ in range(3)]
    rnd = torch.rand(2, n_img, n, dtype=torch.float64, generator=g).to(dev)

    def step(i, fused):
        os.environ["LOCOV_FUSED_RPN"] = "1" if fused else "0"
        logits, deltas = sets[i % len(sets)]
        logits.grad = deltas.grad = None
        labels, boxes = rpn.label_and_sample_anchors(anchors, gt, rnd)
        rpn._defer_log = fused                                   # (RPN.forward hands the counters over behind predict_proposals' read)
        try:
            losses = rpn.losses(anchors, [logits], labels, [deltas], boxes)
        finally:
            rpn._defer_log = False
        (losses["loss_rpn_cls"] + losses["loss_rpn_loc"]).backward()
        return labels, boxes, losses

    def settle():
        rpn._flush_log()
        os.environ.pop("LOCOV_FUSED_RPN", None)

    return {"fused": lambda i: step(i, True), "chain": lambda i: step(i, False)}, settle, n, [len(x.gt_boxes.tensor) for x in gt]


def launches_and_reads(step):
    from torch.profiler import ProfilerActivity, profile
    step(0)
    torch.cuda.synchronize()
    rec = {"host_waits": host_reads(step)}
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        step(1)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    rec["device_kernels"] = len([e for e in ev if not e.name.lower().startswith(("memcpy", "memset"))])
    for key in ("rpn_gt_max", "rpn_label", "rpn_sample", "rpn_loss_kernel", "rpn_loss_finish"):
        us = [e.device_time for e in ev if key in e.name]
        if us:
            rec[key + "_us"] = float(sum(us))
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the record as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rpn_train_step: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rec = {"device": torch.cuda.get_device_name(dev)}
    for name, (n_img, H, W, max_gt, image) in SHAPES.items():
        sides, settle, n, n_gt = make_sides(n_img, H, W, max_gt, image, dev)
        a, b = sides["fused"](0), sides["chain"](0)
        settle()
        r = {"images": n_img, "anchors": n, "gt_boxes": n_gt,
             "same_labels_and_boxes": all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1])),
             "losses": {k: {"fused": float(a[2][k]), "chain": float(b[2][k])} for k in a[2]}}
        r["calls"] = {k: launches_and_reads(s) for k, s in sides.items()}
        r["time"] = alternate(sides, args.iters, args.warmup)
        settle()
        r["fused_over_chain"] = r["time"]["fused"]["median_ms"] / r["time"]["chain"]["median_ms"]
        rec[name] = r
        print(json.dumps({name: r}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
