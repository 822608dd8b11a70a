"""RPN proposal generation at the reference's two shapes: ops.rpn_proposals (csrc/rpn.hip) against the torch chain of
locov_amd/proposal_generator.py (find_top_rpn_proposals: sort, gather, apply_deltas, finite test, clip, nonempty, batched_nms on
ops.nms, slice) on the same device tensors.

    timeout -k 10 600 python tools/rpn_proposals_step.py [--iters 30] [--warmup 5] [--out records.json]

  evaluation   1 image, 50 x 84 x 15 = 63 000 anchors of the default generator, PRE / POST_NMS_TOPK_TEST 6 000 / 1 000
  training     4 images, the same map, PRE / POST_NMS_TOPK_TRAIN 12 000 / 2 000
each with two kinds of input: "scattered" (randn logits, 0.2 randn deltas: the selected boxes rarely overlap at 0.7, the sweep
stops early) and "overlapping" (the logit grows with the anchor's size and the deltas are 0.02 randn, so the selection is the
large anchors of neighbouring cells, which overlap far above 0.7, as a trained RPN's output does: most boxes are suppressed and the
sweep walks many or all of its chunks).  `sweep_chunks` is the number of 64-box chunks the sweep walked of `chunks`, per image,
worked out on the host from the outputs.  NMS threshold 0.7, images 800 x 1333.  The two sides alternate (and swap order) in one process;
device-event time of each call, median and the 10th / 90th percentile.  Also printed, from a torch.profiler run of its own per side:
the device kernels one call enqueues, its host reads (torch's synchronisation debug mode plus the package's event waits), and for
the fused side the time of each of its three kernels -- the share of the sweep.  Both sides' outputs are compared bit for bit before anything is timed.  Needs a ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, NMS, MIN_SIZE, IMAGE = 50, 84, 0.7, 0.0, (800, 1333)
SHAPES = {"evaluation": (1, 6000, 1000), "training": (4, 12000, 2000)}
KINDS = ("scattered", "overlapping")


def make_sides(n_img, pre, post, dev, kind):
    from locov_amd import ops
    from locov_amd.proposal_generator import DefaultAnchorGenerator, find_top_rpn_proposals
    from locov_amd.roi_heads.box_emb_head import Box2BoxTransform
    gen = DefaultAnchorGenerator([[32, 64, 128, 256, 512]], [[0.5, 1.0, 2.0]], [16]).to(dev)
    anchors = gen([torch.zeros(n_img, 1, H, W, device=dev)])[0].tensor
    n = anchors.shape[0]
    g = torch.Generator().manual_seed(n_img)
    if kind == "scattered":
        draw = lambda: (torch.randn(n_img, n, generator=g), 0.2 * torch.randn(n_img, n, 4, generator=g))
    else:
        size = torch.log2((anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])).cpu() / 2      # 5 .. 9
        draw = lambda: (size[None] + 0.5 * torch.randn(n_img, n, generator=g), 0.02 * torch.randn(n_img, n, 4, generator=g))
    sets = [tuple(t.to(dev) for t in draw()) for _ in range(3)]                             # fresh operands from call to call
    sizes, b2b = [IMAGE] * n_img, Box2BoxTransform((1.0, 1.0, 1.0, 1.0))

    def fused(i):
        logits, deltas = sets[i % len(sets)]
        return ops.rpn_proposals(logits, deltas, anchors, sizes, b2b.weights, b2b.scale_clamp, pre, post, MIN_SIZE, NMS)

    def chain(i):
        logits, deltas = sets[i % len(sets)]
        return find_top_rpn_proposals([logits], [deltas], [anchors], sizes, b2b, NMS, pre, post, MIN_SIZE, False)

    return {"fused": fused, "chain": chain}, sets[0][0]


def sweep_chunks(logits, fused_out, pre, post):
    """Per image: the 64-box chunks the sweep walked -- up to the chunk of the post-th survivor, or all of them when fewer survive."""
    _, _, index, counts = fused_out
    P = min(logits.shape[1], pre)
    order = torch.sort(logits, dim=1, descending=True, stable=True)[1]
    out = []
    for n, c in enumerate(counts):
        if c < post:
            out.append((P + 63) // 64)
        else:
            out.append(int((order[n] == index[n, c - 1]).nonzero()[0, 0]) // 64 + 1)
    return out


def same_bits(fused_out, chain_out) -> bool:
    boxes, scores, index, counts = fused_out
    ok = counts == [len(c[2]) for c in chain_out]
    for n, (cb, cs, ci, _) in enumerate(chain_out):
        k = counts[n]
        ok = ok and torch.equal(index[n, :k], ci) and torch.equal(boxes[n, :k].view(torch.int32), cb.view(torch.int32)) \
            and torch.equal(scores[n, :k].view(torch.int32), cs.view(torch.int32))
    return bool(ok)


def alternate(sides, iters, warmup):
    """sides: name -> step(i).  Device-event time of each call, the sides alternating (and swapping order) in one process."""
    ms = {k: [] for k in sides}
    names = list(sides)
    for it in range(warmup + iters):
        for name in (names if it % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sides[name](it)
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[name].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
            for k, v in ms.items()}


def host_reads(step) -> int:
    """Host reads of one call: what torch's synchronisation debug mode reports (item(), nonzero(), blocking copies) plus the event
    waits the package makes for its pinned-memory reads (ops._read_counts_and_flags)."""
    import warnings
    waits = [0]
    plain = torch.cuda.Event.synchronize

    def counted(self):
        waits[0] += 1
        return plain(self)

    torch.cuda.Event.synchronize = counted
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            step(1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.Event.synchronize = plain
    torch.cuda.synchronize()
    return waits[0] + len([w for w in seen if "synchroniz" in str(w.message).lower()])


def launches_and_reads(step):
    from torch.profiler import ProfilerActivity, profile
    step(0)
    torch.cuda.synchronize()
    rec = {"host_reads": host_reads(step)}
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        step(1)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    rec["device_kernels"] = len([e for e in ev if not e.name.lower().startswith(("memcpy", "memset"))])
    for key in ("rpn_select", "rpn_overlap", "rpn_sweep"):
        us = [e.device_time for e in ev if key in e.name]
        if us:
            rec[key + "_us"] = float(sum(us))
    if "rpn_sweep_us" in rec:
        rec["sweep_share_of_kernel_time"] = rec["rpn_sweep_us"] / (rec["rpn_select_us"] + rec["rpn_overlap_us"] + rec["rpn_sweep_us"])
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the record as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rpn_proposals_step: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rec = {"device": torch.cuda.get_device_name(dev), "anchors": H * W * 15}
    for shape, (n_img, pre, post) in SHAPES.items():
        for kind in KINDS:
            name = f"{shape}_{kind}"
            sides, logits0 = make_sides(n_img, pre, post, dev, kind)
            first = sides["fused"](0)
            r = {"images": n_img, "pre_nms_topk": pre, "post_nms_topk": post, "same_bits": same_bits(first, sides["chain"](0)),
                 "proposals": first[3], "sweep_chunks": sweep_chunks(logits0, first, pre, post), "chunks": (min(pre, H * W * 15) + 63) // 64}
            r["calls"] = {k: launches_and_reads(s) for k, s in sides.items()}
            r["time"] = alternate(sides, args.iters, args.warmup)
            r["fused_not_slower"] = r["time"]["fused"]["median_ms"] <= r["time"]["chain"]["median_ms"]
            rec[name] = r
            print(json.dumps({name: r}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
