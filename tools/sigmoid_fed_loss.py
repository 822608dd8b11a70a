"""Developer aid: the sigmoid / federated classification loss of FastRCNNOutputLayers.losses, fused device path vs the torch chain.

    python3 tools/sigmoid_fed_loss.py [--calls 30] [--warmup 5] [--shapes 1536x1204,2048x1204] [--num-fed 50]
                                      [--out profiles/r09_sigmoid_fed_loss.txt]
    python3 tools/sigmoid_fed_loss.py --softmax [--tree DIR]

For each shape [R, K + 1] (logits of standard deviation 3, a quarter of the rows foreground, class-agnostic deltas [R, 4]): ms of
losses() plus the backward to the logits and deltas with USE_SIGMOID_CE + USE_FED_LOSS (median over --calls calls after --warmup,
HIP events), device launches of one call (torch.profiler device events: tools/count_launches.py's method) and host waits of one call
(implicit synchronisations in torch's sync-debug mode + event waits: tools/find_syncs.py's method), for the fused path
(ops.fed_loss_classes + ops.sigmoid_cls_loss) and for the torch chain in the same process.

--softmax: only the existing softmax losses() (USE_SIGMOID_CE off), one line per shape -- for runs that alternate between two
checkouts; --tree DIR imports locov_amd from DIR (a checkout of another commit with its library built) instead of this tree."""
import argparse
import os
import statistics
import sys
import warnings


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="1536x1204,2048x1204")
    ap.add_argument("--num-fed", type=int, default=50)
    ap.add_argument("--softmax", action="store_true", help="time only the softmax losses() of the tree")
    ap.add_argument("--tree", default=None, help="import locov_amd from this checkout")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


ARGS = _args()
sys.path.insert(0, os.path.abspath(ARGS.tree) if ARGS.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import locov_amd
from locov_amd.roi_heads import box_emb_head as beh
from locov_amd.structures import Boxes, Instances


def inputs(R, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    scores = (torch.randn(R, C, generator=g) * 3.0).cuda().requires_grad_(True)
    deltas = (torch.randn(R, 4, generator=g) * 0.1).cuda().requires_grad_(True)
    labels = torch.randint(0, C - 1, (R,), generator=g)
    labels[torch.rand(R, generator=g) < 0.75] = C - 1
    xy = torch.rand(R, 2, generator=g) * 500
    p = Instances((800, 1333))
    p.proposal_boxes = Boxes(torch.cat([xy, xy + 20 + torch.rand(R, 2, generator=g) * 100], 1).cuda())
    p.gt_boxes = Boxes(p.proposal_boxes.tensor + 3.0)
    p.gt_classes = labels.cuda()
    return scores, deltas, [p]


def predictor(K, sigmoid, num_fed):
    kw = {}
    if sigmoid:
        g = torch.Generator().manual_seed(1)
        counts = torch.randint(1, 20000, (K,), generator=g).float()          # (image counts of an LVIS-like long tail)
        kw = dict(use_sigmoid_ce=True, use_fed_loss=True, fed_loss_num_classes=num_fed, get_fed_loss_cls_weights=lambda: counts ** 0.5)
    return beh.FastRCNNOutputLayers(64, box2box_transform=beh.Box2BoxTransform((10.0, 10.0, 5.0, 5.0)), num_classes=K,
                                    cls_agnostic_bbox_reg=True, **kw).cuda().train()


def timed(fn, calls):
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def host_waits(fn):
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


def main():
    args = ARGS
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    what = "softmax losses()" if args.softmax else f"USE_SIGMOID_CE + USE_FED_LOSS (FED_LOSS_NUM_CLASSES {args.num_fed})"
    lines = [f"# tools/sigmoid_fed_loss.py --calls {args.calls} --warmup {args.warmup}{' --softmax' if args.softmax else ''}: "
             f"FastRCNNOutputLayers.losses + backward, {what}, logit sigma 3; {torch.cuda.get_device_name()}",
             "# ms = median (min .. max) of the calls (HIP events around losses() and the backward); launches = device events of one call; "
             "waits = host waits of one call",
             f"{'logits':<14} {'path':<8} {'ms':>9} {'min':>9} {'max':>9} {'launches':>9} {'waits':>6}"]
    print("\n".join(lines), flush=True)
    for R, C in shapes:
        scores, deltas, props = inputs(R, C, seed=R)
        bp = predictor(C - 1, not args.softmax, args.num_fed)
        for path, fused in (("fused", True),) if args.softmax else (("fused", True), ("torch", False)):
            beh._FUSED_BOX_LOSS = fused

            def call():
                losses = bp.losses((scores, deltas), props, boxes_validated=True)
                return torch.autograd.grad(sum(losses.values()), [scores, deltas])

            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            ms, lo, hi = timed(call, args.calls)
            nl = launches(call)
            hw = host_waits(call)
            line = f"{f'[{R}, {C}]':<14} {path:<8} {ms:>9.4f} {lo:>9.4f} {hi:>9.4f} {nl:>9} {hw:>6}"
            print(line, flush=True)
            lines.append(line)
    beh._FUSED_BOX_LOSS = True
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
