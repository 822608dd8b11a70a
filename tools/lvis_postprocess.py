"""Developer aid: the evaluation call's post-processing at LVIS-style vs COCO-style thresholds, torch chain vs fused device path.

    python3 tools/lvis_postprocess.py [--calls 30] [--images 1,8] [--class-specific] [--paths chain,fused]
                                      [--out profiles/r07_lvis_postprocess.txt]

For each case (images x 1000 proposals x 1203 classes, logits of standard deviation 3 as bench.Workload.eval_heads calibrates them):
post-processing ms of FastRCNNOutputLayers.inference (median over --calls calls, HIP events), candidates per image, device launches
of one call (torch.profiler device events: tools/count_launches.py's method) and host waits of one call (implicit synchronisations
in torch's sync-debug mode + event waits).  The fused path's first call at an LVIS threshold finds the overflow of the LDS pipeline
and remembers it; the figures are for the calls after it.  --class-specific: the plain FastRCNNOutputLayers with
CLS_AGNOSTIC_BBOX_REG False (deltas [R, 4K], a box per (proposal, class)) instead of the class-agnostic embedding predictor."""
import argparse
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import locov_amd
from locov_amd.roi_heads import box_emb_head as beh
from locov_amd.structures import Boxes, Instances

CLASSES, PROPOSALS = 1203, 1000


def inputs(n_images, seed=0, class_specific=False):
    g = torch.Generator().manual_seed(seed)
    R = n_images * PROPOSALS
    logits = torch.randn(R, CLASSES + 1, generator=g) * 3.0
    logits[:, -1] = 0.0
    deltas = torch.randn(R, 4, generator=g) * torch.tensor([1.0, 1.0, 0.5, 0.5])
    if class_specific:                          # (drawn after everything else: the scores and proposals are the class-agnostic run's)
        gd = torch.Generator().manual_seed(seed + 1000)
        deltas = (torch.randn(R, CLASSES, 4, generator=gd) * torch.tensor([1.0, 1.0, 0.5, 0.5])).reshape(R, 4 * CLASSES)
    props = []
    for _ in range(n_images):
        xy = torch.rand(PROPOSALS, 2, generator=g) * torch.tensor([1333 * 0.8, 800 * 0.8])
        wh = torch.rand(PROPOSALS, 2, generator=g) * torch.tensor([1333 * 0.4, 800 * 0.4]) + 8.0
        p = Instances((800, 1333))
        p.proposal_boxes = Boxes(torch.cat([xy, xy + wh], dim=1).cuda())
        props.append(p)
    return (logits.cuda(), deltas.cuda()), props


def predictor(thresh, topk, class_specific=False):
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = CLASSES
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = thresh
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = not class_specific
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = not class_specific
    if class_specific:
        cfg.MODEL.ROI_BOX_HEAD.NAME = "FastRCNNOutputLayers"
    cfg.TEST.DETECTIONS_PER_IMAGE = topk
    return beh.build_box_predictor(cfg, 256).cuda().eval()


def timed(fn, calls):
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--images", default="1,8")
    ap.add_argument("--class-specific", action="store_true", help="deltas [R, 4K]: the plain predictor, CLS_AGNOSTIC_BBOX_REG False")
    ap.add_argument("--paths", default="chain,fused", help="which of the two paths to measure")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cs = args.class_specific
    paths = args.paths.split(",")
    lines = [f"# tools/lvis_postprocess.py --calls {args.calls}{' --class-specific' if cs else ''}: FastRCNNOutputLayers.inference, images x {PROPOSALS} proposals x "
             f"{CLASSES} classes, logit sigma 3; {torch.cuda.get_device_name()}",
             "# ms = median of the calls (HIP events around inference()); launches = device events of one call; waits = host waits of one call",
             f"{'case':<24} {'cand/img':>10} {'path':<6} {'ms':>9} {'ms/img':>8} {'launches':>9} {'waits':>6}"]
    print("\n".join(lines), flush=True)
    for n in (int(x) for x in args.images.split(",")):
        predictions, props = inputs(n, seed=n, class_specific=cs)
        for thresh, topk in ((1e-4, 300), (0.05, 100)):
            pred = predictor(thresh, topk, cs)
            probs = torch.softmax(predictions[0], dim=-1)[:, :-1]
            cand = int((probs > thresh).sum()) // n
            for path, fused in (("chain", False), ("fused", True)):
                if path not in paths:
                    continue
                beh._FUSED_POSTPROCESS = fused

                def call():
                    with torch.no_grad():
                        return pred.inference(predictions, props)

                call()
                call()
                torch.cuda.synchronize()
                ms = timed(call, args.calls)
                nl = launches(call)
                hw = host_waits(call)
                line = f"{f'{n} img, {thresh:g}, top-{topk}':<24} {cand:>10} {path:<6} {ms:>9.3f} {ms / n:>8.3f} {nl:>9} {hw:>6}"
                print(line, flush=True)
                lines.append(line)
    beh._FUSED_POSTPROCESS = True
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
