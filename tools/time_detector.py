"""The detector call end to end (locov_amd/meta_arch.py) at the reference's image size, and its two ends against the torch
expressions they replace -- the same expressions the package ships as the fallback, i.e. what a user writes by hand today.

    timeout -k 10 900 python tools/time_detector.py [--images 1 8] [--iters 50] [--warmup 10] [--out records.json]

For each batch size (800 x 1333 uint8 images):
  (a) preprocess   model.preprocess_image on the kernel (ops.preprocess_images: one launch) against
                   ImageList.from_tensors([(x - pixel_mean) / pixel_std ...]); the kernel's bytes per second (image bytes read +
                   batch bytes written) over its device time (torch.profiler: the event time of so short a call is mostly
                   the host's) beside the measured copy rate --copy-tbs; the launches of each side.
  (b) postprocess  GeneralizedRCNN._postprocess at 100 detections per image on the kernel (ops.detector_rescale: one launch, one
                   read) against the per-image torch detector_postprocess with its host waits; device-event time, host wall
                   time, and the launches and device time of each side.
  (c) inference    model.inference (R50-C4, 1000 proposals, 80 classes) and the share of each stage, each stage between its own
                   device events in one pass.
Protocol: >= 10 warm-up and >= 50 timed iterations, device events, the two sides alternating (and swapping order)
in one process; each side's median and 10th / 90th percentile.  "not_slower": the kernel's median is at most the torch side's, or
the two 10th-90th percentile ranges overlap (the run-to-run spread).  Needs a ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_backbone import alternate, kernels, spread  # noqa: E402  (tools/ is the script directory)

H, W = 800, 1333


def not_slower(kernel, torch_side):
    return kernel["median_ms"] <= torch_side["median_ms"] or kernel["p10_ms"] <= torch_side["p90_ms"]


def wall(step, iters, warmup):
    """Host wall time of step() followed by a device synchronisation, ms."""
    ms = []
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def build(dev):
    import locov_amd
    torch.manual_seed(0)
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.META_ARCHITECTURE = "OvrRCNN"
    cfg.MODEL.DEVICE = str(dev)
    cfg.MODEL.BACKBONE.FREEZE_AT = 5
    cfg.MODEL.PIXEL_STD = [57.375, 57.12, 58.395]
    cfg.MODEL.ROI_HEADS.NAME = "EmbeddingRes5ROIHeads"
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    model = locov_amd.build_model(cfg).eval()
    model.roi_heads.box_predictor.set_class_embeddings(torch.randn(81, cfg.MODEL.ROI_BOX_HEAD.EMB_DIM) * 0.05)
    model.roi_heads.num_classes = model.roi_heads.box_predictor.num_classes
    return model


def detections(n_images, dev, per_image=100):
    from locov_amd.structures import Boxes, Instances
    g = torch.Generator().manual_seed(1)
    out = []
    for _ in range(n_images):
        xy = torch.rand(per_image, 2, generator=g) * torch.tensor([W * 1.05, H * 1.05]) - 20.0
        b = torch.cat([xy, xy + torch.rand(per_image, 2, generator=g) * 300.0], dim=1)
        out.append(Instances((H, W), pred_boxes=Boxes(b.to(dev)), scores=torch.rand(per_image, generator=g).to(dev),
                             pred_classes=torch.randint(0, 80, (per_image,), generator=g).to(dev)))
    return out


def stages(model, inputs, iters, warmup):
    """Device time of each stage of model.inference, between the stage's own events (medians over iters passes)."""
    names = ["preprocess", "backbone", "proposal_generator", "roi_heads", "postprocess"]
    ms = {k: [] for k in names}
    for it in range(warmup + iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        images = model.preprocess_image(inputs)
        ev[1].record()
        features = model.backbone(images.tensor)
        ev[2].record()
        proposals, _ = model.proposal_generator(images, features, None)
        ev[3].record()
        results, _ = model.roi_heads(images, features, proposals, None)
        ev[4].record()
        model._postprocess(results, inputs, images.image_sizes)
        ev[5].record()
        ev[5].synchronize()
        if it >= warmup:
            for k, a, b in zip(names, ev, ev[1:]):
                ms[k].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    total = sum(med.values())
    return {k: {"median_ms": v, "share": v / total} for k, v in med.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--copy-tbs", type=float, default=6.29, help="measured device copy rate the kernel's byte rate is put beside, TB/s")
    ap.add_argument("--skip-inference", action="store_true", help="only (a) and (b)")
    ap.add_argument("--out", default=None, help="also write the record as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_detector: needs a ROCm GPU")
    if args.iters < 50 or args.warmup < 10:
        raise SystemExit("time_detector: the protocol asks for >= 10 warm-up and >= 50 timed iterations")
    from locov_amd import detector_postprocess
    from locov_amd.structures import ImageList
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model = build(dev)
    rec = {"device": torch.cuda.get_device_name(dev), "image": [3, H, W], "runs": {}}
    for N in args.images:
        g = torch.Generator().manual_seed(N)
        inputs = [{"image": torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g).to(dev), "height": 480, "width": 800}
                  for _ in range(N)]
        r = {}
        with torch.no_grad():
            # (a)
            def torch_preprocess():
                return ImageList.from_tensors([(x["image"] - model.pixel_mean) / model.pixel_std for x in inputs],
                                              model.backbone.size_divisibility, padding_constraints=model.backbone.padding_constraints)
            a, b = model.preprocess_image(inputs), torch_preprocess()
            assert torch.equal(a.tensor.view(torch.int32), b.tensor.view(torch.int32)), "preprocess: the kernel and the torch expression differ"
            t = alternate({"kernel": lambda: model.preprocess_image(inputs), "torch": torch_preprocess}, args.iters, args.warmup)
            nbytes = N * 3 * H * W + a.tensor.numel() * 4
            dev_time = {"kernel": kernels(lambda: model.preprocess_image(inputs), top=2), "torch": kernels(torch_preprocess, top=4)}
            r["preprocess"] = dict(t, bytes=nbytes, device=dev_time, kernel_tbs=nbytes / (dev_time["kernel"]["total_us"] * 1e-6) / 1e12,
                                   copy_tbs=args.copy_tbs, not_slower=not_slower(t["kernel"], t["torch"]))
            # (b)
            results = detections(N, dev)
            sizes = [(H, W)] * N
            sides = {"kernel": lambda: model._postprocess(results, inputs, sizes),
                     "torch": lambda: [{"instances": detector_postprocess(x, 480, 800)} for x in results]}
            for x, y in zip(sides["kernel"](), sides["torch"]()):
                assert torch.equal(x["instances"].pred_boxes.tensor, y["instances"].pred_boxes.tensor), "postprocess: the two sides differ"
            t = alternate(sides, args.iters, args.warmup)
            r["postprocess"] = dict(t, wall={k: wall(s, args.iters, args.warmup) for k, s in sides.items()},
                                    device={k: kernels(s, top=3) for k, s in sides.items()},
                                    not_slower=not_slower(t["kernel"], t["torch"]))
            print(json.dumps({f"images {N}": r}), flush=True)
            # (c)
            if not args.skip_inference:
                t = alternate({"inference": lambda: model.inference(inputs)}, args.iters, args.warmup)["inference"]
                r["inference"] = dict(t, detections=[len(o["instances"]) for o in model.inference(inputs)],
                                      stages=stages(model, inputs, args.iters, args.warmup))
                print(json.dumps({f"images {N} inference": r["inference"]}), flush=True)
        rec["runs"][f"images_{N}"] = r
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
