"""The C4 backbone at the reference's image size: the fused stem launch beside its two floors, and the whole R50-C4 on the device
path (ops.resnet_stem + Res5Stage.forward_rows) against the module's own torch (MIOpen) path on the same weights.

    timeout -k 10 900 python tools/time_backbone.py --images 1 [--iters 50] [--warmup 10] [--out records.json]
    timeout -k 10 900 python tools/time_backbone.py --images 8
    timeout -k 10 900 python tools/time_backbone.py --train --images 4 [--freeze-at 0 2] [--iters 30]

  stem       ops.resnet_stem on N x 3 x 800 x 1333, device-event time of each call (median, 10th / 90th percentile) beside
             - the traffic floor: 29.9 MB of compulsory traffic per image (12.8 read + 17.1 written) at the HBM rate --peak-tbs
             - the arithmetic floor: 5.0 GFLOP per image (2 x 147 x 64 per conv output) at the fp32 rate --peak-tflops
  backbone   forward of the same module through both paths under torch.no_grad(), alternating A/B/A/B (and swapping order) in one
             process, each side's own median and 10th / 90th percentile; the outputs are compared first.  From a torch.profiler run
             per side: the device time by kernel name, so that a slower side shows which launches lose.
  --train    forward + backward (res4.backward(G)) of the same module with trainable weights through the device training path
             (MODEL.BACKBONE.TRAIN_ON_DEVICE: ops.resnet_stem_train / resnet_stem_wgrad, res5_train.res5_rows per stage) and
             through the torch (MIOpen, torch autograd) path, per MODEL.BACKBONE.FREEZE_AT of --freeze-at: alternating in one
             process as above (>= 10 warm-up, >= 30 timed), the largest relative difference between the two sides' weight
             gradients, each side's peak device memory over one step, and the device time by kernel name.
SURVEY.md 8d protocol: >= 10 warm-up and >= 50 timed iterations, device events, one process.  Needs a ROCm GPU.
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

H, W = 800, 1333
STEM_MB_PER_IMAGE = (3 * H * W + 64 * 200 * 334) * 4 / 1e6          # 12.8 read + 17.1 written
STEM_GFLOP_PER_IMAGE = 2 * 147 * 64 * 400 * 667 / 1e9               # 5.0


def spread(v):
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}


def alternate(sides, iters, warmup):
    """sides: name -> step().  Device-event time of each call, the sides alternating (and swapping order) in one process."""
    ms = {k: [] for k in sides}
    names = list(sides)
    for it in range(warmup + iters):
        for name in (names if it % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sides[name]()
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[name].append(a.elapsed_time(b))
    return {k: spread(v) for k, v in ms.items()}


def kernels(step, top=12):
    """Device time of one call by kernel name (torch.profiler): [(name, launches, total us)], largest first."""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        step()
        torch.cuda.synchronize()
    acc = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.lower().startswith(("memcpy", "memset")):
            n, us = acc.get(e.name, (0, 0.0))
            acc[e.name] = (n + 1, us + e.device_time)
    rows = sorted(acc.items(), key=lambda kv: -kv[1][1])
    return {"total_us": float(sum(v[1] for v in acc.values())), "launches": int(sum(v[0] for v in acc.values())),
            "top": [[k[:96], v[0], round(v[1], 1)] for k, v in rows[:top]]}


def peak_mb(step):
    """Peak device memory of one call above what is allocated in front of it, MB."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def train(args, dev):
    """Forward + backward through both paths, per FREEZE_AT."""
    import locov_amd
    N = args.images
    rec = {"device": torch.cuda.get_device_name(dev), "images": N, "input": [N, 3, H, W], "train": {}}
    for freeze_at in args.freeze_at:
        torch.manual_seed(0)
        cfg = locov_amd.config.get_cfg()
        cfg.MODEL.BACKBONE.FREEZE_AT = freeze_at
        cfg.MODEL.BACKBONE.TRAIN_ON_DEVICE = True
        model = locov_amd.build_backbone(cfg).to(dev)
        x = torch.randn(N, 3, H, W, device=dev)
        G = torch.randn(N, 1024, (H + 15) // 16, (W + 15) // 16, device=dev)

        def step(on_device):
            model.train_on_device = on_device
            assert model.train_path_ok(x) == on_device and not model.device_path_ok(x)
            model.zero_grad(set_to_none=True)
            model(x)["res4"].backward(G)

        sides = {"device": lambda: step(True), "torch": lambda: step(False)}
        grads = {}
        for name, side in sides.items():
            side()
            grads[name] = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        assert set(grads["device"]) == set(grads["torch"]) and grads["device"]
        diff = {k: float((grads["device"][k] - g).abs().max() / g.abs().max().clamp_min(1e-30)) for k, g in grads["torch"].items()}
        worst = max(diff, key=diff.get)
        del grads
        r = {"trained_tensors": len(diff), "max_rel_grad_diff": diff[worst], "max_rel_grad_diff_at": worst}
        r["kernels"] = {k: kernels(s) for k, s in sides.items()}
        r["peak_mb"] = {k: peak_mb(s) for k, s in sides.items()}
        r["step"] = alternate(sides, args.iters, args.warmup)
        r["device_path_not_slower"] = r["step"]["device"]["median_ms"] <= r["step"]["torch"]["median_ms"]
        rec["train"][f"freeze_at_{freeze_at}"] = r
        print(json.dumps({f"train freeze_at {freeze_at} images {N}": {k: v for k, v in r.items() if k != "kernels"}}), flush=True)
        print(json.dumps({"kernels": r["kernels"]}), flush=True)
        del model, x, G
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM rate the traffic floor is quoted at, TB/s")
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="fp32 rate the arithmetic floor is quoted at, TFLOP/s")
    ap.add_argument("--stem-only", action="store_true", help="time the stem launch alone (LOCOV_STEM_BAND=<rows> forces its band height)")
    ap.add_argument("--train", action="store_true", help="time forward + backward of the device training path against the torch path")
    ap.add_argument("--freeze-at", type=int, nargs="+", default=[0, 2], help="--train: the MODEL.BACKBONE.FREEZE_AT settings timed")
    ap.add_argument("--out", default=None, help="also write the record as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_backbone: needs a ROCm GPU")
    if args.train:
        if args.iters < 30 or args.warmup < 10:
            raise SystemExit("time_backbone --train: >= 10 warm-up and >= 30 timed iterations")
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        return train(args, dev)
    if args.iters < 50 or args.warmup < 10:
        raise SystemExit("time_backbone: the protocol asks for >= 10 warm-up and >= 50 timed iterations")
    import locov_amd
    from locov_amd import ops
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    cfg = locov_amd.config.get_cfg()
    cfg.MODEL.BACKBONE.FREEZE_AT = 5
    model = locov_amd.build_backbone(cfg).to(dev).eval()
    N = args.images
    x = torch.randn(N, 3, H, W, device=dev)
    rec = {"device": torch.cuda.get_device_name(dev), "images": N, "input": [N, 3, H, W]}

    scale, shift = ops.frozen_bn_fold(*(getattr(model.stem.conv1.norm, k) for k in ("weight", "bias", "running_mean", "running_var")), 1e-5)
    w = model.stem.conv1.weight.detach()
    out = ops.resnet_stem(x, w, scale, shift)
    t = alternate({"stem": lambda: ops.resnet_stem(x, w, scale, shift, out=out)}, args.iters, args.warmup)["stem"]
    floor_mem, floor_fma = N * STEM_MB_PER_IMAGE / (args.peak_tbs * 1e6) * 1e3, N * STEM_GFLOP_PER_IMAGE / (args.peak_tflops * 1e3) * 1e3
    rec["stem"] = dict(t, traffic_floor_ms=floor_mem, arithmetic_floor_ms=floor_fma, mb=N * STEM_MB_PER_IMAGE,
                       gflop=N * STEM_GFLOP_PER_IMAGE, tflops=N * STEM_GFLOP_PER_IMAGE / t["median_ms"],
                       share_of_arithmetic_floor=floor_fma / t["median_ms"])
    print(json.dumps({"stem": rec["stem"]}), flush=True)
    if args.stem_only:
        return

    with torch.no_grad():
        assert model.device_path_ok(x)
        sides = {"device": lambda: model(x)["res4"], "torch": lambda: model._forward_torch(x)["res4"]}
        a, b = sides["device"](), sides["torch"]()
        rec["max_abs_diff"] = float((a - b).abs().max())
        rec["max_abs"] = float(b.abs().max())
        rec["kernels"] = {k: kernels(s) for k, s in sides.items()}
        rec["backbone"] = alternate(sides, args.iters, args.warmup)
    rec["device_path_not_slower"] = rec["backbone"]["device"]["median_ms"] <= rec["backbone"]["torch"]["median_ms"]
    print(json.dumps({k: rec[k] for k in ("backbone", "device_path_not_slower", "max_abs_diff", "max_abs")}), flush=True)
    print(json.dumps({"kernels": rec["kernels"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
