"""The LSM step's region assembly at the reference's shape: locov_amd.mmss_regions against the reference's statement chain.

distill_prop_mmss_gcnn.py:273-328 / :348-399 turn the ROI heads' outputs into the grid and box region dictionaries
(SPATIAL_DROPOUT = 100 of 25 x 42 cells x 2048 from a 1333 x 800 batch with ragged image sizes; 100 of 200 sampled proposals per
image).  This tool builds those outputs synthetically -- Res5's grid pixel rows [B * 1050, 2048], box features [B * 200, 2048],
Instances -- and times forward + backward of

  (a) "chain":  the reference's statements written with torch ops (tests/regions_ref.py on the device tensors: numpy masks and
                centres, torch.tensor(...).to(device), one index per image, pad_sequence), permutations from np.random.shuffle;
  (b) "fused":  grid_regions + box_regions (csrc/regions.hip), keys from torch.rand on the device,

alternating in one process (device events; median and the 10th-90th percentile spread), and prints each side's device kernels per
call (torch.profiler, as tools/count_launches.py counts) and host waits (torch.cuda.set_sync_debug_mode, as tools/find_syncs.py
counts).  Both sides start from Res5's pixel rows and include the step that hands them out as visual_grid_features: the chain
always gets contiguous NCHW (the transpose and, in backward, its inverse); the fused side gets --layout (nchw: the same transposes;
channels_last: GRID_FEATURES_LAYOUT "channels_last", a view).

    python tools/lsm_region_tail.py [--batch 4 32] [--layout nchw|channels_last] [--iters 50] [--warmup 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GH, GW, V, SD, PER_IMAGE, PADDED = 25, 42, 2048, 100, 200, (800, 1344)


class Tail:
    def __init__(self, B: int, device, layout: str, seed: int = 0):
        from locov_amd.structures import Boxes, Instances
        rng = np.random.default_rng(seed)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.B, self.layout = B, layout
        self.sizes = [(800, 1333)] + [(int(rng.integers(480, 801)), int(rng.integers(640, 1334))) for _ in range(B - 1)]
        self.rows = d(np.maximum(rng.standard_normal((B * GH * GW, V)), 0).astype(np.float32)).requires_grad_(True)
        self.box = d(np.maximum(rng.standard_normal((B * PER_IMAGE, V)), 0).astype(np.float32)).requires_grad_(True)
        self.props = []
        for h, w in self.sizes:
            b = np.zeros((PER_IMAGE, 4), np.float32)
            b[:, 0], b[:, 1] = rng.uniform(0, w - 2, PER_IMAGE), rng.uniform(0, h - 2, PER_IMAGE)
            b[:, 2], b[:, 3] = b[:, 0] + rng.uniform(1, w / 2, PER_IMAGE), b[:, 1] + rng.uniform(1, h / 2, PER_IMAGE)
            p = Instances((h, w))
            p.proposal_boxes = Boxes(d(b))
            self.props.append(p)
        self.up = [d(rng.standard_normal((B, SD, V)).astype(np.float32)) for _ in range(2)]

    def step(self, fused: bool):
        import regions_ref
        from locov_amd import mmss_regions, res5_train
        self.rows.grad = self.box.grad = None
        grid = res5_train.to_nchw(self.rows, self.B, GH, GW, channels_last=fused and self.layout == "channels_last")
        box_list = list((self.box * 1.0).split([PER_IMAGE] * self.B))           # (views of one non-leaf matrix, as the heads return)
        if fused:
            img = mmss_regions.grid_regions(grid, self.sizes, PADDED, SD, True)
            box, _ = mmss_regions.box_regions(box_list, self.props, SD, True)
        else:
            ext = regions_ref.grid_extents(self.sizes, PADDED, GH, GW)
            perms = []
            for i in range(self.B):
                cells = np.arange(GH * GW)
                idx = cells[(cells // GW < ext[i, 0]) & (cells % GW < ext[i, 1])]
                np.random.shuffle(idx)
                perms.append(idx)
            img = regions_ref.grid_regions(grid, self.sizes, PADDED, SD, True, perms)
            bperms = []
            for _ in range(self.B):
                idx = np.arange(PER_IMAGE)
                np.random.shuffle(idx)
                bperms.append(idx)
            box, _ = regions_ref.box_regions(box_list, [p.proposal_boxes.tensor for p in self.props], [p.image_size for p in self.props], SD,
                                             True, bperms)
        torch.autograd.backward([img["region_features"], box["region_features"]], self.up)
        return img, box


def kernel_count(tail: Tail, fused: bool):
    from torch.profiler import ProfilerActivity, profile
    tail.step(fused)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        tail.step(fused)
        torch.cuda.synchronize()
    ev = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return {"device_kernels": len(ev), "locov_kernels": sum("locov" in n for n in ev),
            "region_kernels": sum("regions_" in n for n in ev), "transposes": sum("nchw_to_nhwc" in n for n in ev)}


def host_waits(tail: Tail, fused: bool) -> int:
    tail.step(fused)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            tail.step(fused)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(x.message) for x in w)


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
        out["fused" if fused else "chain"] = {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
                                              "p90_ms": float(np.percentile(v, 90))}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--layout", choices=["nchw", "channels_last"], default="nchw")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the records as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lsm_region_tail: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    np.random.seed(0)
    torch.manual_seed(0)
    recs = []
    for B in args.batch:
        tail = Tail(B, dev, args.layout)
        rec = {"B": B, "layout": args.layout, "device": torch.cuda.get_device_name(dev)}
        for fused in (True, False):
            side = "fused" if fused else "chain"
            rec["kernels_" + side] = kernel_count(tail, fused)
            rec["host_waits_" + side] = host_waits(tail, fused)
        rec.update(timings(tail, args.iters, args.warmup))
        rec["saved_ms"] = rec["chain"]["median_ms"] - rec["fused"]["median_ms"]
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
