"""The LSM step's distillation tail under the reference's own training config, fused against LOCOV_FUSED_LOSSES=0.

configs/coco_lsm.yaml:60-63 turns MMSS_HEAD.DISTILLATION_LOSS on (type KD, temperature 10, weight 1, DETACH_TEACHER off,
TEACHER_TRANSFORMER off).  Then distill_prop_mmss_gcnn.py:337-415 runs the GroundingHead twice with its distributions returned --
on the image grid and on the boxes, SPATIAL_DROPOUT = 100 regions each, V = 2048 -- and :424-442 makes three MultiDistillLoss
calls (grid, boxes, grid transformer costs against the box distributions).  The TransformerHead is out of scope: its costs
(`trans`, `box_trans`) are synthetic inputs that require grad.  bench.py's LSM step sets DISTILLATION_LOSS off, so this tail is
measured here.

    python tools/lsm_distill_tail.py [--batch 4 32] [--iters 50] [--warmup 10]

Prints, per batch size: the device-event time of forward + backward, fused and with LOCOV_FUSED_LOSSES=0, alternating in one
process (median and the spread between the 10th and 90th percentile), and the device kernels one call enqueues in each
configuration (torch.profiler, as tools/count_launches.py counts them).  Needs a ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

NR, V, L, T = 100, 2048, 768, 70          # SPATIAL_DROPOUT regions, res5 width, language width, caption tokens


def _cfg():
    ns = types.SimpleNamespace
    g = ns(LOCAL_METRIC="dot", GLOBAL_METRIC="aligned_local", ALIGNMENT="softmax", ALIGNMENT_TEMPERATURE=10.0,
           LOSS="cross_entropy", NEGATIVE_MINING="random", TRIPLET_MARGIN=1.0, ALIGN_WORDS_TO_REGIONS=True,
           ALIGN_REGIONS_TO_WORDS=True, TEXT_INPUT="input_embeddings")
    return ns(MODEL=ns(MMSS_HEAD=ns(GROUNDING=g, DISTILLATION_LOSS=True)))


class Tail:
    """Two GroundingHeads with distributions (grid, boxes) and the three KD calls, on seeded inputs of batch B."""

    def __init__(self, B: int, device, seed: int = 0):
        from locov_amd.distill_losses import MultiDistillLoss
        from locov_amd.grounding_head import GroundingHead
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        self.B = B
        self.heads = [GroundingHead(_cfg(), V, L).to(device) for _ in range(2)]      # image grid, boxes
        self.kd = MultiDistillLoss(10.0, loss_weight=1.0, detach_teacher=False, transformer_teacher=False)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        attn = np.ones((B, T), np.int64)
        special = np.zeros((B, T), np.int64)
        special[:, 0] = 1
        for b in range(B):
            n = int(rng.integers(12, T))                                                  # caption length
            attn[b, n:] = 0
            special[b, n - 1:] = 1
        self.caption = {"input_embeddings": d(rng.standard_normal((B, T, L)).astype(np.float32) * 0.1),
                        "attention_mask": d(attn), "special_tokens_mask": d(special)}
        self.images = []
        for _ in range(2):
            rmask = np.ones((B, NR), np.uint8)
            self.images.append({"region_features": d(np.maximum(rng.standard_normal((B, NR, V)), 0).astype(np.float32) * 0.05),
                                "region_mask": d(rmask)})
        self.trans = d(rng.standard_normal((B, B)).astype(np.float32) * 3.0)
        self.box_trans = d(rng.standard_normal((B, B)).astype(np.float32) * 3.0)

    def leaves(self):
        return [self.caption["input_embeddings"], self.trans, self.box_trans] + [im["region_features"] for im in self.images] + \
            [p for h in self.heads for p in h.parameters()]

    def forward(self):
        """distill_prop_mmss_gcnn.py:337-442 on the heads' outputs: every loss by name (insertion order as the reference's)."""
        losses, dists = {}, {}
        for k, (head, img) in enumerate(zip(self.heads, self.images)):
            _, l, dist = head(img, self.caption)
            pre = "box_" if k else ""
            losses.update({("Box " if k else "") + n: v for n, v in l.items()})
            dists.update({pre + n: v for n, v in dist.items()})
        losses["kd_loss"] = self.kd(self.trans, dists["w2r"], dists["r2w"])
        losses["box_kd_loss"] = self.kd(self.box_trans, dists["box_w2r"], dists["box_r2w"])
        losses["mixbox_kd_loss"] = self.kd(self.trans, dists["box_w2r"], dists["box_r2w"])
        return losses, dists

    def step(self):
        """forward + backward; returns the losses (detached) and the gradients of every leaf."""
        for t in self.leaves():
            t.requires_grad_(True)
            t.grad = None
        losses, _ = self.forward()
        sum(losses.values()).backward()
        return {k: v.detach() for k, v in losses.items()}, [t.grad for t in self.leaves()]


class _Switch:
    def __init__(self, fused: bool):
        self.fused = fused

    def __enter__(self):
        self.old = os.environ.get("LOCOV_FUSED_LOSSES")
        os.environ["LOCOV_FUSED_LOSSES"] = "1" if self.fused else "0"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("LOCOV_FUSED_LOSSES", None)
        else:
            os.environ["LOCOV_FUSED_LOSSES"] = self.old


def kernel_counts(tail: Tail, fused: bool):
    from torch.profiler import ProfilerActivity, profile
    with _Switch(fused):
        tail.step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            tail.step()
            torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(ev), sum("locov" in e.name for e in ev)


def timings(tail: Tail, iters: int, warmup: int):
    ms = {True: [], False: []}
    for it in range(warmup + iters):
        for fused in ((True, False) if it % 2 == 0 else (False, True)):
            with _Switch(fused):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                tail.step()
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the records as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lsm_distill_tail: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    recs = []
    for B in args.batch:
        tail = Tail(B, dev)
        rec = {"B": B, "device": torch.cuda.get_device_name(dev)}
        for fused in (True, False):
            n, ours = kernel_counts(tail, fused)
            rec["kernels_" + ("fused" if fused else "torch")] = {"device_kernels": n, "locov_kernels": ours}
        rec.update(timings(tail, args.iters, args.warmup))
        rec["saved_ms"] = rec["torch"]["median_ms"] - rec["fused"]["median_ms"]
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
