"""GroundingHead's hardmax and triplet variants on the kernels against their torch chain (LOCOV_FUSED_LOSSES=0).

Two configurations off the shipped one (grounding_head.py:169-174, :279-343): ALIGNMENT "hardmax" with LOSS "cross_entropy", and
ALIGNMENT "softmax" with LOSS "triplet", NEGATIVE_MINING "hardest".  As in the LSM step (distill_prop_mmss_gcnn.py:337-415) the head
runs twice per step, on the image grid and on the boxes: SPATIAL_DROPOUT = 100 regions each, 70 caption tokens, V = 2048, L = 768.

    python tools/grounding_variant_tail.py [--batch 4 32] [--iters 50] [--warmup 10]

Prints, per configuration and batch size: the device-event time of forward + backward, fused and with LOCOV_FUSED_LOSSES=0,
alternating in one process (median and the spread between the 10th and 90th percentile), the device kernels one step enqueues
(torch.profiler, as tools/count_launches.py counts them) and the host reads it makes (torch's synchronisation debug mode).  Needs a
ROCm GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lsm_distill_tail import NR, V, L, T, _Switch, kernel_counts, timings  # noqa: E402

CONFIGS = {
    "hardmax_ce": dict(ALIGNMENT="hardmax"),
    "softmax_triplet_hardest": dict(LOSS="triplet", NEGATIVE_MINING="hardest"),
}


def _cfg(over):
    ns = types.SimpleNamespace
    g = ns(LOCAL_METRIC="dot", GLOBAL_METRIC="aligned_local", ALIGNMENT="softmax", ALIGNMENT_TEMPERATURE=10.0,
           LOSS="cross_entropy", NEGATIVE_MINING="random", TRIPLET_MARGIN=1.0, ALIGN_WORDS_TO_REGIONS=True,
           ALIGN_REGIONS_TO_WORDS=True, TEXT_INPUT="input_embeddings")
    for k, v in over.items():
        setattr(g, k, v)
    return ns(MODEL=ns(MMSS_HEAD=ns(GROUNDING=g, DISTILLATION_LOSS=False)))


class Tail:
    """Two GroundingHeads of one configuration (grid, boxes) on seeded inputs of batch B."""

    def __init__(self, B: int, device, over: dict, seed: int = 0):
        from locov_amd.grounding_head import GroundingHead
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        self.B = B
        self.heads = [GroundingHead(_cfg(over), V, L).to(device) for _ in range(2)]
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
        self.images = [{"region_features": d(np.maximum(rng.standard_normal((B, NR, V)), 0).astype(np.float32) * 0.05),
                        "region_mask": d(np.ones((B, NR), np.uint8))} for _ in range(2)]

    def leaves(self):
        return [self.caption["input_embeddings"]] + [im["region_features"] for im in self.images] + \
            [p for h in self.heads for p in h.parameters()]

    def step(self):
        """forward + backward; returns the losses (detached) and the gradients of every leaf."""
        for t in self.leaves():
            t.requires_grad_(True)
            t.grad = None
        losses = {}
        for k, (head, img) in enumerate(zip(self.heads, self.images)):
            losses.update({("Box " if k else "") + n: v for n, v in head(img, self.caption)[1].items()})
        sum(losses.values()).backward()
        return {k: v.detach() for k, v in losses.items()}, [t.grad for t in self.leaves()]


def host_reads(tail: Tail, fused: bool) -> int:
    """Synchronising calls one step makes, as torch's synchronisation debug mode reports them."""
    with _Switch(fused):
        tail.step()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                tail.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message) for w in seen)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the records as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("grounding_variant_tail: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    recs = []
    for name, over in CONFIGS.items():
        for B in args.batch:
            tail = Tail(B, dev, over)
            rec = {"config": name, "B": B, "device": torch.cuda.get_device_name(dev)}
            for fused in (True, False):
                n, ours = kernel_counts(tail, fused)
                rec["kernels_" + ("fused" if fused else "torch")] = {"device_kernels": n, "locov_kernels": ours,
                                                                     "host_reads": host_reads(tail, fused)}
            rec.update(timings(tail, args.iters, args.warmup))
            rec["saved_ms"] = rec["torch"]["median_ms"] - rec["fused"]["median_ms"]
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
