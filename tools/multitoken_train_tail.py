"""Forward + backward of the multi-token class predictor's tail at the STT shape on an LVIS-size bank, against the reference's
arithmetic written as torch ops.

The tail: emb_pred -> (normalise) -> token similarities -> masked softmax attention over a class's tokens -> attention-weighted
distance -> cross-entropy, differentiated down to the pooled features (box_emb_grounding_head.py:395-427 with
DETACH_CLASS_PREDICTOR off; emb_pred frozen but passed through, configs/coco_stt.yaml:36).  1 536 rows (3 images x 512 sampled
proposals), C5 = 2 048, D = 768, 1 203 classes of 1-4 tokens.
  (a) this package: EmbeddingGroundingFastRCNNOutputLayers.forward_cls_prediction on the HIP kernels and their backward entry points;
  (b) the same arithmetic as torch ops under autograd on the same GPU, formed as the reference forms it: padded [R, K1, Tmax]
      similarity / distance tensors filled by a per-class copy loop, torch.where mask, softmax, masked sum.
The parent of this path had no backward, so (b) is the yardstick.

    python tools/multitoken_train_tail.py [--metric dot cosine] [--iters 30] [--warmup 5]

Prints one JSON record per metric: median device-event time of forward + backward of both forms, alternating in one process
(with the 10th / 90th percentile), and the device kernels one step enqueues (torch.profiler).  Needs a ROCm GPU.
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
import torch.nn.functional as F  # noqa: E402

R, C5, D, K = 1536, 2048, 768, 1203


class Tail:
    def __init__(self, metric: str, device, seed: int = 0):
        import locov_amd
        cfg = locov_amd.config.get_cfg()
        cfg.MODEL.ROI_BOX_HEAD.NAME = "EmbeddingGroundingFastRCNNOutputLayers"
        cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
        cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
        cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = D
        cfg.MODEL.ROI_BOX_HEAD.NORMALIZE_EMB_PRED = metric == "cosine"
        cfg.MODEL.MMSS_HEAD.GROUNDING.LOCAL_METRIC = metric
        cfg.MODEL.ROI_HEADS.NUM_CLASSES = K
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        self.cosine = metric == "cosine"
        self.temp = float(cfg.MODEL.MMSS_HEAD.GROUNDING.ALIGNMENT_TEMPERATURE)
        self.pred = locov_amd.build_box_predictor(cfg, C5).to(device).train()
        for p in self.pred.emb_pred.parameters():
            p.requires_grad_(False)                                              # coco_stt.yaml:36
        self.ntok = [int(n) for n in rng.integers(1, 5, size=K)]
        self.pred.set_class_embeddings({k: torch.from_numpy((rng.standard_normal((n, D)) * 0.2).astype(np.float32))
                                        for k, n in enumerate(self.ntok)})
        self.x = torch.from_numpy(np.maximum(rng.standard_normal((R, C5)), 0).astype(np.float32)).to(device)
        self.labels = torch.from_numpy(rng.integers(0, K + 1, size=R)).to(device)
        gm = self.pred.cls_score
        self.bank, self.mask = gm.token_score.weight.detach(), gm.mask_emb
        self.split = [max(n, 1) for n in self.ntok] + [1]
        self.counts = self.ntok + [1]            # (the reference's in-place split_sizes[... == 0] = 1 reaches num_tok: bg copies one slot)

    def hip(self, x):
        return self.pred.forward_cls_prediction(x)

    def torch_ops(self, x):
        emb = F.linear(x, self.pred.emb_pred.weight, self.pred.emb_pred.bias)
        if self.cosine:
            emb = F.normalize(emb, p=2, dim=1)
        sim = F.linear(emb, self.bank)
        if self.cosine:
            sim = torch.where(torch.isnan(sim), torch.zeros_like(sim), sim)
            dis = 1 - sim
        else:
            dis = -sim
        sims, diss = torch.split(sim / self.temp, self.split, dim=1), torch.split(dis / self.temp, self.split, dim=1)
        tmax = self.mask.shape[1]
        all_sim = torch.zeros(x.shape[0], len(self.counts), tmax, device=x.device)
        all_dis = torch.zeros(x.shape[0], len(self.counts), tmax, device=x.device)
        for k, (s, d) in enumerate(zip(sims, diss)):                             # the per-class copy loop
            all_sim[:, k, :self.counts[k]] = s
            all_dis[:, k, :self.counts[k]] = d
        all_sim = torch.where(self.mask > 0, all_sim, all_sim.min().detach() - 100.0)
        att = F.softmax(all_sim, dim=2) * self.mask[None]
        return -(att * all_dis).sum(dim=2)

    def step(self, which: str):
        x = self.x.detach().requires_grad_(True)
        scores = self.hip(x) if which == "hip" else self.torch_ops(x)
        loss = F.cross_entropy(scores, self.labels)
        loss.backward()
        return loss.detach(), x.grad


def kernel_count(tail: Tail, which: str):
    from torch.profiler import ProfilerActivity, profile
    tail.step(which)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        tail.step(which)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return {"device_kernels": len(ev), "locov_kernels": sum("locov" in e.name for e in ev)}


def timings(tail: Tail, iters: int, warmup: int):
    ms = {"hip": [], "torch": []}
    for it in range(warmup + iters):
        for which in (("hip", "torch") if it % 2 == 0 else ("torch", "hip")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tail.step(which)
            b.record()
            b.synchronize()
            if it >= warmup:
                ms[which].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}
            for k, v in ms.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--metric", nargs="+", default=["dot", "cosine"], choices=["dot", "cosine"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the records as JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("multitoken_train_tail: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    recs = []
    for metric in args.metric:
        tail = Tail(metric, dev)
        (la, ga), (lb, gb) = tail.step("hip"), tail.step("torch")
        rec = {"metric": metric, "R": R, "C5": C5, "D": D, "classes": K, "token_columns": int(tail.bank.shape[0]),
               "device": torch.cuda.get_device_name(dev), "loss_hip": float(la), "loss_torch": float(lb),
               "grad_rel_l2": float((ga.double() - gb.double()).norm() / gb.double().norm())}
        rec["kernels_hip"], rec["kernels_torch"] = kernel_count(tail, "hip"), kernel_count(tail, "torch")
        rec.update(timings(tail, args.iters, args.warmup))
        rec["speedup"] = rec["torch"]["median_ms"] / rec["hip"]["median_ms"]
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
