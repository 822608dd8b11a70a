"""The weight-derived GEMM operands of the Res5 stage, and the power-of-two scales of their split packings: one owner.

An operand is (conv, tag):
    "plain"  W [N,K]                         forward of a 1x1 convolution
    "t"      (s W)^T [K,N]                   its data gradient
    "wino"   U = (G (x) G) w [121,N,Cin]     forward of a 3x3 convolution on 7x7 tiles
    "col"    [N, 9 Cin]                      ... on a general grid (direct / im2col GEMM)
    "flip"   flip(s w) [Cin,N,3,3]           the filter both data-gradient forms are packed from (fp32 only)
    "uflip"  (G (x) G) flip(s w) [121,Cin,N] data gradient on 7x7 tiles
    "flip9"  [Cin, 9 N] of flip(s w)         ... on a general grid
or, with block 0 in the place of conv, one of its two concatenations (inference):
    "tail"   [s3 W3 | ss Ws] [Cout, mid + Cin]   conv3 + projection shortcut as ONE GEMM over [conv2 output | stage input]
    "on_map" [W1 ; ss Ws] [mid + Cout, Cin]      conv1 + shortcut on the feature map, in front of the pooler
             (both also hold "shift" = b3 + bs, the summed FrozenBN shifts)
in a form: "fp32", "bf16" (ops.to_bf16) or "split" (ops.SplitWeight: (hi, lo) f16 pairs of scale * operand).  An entry lives until
its convolution or FrozenBN changes (conv_version); its bf16 / split forms hang off it and go with it.
"""
from __future__ import annotations

import math
import os

import torch

from . import ops

_ONE_LAUNCH_PREP = os.environ.get("LOCOV_RES5_PREP", "1") != "0"    # developer A/B: a training step's operands from one launch (TrainOperands)

ROW_SCALED = ("t", "uflip", "flip9")         # operands of the data gradients: the FrozenBN scale is folded into their rows
BLOCK0 = ("tail", "on_map")


def conv_version(conv, weight: bool = True) -> tuple:
    """What an entry made from `conv` is valid for -- THE answer to "has this convolution or its FrozenBN changed": storage and
    in-place version of the weight (checkpoint load, optimizer step), storage of the FrozenBN weight and the versions of its four
    buffers.  weight=False: the FrozenBN part alone (the fold survives optimizer steps, which only move conv.weight)."""
    n = conv.norm
    norm = (n.weight.data_ptr(), n.weight._version, n.bias._version, n.running_mean._version, n.running_var._version)
    return (conv.weight.data_ptr(), conv.weight._version) + norm if weight else norm


class Res5Operands:
    """Every weight-derived operand of a Res5Stage, its FrozenBN folds, the remembered split scales and the per-step operand sets
    of training (TrainOperands).  A plain object the stage creates: no parameters, nothing in the state dict."""

    REUSE = 64                # packings of the on-demand chain that re-use a remembered scale before it is chosen from the data again
    REFRESH = 64              # steps of the one-launch preparation between two re-choices from the bound
    WINO_GAIN = 2.25          # max_f (sum_a |G[f][a]|)^2 of csrc/winograd_tables.h: |((G (x) G) w)[f]| <= 2.25 max |w|

    def __init__(self, stage):
        self.stage = stage
        self.entries = {}             # (conv | block 0, tag) -> {"version", "fp32"[, "bf16"][, "split"][, "shift"]}
        self.folds = {}               # conv -> (FrozenBN version, (scale, shift))
        self.scales = {}              # (conv, tag) -> (scale of the split packing, uses since it was chosen)
        self.sets = {}                # (split, grid, rois) -> (versions of every convolution, TrainOperands)
        self.latest = None            # the operand set handed out last
        self.step_versions = None     # the weight versions of the last COUNTED training step
        self.prep_bufs = {}           # (grid, rois, conv, tag) -> output of the one-launch preparation (storage only)
        self.steps = 0                # counted split-arithmetic training steps
        self.refresh = None           # the refresh in flight: (event, pinned values, convs, wanted, step it was asked at)
        self.refresh_host = None      # its pinned buffer (one refresh in flight, adopted before the next starts)

    # -- operands and their forms ----------------------------------------------------------------------------------------------
    def fold(self, conv):
        """(scale, shift) of conv's FrozenBN (kept until the statistics change; no launch after the first call)."""
        version = conv_version(conv, weight=False)
        hit = self.folds.get(conv)
        if hit is None or hit[0] != version:
            n = conv.norm
            hit = self.folds[conv] = (version, ops.frozen_bn_fold(n.weight, n.bias, n.running_mean, n.running_var, n.eps))
        return hit[1]

    def get(self, conv, tag: str, form: str = "fp32"):
        """Operand (conv, tag) in `form`, built on demand and kept until conv changes: the two Res5 calls of a training step run the
        same kernels on the same weights, the second one reuses the first one's operands.  A new version supersedes the entry with
        all its forms (ONE live packing per operand)."""
        block0 = tag in BLOCK0
        version = tuple(conv_version(c) for c in (conv.conv1, conv.conv3, conv.shortcut)) if block0 else conv_version(conv)
        e = self.entries.get((conv, tag))
        if e is None or e["version"] != version:
            e = self.entries[(conv, tag)] = self._block0(conv, tag) if block0 else {"fp32": self._derive(conv, tag)}
            e["version"] = version
        if form not in e:
            t = e["fp32"]
            if form == "bf16":
                e[form] = ops.to_bf16(t.contiguous())
            else:
                # (block 0's concatenations: chosen from the data at each packing by split_pack, not remembered)
                scale = None if block0 else self._packing_scale((conv, tag), t)
                e[form] = ops.split_pack(t.contiguous(), scale)
        return e[form]

    def for_gemm(self, conv, tag: str, split: bool):
        """What a GEMM takes: the split form (ops.SplitWeight) in split arithmetic when the shape allows, else the fp32 tensor."""
        t = self.get(conv, tag)
        if split and t.shape[-1] % 32 == 0 and t.shape[-2] % 4 == 0:
            return self.get(conv, tag, "split")
        return t

    def _derive(self, conv, tag: str) -> torch.Tensor:
        w = conv.weight.detach()
        if tag == "plain":
            return w.reshape(w.shape[0], w.shape[1])
        if tag == "col":
            return ops.pack_conv3x3_weight(w)
        if tag == "wino":
            return ops.winograd_pack_weight(w)
        s = self.fold(conv)[0]
        if tag == "t":
            return ops.weight_transpose_scale(self.get(conv, "plain"), s)
        if tag == "flip":
            return ops.conv3x3_weight_flip(w, s)
        return (ops.winograd_pack_weight if tag == "uflip" else ops.pack_conv3x3_weight)(self.get(conv, "flip"))

    def _block0(self, b0, tag: str) -> dict:
        """"tail": relu(s3*(W3 y) + b3 + ss*(Ws x) + bs) = relu([y | x] . [s3*W3 | ss*Ws]^T + (b3 + bs)) -- the FrozenBN scales go into
        the weight rows (the sum of two differently scaled products cannot use the epilogue's single scale).  "on_map": the shortcut's
        scale is folded into its rows, conv1's FrozenBN is applied after the pooling."""
        (s3, b3), (ss, bs) = self.fold(b0.conv3), self.fold(b0.shortcut)
        ws = self.get(b0.shortcut, "plain") * ss[:, None]
        if tag == "tail":
            cat = torch.cat([self.get(b0.conv3, "plain") * s3[:, None], ws], dim=1)
        else:
            cat = torch.cat([self.get(b0.conv1, "plain"), ws], dim=0)
        return {"fp32": cat.contiguous(), "shift": (b3 + bs).contiguous()}

    # -- the scale policy of the split form ------------------------------------------------------------------------------------
    # A scale is the power of two that puts max |scale * operand| in [2^12, 2^13): 8x headroom, weights drift slowly against it,
    # and the pack kernels raise the range-guard word if a re-used scale ever stops covering its operand (the caller then repeats
    # the pass on the f32 MFMA and calls forget_scales).
    def _packing_scale(self, key, t: torch.Tensor) -> float:
        """The on-demand chain: choosing a scale needs max |t| on the host, i.e. a device sync per packing, ten per training step --
        so it is remembered and re-used, one use per packing, and chosen from the data again after REUSE of them."""
        rec = self.scales.get(key)
        if rec is not None and rec[1] < self.REUSE:
            self.scales[key] = (rec[0], rec[1] + 1)
            return rec[0]
        scale = ops.split_scale_for(t)
        self.scales[key] = (scale, 0)
        return scale

    def _start_refresh(self, wanted) -> None:
        """A count reached REFRESH in the one-launch preparation: enqueue max |w| / max |s| of every convolution of `wanted`
        towards pinned memory (two launches, no wait); one refresh in flight."""
        if self.refresh is not None:
            return
        convs = list({c: None for c, _ in wanted})
        ts = [c.weight.detach() for c in convs] + [self.fold(c)[0] for c in convs]
        try:
            norms = torch._foreach_norm(ts, float("inf"))
        except (RuntimeError, TypeError):                    # (a torch without the foreach form of the max norm)
            norms = [t.abs().max() for t in ts]
        dev = torch.stack([n.reshape(()).to(torch.float32) for n in norms])
        if self.refresh_host is None or self.refresh_host.numel() < dev.numel():
            self.refresh_host = torch.empty(max(dev.numel(), 64), dtype=torch.float32).pin_memory()
        host = self.refresh_host[:dev.numel()]
        host.copy_(dev, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(dev.device))
        self.refresh = (event, host, convs, list(wanted), self.steps)

    def _count_step(self) -> None:
        """Once per counted step.  A FIXED two steps after a refresh was enqueued (its event completed a step ago -- every step waits
        for the GPU once -- so the wait below is free: the schedule of scales does not depend on timing) every operand's scale is
        derived from the BOUND  max |operand| <= max |s| * max |w| (* WINO_GAIN in the Winograd domain)  and its count starts again;
        the steps in between kept the old scales, which the headroom still covers."""
        self.steps += 1
        pending = self.refresh
        if pending is None or self.steps - pending[4] < 2:
            return
        pending[0].synchronize()
        self.refresh = None
        _, host, convs, wanted, _ = pending
        vals = host.tolist()
        n = len(convs)
        amax_w, amax_s = dict(zip(convs, vals[:n])), dict(zip(convs, vals[n:]))
        for conv, tag in wanted:
            if (conv, tag) not in self.scales:               # (dropped in between -- a guard tripped: the chain chooses afresh)
                continue
            bound = amax_w[conv] * (amax_s[conv] if tag in ROW_SCALED else 1.0) * (self.WINO_GAIN if tag in ("wino", "uflip") else 1.0)
            scale = 2.0 ** (12 - math.floor(math.log2(bound))) if bound > 0 and math.isfinite(bound) else 1.0
            self.scales[(conv, tag)] = (min(max(scale, 2.0 ** -100), 2.0 ** 100), 0)

    def forget_scales(self) -> None:
        """A range guard tripped, and what no longer fits may be a remembered scale: the scales are chosen afresh at the next
        packing, also at unchanged weight versions.  Drops the scales, every operand in every form, the folds and the operand
        sets.  Keeps the step counter, the weight versions of the last counted step and a refresh in flight (its adoption skips
        the keys dropped here), and the preparation buffers (storage only)."""
        self.scales.clear()
        self.entries.clear()
        self.folds.clear()
        self.sets.clear()
        self.latest = None

    # -- the operand sets of training ------------------------------------------------------------------------------------------
    def train_operands(self, split: bool, grid: bool = True, rois: bool = True) -> "TrainOperands":
        """The GEMM operands of one training step (forward and backward of every convolution), valid for the current weight
        versions: built once per step and FLAVOUR (arithmetic, which 3x3 forms are needed), by the first Res5 call that asks.  A
        step that calls the stage through different flavours (res5_grid and res5_rois separately instead of one Res5Step) gets one
        operand set per flavour, each in its own buffers: a later set never re-packs, in place, the buffers an earlier set's
        SplitWeight objects still point at for their backward."""
        versions = tuple(conv_version(c) for blk in self.stage for c in (blk.conv1, blk.conv2, blk.conv3, blk.shortcut) if c is not None)
        flavour = (bool(split), bool(grid), bool(rois))
        hit = self.sets.get(flavour)
        if hit is None or hit[0] != versions:
            # a NEW step (the weights moved since the last operand set of any flavour): steps are counted and scale refreshes
            # adopted once per weight version, not once per construction
            new_step, self.step_versions = self.step_versions != versions, versions
            hit = self.sets[flavour] = (versions, TrainOperands(self, *flavour, new_step=new_step))
        self.latest = hit[1]
        return hit[1]

    def _prepare(self, grid: bool, rois: bool, new_step: bool) -> dict:
        """{(conv, tag): SplitWeight} of a split-arithmetic step out of ONE launch (ops.res5_weight_prep) into buffers kept here,
        once a scale is remembered for every operand; {} sends the step to the on-demand chain, which chooses them (first step,
        odd shapes).  A remembered scale is used once per counted step."""
        wanted = []
        for blk in self.stage:
            for conv in (blk.conv1, blk.conv3, blk.shortcut):
                if conv is not None:
                    wanted += [(conv, "plain"), (conv, "t")]
            wanted += [(blk.conv2, "wino"), (blk.conv2, "uflip")] if rois else []
            wanted += [(blk.conv2, "col"), (blk.conv2, "flip9")] if grid else []
        if new_step:
            self._count_step()
        recs = [self.scales.get(key) for key in wanted]
        if not (_ONE_LAUNCH_PREP and any(r is not None for r in recs) and all(
                conv.weight.is_cuda and conv.weight.dtype == torch.float32 and conv.weight.is_contiguous()
                and conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0 and conv.groups == 1 for conv, _ in wanted)):
            return {}
        if None in recs:
            # SOME scales are remembered: the others belong to operands the previous steps never asked for (block 0's data
            # gradient when the stage input needs none: a frozen backbone) -- on the on-demand chain they would stay unknown for
            # good and keep every step off the one launch.  They are built here by that chain (one host read each).
            for (conv, tag), rec in zip(wanted, recs):
                if rec is None:
                    self.for_gemm(conv, tag, True)
            recs = [self.scales.get(key) for key in wanted]
            if None in recs:
                return {}
        if any(r[1] >= self.REFRESH for r in recs):          # (the old scales stay in use until the new ones are adopted)
            self._start_refresh(wanted)
        ready, jobs = {}, []
        for (conv, tag), (scale, uses) in zip(wanted, recs):
            w = conv.weight.detach()
            shape = ops.prep_shape(tag, w)
            buf = self.prep_bufs.get((grid, rois, conv, tag))                # (per flavour: see train_operands)
            if buf is None or tuple(buf.shape) != shape or buf.device != w.device:
                buf = self.prep_bufs[(grid, rois, conv, tag)] = torch.empty(shape, dtype=torch.float32, device=w.device)
            jobs.append((tag, w, self.fold(conv)[0] if tag in ROW_SCALED else None, buf, scale))
            if new_step:
                self.scales[(conv, tag)] = (scale, uses + 1)
            ready[(conv, tag)] = ops.SplitWeight(buf, scale)
        ops.res5_weight_prep(jobs)
        return ready


class TrainOperands:
    """Every weight-derived GEMM operand of ONE training step of the stage: get(conv, tag) -> ops.SplitWeight (split arithmetic,
    eligible shape) | fp32 tensor.  `ready` holds what the step's one preparation launch made (Res5Operands._prepare); everything
    else (first step, the f32 MFMA, odd shapes) is built on demand by the owner's multi-launch chain, which also chooses the scales."""

    def __init__(self, owner: Res5Operands, split: bool, grid: bool, rois: bool, new_step: bool = True):
        self.owner, self.split = owner, bool(split)
        self.ready = owner._prepare(grid, rois, new_step) if self.split else {}

    def get(self, conv, tag: str):
        hit = self.ready.get((conv, tag))
        return hit if hit is not None else self.owner.for_gemm(conv, tag, self.split)
