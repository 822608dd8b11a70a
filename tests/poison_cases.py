"""The case table of the poisoned-output tests (tests/poison.py): one small invocation per C entry point that launches a kernel or
writes device memory, at the smallest shape at which the kernel can still go wrong -- more than one workgroup, one full tile plus
a ragged remainder in every tiled dimension, at least two images (one empty where the op takes it), one case per dispatch tier
that is cheap to reach.

Importable without a GPU: build() makes CPU inputs from a seed; run(d) receives them on the device and returns EVERY tensor the
op returns or documents as written (outputs, saved-for-backward buffers, gradients, counts, flag words; None for an absent one).
history: a second, larger build() whose call runs first in the same scratch (the stale data are then a real call's).
env: LOCOV_* dispatch switches the case is run under.  tier(n, inputs): asserts that the case ran on the dispatch tier its
name claims -- n[class] are the GEMM launches the library recorded during the run (locov_gemm_timing_read's classes: 0 the f32
128 x 128 tile, 2 the other f32 tiles, 5 the split 128 x 128 tile, 6 / 7 the TN kernel in f32 / split arithmetic, 8 the 256 x 256
tile with the Winograd epilogue, 9 / 10 / 11 that tile plain / batched / mean-fused); where the choice is made outside the GEMM
kernels it restates the library's rule on the case's own inputs (as caption_cases.fwd_tier does).  unspecified: (output index, mask builder(outputs) -> bool tensor that is
True where the content is DEFINED, the sentence of include/locov_hip.h or of the docstring that leaves the rest open)."""
from __future__ import annotations

import ctypes
import math
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch

import poison

CLAMP = math.log(1000.0 / 16)
W1 = (1.0, 1.0, 1.0, 1.0)
W10 = (10.0, 10.0, 5.0, 5.0)
INF = float("inf")


class Case(NamedTuple):
    name: str
    covers: Tuple[str, ...]
    build: Callable[[], dict]
    run: Callable[[dict], list]
    history: Optional[Callable[[], dict]] = None
    env: Optional[dict] = None
    unspecified: tuple = ()
    tier: Optional[Callable] = None


CASES = []


GEMM_CLASSES = (0, 2, 5, 6, 7, 8, 9, 10, 11)


def launches(**want):
    """tier check on the launch record: launches(c5=2, c9=0) -> class 5 launched twice, class 9 not at all."""
    def check(n, inputs):
        got = {k: n[int(k[1:])] for k in want}
        assert got == want, f"GEMM launches by class: want {want}, the library recorded {n}"
    return check


def case(name, covers, build, history=None, env=None, unspecified=(), tier=None):
    def deco(run):
        CASES.append(Case(name, tuple(covers), build, run, history, env, tuple(unspecified), tier))
        return run
    return deco


def to_device(obj, device="cuda"):
    if isinstance(obj, torch.Tensor):
        return obj.to(device)
    if isinstance(obj, dict):
        return {k: to_device(v, device) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and obj and all(isinstance(v, torch.Tensor) for v in obj):
        return type(obj)(to_device(v, device) for v in obj)
    return obj


# ------------------------------------------------------------------------------------------------ input builders (CPU, seeded)
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _rand(g, *shape):
    return torch.rand(*shape, generator=g)


def _boxes(g, n, extent=(800.0, 600.0), max_side=200.0, crowd=0):
    """n XYXY fp32 boxes on a half-pixel lattice; crowd > 0: jittered copies of that many boxes (suppression chains)."""
    m = crowd or n
    xy = _rand(g, m, 2) * torch.tensor(extent)
    wh = _rand(g, m, 2) * max_side + 4.0
    b = torch.cat([xy, xy + wh], dim=1)
    if crowd:
        b = b[torch.arange(n) % crowd] + _randn(g, n, 4, scale=3.0)
        b[:, 2:] = torch.maximum(b[:, 2:], b[:, :2] + 2.0)
    return (b * 2).round() / 2


def _ints(g, lo, hi, *shape, dtype=torch.int64):
    return torch.randint(lo, hi, shape, generator=g).to(dtype)


def _ops():
    from locov_amd import ops
    return ops


def _lib():
    from locov_amd import _lib
    return _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check(rc, what):
    from locov_amd import _lib
    _lib.check(rc, what)


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _i32(values, dev):
    return torch.tensor(list(values), dtype=torch.int32, device=dev)


# ================================================================================================ cached scratch / multi-launch ops
def _rpn_inputs(N, HWA, seed, crowd):
    def build():
        g = _g(seed)
        return dict(logits=_randn(g, N, HWA), deltas=_randn(g, N, HWA, 4, scale=0.2), anchors=_boxes(g, HWA, crowd=crowd), N=N)
    return build


def _rpn_run(pre, post):
    def run(d):
        ops = _ops()
        out, flags = ops._rpn_proposals_flags(d["logits"], d["deltas"], d["anchors"], [(600, 800), (480, 640)][:d["N"]], W1, CLAMP, pre, post,
                                              0.0, 0.7)
        return [out[0], out[1], out[2], _i32(out[3], out[0].device), _i32([flags], out[0].device)]
    return run


case("rpn_proposals_chain129", ["locov_rpn_proposals"], _rpn_inputs(2, 321, 1, crowd=37),
     history=_rpn_inputs(2, 2000, 2, crowd=300))(_rpn_run(129, 100))
case("rpn_proposals_hwa65", ["locov_rpn_proposals"], _rpn_inputs(2, 65, 3, crowd=0))(_rpn_run(65, 20))


def _nms_inputs(K, seed, crowd):
    def build():
        g = _g(seed)
        return dict(boxes=_boxes(g, K, crowd=crowd), scores=_rand(g, K))
    return build


@case("nms_321", ["locov_nms_sorted"], _nms_inputs(321, 4, 40), history=_nms_inputs(1500, 5, 200))
def _(d):
    return [_ops().nms(d["boxes"], d["scores"], 0.5)]


def _detect_inputs(sizes, K, seed, cs=False, crowd=25):
    def build():
        g = _g(seed)
        R = sum(sizes)
        probs = torch.softmax(_randn(g, R, K + 1, scale=2.0), dim=1)
        return dict(probs=probs, deltas=_randn(g, R, 4 * K if cs else 4, scale=0.2), props=_boxes(g, R, crowd=crowd), sizes=list(sizes), K=K)
    return build


def _detect_run(per_class_above, topk=40):
    def run(d):
        ops = _ops()
        shapes = [(600, 800), (480, 640), (333, 500)][:len(d["sizes"])]
        out, flags = ops._detect_postprocess_flags(d["probs"], d["deltas"], d["props"], d["sizes"], shapes, W10, CLAMP, 0.05, 0.5, topk,
                                                   per_class_above=per_class_above)
        return [out[0], out[1], out[2], out[3], _i32(out[4], out[0].device), _i32([flags], out[0].device)]
    return run


_DET = ([70, 0, 61], 5)
case("detect_postprocess", ["locov_detect_postprocess"], _detect_inputs(*_DET, 6),
     history=_detect_inputs([400, 300, 100], 7, 7))(_detect_run(None))
case("detect_postprocess_cs", ["locov_detect_postprocess_cs"], _detect_inputs(*_DET, 8, cs=True),
     history=_detect_inputs([400, 300, 100], 7, 9, cs=True))(_detect_run(None))
case("detect_postprocess_wide_shifted", ["locov_detect_postprocess_wide"], _detect_inputs(*_DET, 10),
     history=_detect_inputs([400, 300, 100], 7, 11))(_detect_run(2 ** 31 - 1))
case("detect_postprocess_wide_per_class", ["locov_detect_postprocess_wide"], _detect_inputs(*_DET, 12),
     history=_detect_inputs([400, 300, 100], 7, 13))(_detect_run(0))
case("detect_postprocess_wide_cs_shifted", ["locov_detect_postprocess_wide_cs"], _detect_inputs(*_DET, 14, cs=True),
     history=_detect_inputs([400, 300, 100], 7, 15, cs=True))(_detect_run(2 ** 31 - 1))
case("detect_postprocess_wide_cs_per_class", ["locov_detect_postprocess_wide_cs"], _detect_inputs(*_DET, 16, cs=True),
     history=_detect_inputs([400, 300, 100], 7, 17, cs=True))(_detect_run(0))


# a call without a single proposal launches nothing: the entry points (det_run of detect.hip, dw_run of detect_wide.hip) fill the slots
_NONE = ([0, 0], 5)
case("detect_postprocess_no_proposals", ["locov_detect_postprocess"], _detect_inputs(*_NONE, 18))(_detect_run(None))
case("detect_postprocess_cs_no_proposals", ["locov_detect_postprocess_cs"], _detect_inputs(*_NONE, 19, cs=True))(_detect_run(None))
case("detect_postprocess_wide_no_proposals", ["locov_detect_postprocess_wide"], _detect_inputs(*_NONE, 20))(_detect_run(0))
case("detect_postprocess_wide_cs_no_proposals", ["locov_detect_postprocess_wide_cs"], _detect_inputs(*_NONE, 21, cs=True))(_detect_run(2 ** 31 - 1))


# ------------------------------------------------------------------------------------------------ Winograd convolutions
def _wino_inputs(R, C, N, seed):
    def build():
        g = _g(seed)
        return dict(x=_randn(g, 49 * R, C).relu(), w=_randn(g, N, C, 3, 3, scale=0.05), sc=_rand(g, N) + 0.5, sh=_randn(g, N, scale=1e-3),
                    mask=_randn(g, 49 * R, N), gy=_randn(g, 49 * R, N, scale=1e-3), rs=_rand(g, N) + 0.5, R=R)
    return build


_WINO, _WINO_BIG = _wino_inputs(5, 32, 36, 20), _wino_inputs(19, 64, 96, 21)


@case("winograd_conv3x3_f32", ["locov_winograd_pack_weight", "locov_winograd_conv3x3_f32"], _WINO, history=_WINO_BIG)
def _(d):
    ops = _ops()
    U = ops.winograd_pack_weight(d["w"])
    pos = ops.winograd_conv3x3(d["x"], U, scale=d["sc"], shift=d["sh"], relu=True)
    poison.repoison_scratch()                                              # the ROI-major form starts on poisoned V and M too
    return [U, pos, ops.winograd_conv3x3(d["x"], U, roi_major=True, in_roi_major=True)]


def _wino_split(d, **kw):
    ops = _ops()
    Up = ops.split_pack(ops.winograd_pack_weight(d["w"]))
    return [Up.data, ops.winograd_conv3x3(d["x"], Up, scale=d["sc"], shift=d["sh"], relu=True, **kw)]


case("winograd_conv3x3_split_128", ["locov_winograd_conv3x3_f32_split_ex", "locov_split_f16x2_pack"], _wino_inputs(5, 32, 36, 22),
     history=_wino_inputs(19, 64, 96, 23), env={"LOCOV_SPLIT_BIG": "0"}, tier=launches(c5=1, c10=0))(lambda d: _wino_split(d, roi_major=True, in_roi_major=True))
case("winograd_conv3x3_split_256", ["locov_winograd_conv3x3_f32_split_ex"], _wino_inputs(5, 64, 40, 24),
     history=_wino_inputs(19, 64, 96, 25), env={"LOCOV_SPLIT_BIG": "1"}, tier=launches(c5=0, c10=1))(lambda d: _wino_split(d))
case("winograd_conv3x3_split_outsplit", ["locov_winograd_conv3x3_f32_split_ex"], _wino_inputs(5, 32, 64, 26),
     env={"LOCOV_SPLIT_BIG": "0"}, tier=launches(c5=1, c10=0))(lambda d: _wino_split(d, roi_major=True, in_roi_major=True, out_split_scale=16.0))


@case("winograd_conv3x3_split_legacy_entry", ["locov_winograd_conv3x3_f32_split"], _wino_inputs(5, 32, 36, 27), history=_wino_inputs(19, 64, 96, 28))
def _(d):
    ops, lib = _ops(), _lib()
    Up = ops.split_pack(ops.winograd_pack_weight(d["w"]))
    x, R = d["x"], d["R"]
    Cin, N = x.shape[1], Up.data.shape[1]
    y = torch.empty((49 * R, N), dtype=torch.float32, device=x.device)
    ws = ops._workspace("wino", x, int(lib.locov_winograd_workspace_bytes(R, Cin, N)))
    word = torch.zeros(1, dtype=torch.int32, device=x.device)
    _check(lib.locov_winograd_conv3x3_f32_split(_p(x), R, Cin, _p(Up.data), Up.scale, 0.25, _p(d["sc"]), _p(d["sh"]), _p(y), N, N, 1, _p(ws),
                                                ws.numel(), _p(word), _stream(x)), "locov_winograd_conv3x3_f32_split")
    return [y, word]


@case("winograd_conv3x3_ex_masked", ["locov_winograd_conv3x3_f32_ex"], _wino_inputs(5, 32, 36, 29), history=_wino_inputs(19, 64, 96, 30))
def _(d):
    ops = _ops()
    return [ops.winograd_conv3x3_ex(d["x"], ops.winograd_pack_weight(d["w"]), mask=d["mask"])]


@case("winograd_conv3x3_split_ex_device_scale", ["locov_winograd_conv3x3_f32_split_ex"], _wino_inputs(5, 32, 36, 31),
      history=_wino_inputs(19, 64, 96, 32))
def _(d):
    ops = _ops()
    Up = ops.split_pack(ops.winograd_pack_weight(d["w"]))
    amax = torch.zeros(4, dtype=torch.float32, device=d["x"].device)
    y = ops.winograd_conv3x3_split_ex(d["x"], Up, mask=d["mask"], amax_out=amax)
    slot = ops.winograd_scale_slot(d["x"], d["R"], d["x"].shape[1], Up.data.shape[1]).clone()
    return [y, amax, slot[:3]]


def _wgrad_run(split, v_split=False):
    def run(d):
        ops = _ops()
        x, gy = d["x"], d["gy"]
        if not v_split:
            return [ops.winograd_wgrad(x, gy, d["rs"], split=split)]
        Up = ops.split_pack(ops.winograd_pack_weight(d["w"]))
        ws = torch.empty(ops.winograd_workspace_bytes(d["R"], x.shape[1], gy.shape[1]), dtype=torch.uint8, device=x.device)
        y = ops.winograd_conv3x3(x, Up, roi_major=True, in_roi_major=True, workspace=ws)
        return [y, ops.winograd_wgrad(x, gy, d["rs"], split=True, v_split=ws)]
    return run


case("winograd_wgrad_f32", ["locov_winograd_wgrad_f32"], _wino_inputs(5, 32, 36, 33), history=_wino_inputs(19, 64, 96, 34))(_wgrad_run(False))
case("winograd_wgrad_split", ["locov_winograd_wgrad_f32_split"], _wino_inputs(5, 32, 36, 35), history=_wino_inputs(19, 64, 96, 36))(_wgrad_run(True))
case("winograd_wgrad_split_v", ["locov_winograd_wgrad_f32_split_v"], _wino_inputs(5, 32, 36, 37),
     history=_wino_inputs(19, 64, 96, 38))(_wgrad_run(True, v_split=True))


def _c1w_inputs(R, K, C, N, seed):
    def build():
        g = _g(seed)
        return dict(x=_randn(g, 49 * R, K).relu(), w1=_randn(g, C, K, scale=0.05), s1=_rand(g, C) + 0.5, b1=_randn(g, C, scale=1e-3),
                    w2=_randn(g, N, C, 3, 3, scale=0.03), s2=_rand(g, N) + 0.5, b2=_randn(g, N, scale=1e-3))
    return build


def _c1w_run(d):
    ops = _ops()
    xs = ops.split_pack(d["x"], 16.0).data
    w1p = ops.split_pack(d["w1"])
    Up = ops.split_pack(ops.winograd_pack_weight(d["w2"]))
    return [ops.conv1x1_winograd_conv3x3(xs, w1p, d["b1"], Up, scale1=d["s1"], scale2=d["s2"], shift2=d["b2"], relu=True, x_scale=16.0)]


case("conv1x1_winograd_fused", ["locov_conv1x1_winograd_conv3x3_f32_split"], _c1w_inputs(7, 64, 256, 64, 40),
     history=_c1w_inputs(23, 192, 256, 64, 41), env={"LOCOV_WINO_FUSE": "1", "LOCOV_SPLIT_BIG": "1"}, tier=launches(c8=1, c9=0, c10=1, c5=0))(_c1w_run)
case("conv1x1_winograd_unfused", ["locov_conv1x1_winograd_conv3x3_f32_split"], _c1w_inputs(7, 64, 96, 36, 42),
     history=_c1w_inputs(23, 192, 256, 64, 43), env={"LOCOV_WINO_FUSE": "0", "LOCOV_SPLIT_BIG": "0"}, tier=launches(c8=0, c9=0, c10=0, c5=2))(_c1w_run)


def _raw_inputs(Nimg, H, W, C, R, N, seed):
    def build():
        g = _g(seed)
        wh = _rand(g, R, 2) * torch.tensor([W * 16.0, H * 16.0]) * 0.9 + 4.0
        xy = _rand(g, R, 2) * torch.tensor([W * 16.0, H * 16.0]) - 20.0
        rois = torch.cat([_ints(g, 0, Nimg, R, 1).float(), xy, xy + wh], dim=1)
        return dict(feat=_randn(g, Nimg, H, W, C), rois=rois, s1=_rand(g, C) + 0.5, b1=_randn(g, C, scale=1e-4),
                    w2=_randn(g, N, C, 3, 3, scale=0.03), s2=_rand(g, N) + 0.5, b2=_randn(g, N, scale=1e-3))
    return build


def _raw_tier(fused):
    """roi_align_nhwc.hip's rule (the choice is made in the ROIAlign kernel, which the GEMM record does not see): the pooled rows stay
    in the workgroup when LOCOV_WINO_FUSE is not 0 and C % 64 == 0."""
    def check(n, inputs):
        import os
        C = inputs["feat"].shape[3]
        assert (os.environ.get("LOCOV_WINO_FUSE") != "0" and C % 64 == 0) == fused, (os.environ.get("LOCOV_WINO_FUSE"), C)
    return check


def _raw_run(d):
    ops = _ops()
    Up = ops.split_pack(ops.winograd_pack_weight(d["w2"]))
    return [ops.roi_align_winograd_conv3x3(d["feat"], d["rois"], 14, 1.0 / 16, 0, True, Up, ch_scale=d["s1"], ch_shift=d["b1"], scale2=d["s2"],
                                           shift2=d["b2"], relu=True)]


case("roi_align_winograd_fused", ["locov_roi_align_winograd_conv3x3_f32_split"], _raw_inputs(2, 13, 17, 64, 9, 36, 44),
     history=_raw_inputs(2, 25, 38, 128, 37, 64, 45), env={"LOCOV_WINO_FUSE": "1"}, tier=_raw_tier(True))(_raw_run)
case("roi_align_winograd_unfused", ["locov_roi_align_winograd_conv3x3_f32_split"], _raw_inputs(2, 13, 17, 32, 9, 36, 46),
     history=_raw_inputs(2, 25, 38, 128, 37, 64, 47), env={"LOCOV_WINO_FUSE": "0"}, tier=_raw_tier(False))(_raw_run)


# ------------------------------------------------------------------------------------------------ TN GEMMs, mean-fused GEMM
def _tn_inputs(M, N, K, seed):
    def build():
        g = _g(seed)
        return dict(a=_randn(g, M, N, scale=1e-3), b=_randn(g, M, K).relu(), rs=_rand(g, N) + 0.5)
    return build


@case("gemm_tn_777x64x96", ["locov_gemm_tn_f32"], _tn_inputs(777, 64, 96, 50), history=_tn_inputs(49 * 31, 132, 96, 51),
      tier=launches(c6=1, c7=0))
def _(d):
    return [_ops().gemm_tn(d["a"], d["b"], d["rs"])]


@case("gemm_tn_split", ["locov_gemm_tn_f32_split", "locov_split_scale_from_amax_zeroed"], _tn_inputs(777, 64, 96, 52),
      history=_tn_inputs(49 * 31, 132, 96, 53), tier=launches(c6=0, c7=1))
def _(d):
    ops = _ops()
    slot = ops.split_scale_from_amax(d["a"])
    return [ops.gemm_tn_split(d["a"], d["b"], d["rs"], slot, 16.0), slot.clone()]


@case("gemm_tn_split_b", ["locov_gemm_tn_f32_split_b"], _tn_inputs(777, 64, 96, 54), history=_tn_inputs(49 * 31, 132, 96, 55),
      tier=launches(c6=0, c7=1))
def _(d):
    ops = _ops()
    slot = ops.split_scale_from_amax(d["a"])
    bs = ops.split_pack(d["b"], 16.0).data
    return [ops.gemm_tn_split(d["a"], bs, d["rs"], slot, 16.0, b_is_split=True)]


def _segmean_inputs(R, N, K, seed):
    def build():
        g = _g(seed)
        M = 49 * R
        return dict(x=_randn(g, M, K).relu(), w=_randn(g, N, K, scale=0.05), sc=_rand(g, N) + 0.5, sh=_randn(g, N, scale=1e-3),
                    res=_randn(g, M, N, scale=1e-2))
    return build


@case("linear_split_segmean_128", ["locov_gemm_nt_f32_split_segmean"], _segmean_inputs(7, 132, 64, 56), history=_segmean_inputs(53, 264, 160, 57),
      env={"LOCOV_SPLIT_BIG": "0"}, tier=launches(c5=1, c11=0))
def _(d):
    ops = _ops()
    return [ops.linear_split_segmean(d["x"], ops.split_pack(d["w"]), d["sh"], d["res"], 49, scale=d["sc"])]


@case("linear_split_segmean_256", ["locov_gemm_nt_f32_split_segmean"], _segmean_inputs(7, 136, 64, 58), history=_segmean_inputs(53, 264, 192, 59),
      env={"LOCOV_SPLIT_BIG": "1"}, tier=launches(c5=0, c11=1))
def _(d):
    ops = _ops()
    xs = ops.split_pack(d["x"], 16.0).data
    return [ops.linear_split_segmean(xs, ops.split_pack(d["w"]), d["sh"], d["res"], 49, scale=d["sc"], residual_roi_major=True, x_is_split=True)]


# ------------------------------------------------------------------------------------------------ predictor backward
def _poolfc_inputs(R, C5, D, seed):
    def build():
        g = _g(seed)
        return dict(x=_randn(g, R, C5), ew=_randn(g, D, C5, scale=0.05), eb=_randn(g, D, scale=0.1), bw=_randn(g, 4, C5, scale=0.05),
                    bb=_randn(g, 4, scale=0.1), ge=_randn(g, R, D), gb=_randn(g, R, 4))
    return build


@case("pool_fc_autograd", ["locov_pool_fc_bwd", "locov_gemm_nt_f32"], _poolfc_inputs(133, 68, 36, 60), history=_poolfc_inputs(600, 256, 96, 61))
def _(d):
    leaves = [_leaf(d[k]) for k in ("x", "ew", "eb", "bw", "bb")]
    emb, box = _ops().pool_fc_autograd(*leaves)
    torch.autograd.backward([emb, box], [d["ge"], d["gb"]])
    return [emb.detach(), box.detach()] + [t.grad for t in leaves]


def _sim_inputs(R, D, K1, seed):
    def build():
        g = _g(seed)
        return dict(emb=_randn(g, R, D), bank=_randn(g, K1, D, scale=0.2), bias=_randn(g, K1, scale=0.1), g=_randn(g, R, K1))
    return build


@case("sim_gemm_autograd", ["locov_sim_gemm_bwd"], _sim_inputs(133, 36, 68, 62), history=_sim_inputs(600, 96, 132, 63))
def _(d):
    leaves = [_leaf(d[k]) for k in ("emb", "bank", "bias")]
    y = _ops().sim_gemm_autograd(*leaves)
    y.backward(d["g"])
    return [y.detach()] + [t.grad for t in leaves]


# ------------------------------------------------------------------------------------------------ ResNet stem
def _stem_inputs(N, H, W, seed):
    def build():
        g = _g(seed)
        PH, PW = ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2
        return dict(images=_randn(g, N, 3, H, W), w=_randn(g, 64, 3, 7, 7, scale=0.05), sc=_rand(g, 64) + 0.5, sh=_randn(g, 64, scale=0.1),
                    g=_randn(g, N, PH, PW, 64))
    return build


@case("resnet_stem_train_wgrad", ["locov_resnet_stem_fwd_sel", "locov_resnet_stem_wgrad", "locov_resnet_stem_fwd"], _stem_inputs(2, 37, 51, 64),
      history=_stem_inputs(2, 90, 131, 65))
def _(d):
    ops = _ops()
    y, sel = ops.resnet_stem_train(d["images"], d["w"], d["sc"], d["sh"])
    return [y, sel, ops.resnet_stem_wgrad(d["images"], d["g"], sel, d["sc"]), ops.resnet_stem(d["images"], d["w"], d["sc"], d["sh"])]


# ------------------------------------------------------------------------------------------------ SGD
def _sgd_inputs(counts, seed):
    def build():
        g = _g(seed)
        return dict(params=[_randn(g, c + 3) for c in counts], grads=[_randn(g, c + 3) for c in counts], counts=list(counts))
    return build


def _sgd_run(clip, offset):
    def run(d):
        ops = _ops()
        # offset 0: every chunk 16-byte aligned (the vector form); 1: views one float past alignment (the scalar form)
        cut = lambda t, c: t[offset:offset + c]
        params = [cut(p.clone(), c) for p, c in zip(d["params"], d["counts"])]
        grads = [cut(q, c) for q, c in zip(d["grads"], d["counts"])]
        bufs = [torch.empty_like(p) for p in params]
        n = len(params)
        table = ops.SgdTable()
        ops.sgd_step(table, params, grads, bufs, [i % 2 for i in range(n)], [True] * n, [0.1, 0.02], [1e-4, 0.0], momentum=0.9, clip_type=clip,
                     clip_value=0.5)
        poison.repoison_scratch(table._workspace)                          # the second step's partial sums and coefficients: its own
        ops.sgd_step(table, params, grads, bufs, [i % 2 for i in range(n)], [False] * n, [0.1, 0.02], [1e-4, 0.0], momentum=0.9, nesterov=True,
                     clip_type=clip, clip_value=0.5)
        return params + bufs
    return run


_SGD = [4096 + 5, 7, 4096, 2 * 4096 + 1]
case("sgd_step_norm_clip_aligned", ["locov_sgd_step"], _sgd_inputs(_SGD, 66))(_sgd_run("norm", 0))
case("sgd_step_norm_clip_scalar", ["locov_sgd_step"], _sgd_inputs(_SGD, 68))(_sgd_run("norm", 1))
case("sgd_step_value_clip", ["locov_sgd_step"], _sgd_inputs(_SGD, 69))(_sgd_run("value", 0))


# ------------------------------------------------------------------------------------------------ classification losses
def _cls_inputs(R, C, seed):
    def build():
        g = _g(seed)
        gt = _ints(g, 0, C, R)
        gt[::7] = C - 1
        return dict(scores=_randn(g, R, C, scale=2.0), gt=gt, w=_rand(g, C - 1) + 0.1, rnd=-torch.log(_rand(g, C - 1).clamp_min(1e-6)))
    return build


@case("cls_loss", ["locov_cls_loss"], _cls_inputs(333, 81, 70), history=_cls_inputs(2000, 81, 71))
def _(d):
    s = _leaf(d["scores"])
    loss, stats = _ops().cls_loss(s, d["gt"])
    loss.backward()
    return [loss.detach(), stats, s.grad]


@case("sigmoid_cls_loss_fed", ["locov_sigmoid_cls_loss", "locov_fed_loss_classes"], _cls_inputs(333, 81, 72), history=_cls_inputs(2000, 81, 73))
def _(d):
    ops = _ops()
    mask, counts = ops.fed_loss_classes(d["gt"], d["w"], 20, rnd=d["rnd"])
    s = _leaf(d["scores"])
    loss, stats = ops.sigmoid_cls_loss(s, d["gt"], mask)
    loss.backward()
    return [mask, counts, loss.detach(), stats, s.grad]


# ------------------------------------------------------------------------------------------------ RPN training
def _rpnt_inputs(N, HWA, n_gt, seed):
    def build():
        g = _g(seed)
        anchors = _boxes(g, HWA, crowd=max(HWA // 6, 1))
        # every second box lies far from every anchor: its best anchor stays below the upper threshold, so only the low-quality rule
        # (the per-box maxima kept in the workspace) makes that anchor a positive
        M = sum(n_gt)
        gt = anchors[torch.randperm(HWA, generator=g)[:M]] + _randn(g, M, 4, scale=2.0)
        gt[::2] = gt[::2] + torch.tensor([-35.0, -30.0, 40.0, 45.0])
        return dict(anchors=anchors, gt=gt, n_gt=list(n_gt), rnd=_rand(g, 2, N, HWA).double(), logits=_randn(g, N, HWA),
                    deltas=_randn(g, N, HWA, 4, scale=0.3))
    return build


@case("rpn_label_sample_loss", ["locov_rpn_label_anchors", "locov_rpn_sample_anchors", "locov_rpn_loss"], _rpnt_inputs(3, 321, [5, 0, 3], 74),
      history=_rpnt_inputs(3, 3000, [20, 1, 9], 75))
def _(d):
    ops = _ops()
    N = len(d["n_gt"])
    labels, matched, counts = ops.rpn_label_anchors(d["anchors"], d["gt"], d["n_gt"], [(600, 800)] * N, [-INF, 0.3, 0.7, INF], [0, -1, 1],
                                                    boundary_thresh=0.0)
    before = counts.clone()
    final = ops.rpn_sample_anchors(labels, counts, d["rnd"], 64, 32)
    lg, dl = _leaf(d["logits"]), _leaf(d["deltas"])
    loss, flags = ops.rpn_loss(lg, dl, final, d["anchors"], matched, W1, 1.0 / 9, 1.0 / 192, 1.0 / 192)
    (loss[0] + 2.0 * loss[1]).backward()
    return [labels, matched, before, final, counts, loss.detach(), flags, lg.grad, dl.grad]


# ------------------------------------------------------------------------------------------------ proposal labelling / sampling
def _label_inputs(n_props, n_gt, seed):
    def build():
        g = _g(seed)
        R, M = sum(n_props), sum(n_gt)
        gt = _boxes(g, M, max_side=300.0)
        boxes = torch.cat([gt[_ints(g, 0, M, R // 2)] + _randn(g, R // 2, 4, scale=6.0), _boxes(g, R - R // 2)])
        boxes[:, 2:] = torch.maximum(boxes[:, 2:], boxes[:, :2] + 2.0)
        return dict(boxes=boxes[torch.randperm(R, generator=g)], gt=gt, gt_cls=_ints(g, 0, 20, M), n_props=list(n_props), n_gt=list(n_gt),
                    rnd=_rand(g, 2, R).double(), field=_randn(g, R))
    return build


@case("label_sample_proposals", ["locov_label_proposals", "locov_sample_proposals"], _label_inputs([130, 70], [4, 2], 76))
def _(d):
    ops = _ops()
    gt_index, labels, kp, kn, rows = ops.label_proposals(d["boxes"], d["n_props"], d["gt"], d["gt_cls"], d["n_gt"], [-INF, 0.5, INF], [0, 1], 20,
                                                         d["rnd"])
    out = ops.sample_proposals(kp, kn, labels, gt_index, rows, d["boxes"], d["gt"], d["n_props"], d["n_gt"], 64, 16, 20, field=d["field"])
    return [gt_index, labels, kp, kn, rows, *out]


# ------------------------------------------------------------------------------------------------ evaluation
def _eval_inputs(I, K, n_det, gts_per_cell, seed, lvis=False):
    def build():
        g = _g(seed)
        C = I * K
        gcount = [(gts_per_cell if (c % 3) else 0) for c in range(C)]
        G = sum(gcount)
        gt_xyxy = _boxes(g, G, max_side=120.0)
        gt_xywh = torch.cat([gt_xyxy[:, :2], gt_xyxy[:, 2:] - gt_xyxy[:, :2]], dim=1).double()
        cell_of_gt = torch.repeat_interleave(torch.arange(C), torch.tensor(gcount))
        # dets: half of them jittered copies of ground truth of their own cell, the rest anywhere
        pick = _ints(g, 0, G, n_det)
        near = torch.arange(n_det) % 2 == 0
        det = torch.where(near[:, None], gt_xyxy[pick] + _randn(g, n_det, 4, scale=4.0), _boxes(g, n_det, max_side=120.0))
        det[:, 2:] = torch.maximum(det[:, 2:], det[:, :2] + 1.0)
        cell = torch.where(near, cell_of_gt[pick], _ints(g, 0, C, n_det))
        return dict(img=cell % I, cls=cell // I, score=(_ints(g, 0, 64, n_det).double() / 64), det=det, I=I, K=K,
                    gt_off=torch.tensor([0] + list(np.cumsum(gcount)), dtype=torch.int32), gt=gt_xywh, area=gt_xywh[:, 2] * gt_xywh[:, 3],
                    flag=(_ints(g, 0, 8, G) == 0).to(torch.uint8), cell_flags=_ints(g, 0, 4, C).to(torch.uint8),
                    npig=_ints(g, 1, 9, K, 2, dtype=torch.int32))
    return build


_AREAS, _THRS = [[0.0, 1e10], [0.0, 4096.0]], [0.5, 0.75]


def _eval_run(lvis):
    def run(d):
        ops = _ops()
        o = ops.coco_order(d["img"], d["cls"], d["score"], d["det"], d["I"], d["K"])
        if lvis:
            bits, ign = ops.lvis_match(o.det_offsets, d["gt_off"], d["cell_flags"], o.boxes, d["gt"], d["area"], d["flag"], _AREAS, _THRS, 300)
        else:
            bits, ign = ops.coco_match(o.det_offsets, d["gt_off"], o.boxes, d["gt"], d["area"], d["flag"], _AREAS, _THRS, 100)
        flat = ops.coco_accumulate(o.cat_offsets, o.acc_index, o.acc_rank, o.acc_score, bits, d["npig"], len(_THRS), [1, 10, 100],
                                   np.linspace(0.0, 1.0, 11))
        return [bits, ign, flat]
    return run


def _cell_tier(lds, max_det):
    """coco_eval.hip's rule for a cell of D dets (capped) and G gts: matrix and flags in the wave's LDS slice while
    D * G * 8 + G * 64 <= 8192, else in the workspace."""
    def check(n, d):
        C = d["I"] * d["K"]
        cell = (d["cls"] * d["I"] + d["img"]).tolist()
        off = d["gt_off"].tolist()
        fits = []
        for c in range(C):
            D, G = min(cell.count(c), max_det), off[c + 1] - off[c]
            if D and G:
                fits.append(D * G * 8 + G * 64 <= 8192)
        assert fits and (all(fits) if lds else not any(fits)), fits
    return check


# (cells of ~8 dets and 3 gts keep the IoU matrix in LDS; ~80 dets and 30 gts put it in the workspace: D * G * 8 + G * 64 > 8192)
case("coco_match_accumulate_lds", ["locov_coco_match", "locov_coco_accumulate"], _eval_inputs(3, 2, 60, 3, 80),
     history=_eval_inputs(3, 2, 600, 30, 81), tier=_cell_tier(True, 100))(_eval_run(False))
case("coco_match_workspace", ["locov_coco_match", "locov_coco_accumulate"], _eval_inputs(2, 2, 330, 30, 82),
     history=_eval_inputs(3, 2, 900, 60, 83), tier=_cell_tier(False, 100))(_eval_run(False))
case("lvis_match_lds", ["locov_lvis_match"], _eval_inputs(3, 2, 60, 3, 84), history=_eval_inputs(3, 2, 600, 30, 85), tier=_cell_tier(True, 300))(_eval_run(True))
case("lvis_match_workspace", ["locov_lvis_match"], _eval_inputs(2, 2, 330, 30, 86), history=_eval_inputs(3, 2, 900, 60, 87),
     tier=_cell_tier(False, 300))(_eval_run(True))


def _recall_inputs(I, n_props, n_gt, seed):
    def build():
        g = _g(seed)
        gcount = [n_gt if i != 1 else 0 for i in range(I)]
        G = sum(gcount)
        gt = _boxes(g, G, max_side=150.0)
        pick = _ints(g, 0, G, n_props)
        near = torch.arange(n_props) % 2 == 0
        boxes = torch.where(near[:, None], gt[pick] + _randn(g, n_props, 4, scale=5.0), _boxes(g, n_props, max_side=150.0))
        boxes[:, 2:] = torch.maximum(boxes[:, 2:], boxes[:, :2] + 1.0)
        gimg = torch.repeat_interleave(torch.arange(I), torch.tensor(gcount))
        return dict(img=torch.where(near, gimg[pick], _ints(g, 0, I, n_props)), logits=_randn(g, n_props).double(), boxes=boxes,
                    gt_off=torch.tensor([0] + list(np.cumsum(gcount)), dtype=torch.int32), gt=gt, area=(gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]),
                    skip=(_ints(g, 0, 6, G) == 0).to(torch.uint8), n_gt=n_gt)
    return build


@case("proposal_recall", ["locov_proposal_recall"], _recall_inputs(3, 330, 9, 88))
def _(d):
    totals, overlaps = _ops().proposal_recall(d["img"], d["logits"], d["boxes"], d["gt_off"], d["gt"], d["area"], d["skip"], d["n_gt"],
                                              [[0.0, 1e10], [0.0, 9216.0]], [10, 100], np.arange(0.5, 0.96, 0.05))
    return [totals, overlaps]


# ------------------------------------------------------------------------------------------------ caption path
def _caption_inputs(B, T, H, V, seed):
    def build():
        g = _g(seed)
        N = B * T
        ids = _ints(g, 0, V, N, dtype=torch.int32)
        types = _ints(g, 0, 2, N, dtype=torch.int32)
        lens = _ints(g, 2, T + 1, B)
        att = (torch.arange(T)[None, :] < lens[:, None]).reshape(N).to(torch.int32)
        special = ((torch.arange(T)[None, :] == 0) | (torch.arange(T)[None, :] == lens[:, None] - 1)).reshape(N).to(torch.int32) * att
        return dict(packed=torch.stack([ids, types, att, special]), draws=_rand(g, 2, N).double(), T=T, V=V, W=_randn(g, V, H, scale=0.1),
                    P=_randn(g, T + 3, H, scale=0.1), Tt=_randn(g, 2, H, scale=0.1), gamma=_rand(g, H) + 0.5, beta=_randn(g, H, scale=0.1),
                    keep=(_rand(g, N, H) > 0.1).to(torch.uint8), g_in=_randn(g, N, H), g_enc=_randn(g, N, H))
    return build


def _caption_run(layer_norm):
    def run(d):
        ops = _ops()
        W = _leaf(d["W"])
        kw = dict(position=d["P"], token_type=d["Tt"], ln_weight=d["gamma"], ln_bias=d["beta"], keep=d["keep"], p_drop=0.1) if layer_norm else {}
        ints, emb, enc = ops.caption_embed(d["packed"], d["draws"], d["T"], W, mlm=ops.CaptionMlm(0.15, 0.8, 0.9, d["V"] - 1, d["V"]), **kw)
        if layer_norm:
            torch.autograd.backward([emb, enc], [d["g_in"], d["g_enc"]])
        else:
            emb.backward(d["g_in"])
        return [ints, emb.detach(), enc.detach() if enc is not None else None, W.grad]
    return run


case("caption_embed_layer_norm_h258", ["locov_caption_embed_fwd", "locov_caption_embed_bwd"], _caption_inputs(3, 7, 258, 50, 90),
     history=_caption_inputs(9, 33, 258, 300, 91))(_caption_run(True))
case("caption_embed_plain_h64", ["locov_caption_embed_fwd", "locov_caption_embed_bwd"], _caption_inputs(3, 7, 64, 50, 92),
     history=_caption_inputs(9, 33, 64, 300, 93))(_caption_run(False))
case("caption_embed_two_rank_rounds", ["locov_caption_embed_fwd", "locov_caption_embed_bwd"], _caption_inputs(25, 41, 8, 50, 94))(_caption_run(True))


# ------------------------------------------------------------------------------------------------ grounding regions
def _regions_grid_inputs(B, C, gh, gw, seed):
    def build():
        g = _g(seed)
        return dict(feat=_randn(g, B, C, gh, gw), keys=_rand(g, B, gh * gw).double(), g=_randn(g, B, 40, C), ext_h=[gh, 2, gh - 1][:B],
                    ext_w=[gw, 3, gw - 2][:B], gw=gw)
    return build


def _regions_grid_run(channels_last):
    def run(d):
        ops = _ops()
        B, C, gh, gw = d["feat"].shape
        hw = gh * gw
        n = max(min(40, h * w) for h, w in zip(d["ext_h"], d["ext_w"]))
        sel = ops.regions_select("grid", d["keys"].reshape(-1), [hw] * B, d["ext_h"], d["ext_w"], n, 40, 40, hw, grid_w=gw)
        leaf = _leaf(d["feat"].permute(0, 2, 3, 1).contiguous() if channels_last else d["feat"])
        out = ops.regions_gather(leaf.permute(0, 3, 1, 2) if channels_last else leaf, sel)
        out.backward(d["g"][:, :n])
        al = ops.regions_select("grid_all", None, [hw] * B, d["ext_h"], d["ext_w"], hw, hw, hw, hw, grid_w=gw, device=d["feat"].device)
        return [*sel, out.detach(), leaf.grad, al.mask, al.loc, al.mvm]
    return run


case("regions_grid_nchw", ["locov_regions_select", "locov_regions_gather_fwd", "locov_regions_gather_bwd"],
     _regions_grid_inputs(3, 36, 9, 14, 95))(_regions_grid_run(False))
case("regions_grid_channels_last", ["locov_regions_select", "locov_regions_gather_fwd", "locov_regions_gather_bwd"],
     _regions_grid_inputs(3, 36, 9, 14, 96))(_regions_grid_run(True))


def _regions_box_inputs(lengths, C, seed):
    def build():
        g = _g(seed)
        R = sum(lengths)
        return dict(feat=_randn(g, R, C), keys=_rand(g, R).double(), boxes=[_boxes(g, n) for n in lengths], lengths=list(lengths),
                    g=_randn(g, len(lengths), min(lengths), C))
    return build


@case("regions_boxes", ["locov_regions_select", "locov_regions_gather_fwd", "locov_regions_gather_bwd"], _regions_box_inputs([70, 37, 50], 68, 97))
def _(d):
    ops = _ops()
    n = min(d["lengths"])
    sel = ops.regions_select("boxes", d["keys"], d["lengths"], [600, 480, 333], [800, 640, 500], n, n, n, n, boxes=d["boxes"])
    leaf = _leaf(d["feat"])
    out = ops.regions_gather(leaf, sel)
    out.backward(d["g"])
    return [*sel, out.detach(), leaf.grad]


# ------------------------------------------------------------------------------------------------ dataset mapper
def _image_inputs(sizes, seed, hwc):
    def build():
        g = _g(seed)
        return dict(images=[_ints(g, 0, 256, *((h, w, 3) if hwc else (3, h, w)), dtype=torch.uint8) for h, w in sizes], noise=_randn(g, 5000))
    return build


@case("resize_flip_images", ["locov_resize_flip_images"], _image_inputs([(37, 51), (20, 90), (64, 64)], 98, True))
def _(d):
    return _ops().resize_flip_images(d["images"], [(70, 45), (11, 33), (64, 64)], [0, 1, 2])


def _draws(order=(), factors=(1.0, 1.0, 1.0, 0.0), gray=False, sigma=None, erase=()):
    b, c, s, h = factors
    return {"jitter": len(order) > 0, "order": list(order), "brightness": float(b), "contrast": float(c), "saturation": float(s), "hue": float(h),
            "gray": bool(gray), "blur": sigma is not None, "sigma": 0.0 if sigma is None else float(sigma), "erase": list(erase)}


@case("augment_images", ["locov_augment_images"], _image_inputs([(37, 51), (20, 90), (70, 150)], 99, False))
def _(d):
    draws = [_draws((1, 2, 3, 4), (0.6, 1.4, 0.6, -0.1), sigma=1.3, erase=[(3, 5, 10, 12), None, (0, 0, 4, 4)]),
             _draws((4, 3), (1.4, 0.6, 1.4, 0.1), gray=True),
             _draws((), sigma=0.45, erase=[(10, 20, 30, 40)])]
    return _ops().augment_images(d["images"], draws, noise=d["noise"])


def _props_inputs(n_rows, dtype, seed):
    def build():
        g = _g(seed)
        R = sum(n_rows) + 5
        rows = torch.cat([_boxes(g, R, extent=(600.0, 400.0), max_side=150.0), _randn(g, R, 1)], dim=1).to(dtype)
        rows[::11, 2] = rows[::11, 0]                                     # empty boxes
        return dict(rows=rows, n_rows=list(n_rows))
    return build


def _props_run(d):
    ops = _ops()
    n = d["n_rows"]
    starts = [2] + [2 + int(s) for s in np.cumsum(n)[:-1]]
    out = ops.proposal_buffers(sum(n), len(n), d["rows"].device)
    ops.map_proposals(d["rows"], starts, n, [(1.5, 1.25), (0.5, 0.75), (1.0, 1.0)], [1, 0, 2], [(500, 900), (300, 300), (400, 600)], 40, 0.0, out=out)
    return list(out)


case("map_proposals_f32", ["locov_map_proposals"], _props_inputs([65, 0, 130], torch.float32, 100))(_props_run)
case("map_proposals_f64", ["locov_map_proposals"], _props_inputs([65, 0, 130], torch.float64, 101))(_props_run)


# ------------------------------------------------------------------------------------------------ attention
def _mha_inputs(nseq, H, S, d, seed):
    def build():
        g = _g(seed)
        E = H * d
        bias = torch.zeros(nseq, S)
        bias[:, S - 3:] = -10000.0
        return dict(q=_randn(g, nseq * S, E), k=_randn(g, nseq * S, E), v=_randn(g, nseq * S, E), bias=bias,
                    keep=(_rand(g, nseq, H, S, S) > 0.1).to(torch.uint8), g=_randn(g, nseq * S, E), H=H)
    return build


def _mha_run(packed):
    def run(d):
        ops = _ops()
        if packed:
            qkv = _leaf(torch.cat([d["q"], d["k"], d["v"]], dim=1))
            out = ops.mha_packed(qkv, d["bias"], d["H"], keep=d["keep"], p_drop=0.1)
            lse = out.grad_fn.saved_tensors[-1].detach().clone()
            out.backward(d["g"])
            return [out.detach(), lse, qkv.grad]
        q, k, v = _leaf(d["q"]), _leaf(d["k"]), _leaf(d["v"])
        out = ops.mha(q, k, v, d["bias"], d["H"], keep=d["keep"], p_drop=0.1)
        lse = out.grad_fn.saved_tensors[-1].detach().clone()
        out.backward(d["g"])
        return [out.detach(), lse, q.grad, k.grad, v.grad]
    return run


case("mha_3x2x17x32", ["locov_mha_fwd", "locov_mha_bwd"], _mha_inputs(3, 2, 17, 32, 102))(_mha_run(False))
case("mha_2x3x65x96_packed", ["locov_mha_fwd", "locov_mha_bwd"], _mha_inputs(2, 3, 65, 96, 103))(_mha_run(True))


# ------------------------------------------------------------------------------------------------ ROIAlign
def _roi_inputs(N, C, H, W, R, seed, scale=16.0):
    def build():
        g = _g(seed)
        wh = _rand(g, R, 2) * torch.tensor([W * scale, H * scale]) * 0.6 + 4.0
        xy = _rand(g, R, 2) * torch.tensor([W * scale, H * scale]) - 10.0
        idx = _ints(g, 0, N, R, 1).float()
        idx[idx == 1] = 0.0 if N > 2 else 1.0                              # with three images, image 1 has no ROI
        return dict(feat=_randn(g, N, C, H, W), rois=torch.cat([idx, xy, xy + wh], dim=1), g=_randn(g, R, C, 7, 7))
    return build


def _roi_align_run(mode):
    def run(d):
        feat = _leaf(d["feat"])
        out = _ops().roi_align(feat, d["rois"], 7, 1.0 / 16, 2, True, mode=mode)
        out.backward(d["g"])
        return [out.detach(), feat.grad]
    return run


case("roi_align_plan_path", ["locov_roi_align_from_nhwc_fwd_ex", "locov_nchw_to_nhwc", "locov_roi_align_bwd"], _roi_inputs(3, 36, 13, 17, 45, 104),
     history=_roi_inputs(3, 36, 25, 38, 700, 105))(_roi_align_run("fast"))
case("roi_align_exact_nhwc_copy", ["locov_roi_align_from_nhwc_fwd_ex"], _roi_inputs(3, 36, 13, 17, 45, 106))(_roi_align_run("exact"))
case("roi_align_nchw", ["locov_roi_align_fwd", "locov_roi_align_bwd"], _roi_inputs(3, 5, 13, 17, 45, 107))(_roi_align_run("exact"))


@case("roi_align_from_nhwc_legacy_entry", ["locov_roi_align_from_nhwc_fwd"], _roi_inputs(3, 36, 13, 17, 45, 108))
def _(d):
    ops, lib = _ops(), _lib()
    nhwc = ops.nchw_to_nhwc(d["feat"])
    N, H, W, C = nhwc.shape
    R = d["rois"].shape[0]
    out = torch.empty((R, C, 7, 7), dtype=torch.float32, device=nhwc.device)
    _check(lib.locov_roi_align_from_nhwc_fwd(_p(nhwc), N, H, W, C, _p(d["rois"]), R, 7, 7, 1.0 / 16, 2, 1, _p(out), _stream(nhwc)),
           "locov_roi_align_from_nhwc_fwd")
    return [nhwc, out]


@case("roi_align_levels", ["locov_roi_align_levels_fwd", "locov_level_assign"], _roi_inputs(2, 8, 26, 34, 45, 109, scale=8.0))
def _(d):
    ops = _ops()
    lv = ops.level_assign(d["rois"][:, 1:].contiguous() * 4.0, 2, 3)
    feats = [d["feat"], d["feat"][:, :, ::2, ::2].contiguous()]
    return [lv, ops.roi_align_levels(feats, [1.0 / 8, 1.0 / 16], d["rois"], lv, 7, 2, True)]


def _nhwc_run(bin_stride, pos_major, dtype, affine):
    def run(d):
        ops = _ops()
        nhwc = ops.nchw_to_nhwc(d["feat"], dtype)
        C = nhwc.shape[3]
        kw = dict(ch_scale=d["feat"][0, :, 0, 0].abs().contiguous() + 0.5, ch_shift=d["feat"][0, :, 1, 1].contiguous(), relu=True) if affine else {}
        out = ops.roi_align_nhwc(nhwc, d["rois"], 14, 1.0 / 16, 0, True, bin_stride=bin_stride, pos_major=pos_major, **kw)
        o = (14 + bin_stride - 1) // bin_stride
        gr = out.reshape(-1, C).float() * 0.5
        back = ops.roi_align_nhwc_bwd(gr.contiguous(), tuple(nhwc.shape), d["rois"], 14, 1.0 / 16, 0, True, bin_stride=bin_stride,
                                      pos_major=pos_major)
        assert o * o * d["rois"].shape[0] == gr.shape[0]
        return [nhwc, out, back]
    return run


case("roi_align_nhwc_even_bins_pos_major", ["locov_roi_align_nhwc_affine_fwd", "locov_roi_align_nhwc_bwd", "locov_nchw_to_nhwc"],
     _roi_inputs(3, 36, 13, 17, 45, 110))(_nhwc_run(2, True, torch.float32, True))
case("roi_align_nhwc_all_bins_bf16_map", ["locov_roi_align_nhwc_affine_fwd", "locov_nchw_to_nhwc"],
     _roi_inputs(3, 40, 13, 17, 45, 111))(_nhwc_run(1, False, torch.bfloat16, False))


@case("roi_align_nhwc_legacy_entries", ["locov_roi_align_nhwc_fwd", "locov_roi_align_nhwc_ld_fwd"], _roi_inputs(3, 36, 13, 17, 45, 112))
def _(d):
    ops, lib = _ops(), _lib()
    nhwc = ops.nchw_to_nhwc(d["feat"])
    N, H, W, C = nhwc.shape
    R = d["rois"].shape[0]
    a = torch.empty((R, 7, 7, C), dtype=torch.float32, device=nhwc.device)
    _check(lib.locov_roi_align_nhwc_fwd(_p(nhwc), 0, N, H, W, C, _p(d["rois"]), R, 14, 14, 1.0 / 16, 0, 1, 2, 0, _p(a), 0, _stream(nhwc)),
           "locov_roi_align_nhwc_fwd")
    b = torch.empty((49 * R, C), dtype=torch.float32, device=nhwc.device)
    _check(lib.locov_roi_align_nhwc_ld_fwd(_p(nhwc), 0, N, H, W, C, _p(d["rois"]), R, 14, 14, 1.0 / 16, 0, 1, 2, 1, _p(b), C, 0, _stream(nhwc)),
           "locov_roi_align_nhwc_ld_fwd")
    return [a, b]


# ================================================================================================ single-launch ops
def _gemm_inputs(M, N, K, seed):
    def build():
        g = _g(seed)
        return dict(x=_randn(g, M, K), w=_randn(g, N, K, scale=0.1), b=_randn(g, N, scale=0.1), sc=_rand(g, N) + 0.5, res=_randn(g, M, N),
                    mask=_randn(g, M, N))
    return build


# (GEMM tile choices of launch_gemm_nt: N <= 32 the 128 x 32 tile, a plain problem of fewer than 128 tiles of 128 x 128 the 64 x 64
#  tile, otherwise the 128 x 128 tile; the predictor cases above run the 128 x 64 one, N <= 64)
@case("linear_f32_64x64_tile_133x68x36", ["locov_gemm_nt_f32", "locov_gemm_nt_f32_ex"], _gemm_inputs(133, 68, 36, 120),
      tier=launches(c0=0, c2=2))
def _(d):
    ops = _ops()
    wide = torch.cat([d["w"], d["w"]], dim=1)                              # weight rows as a column block of a wider matrix
    return [ops.linear(d["x"], d["w"], d["b"], scale=d["sc"], residual=d["res"], relu=True),
            ops.linear_ex(d["x"], wide[:, :36], d["b"], mask=d["mask"])]


@case("linear_f32_128x128_tile_2053x1028x36", ["locov_gemm_nt_f32"], _gemm_inputs(2053, 1028, 36, 121), tier=launches(c0=1, c2=0))
def _(d):
    return [_ops().linear(d["x"], d["w"], d["b"])]


@case("linear_f32_128x32_tile_k_not_multiple_of_4", ["locov_gemm_nt_f32"], _gemm_inputs(65, 20, 35, 122), tier=launches(c0=0, c2=1))
def _(d):
    return [_ops().linear(d["x"], d["w"], d["b"])]


@case("linear_autograd", ["locov_gemm_nt_f32", "locov_weight_transpose_scale", "locov_gemm_tn_f32"], _gemm_inputs(133, 68, 36, 123))
def _(d):
    leaves = [_leaf(d[k]) for k in ("x", "w", "b")]
    y = _ops().linear_autograd(*leaves)
    y.backward(d["res"])
    return [y.detach()] + [t.grad for t in leaves]


def _split_inputs(M, N, K, seed):
    def build():
        g = _g(seed)
        return dict(x=_randn(g, M, K).relu(), w=_randn(g, N, K, scale=0.05), b=_randn(g, N, scale=1e-2), sc=_rand(g, N) + 0.5,
                    res=_randn(g, M, N, scale=1e-2), mask=_randn(g, M, N))
    return build


@case("linear_split_128", ["locov_gemm_nt_f32_split", "locov_split_f16x2_pack"], _split_inputs(133, 68, 64, 124), env={"LOCOV_SPLIT_BIG": "0"},
      tier=launches(c5=2, c9=0))
def _(d):
    ops = _ops()
    wp = ops.split_pack(d["w"])
    y = ops.linear_split(d["x"], wp, d["b"], scale=d["sc"], residual=d["res"], relu=True)
    return [wp.data, y, ops.linear_split(d["x"], ops.split_pack(d["w"][:64]), relu=True, out_split=True)]


@case("linear_split_256_presplit", ["locov_gemm_nt_f32_split"], _split_inputs(300, 72, 64, 125), env={"LOCOV_SPLIT_BIG": "1"},
      tier=launches(c5=0, c9=1))
def _(d):
    ops = _ops()
    xs = ops.split_pack(d["x"], 16.0).data
    return [xs, ops.linear_split(xs, ops.split_pack(d["w"]), d["b"], relu=True, x_is_split=True)]


@case("linear_split_ex_device_scale", ["locov_gemm_nt_f32_split_ex", "locov_split_scale_from_amax_zeroed"], _split_inputs(133, 68, 64, 126))
def _(d):
    ops = _ops()
    slot = ops.split_scale_from_amax(d["x"])
    amax = torch.zeros(4, dtype=torch.float32, device=d["x"].device)
    y = ops.linear_split_ex(d["x"], ops.split_pack(d["w"]), d["b"], mask=d["mask"], x_scale_dev=slot, amax_out=amax)
    return [slot.clone(), y, amax]


@case("split_scale_from_amax_with_memset", ["locov_split_scale_from_amax"], _split_inputs(133, 68, 64, 127))
def _(d):
    lib = _lib()
    x = d["x"]
    slot = torch.empty(4, dtype=torch.float32, device=x.device)
    _check(lib.locov_split_scale_from_amax(_p(x), x.numel(), 13.0, _p(slot), _stream(x)), "locov_split_scale_from_amax")
    return [slot]


@case("amax_bound", ["locov_amax_bound"], _split_inputs(133, 68, 64, 128))
def _(d):
    return [_ops().amax_bound([d["x"], d["res"]], [0.5, 2.0]).clone()]


def _batched_inputs(B, M, N, K, seed):
    def build():
        g = _g(seed)
        return dict(x=_randn(g, B, M, K), w=_randn(g, B, N, K, scale=0.1))
    return build


@case("gemm_nt_batched", ["locov_gemm_nt_batched_f32", "locov_gemm_nt_batched_f32_split"], _batched_inputs(5, 133, 68, 64, 129))
def _(d):
    ops = _ops()
    return [ops.gemm_nt_batched(d["x"], d["w"]), ops.gemm_nt_batched_split(d["x"], ops.split_pack(d["w"]), x_scale=4.0)]


def _conv_inputs(R, H, W, Cin, N, seed):
    def build():
        g = _g(seed)
        M = R * H * W
        return dict(x=_randn(g, M, Cin), w=_randn(g, N, Cin, 3, 3, scale=0.1), sc=_rand(g, N) + 0.5, sh=_randn(g, N, scale=0.1),
                    res=_randn(g, M, N), mask=_randn(g, M, N), rs=_rand(g, N) + 0.5, H=H, W=W)
    return build


@case("conv3x3_nhwc", ["locov_pack_conv3x3_weight", "locov_conv3x3_nhwc_f32", "locov_conv3x3_nhwc_f32_ex", "locov_im2col3x3_nhwc",
                       "locov_conv3x3_wgrad_unpack", "locov_conv3x3_weight_flip"], _conv_inputs(5, 7, 7, 32, 40, 130))
def _(d):
    ops = _ops()
    wp = ops.pack_conv3x3_weight(d["w"])
    return [wp, ops.conv3x3_nhwc(d["x"], wp, d["H"], d["W"], scale=d["sc"], shift=d["sh"], residual=d["res"], relu=True),
            ops.conv3x3_nhwc(d["x"], wp, d["H"], d["W"], pos_major=True),
            ops.conv3x3_nhwc_ex(d["x"], wp, d["H"], d["W"], mask=d["mask"]), ops.im2col3x3(d["x"], d["H"], d["W"]),
            ops.conv3x3_wgrad_unpack(wp, d["rs"]), ops.conv3x3_weight_flip(d["w"], d["rs"])]


@case("bf16_gemm_conv_sim", ["locov_f32_to_bf16", "locov_gemm_nt_bf16", "locov_conv3x3_nhwc_bf16", "locov_sim_gemm_bf16",
                            "locov_pack_conv3x3_weight"], _conv_inputs(5, 7, 7, 64, 36, 131))
def _(d):
    ops = _ops()
    xb = ops.to_bf16(d["x"])
    wpb = ops.pack_conv3x3_weight(d["w"], torch.bfloat16)
    w2 = ops.to_bf16(d["w"][:, :, 0, 0].contiguous())
    return [xb, wpb, ops.conv3x3_nhwc_bf16(xb, wpb, d["H"], d["W"], scale=d["sc"], shift=d["sh"], relu=True),
            ops.linear_bf16(xb, w2, d["sh"], scale=d["sc"], residual=d["res"], relu=True), ops.sim_gemm_bf16(xb, w2),
            ops.to_bf16(d["x"].reshape(-1)[1:4 * 1000 + 2])]


@case("res5_weight_prep", ["locov_res5_weight_prep"], _conv_inputs(1, 7, 7, 64, 96, 132))
def _(d):
    ops = _ops()
    w3, w1, rs = d["w"], d["w"][:, :, 1, 1].contiguous(), d["rs"]
    jobs = []
    for kind, w in (("plain", w1), ("t", w1), ("col", w3), ("flip9", w3), ("wino", w3), ("uflip", w3)):
        out = torch.empty(ops.prep_shape(kind, w), dtype=torch.float32, device=w.device)
        jobs.append((kind, w, rs if kind != "plain" else None, out, 4096.0))
    ops.res5_weight_prep(jobs)
    return [j[3] for j in jobs]


@case("frozen_bn_fold", ["locov_frozen_bn_fold"], lambda: dict(v=_rand(_g(133), 4, 300) + 0.1))
def _(d):
    v = d["v"]
    return list(_ops().frozen_bn_fold(v[0].contiguous(), v[1].contiguous(), v[2].contiguous(), v[3].contiguous()))


def _rows_inputs(R, C, hw, seed):
    def build():
        g = _g(seed)
        return dict(g=_randn(g, R, C), act=_randn(g, R * hw, C), x4=_randn(g, R, C, 7, 7), x9=_randn(g, R, C, 9, 9), hw=hw)
    return build


@case("res5_backward_elementwise", ["locov_relu_mask", "locov_spatial_mean_bwd", "locov_zero_if_raised", "locov_rows_stride2"],
      _rows_inputs(37, 36, 49, 134))
def _(d):
    ops = _ops()
    dev = d["g"].device
    slot = torch.zeros(4, dtype=torch.float32, device=dev)
    up = ops.spatial_mean_bwd(d["g"], d["act"], d["hw"], amax_out=slot)
    rm = ops.relu_mask(d["act"], up)
    raised, quiet = torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    a, b = up.clone(), rm.clone()
    ops.zero_if_raised([a], raised)
    ops.zero_if_raised([b], quiet)
    m = d["x4"].permute(0, 2, 3, 1).contiguous()                           # [37, 7, 7, 36]
    down = ops.rows_stride2(m, 37, 7, 7, True)
    return [up, slot, rm, a, b, down, ops.rows_stride2(down, 37, 7, 7, False)]


def _mean_tier(n, d):
    """head.hip's rule for [R, C, h, w]: the LDS rows kernel while 256 rows x h w floats fit 64 KB, else the wave kernel"""
    hw4, hw9 = d["x4"].shape[2] * d["x4"].shape[3], d["x9"].shape[2] * d["x9"].shape[3]
    assert 256 * hw4 * 4 <= 64 * 1024 < 256 * hw9 * 4, (hw4, hw9)


@case("spatial_mean_tiers", ["locov_spatial_mean_fwd", "locov_nchw_to_nhwc"], _rows_inputs(37, 36, 49, 135), tier=_mean_tier)
def _(d):
    ops = _ops()
    cl = d["x4"].permute(0, 2, 3, 1).contiguous()
    pm = d["x4"].permute(2, 3, 0, 1).contiguous()
    # 7 x 7 windows: the LDS rows kernel; 9 x 9: the wave kernel; the two channels-last orders
    return [ops.spatial_mean(d["x4"]), ops.spatial_mean(d["x9"]), ops.spatial_mean(cl, 1), ops.spatial_mean(pm, 2), ops.nhwc_to_nchw(cl)]


def _head_inputs(R, C5, D, K1, seed):
    def build():
        g = _g(seed)
        return dict(x=_randn(g, R, C5, 7, 7).relu(), ew=_randn(g, D, C5, scale=0.05), eb=_randn(g, D, scale=0.1), bw=_randn(g, 4, C5, scale=0.05),
                    bb=_randn(g, 4, scale=0.1), bank=_randn(g, K1, D, scale=0.2))
    return build


@case("box_head", ["locov_box_head_fwd"], _head_inputs(133, 68, 40, 21, 136))
def _(d):
    ops = _ops()
    a = ops.box_head(d["x"], d["ew"], d["eb"], d["bw"], d["bb"], d["bank"], norm_mode=ops.NORM_L2)
    b = ops.box_head(d["x"].permute(2, 3, 0, 1).contiguous(), d["ew"], d["eb"], d["bw"], d["bb"], d["bank"], sim_dtype=ops.BF16, channels_last=2)
    return [*a, *b]


def _tok_inputs(R, K1, tmax, seed):
    def build():
        g = _g(seed)
        num = _ints(g, 0, tmax + 1, K1, dtype=torch.int32)
        num[0], num[1] = tmax, 0
        width = num.clamp_min(1)
        off = (torch.cumsum(width, 0) - width).to(torch.int32)
        Ttot = int(width.sum())
        return dict(sim=_randn(g, R, Ttot), off=off, num=num, tmax=tmax, gmin=torch.tensor([-3.0]), gs=_randn(g, R, K1), ga=_randn(g, R, K1, tmax))
    return build


def _tok_run(hardmax):
    def run(d):
        sim = _leaf(d["sim"])
        scores, att = _ops().token_attention_autograd(sim, d["off"], d["num"], d["tmax"], 0.5, d["gmin"], cosine=False, hardmax=hardmax)
        torch.autograd.backward([scores, att], [d["gs"], d["ga"]])
        return [scores.detach(), att.detach(), sim.grad]
    return run


case("token_attention_softmax", ["locov_token_attention_fwd", "locov_token_attention_bwd"], _tok_inputs(133, 21, 5, 137))(_tok_run(False))
case("token_attention_hardmax", ["locov_token_attention_fwd", "locov_token_attention_bwd"], _tok_inputs(133, 21, 5, 138))(_tok_run(True))


@case("rownorm", ["locov_rownorm_fwd", "locov_rownorm_bwd"], lambda: dict(x=_randn(_g(139), 133, 70), g=_randn(_g(140), 133, 70)))
def _(d):
    ops = _ops()
    out = []
    for mode in (ops.NORM_L2, ops.NORM_STANDARDIZE):
        x = _leaf(d["x"])
        y = ops.rownorm_autograd(x, mode)
        y.backward(d["g"])
        out += [y.detach(), x.grad]
    return out


# ------------------------------------------------------------------------------------------------ grounding
def _ground_inputs(B, T, NR, seed):
    def build():
        g = _g(seed)
        cm = (torch.arange(T)[None, :] < _ints(g, 1, T + 1, B)[:, None]).float()
        rm = (torch.arange(NR)[None, :] < _ints(g, 1, NR + 1, B)[:, None]).float()
        rm[0] = 1.0
        return dict(S=_randn(g, B * T, B * NR), cm=cm, rm=rm, g0=_randn(g, B, B), g1=_randn(g, B, B),
                    neg=_ints(g, 0, max(B - 1, 1), 2, 2, B), trans=_randn(g, B, B))
    return build


def _costs_run(alignment, words=True, regions=True):
    def run(d):
        S = _leaf(d["S"])
        c0, c1 = _ops().grounding_costs(S, d["cm"], d["rm"], 0.1, alignment, words=words, regions=regions)
        torch.autograd.backward([c for c in (c0, c1) if c is not None], [g for g, c in ((d["g0"], c0), (d["g1"], c1)) if c is not None])
        return [c0.detach() if c0 is not None else None, c1.detach() if c1 is not None else None, S.grad]
    return run


def _ground_tier(above):
    """grounding.hip's LDS request (T * NR + 3 T + 8) floats against the 64 KB a kernel gets without the raised limit"""
    def check(n, d):
        T, NR = d["cm"].shape[1], d["rm"].shape[1]
        assert ((T * NR + 3 * T + 8) * 4 > 64 * 1024) == above, (T, NR)
    return check


# (3, 11, 70): the similarity tile fits 64 KB of LDS; (2, 70, 250): it takes the larger dynamic allocation
case("grounding_costs_softmax_3x11x70", ["locov_grounding_align_fwd", "locov_grounding_align_bwd"], _ground_inputs(3, 11, 70, 141),
     tier=_ground_tier(False))(_costs_run("softmax"))
case("grounding_costs_hardmax_2x70x250", ["locov_grounding_align_fwd", "locov_grounding_align_bwd"], _ground_inputs(2, 70, 250, 142),
     tier=_ground_tier(True))(_costs_run("hardmax"))
case("grounding_costs_words_only", ["locov_grounding_align_fwd", "locov_grounding_align_bwd"],
     _ground_inputs(3, 11, 70, 143))(_costs_run("softmax", regions=False))


@case("grounding_legacy_entries", ["locov_grounding_fwd", "locov_grounding_bwd"], _ground_inputs(3, 11, 70, 144))
def _(d):
    lib = _lib()
    S, B, T, NR = d["S"], 3, 11, 70
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=S.device)
    c0, c1, dS = new(B, B), new(B, B), new(*S.shape)
    _check(lib.locov_grounding_fwd(_p(S), B, T, NR, _p(d["cm"]), _p(d["rm"]), 0.1, _p(c0), _p(c1), _stream(S)), "locov_grounding_fwd")
    _check(lib.locov_grounding_bwd(_p(S), B, T, NR, _p(d["cm"]), _p(d["rm"]), 0.1, _p(d["g0"]), _p(d["g1"]), _p(dS), _stream(S)),
           "locov_grounding_bwd")
    return [c0, c1, dS]


def _tail_run(kind, one_sided=False):
    def run(d):
        ops = _ops()
        c0, c1 = _leaf(d["g0"]), (None if one_sided else _leaf(d["g1"]))
        if kind == "ce":
            vals, pw0, pw1 = ops.grounding_ce(c0, c1, d["cm"], d["rm"]), None, None
        elif kind == "ce_dist":
            vals, pw0, pw1 = ops.grounding_ce_dist(c0, c1, d["cm"], d["rm"])
        else:
            vals, pw0, pw1 = ops.grounding_triplet(c0, c1, d["cm"], d["rm"], kind, 0.2, neg_idx=d["neg"] if kind == "given" else None,
                                                   with_dist=True)
        loss = vals[0] + 2.0 * vals[1] + (0 if one_sided else 3.0 * vals[4] + 4.0 * vals[5])
        for pw in (pw0, pw1):
            if pw is not None:
                loss = loss + (pw * d["trans"]).sum()
        loss.backward()
        return [torch.stack([v.detach() for v in vals]), pw0.detach() if pw0 is not None else None, pw1.detach() if pw1 is not None else None,
                c0.grad, c1.grad if c1 is not None else None]
    return run


_TAIL = _ground_inputs(5, 6, 9, 145)
case("grounding_ce", ["locov_grounding_ce_fwd", "locov_grounding_ce_bwd"], _TAIL)(_tail_run("ce"))
case("grounding_ce_one_sided", ["locov_grounding_ce_fwd", "locov_grounding_ce_bwd"], _TAIL)(_tail_run("ce", one_sided=True))
case("grounding_ce_dist", ["locov_grounding_ce_dist_fwd", "locov_grounding_ce_dist_bwd"], _TAIL)(_tail_run("ce_dist"))
case("grounding_triplet_hardest", ["locov_grounding_triplet_fwd", "locov_grounding_triplet_bwd"], _TAIL)(_tail_run("hardest"))
case("grounding_triplet_given_one_sided", ["locov_grounding_triplet_fwd", "locov_grounding_triplet_bwd"], _TAIL)(_tail_run("given", one_sided=True))


def _distill_run(kind):
    def run(d):
        t, a, b = _leaf(d["trans"]), _leaf(d["g0"]), _leaf(d["g1"])
        loss = _ops().distill_loss(kind, t, a, b, 2.0, loss_weight=0.5)
        loss.backward()
        return [loss.detach(), t.grad, a.grad, b.grad]
    return run


for _kind in ("kd", "js", "mse"):
    case(f"distill_loss_{_kind}", ["locov_distill_loss_fwd", "locov_distill_loss_bwd"], _TAIL)(_distill_run(_kind))


# ------------------------------------------------------------------------------------------------ box losses
def _boxloss_inputs(R, K, seed, cs):
    def build():
        g = _g(seed)
        props = _boxes(g, R)
        gt = props + _randn(g, R, 4, scale=5.0)
        gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 2.0)
        return dict(pred=_randn(g, R, 4 * K if cs else 4, scale=0.3), props=props, gt=gt, cls=_ints(g, 0, K + 1, R), K=K)
    return build


def _boxloss_run(kind):
    def run(d):
        ops = _ops()
        pred = _leaf(d["pred"])
        if kind == "smooth_l1":
            loss = ops.box_reg_loss(pred, d["props"], d["gt"], d["cls"], d["K"], W10, 0.5)
        else:
            loss = ops.box_iou_loss(pred, d["props"], d["gt"], d["cls"], d["K"], W10, CLAMP, kind)
        loss.backward()
        return [loss.detach(), pred.grad]
    return run


case("box_reg_loss_agnostic", ["locov_box_reg_loss"], _boxloss_inputs(333, 7, 146, False))(_boxloss_run("smooth_l1"))
case("box_reg_loss_class_specific", ["locov_box_reg_loss"], _boxloss_inputs(333, 7, 147, True))(_boxloss_run("smooth_l1"))
for _kind in ("giou", "diou", "ciou"):
    case(f"box_iou_loss_{_kind}", ["locov_box_iou_loss"], _boxloss_inputs(333, 7, 148, _kind == "diou"))(_boxloss_run(_kind))


# ------------------------------------------------------------------------------------------------ the two ends of the detector call
@case("preprocess_images", ["locov_preprocess_images"], _image_inputs([(37, 51), (20, 90), (64, 64)], 149, False))
def _(d):
    ops = _ops()
    u8, _ = ops.preprocess_images(d["images"], [103.53, 116.28, 123.675], [57.375, 57.12, 58.395], size_divisibility=32)
    f32, _ = ops.preprocess_images([t.float() for t in d["images"]], [103.53, 116.28, 123.675], [1.0, 1.0, 1.0], pad_value=-1.0)
    return [u8, f32]


@case("detector_rescale", ["locov_detector_rescale"], lambda: dict(boxes=_boxes(_g(150), 200, extent=(700.0, 500.0))))
def _(d):
    out, src, counts = _ops().detector_rescale(d["boxes"], [70, 0, 130], [(600, 800)] * 3, [(300, 400), (480, 640), (100, 90)])
    return [out, src, _i32(counts, out.device)]
