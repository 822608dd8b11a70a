"""Tensor-level wrappers over the C ABI (include/locov_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every function below checks
its arguments, allocates the outputs and enqueues the hand-written gfx950 kernels on
torch's current stream.  Nothing in this module computes with torch ops, and there is no
CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
import itertools
import math
import threading
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import BF16, F32, NORM_L2, NORM_NONE, NORM_STANDARDIZE, LocovError, check

__all__ = [
    "level_assign", "roi_align", "roi_align_levels", "nchw_to_nhwc", "roi_align_nhwc", "spatial_mean",
    "linear", "rownorm", "to_bf16", "sim_gemm_bf16", "box_head", "NORM_NONE", "NORM_L2",
    "NORM_STANDARDIZE", "F32", "BF16",
]


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise LocovError(f"{name} is on {t.device}: the LSM ROI-head kernels only run on a ROCm GPU "
                         "(there is no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    """2-D fp32 device matrix whose rows may be a column block of a wider matrix (stride(1) == 1, any
    16-byte-aligned row stride); anything else is made contiguous."""
    if (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] > 0
            and t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0):
        return t
    return _dev(t, name)


def _out(out: Optional[torch.Tensor], shape, ref: torch.Tensor, name: str) -> torch.Tensor:
    """The result tensor of an op: a fresh one, or the caller's `out` (a contiguous fp32 device tensor of that shape -- e.g. a
    row slice of a larger matrix: the training step keeps the rows of both Res5 calls in ONE matrix per activation)."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=ref.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != ref.device or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous fp32 {tuple(shape)} tensor on {ref.device}")
    return out


def _stream(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _images(images: Sequence[torch.Tensor], axis: int, dtype=torch.uint8) -> Tuple[List[torch.Tensor], int]:
    """A data-side op's device images, contiguous, and their channel count: -1 unless all are rank 3, one size on `axis`, on one device."""
    ims = [_dev(t, f"images[{i}]", dtype=dtype) for i, t in enumerate(images)]
    C = int(ims[0].shape[axis]) if ims[0].dim() == 3 else -1
    return ims, -1 if any(t.dim() != 3 or t.shape[axis] != C or t.device != ims[0].device for t in ims) else C


def _ptrs(tensors: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _ints(values: Sequence[int]):
    return (ctypes.c_int * len(values))(*values)


def _out_images(out: Sequence[torch.Tensor], shapes, device, what: str, apart_from=()) -> List[torch.Tensor]:
    """A data-side op's `out` as a list: a contiguous uint8 tensor per shape on `device`, none the one at its place in `apart_from`."""
    outs = list(out)
    if len(outs) != len(shapes) or any(o.dtype != torch.uint8 or tuple(o.shape) != tuple(s) or o.device != device or not o.is_contiguous()
                                       for o, s in zip(outs, shapes)) or any(o.data_ptr() == t.data_ptr() for o, t in zip(outs, apart_from)):
        raise ValueError(what)
    return outs


def _dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {dt}")


# --------------------------------------------------------------------------------------
def level_assign(boxes: torch.Tensor, min_level: int, max_level: int, canonical_box_size: int = 224,
                 canonical_level: int = 4) -> torch.Tensor:
    """boxes [R,4] XYXY fp32 -> int64 [R] level index in [0, max_level-min_level]."""
    boxes = _dev(boxes, "boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError(f"boxes must be [R,4], got {tuple(boxes.shape)}")
    out = torch.empty((boxes.shape[0],), dtype=torch.int64, device=boxes.device)
    with torch.cuda.device(boxes.device):
        check(_lib.load().locov_level_assign(_ptr(boxes), boxes.shape[0], int(min_level), int(max_level),
                                             int(canonical_box_size), int(canonical_level), _ptr(out),
                                             _stream(boxes)), "locov_level_assign")
    return out


class _ROIAlignFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, rois, ph, pw, scale, sampling_ratio, aligned, mode=0):
        N, C, H, W = feat.shape
        R = rois.shape[0]
        out = torch.empty((R, C, ph, pw), dtype=torch.float32, device=feat.device)
        with torch.cuda.device(feat.device):
            if C % 4 == 0 and R > 0 and ph * pw <= 2048:
                # fast path (same bits): gather from a channels-last copy, transpose in LDS
                nhwc = torch.empty((N, H, W, C), dtype=torch.float32, device=feat.device)
                check(_lib.load().locov_nchw_to_nhwc(_ptr(feat), N, C, H, W, _ptr(nhwc), F32, _stream(feat)),
                      "locov_nchw_to_nhwc")
                lib = _lib.load()
                ws = _workspace("roi_plan", feat, int(lib.locov_roi_align_plan_bytes(R))) if mode else None
                check(lib.locov_roi_align_from_nhwc_fwd_ex(_ptr(nhwc), N, H, W, C, _ptr(rois), R, ph, pw, float(scale),
                                                           int(sampling_ratio), int(aligned), int(mode), _ptr(ws),
                                                           ws.numel() if ws is not None else 0, _ptr(out), _stream(feat)),
                      "locov_roi_align_from_nhwc_fwd_ex")
            else:
                check(_lib.load().locov_roi_align_fwd(_ptr(feat), N, C, H, W, _ptr(rois), R, ph, pw, float(scale),
                                                      int(sampling_ratio), int(aligned), _ptr(out), _stream(feat)),
                      "locov_roi_align_fwd")
        ctx.save_for_backward(rois)
        ctx.args = (N, C, H, W, ph, pw, scale, sampling_ratio, aligned)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (rois,) = ctx.saved_tensors
        N, C, H, W, ph, pw, scale, sampling_ratio, aligned = ctx.args
        grad_out = _dev(grad_out, "grad_out")
        gf = torch.zeros((N, C, H, W), dtype=torch.float32, device=grad_out.device)
        with torch.cuda.device(gf.device):
            check(_lib.load().locov_roi_align_bwd(_ptr(grad_out), N, C, H, W, _ptr(rois), rois.shape[0], ph, pw,
                                                  float(scale), int(sampling_ratio), int(aligned), _ptr(gf),
                                                  _stream(gf)), "locov_roi_align_bwd")
        return gf, None, None, None, None, None, None, None


ROIALIGN_MODES = {"exact": 0, "fast": 1}


def roi_align(feat: torch.Tensor, rois: torch.Tensor, output_size, spatial_scale: float,
              sampling_ratio: int = 0, aligned: bool = True, mode: str = "exact") -> torch.Tensor:
    """feat [N,C,H,W] fp32, rois [R,5] (batch_idx,x0,y0,x1,y1) -> [R,C,ph,pw] (differentiable in feat).
    mode "exact": torchvision's per-sample order, bit-identical to the CPU oracle; "fast": within 1e-5 of it -- separable
    per-pixel weights and the proposal's pixel window staged in LDS (include/locov_hip.h, LOCOV_ROIALIGN_FAST)."""
    feat = _dev(feat, "feat")
    rois = _dev(rois, "rois")
    if feat.dim() != 4:
        raise ValueError(f"feat must be [N,C,H,W], got {tuple(feat.shape)}")
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise ValueError(f"rois must be [R,5], got {tuple(rois.shape)}")
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    return _ROIAlignFn.apply(feat, rois, int(ph), int(pw), float(spatial_scale), int(sampling_ratio), bool(aligned),
                             ROIALIGN_MODES[mode])


def roi_align_levels(feats: Sequence[torch.Tensor], scales: Sequence[float], rois: torch.Tensor,
                     levels: Optional[torch.Tensor], output_size: int, sampling_ratio: int = 0,
                     aligned: bool = True) -> torch.Tensor:
    """Multi-level pooler in one launch: ROI r reads feats[levels[r]]."""
    L = len(feats)
    if not (1 <= L <= _lib.MAX_LEVELS) or len(scales) != L:
        raise ValueError("need 1..8 feature levels with one scale each")
    feats = [_dev(f, f"feats[{i}]") for i, f in enumerate(feats)]
    rois = _dev(rois, "rois")
    N, C = feats[0].shape[:2]
    for f in feats:
        if f.shape[0] != N or f.shape[1] != C:
            raise ValueError("all levels must share N and C")
    if L > 1:
        levels = _dev(levels, "levels", torch.int64)
        if levels.shape[0] != rois.shape[0]:
            raise ValueError("levels must have one entry per ROI")
    R = rois.shape[0]
    out = torch.empty((R, C, output_size, output_size), dtype=torch.float32, device=rois.device)
    fp = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    hh = (ctypes.c_int * L)(*[f.shape[2] for f in feats])
    ww = (ctypes.c_int * L)(*[f.shape[3] for f in feats])
    sc = (ctypes.c_float * L)(*[float(s) for s in scales])
    with torch.cuda.device(rois.device):
        check(_lib.load().locov_roi_align_levels_fwd(fp, hh, ww, sc, L, N, C, _ptr(rois),
                                                     _ptr(levels if L > 1 else None), R, output_size, output_size,
                                                     int(sampling_ratio), int(aligned), _ptr(out), _stream(rois)),
              "locov_roi_align_levels_fwd")
    return out


def nchw_to_nhwc(feat: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    feat = _dev(feat, "feat")
    N, C, H, W = feat.shape
    out = torch.empty((N, H, W, C), dtype=dtype, device=feat.device)
    with torch.cuda.device(feat.device):
        check(_lib.load().locov_nchw_to_nhwc(_ptr(feat), N, C, H, W, _ptr(out), _dtype_code(dtype), _stream(feat)),
              "locov_nchw_to_nhwc")
    return out


def roi_align_nhwc(feat: torch.Tensor, rois: torch.Tensor, output_size: int, spatial_scale: float,
                   sampling_ratio: int = 0, aligned: bool = True, bin_stride: int = 1,
                   out_dtype: torch.dtype = torch.float32, pos_major: bool = False,
                   out: Optional[torch.Tensor] = None, ch_scale: Optional[torch.Tensor] = None,
                   ch_shift: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """feat [N,H,W,C] (fp32|bf16) -> [R, o, o, C] with o = ceil(P/bin_stride), or, with pos_major,
    [o, o, R, C] (position-major pixel rows, the fast layout of the Res5 GEMMs).
    feat may be a channel slice of a wider channels-last map (pixel stride > C).
    out: optional destination given as the pixel-row matrix [o*o*R, C]; its rows may be a column block
    of a wider matrix (row stride >= C).
    ch_scale / ch_shift [C], relu: per-channel affine + ReLU applied to the pooled values."""
    if not isinstance(feat, torch.Tensor) or feat.dim() != 4:
        raise ValueError("roi_align_nhwc: feat must be [N,H,W,C]")
    N, H, W, C = feat.shape
    fld = C
    if (feat.is_cuda and feat.stride(3) == 1 and feat.stride(2) > C and feat.stride(2) % 4 == 0
            and feat.stride(1) == W * feat.stride(2) and feat.stride(0) == H * W * feat.stride(2)
            and feat.data_ptr() % 16 == 0):
        fld = feat.stride(2)                       # channel slice of a wider map: no copy
    else:
        feat = _dev(feat, "feat", None)
    rois = _dev(rois, "rois")
    ch_scale = _dev(ch_scale, "ch_scale") if ch_scale is not None else None
    ch_shift = _dev(ch_shift, "ch_shift") if ch_shift is not None else None
    R = rois.shape[0]
    o = (output_size + bin_stride - 1) // bin_stride
    ld = C
    if out is None:
        out = torch.empty((o, o, R, C) if pos_major else (R, o, o, C), dtype=out_dtype, device=feat.device)
    else:
        if (out.dim() != 2 or tuple(out.shape) != (o * o * R, C) or out.dtype != out_dtype or not out.is_cuda
                or (R and (out.stride(1) != 1 or out.stride(0) < C or out.stride(0) % 4 or out.data_ptr() % 16))):
            raise ValueError("roi_align_nhwc: out must be a [o*o*R, C] device matrix with unit column stride")
        ld = out.stride(0) if R else C
    with torch.cuda.device(feat.device):
        check(_lib.load().locov_roi_align_nhwc_affine_fwd(_ptr(feat), _dtype_code(feat.dtype), N, H, W, C, fld, _ptr(rois), R,
                                                          output_size, output_size, float(spatial_scale),
                                                          int(sampling_ratio), int(aligned), int(bin_stride),
                                                          int(pos_major), _ptr(ch_scale), _ptr(ch_shift), int(relu),
                                                          _ptr(out), ld, _dtype_code(out_dtype), _stream(feat)),
              "locov_roi_align_nhwc_affine_fwd")
    return out


def _layout_dims(x: torch.Tensor, channels_last) -> Tuple[int, int, int, int]:
    """(R, C, HW, layout code) of a region-feature tensor: False/0 = [R,C,h,w]; True/1 = [R,h,w,C];
    2 = position-major [h,w,R,C]."""
    code = int(channels_last)
    if x.dim() == 2:
        return x.shape[0], x.shape[1], 1, 0
    if code == 2:
        R, C = x.shape[-2], x.shape[-1]
        return R, C, (x.numel() // (R * C) if R else 1), 2
    R = x.shape[0]
    C = x.shape[-1] if code == 1 else x.shape[1]
    return R, C, (x[0].numel() // C if R else 1), code


def spatial_mean(x: torch.Tensor, channels_last=False) -> torch.Tensor:
    """[R,C,h,w] (channels_last=1: [R,h,w,C]; =2: position-major [h,w,R,C]) -> [R,C]."""
    x = _dev(x, "x")
    if x.dim() == 2:
        return x
    R, C, hw, code = _layout_dims(x, channels_last)
    out = torch.empty((R, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_spatial_mean_fwd(_ptr(x), R, C, max(hw, 1), code, _ptr(out), _stream(x)),
              "locov_spatial_mean_fwd")
    return out


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
           scale: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = epi(x . weight^T): fp32 on the f32 MFMA pipe.  x [M,K] (rows may be strided), weight [N,K]."""
    x = _rows(x, "x")
    weight = _dev(weight, "weight")
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} weight {tuple(weight.shape)}")
    if K % 4 != 0:
        # the kernel stages 16-byte chunks: zero-pad the contraction dim (rows stay 16-byte aligned)
        pad = 4 - K % 4
        x = torch.nn.functional.pad(x, (0, pad)).contiguous()
        weight = torch.nn.functional.pad(weight, (0, pad))
        K += pad
    bias = _dev(bias, "bias") if bias is not None else None
    scale = _dev(scale, "scale") if scale is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    if residual is not None and tuple(residual.shape) != (M, N):
        raise ValueError("residual must be [M,N]")
    y = _out(out, (M, N), x, "linear")
    with torch.cuda.device(x.device):
        check(_lib.load().locov_gemm_nt_f32(_ptr(x), x.stride(0) if M else K, _ptr(weight), _ptr(scale), _ptr(bias), _ptr(residual),
                                            _ptr(y), N, M, N, K, _lib.EPI_RELU if relu else 0, _stream(x)),
              "locov_gemm_nt_f32")
    return y


def conv3x3_nhwc(x: torch.Tensor, w_packed: torch.Tensor, H: int, W: int, *, scale=None, shift=None,
                 residual=None, relu: bool = False, pos_major: bool = False) -> torch.Tensor:
    """3x3 / pad 1 / stride 1 convolution over R independent HxW channels-last tiles.
    x [R*H*W, Cin], w_packed [N, 9*Cin] (pack_conv3x3_weight) -> [R*H*W, N].
    Rows are ROI-major (r*H*W + pos) or, with pos_major, position-major (pos*R + r)."""
    x = _dev(x, "x")
    w_packed = _dev(w_packed, "w_packed")
    M, Cin = x.shape
    N = w_packed.shape[0]
    if w_packed.shape[1] != 9 * Cin or M % (H * W) != 0:
        raise ValueError("conv3x3_nhwc: inconsistent shapes")
    scale = _dev(scale, "scale") if scale is not None else None
    shift = _dev(shift, "shift") if shift is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_conv3x3_nhwc_f32(_ptr(x), M // (H * W), H, W, Cin, int(pos_major), _ptr(w_packed), _ptr(scale),
                                                 _ptr(shift), _ptr(residual), _ptr(y), N,
                                                 _lib.EPI_RELU if relu else 0, _stream(x)), "locov_conv3x3_nhwc_f32")
    return y


def pack_conv3x3_weight(w: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[N,Cin,3,3] -> [N, 9*Cin] with k = (ky*3+kx)*Cin + c."""
    w = _dev(w, "w")
    N, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3):
        raise ValueError("pack_conv3x3_weight expects [N,Cin,3,3]")
    out = torch.empty((N, 9 * Cin), dtype=dtype, device=w.device)
    with torch.cuda.device(w.device):
        check(_lib.load().locov_pack_conv3x3_weight(_ptr(w), N, Cin, _ptr(out), _dtype_code(dtype), _stream(w)),
              "locov_pack_conv3x3_weight")
    return out


_WINO_WS = {}      # (device, stream) -> cached transform-domain workspace (grows to the largest request);
                   # per stream, because calls enqueued on different streams may run concurrently


def winograd_pack_weight(w: torch.Tensor) -> torch.Tensor:
    """[N,Cin,3,3] -> U [121, N, Cin]: the filter in the F(4,3)|F(3,3) minimal-filtering domain."""
    w = _dev(w, "w")
    N, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3):
        raise ValueError("winograd_pack_weight expects [N,Cin,3,3]")
    out = torch.empty((121, N, Cin), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        check(_lib.load().locov_winograd_pack_weight(_ptr(w), N, Cin, _ptr(out), _stream(w)), "locov_winograd_pack_weight")
    return out


def winograd_conv3x3(x: torch.Tensor, U, *, scale=None, shift=None, relu: bool = False,
                     out: Optional[torch.Tensor] = None, v_scale: float = 0.25, roi_major: bool = False,
                     in_roi_major: bool = False, out_split_scale: Optional[float] = None,
                     range_check_scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 / pad 1 / stride 1 convolution of 7x7 position-major tiles in the Winograd domain.
    x [49*R, Cin] (row = pos*R + r), U [121, N, Cin] (winograd_pack_weight) -> [49*R, N].
    out: optional [49*R, N] destination whose rows may be a column block of a wider matrix.
    U may be a SplitWeight (split_pack(winograd_pack_weight(w))): the 121 transform-domain GEMMs then run with
    split operands on the f16 matrix pipe, the transformed input scaled by v_scale (the input transform amplifies
    non-negative data by up to 64x, any data by up to 100x: 0.25 keeps |x| < 4094 in fp16's range, as for the 1x1s).
    roi_major: write the output rows ROI-major (row = r*49 + pos), the order linear_split_segmean reads;
    in_roi_major: x is given in that order.
    out_split_scale (split U only): write the output in the split layout of split_pack scaled by that power of two -- the
    pre-split A operand (`x_is_split`) of the split GEMM that consumes it, which then stages it by LDS DMA with no conversion.
    The returned tensor is float32-TYPED storage of that layout (same shape and size), not fp32 values.
    range_check_scale (split U, fp32 output): raise the range guard here when |range_check_scale * y| >= 65504 -- the check the
    split GEMM reading y at that operand scale would make, one launch earlier.
    workspace: a caller-owned uint8 device buffer of at least winograd_workspace_bytes(R, Cin, N) bytes instead of the cached one; with
    a split U it starts with the transformed input [121, R, Cin] in the split layout x v_scale, which winograd_wgrad(v_split=...)
    takes as it is (a training step keeps one per bottleneck)."""
    x = _dev(x, "x")
    split = U if isinstance(U, SplitWeight) else None
    U = _dev(split.data if split is not None else U, "U")
    M, Cin = x.shape
    if U.dim() != 3 or U.shape[0] != 121 or U.shape[2] != Cin or M % 49 != 0:
        raise ValueError("winograd_conv3x3: inconsistent shapes")
    N, R = U.shape[1], M // 49
    scale = _dev(scale, "scale") if scale is not None else None
    shift = _dev(shift, "shift") if shift is not None else None
    if out is None:
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    else:
        y = out
        if (y.dim() != 2 or tuple(y.shape) != (M, N) or y.dtype != torch.float32 or not y.is_cuda
                or (M and (y.stride(1) != 1 or y.stride(0) < N or y.stride(0) % 2 or y.data_ptr() % 16))):
            raise ValueError("winograd_conv3x3: out must be a [49*R, N] fp32 device matrix with unit column stride")
    ldy = y.stride(0) if M else N
    lib = _lib.load()
    need = int(lib.locov_winograd_workspace_bytes(R, Cin, N))
    if workspace is not None:
        ws = workspace
        if not (ws.is_cuda and ws.device == x.device and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= need
                and ws.data_ptr() % 16 == 0):
            raise ValueError(f"winograd_conv3x3: workspace must be a contiguous uint8 device buffer of >= {need} bytes")
    else:
        key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
        ws = _WINO_WS.get(key)
        if ws is None or ws.numel() < need:
            ws = None
            _WINO_WS.pop(key, None)
            ws = _WINO_WS[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    wflags = ((_lib.EPI_RELU if relu else 0) | (_lib.WINO_OUT_ROI_MAJOR if roi_major else 0)
              | (_lib.WINO_IN_ROI_MAJOR if in_roi_major else 0))
    with torch.cuda.device(x.device):
        if split is not None:
            if out_split_scale is not None and (N % 32 or ldy != N):
                raise ValueError("winograd_conv3x3: a split-layout output needs N % 32 == 0 and a dense destination")
            check(lib.locov_winograd_conv3x3_f32_split_ex(_ptr(x), R, Cin, _ptr(U), split.scale, float(v_scale), 0, _ptr(scale),
                                                          _ptr(shift), None, _ptr(y), ldy, N, wflags,
                                                          float(out_split_scale or (-range_check_scale if range_check_scale else 0.0)),
                                                          _ptr(ws), ws.numel(),
                                                          _ptr(_overflow_word(x)), None, _stream(x)),
                  "locov_winograd_conv3x3_f32_split_ex")
        else:
            if out_split_scale is not None:
                raise ValueError("winograd_conv3x3: out_split_scale needs a split U")
            check(lib.locov_winograd_conv3x3_f32(_ptr(x), R, Cin, _ptr(U), _ptr(scale), _ptr(shift), _ptr(y), ldy, N,
                                                 wflags, _ptr(ws), ws.numel(), _stream(x)),
                  "locov_winograd_conv3x3_f32")
    return y


def winograd_workspace_bytes(R: int, Cin: int, N: int) -> int:
    """Bytes of the workspace winograd_conv3x3 needs for R tiles (locov_winograd_workspace_bytes)."""
    return int(_lib.load().locov_winograd_workspace_bytes(int(R), int(Cin), int(N)))


def conv1x1_winograd_conv3x3(x: torch.Tensor, w1: SplitWeight, b1: Optional[torch.Tensor], U: SplitWeight, *,
                             scale1: Optional[torch.Tensor] = None, scale2: Optional[torch.Tensor] = None,
                             shift2: Optional[torch.Tensor] = None, relu: bool = True, x_scale: float = 16.0, v_scale: float = 0.25,
                             roi_major: bool = True, out_split_scale: Optional[float] = None) -> torch.Tensor:
    """A bottleneck's conv1 (1x1 + FrozenBN + ReLU) and conv2 (3x3 + FrozenBN + ReLU?) in one call, split arithmetic:
        winograd_conv3x3(linear_split(x, w1, b1, scale=scale1, relu=True, x_is_split=True), U, in_roi_major=True, ...)
    and the same bits.  x [49*R, K]: the block input in the split layout (x x_scale), ROI-major rows.  Where the launch fills the
    chip with 256x256 tiles the pixel tensor between the two convolutions is never written: conv1's epilogue applies the Winograd
    input transform (gemm_split_big.hip, MODE_WINO)."""
    x = _rows(x, "x")
    w1d, Ud = _dev(w1.data, "w1"), _dev(U.data, "U")
    M, K = x.shape
    C = w1d.shape[0]
    if w1d.shape[1] != K or K % 32 or M % 49 or Ud.dim() != 3 or Ud.shape[0] != 121 or Ud.shape[2] != C or C % 32:
        raise ValueError(f"conv1x1_winograd_conv3x3: x {tuple(x.shape)} w1 {tuple(w1d.shape)} U {tuple(Ud.shape)}")
    N, R = Ud.shape[1], M // 49
    if N % 4 or (out_split_scale is not None and N % 32):
        raise ValueError("conv1x1_winograd_conv3x3: N % 4 == 0 (N % 32 == 0 for a split-layout output)")
    b1 = _dev(b1, "b1") if b1 is not None else None
    scale1 = _dev(scale1, "scale1") if scale1 is not None else None
    scale2 = _dev(scale2, "scale2") if scale2 is not None else None
    shift2 = _dev(shift2, "shift2") if shift2 is not None else None
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    need = int(lib.locov_conv1x1_winograd_workspace_bytes_for(R, K, C, N, x.stride(0) if M else K))     # no pixel scratch for the fused form
    key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
    ws = _WINO_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = None
        _WINO_WS.pop(key, None)
        ws = _WINO_WS[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    wflags = (_lib.EPI_RELU if relu else 0) | (_lib.WINO_OUT_ROI_MAJOR if roi_major else 0) | _lib.WINO_IN_ROI_MAJOR
    with torch.cuda.device(x.device):
        check(lib.locov_conv1x1_winograd_conv3x3_f32_split(_ptr(x), x.stride(0) if M else K, K, float(x_scale), _ptr(w1d), w1.scale,
                                                           _ptr(scale1), _ptr(b1), R, C, _ptr(Ud), U.scale, float(v_scale),
                                                           _ptr(scale2), _ptr(shift2), _ptr(y), N, N, wflags,
                                                           float(out_split_scale or 0.0), _ptr(ws), ws.numel(),
                                                           _ptr(_overflow_word(x)), _stream(x)),
              "locov_conv1x1_winograd_conv3x3_f32_split")
    return y


def roi_align_winograd_conv3x3(feat: torch.Tensor, rois: torch.Tensor, output_size: int, spatial_scale: float, sampling_ratio: int,
                               aligned: bool, U: SplitWeight, *, ch_scale: Optional[torch.Tensor] = None,
                               ch_shift: Optional[torch.Tensor] = None, scale2: Optional[torch.Tensor] = None,
                               shift2: Optional[torch.Tensor] = None, relu: bool = True, v_scale: float = 0.25,
                               roi_major: bool = True, out_split_scale: Optional[float] = None) -> torch.Tensor:
    """Block 0's pooler + FrozenBN + ReLU + conv2 in one call, split arithmetic:
        winograd_conv3x3(roi_align_nhwc(feat, rois, 14, ..., bin_stride=2, ch_scale, ch_shift, relu=True).view(49 R, C), U,
                         in_roi_major=True, ...)
    and the same bits.  feat [N,H,W,C] fp32, possibly a channel slice of a wider channels-last map.  With C % 64 == 0 the pooled
    rows never leave the ROIAlign workgroup: it writes their Winograd input transform itself (roi_align_nhwc.hip, WINO)."""
    if not isinstance(feat, torch.Tensor) or feat.dim() != 4 or feat.dtype != torch.float32:
        raise ValueError("roi_align_winograd_conv3x3: feat must be fp32 [N,H,W,C]")
    Nimg, H, W, C = feat.shape
    fld = C
    if (feat.is_cuda and feat.stride(3) == 1 and feat.stride(2) > C and feat.stride(2) % 4 == 0
            and feat.stride(1) == W * feat.stride(2) and feat.stride(0) == H * W * feat.stride(2)
            and feat.data_ptr() % 16 == 0):
        fld = feat.stride(2)                       # channel slice of a wider map: no copy
    else:
        feat = _dev(feat, "feat")
    rois = _dev(rois, "rois")
    Ud = _dev(U.data, "U")
    if Ud.dim() != 3 or Ud.shape[0] != 121 or Ud.shape[2] != C or C % 32 or output_size not in (13, 14):
        raise ValueError(f"roi_align_winograd_conv3x3: feat {tuple(feat.shape)} U {tuple(Ud.shape)} output_size {output_size}")
    N, R = Ud.shape[1], rois.shape[0]
    if N % 4 or (out_split_scale is not None and N % 32):
        raise ValueError("roi_align_winograd_conv3x3: N % 4 == 0 (N % 32 == 0 for a split-layout output)")
    ch_scale = _dev(ch_scale, "ch_scale") if ch_scale is not None else None
    ch_shift = _dev(ch_shift, "ch_shift") if ch_shift is not None else None
    scale2 = _dev(scale2, "scale2") if scale2 is not None else None
    shift2 = _dev(shift2, "shift2") if shift2 is not None else None
    y = torch.empty((49 * R, N), dtype=torch.float32, device=feat.device)
    lib = _lib.load()
    need = int(lib.locov_roi_align_winograd_workspace_bytes(R, C, N))       # no pixel scratch for the fused form
    key = (feat.device, torch.cuda.current_stream(feat.device).cuda_stream)
    ws = _WINO_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = None
        _WINO_WS.pop(key, None)
        ws = _WINO_WS[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=feat.device)
    wflags = (_lib.EPI_RELU if relu else 0) | (_lib.WINO_OUT_ROI_MAJOR if roi_major else 0) | _lib.WINO_IN_ROI_MAJOR
    with torch.cuda.device(feat.device):
        check(lib.locov_roi_align_winograd_conv3x3_f32_split(_ptr(feat), Nimg, H, W, C, fld, _ptr(rois), R, int(output_size),
                                                             float(spatial_scale), int(sampling_ratio), int(aligned), _ptr(ch_scale),
                                                             _ptr(ch_shift), _ptr(Ud), U.scale, float(v_scale), _ptr(scale2), _ptr(shift2),
                                                             _ptr(y), N, N, wflags, float(out_split_scale or 0.0), _ptr(ws), ws.numel(),
                                                             _ptr(_overflow_word(feat)), _stream(feat)),
              "locov_roi_align_winograd_conv3x3_f32_split")
    return y


def gemm_nt_batched(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x [B,M,K], w [B,N,K] -> [B,M,N] (fp32, one launch)."""
    x = _dev(x, "x")
    w = _dev(w, "w")
    B, M, K = x.shape
    if w.shape[0] != B or w.shape[2] != K:
        raise ValueError("gemm_nt_batched: inconsistent shapes")
    N = w.shape[1]
    y = torch.empty((B, M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_gemm_nt_batched_f32(_ptr(x), K, M * K, _ptr(w), N * K, _ptr(y), N, M * N, M, N, K, B,
                                                    _stream(x)), "locov_gemm_nt_batched_f32")
    return y


class RangeGuard:
    """One range-guard word of the split arithmetic: a device int32 every split-operand launch made while the guard is
    ACTIVE (`with ops.range_guard(g):`) ORs 1 into when it saw |scale * x| >= 65504, plus a pinned host mirror.

        g.reset()            zero the word (enqueued on the current stream)
        g.snapshot()         enqueue the 4-byte copy to pinned memory + an event (no host wait)
        g.raised()           the mirrored value; waits for the snapshot's event only (takes the snapshot first if none is pending)

    A guard belongs to ONE caller (a module and a stream): nothing else clears or reads it, so a reset enqueued by another
    module, stream or thread cannot hide a flag raised for this caller."""

    def __init__(self, device, deferred: bool = False):
        self.device = torch.device(device)
        self.word = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = None
        # deferred: nobody reads this word before the results are used -- whoever holds the guard zero-fills what the guarded
        # launches produced ON THE DEVICE when it is set (zero_if_raised) and reads the word whenever it next talks to the host
        # (the training forward: res5_train.Res5BlockFn / EmbeddingProposalsRes5ROIHeads.forward)
        self.deferred = deferred

    def reset(self) -> None:
        self.word.zero_()
        self.event = None

    def snapshot(self) -> None:
        self.host.copy_(self.word, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(self.device))

    def raised(self) -> bool:
        if self.event is None:
            self.snapshot()
        self.event.synchronize()
        self.event = None
        return bool(int(self.host[0]))


_GUARDS = threading.local()
_OVERFLOW = {}


class range_guard:
    """Context manager: split-operand launches on `guard.device` made inside the block raise `guard`'s word."""

    def __init__(self, guard: Optional[RangeGuard]):
        self.guard = guard

    def __enter__(self):
        st = getattr(_GUARDS, "stack", None)
        if st is None:
            st = _GUARDS.stack = []
        st.append(self.guard)
        return self.guard

    def __exit__(self, *exc):
        _GUARDS.stack.pop()
        return False


def active_guard(device) -> Optional[RangeGuard]:
    """The innermost active guard of this thread for `device` (None outside every range_guard block)."""
    for g in reversed(getattr(_GUARDS, "stack", None) or ()):
        if g is not None and g.device == torch.device(device):
            return g
    return None


def _overflow_word(ref: torch.Tensor) -> torch.Tensor:
    """The device word a split-operand launch ORs its range-guard result into: the active guard's (range_guard), else a
    per-(device, stream) word that nobody reads (launches outside every guard are unguarded by the caller's choice)."""
    g = active_guard(ref.device)
    if g is not None:
        return g.word
    key = (ref.device, torch.cuda.current_stream(ref.device).cuda_stream)
    w = _OVERFLOW.get(key)
    if w is None:
        w = _OVERFLOW[key] = torch.zeros(1, dtype=torch.int32, device=ref.device)
    return w


def split_overflow_reset(device) -> None:
    """Clear the default (unguarded-launch) word of `device` and the current stream.  Kept for callers that drive single
    launches by hand (tests, tools); modules own a RangeGuard instead."""
    _overflow_word(torch.empty(0, device=device)).zero_()


def split_overflow_raised(device) -> bool:
    """True when a split-operand launch on the current stream, outside every guard, since the last reset saw
    |x_scale * x| >= 65504 (ONE host read: it waits for the launches enqueued so far)."""
    return bool(_overflow_word(torch.empty(0, device=device)).item())


class SplitWeight(NamedTuple):
    """A weight matrix in the split-operand layout (split_pack) and the power-of-two scale it was packed with."""
    data: torch.Tensor
    scale: float


def split_pack(w: torch.Tensor, scale: Optional[float] = None) -> SplitWeight:
    """fp32 [..., K] (K % 32 == 0) -> the split-operand layout of locov_split_f16x2_pack: a float32-typed tensor of
    the same shape whose bytes hold, per row and group of 8 columns, 8 fp16 hi halves then 8 fp16 lo halves of
    scale * w (scale * w = hi + lo).  scale defaults to the power of two that puts max |scale * w| in [2^12, 2^13).
    Only meaningful as the `weight` of linear_split / gemm_nt_batched_split."""
    w = _dev(w, "w")
    K = w.shape[-1]
    if K % 32:
        raise ValueError(f"split_pack: K = {K} must be a multiple of 32")
    if scale is None:
        amax = float(w.abs().max()) if w.numel() else 1.0
        scale = 2.0 ** (12 - math.floor(math.log2(amax))) if amax > 0 and math.isfinite(amax) else 1.0
        scale = min(max(scale, 2.0 ** -100), 2.0 ** 100)
    out = torch.empty_like(w)
    rows = w.numel() // K
    with torch.cuda.device(w.device):
        check(_lib.load().locov_split_f16x2_pack(_ptr(w), rows, K, K, float(scale), _ptr(out), _ptr(_overflow_word(w)),
                                                 _stream(w)), "locov_split_f16x2_pack")
    return SplitWeight(out, float(scale))


def split_scale_for(w: torch.Tensor) -> float:
    """The power of two split_pack would choose for w (max |scale * w| in [2^12, 2^13)); ONE host read of max |w|."""
    amax = float(w.detach().abs().max()) if w.numel() else 1.0
    scale = 2.0 ** (12 - math.floor(math.log2(amax))) if amax > 0 and math.isfinite(amax) else 1.0
    return min(max(scale, 2.0 ** -100), 2.0 ** 100)


def linear_split(x: torch.Tensor, weight: SplitWeight, bias: Optional[torch.Tensor] = None, *,
                 scale: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                 relu: bool = False, x_scale: float = 16.0, x_is_split: bool = False, out_split: bool = False,
                 residual_is_split: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = epi(x . W^T), fp32 in / fp32 out, products on the f16 matrix pipe with split operands (opt-in "f16x2"
    arithmetic).  x [M,K] fp32 (rows may be strided), weight = split_pack(W [N,K]); x_scale = the power of two x is
    multiplied by before the split (|x_scale * x| must stay below 65504: |x| < 4094 at the default).
    out_split: y is written in the split layout scaled by x_scale (float32-TYPED storage of that layout: the pre-split x of
    the next split GEMM, and its residual with residual_is_split); residual_is_split: the residual is such a tensor."""
    x = _rows(x, "x")
    wd = _dev(weight.data, "weight")
    M, K = x.shape
    N = wd.shape[0]
    if wd.shape[1] != K or K % 32 or N % 4:
        raise ValueError(f"linear_split: x {tuple(x.shape)} weight {tuple(wd.shape)} (K % 32 == 0, N % 4 == 0)")
    bias = _dev(bias, "bias") if bias is not None else None
    scale = _dev(scale, "scale") if scale is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    if residual is not None and tuple(residual.shape) != (M, N):
        raise ValueError("residual must be [M,N]")
    y = _out(out, (M, N), x, "linear_split")
    with torch.cuda.device(x.device):
        check(_lib.load().locov_gemm_nt_f32_split(_ptr(x), x.stride(0) if M else K, _ptr(wd), _ptr(scale), _ptr(bias),
                                                  _ptr(residual), _ptr(y), N, M, N, K,
                                                  (_lib.EPI_RELU if relu else 0) | (_lib.GEMM_A_SPLIT if x_is_split else 0)
                                                  | (_lib.EPI_OUT_SPLIT if out_split else 0)
                                                  | (_lib.EPI_RES_SPLIT if residual_is_split and residual is not None else 0),
                                                  float(x_scale), weight.scale, _ptr(_overflow_word(x)), _stream(x)),
              "locov_gemm_nt_f32_split")
    return y


def split_unpack(t: torch.Tensor, scale: float) -> torch.Tensor:
    """fp32 values of a tensor held in the split layout (split_pack / out_split): (hi + lo) / scale.  Test / debug aid."""
    K = t.shape[-1]
    h = t.contiguous().view(torch.float16).view(*t.shape[:-1], K // 8, 2, 8).float()
    return ((h[..., 0, :] + h[..., 1, :]) / scale).reshape(t.shape)


_SEGMEAN_WS = {}


def segmean_supported(M: int, N: int, K: int, seg: int, lda: Optional[int] = None, *, residual_roi_major: bool = False,
                      x_is_split: bool = False, residual_is_split: bool = False) -> bool:
    """Can linear_split_segmean launch this shape?  (The 256 x 256 tile takes any M; the 128 x 128 one needs M * N * 4 < 2^32.)"""
    flags = ((_lib.SEGMEAN_RES_ROI_MAJOR if residual_roi_major else 0) | (_lib.GEMM_A_SPLIT if x_is_split else 0)
             | (_lib.EPI_RES_SPLIT if residual_is_split else 0) | _lib.EPI_RELU)
    return bool(_lib.load().locov_gemm_segmean_supported(int(K if lda is None else lda), int(M), int(N), int(K), int(seg), flags))


def linear_split_segmean(x: torch.Tensor, weight: SplitWeight, bias: Optional[torch.Tensor], residual: torch.Tensor, seg: int, *,
                         scale: Optional[torch.Tensor] = None, relu: bool = True, x_scale: float = 16.0,
                         residual_roi_major: bool = False, x_is_split: bool = False,
                         residual_is_split: bool = False) -> torch.Tensor:
    """Res5's last 1x1 convolution fused with the spatial mean behind it:
        out[q, :] = mean_{p < seg} relu(scale * (x[q*seg + p, :] . W^T) + bias + residual[p*R + q, :]),   R = M // seg
    x [M,K] with ROI-major rows, residual [M,N] with POSITION-major rows (the previous block's output; ROI-major rows
    q*seg + p with residual_roi_major), -> [R,N].
    The [M,N] tensor is neither written nor re-read; deterministic (fixed summation order)."""
    x = _rows(x, "x")
    wd = _dev(weight.data, "weight")
    residual = _dev(residual, "residual")
    M, K = x.shape
    N = wd.shape[0]
    if wd.shape[1] != K or K % 32 or N % 4 or seg <= 0 or M % seg or tuple(residual.shape) != (M, N):
        raise ValueError(f"linear_split_segmean: x {tuple(x.shape)} weight {tuple(wd.shape)} residual {tuple(residual.shape)} seg {seg}")
    bias = _dev(bias, "bias") if bias is not None else None
    scale = _dev(scale, "scale") if scale is not None else None
    out = torch.empty((M // seg, N), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    need = int(lib.locov_gemm_segmean_workspace_bytes(M, N))
    key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
    ws = _SEGMEAN_WS.get(key)
    if ws is None or ws.numel() < need:
        _SEGMEAN_WS.pop(key, None)
        ws = _SEGMEAN_WS[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.locov_gemm_nt_f32_split_segmean(_ptr(x), x.stride(0) if M else K, _ptr(wd), _ptr(scale), _ptr(bias),
                                                  _ptr(residual), _ptr(out), M, N, K, int(seg),
                                                  (_lib.EPI_RELU if relu else 0) | (_lib.SEGMEAN_RES_ROI_MAJOR if residual_roi_major else 0)
                                                  | (_lib.GEMM_A_SPLIT if x_is_split else 0) | (_lib.EPI_RES_SPLIT if residual_is_split else 0),
                                                  float(x_scale), weight.scale, _ptr(ws), ws.numel(), _ptr(_overflow_word(x)),
                                                  _stream(x)),
              "locov_gemm_nt_f32_split_segmean")
    return out


def gemm_nt_batched_split(x: torch.Tensor, w: SplitWeight, x_scale: float = 1.0) -> torch.Tensor:
    """x [B,M,K] fp32, w = split_pack(w [B,N,K]) -> [B,M,N] fp32 (one launch, split-operand arithmetic)."""
    x = _dev(x, "x")
    wd = _dev(w.data, "w")
    B, M, K = x.shape
    if wd.shape[0] != B or wd.shape[2] != K or K % 32:
        raise ValueError("gemm_nt_batched_split: inconsistent shapes")
    N = wd.shape[1]
    y = torch.empty((B, M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_gemm_nt_batched_f32_split(_ptr(x), K, M * K, _ptr(wd), N * K, _ptr(y), N, M * N, M, N, K,
                                                          B, float(x_scale), w.scale, _ptr(_overflow_word(x)), _stream(x)),
              "locov_gemm_nt_batched_f32_split")
    return y


def frozen_bn_fold(weight, bias, running_mean, running_var, eps: float = 1e-5):
    """FrozenBatchNorm2d -> per-channel (scale, shift)."""
    weight = _dev(weight, "weight")
    C = weight.numel()
    scale = torch.empty(C, dtype=torch.float32, device=weight.device)
    shift = torch.empty(C, dtype=torch.float32, device=weight.device)
    with torch.cuda.device(weight.device):
        check(_lib.load().locov_frozen_bn_fold(_ptr(weight), _ptr(_dev(bias, "bias")),
                                               _ptr(_dev(running_mean, "running_mean")),
                                               _ptr(_dev(running_var, "running_var")), float(eps), C, _ptr(scale),
                                               _ptr(shift), _stream(weight)), "locov_frozen_bn_fold")
    return scale, shift


def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """torchvision.ops.nms semantics on the device: indices of the kept boxes in descending score
    order.  The sort uses torch (plumbing); the IoU bit matrix and the greedy sweep are HIP kernels
    and nothing is copied to the host except the final count."""
    boxes = _dev(boxes, "boxes")
    scores = _dev(scores, "scores")
    K = boxes.shape[0]
    if K == 0:
        return torch.zeros((0,), dtype=torch.int64, device=boxes.device)
    order = torch.argsort(scores, descending=True, stable=True)
    sorted_boxes = boxes[order].contiguous()
    lib = _lib.load()
    ws = _workspace("nms", boxes, int(lib.locov_nms_workspace_bytes(K)))        # cached: grows to the largest request
    keep = torch.empty((K,), dtype=torch.uint8, device=boxes.device)
    num = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        check(lib.locov_nms_sorted(_ptr(sorted_boxes), K, float(iou_threshold), _ptr(ws), _ptr(keep), _ptr(num),
                                   _stream(boxes)), "locov_nms_sorted")
    return order[keep.bool()]


DETECT_MAX_IMAGES = _lib.LABEL_MAX_IMAGES
DETECT_MAX_ROWS_PER_IMAGE, DETECT_MAX_CLASSES, DETECT_MAX_TOPK = (1 << 14) - 1, (1 << 15) - 1, _lib.DETECT_MAX_CANDIDATES
_DETECT_PINNED = {}


def detect_postprocess(probs: torch.Tensor, deltas: torch.Tensor, proposal_boxes: torch.Tensor, sizes, image_shapes, weights,
                       scale_clamp: float, score_thresh: float, nms_thresh: float, topk: int):
    """The detection post-processing of a batch on the device (csrc/detect.hip): box decoding, clipping, score threshold,
    class-wise NMS, top-k -- seven launches and ONE host read (the detections per image + the flag word) instead of the torch
    chain's ~100 launches and four reads.
    probs [R, K + 1] = softmax of the logits, proposal_boxes [R, 4], deltas [R, 4] (class-agnostic regression) or [R, 4K]
    (class-specific: candidate (r, c) has the box decoded from deltas[r, 4c:4c + 4]), sizes: rows per image, image_shapes:
    (height, width) per image, weights: Box2BoxTransform's.
    Returns (boxes [B, topk, 4], scores [B, topk], classes [B, topk] int64, rows [B, topk] int64, counts: list of B ints) -- the
    slots at or beyond an image's count are empty (box 0, score 0, class -1, row -1) --, or None when the kernels flagged a case
    they do not take (non-finite values, more than DETECT_MAX_CANDIDATES candidates in an image): the caller then runs the torch
    chain."""
    out, flags = _detect_postprocess_flags(probs, deltas, proposal_boxes, sizes, image_shapes, weights, scale_clamp, score_thresh,
                                           nms_thresh, topk)
    return None if flags else out


def _detect_postprocess_flags(probs, deltas, proposal_boxes, sizes, image_shapes, weights, scale_clamp, score_thresh, nms_thresh, topk,
                              per_class_above=None):
    """detect_postprocess's work, with the flag word (DETECT_FLAG_*) returned next to the outputs instead of folded into None.
    per_class_above=None: the LDS pipeline (locov_detect_postprocess); an int: the wide one (locov_detect_postprocess_wide).
    deltas [R, 4K] with K > 1 go to the class-specific entry points (locov_detect_postprocess_cs / _wide_cs)."""
    probs, deltas, proposal_boxes = _dev(probs, "probs"), _dev(deltas, "deltas"), _dev(proposal_boxes, "proposal_boxes")
    B, R, K = len(sizes), probs.shape[0], probs.shape[1] - 1
    if not (deltas.dim() == 2 and deltas.shape[0] == R and deltas.shape[1] in (4, 4 * K) and tuple(proposal_boxes.shape) == (R, 4)
            and sum(sizes) == R and len(image_shapes) == B):
        raise ValueError("detect_postprocess: inconsistent shapes (deltas must be [R, 4] or [R, 4K])")
    box_classes = deltas.shape[1] // 4
    if not (0 < B <= DETECT_MAX_IMAGES and 1 <= K <= DETECT_MAX_CLASSES and 1 <= topk <= DETECT_MAX_TOPK
            and max(sizes, default=0) <= DETECT_MAX_ROWS_PER_IMAGE and R * box_classes < 2 ** 31):
        raise ValueError("detect_postprocess: outside the kernels' limits (images, classes, rows per image, rows x classes or top-k)")
    lib = _lib.load()
    dev = probs.device
    offs = (ctypes.c_int * (B + 1))(0, *itertools.accumulate(int(n) for n in sizes))
    hw = (ctypes.c_float * (2 * B))(*[float(v) for shape in image_shapes for v in shape[:2]])
    if per_class_above is None:
        if box_classes == 1:
            nbytes = int(lib.locov_detect_postprocess_workspace_bytes(max(R, 1), B))
        else:
            nbytes = int(lib.locov_detect_postprocess_cs_workspace_bytes(max(R, 1), B, K, deltas.stride(0), box_classes))
            if nbytes < 0:
                check(nbytes, "locov_detect_postprocess_cs_workspace_bytes")
    else:
        per_class_above = max(min(int(per_class_above), 2 ** 31 - 1), -2 ** 31)
        if box_classes == 1:
            nbytes = int(lib.locov_detect_postprocess_wide_workspace_bytes(offs, B, K, per_class_above))
        else:
            nbytes = int(lib.locov_detect_postprocess_wide_cs_workspace_bytes(offs, B, K, per_class_above, deltas.stride(0), box_classes))
        if nbytes < 0:
            check(nbytes, "locov_detect_postprocess_wide_workspace_bytes")
    ws = _workspace("detect", probs, nbytes)
    out_boxes = torch.empty((B, topk, 4), dtype=torch.float32, device=dev)
    out_scores = torch.empty((B, topk), dtype=torch.float32, device=dev)
    out_classes = torch.empty((B, topk), dtype=torch.int64, device=dev)
    out_rows = torch.empty((B, topk), dtype=torch.int64, device=dev)
    counts = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    wx, wy, ww, wh = (float(w) for w in weights)
    with torch.cuda.device(dev):
        if box_classes > 1 and per_class_above is None:
            check(lib.locov_detect_postprocess_cs(_ptr(probs), probs.stride(0), K, _ptr(deltas), deltas.stride(0), box_classes,
                                                  _ptr(proposal_boxes), offs, hw, B, wx, wy, ww, wh, float(scale_clamp), float(score_thresh),
                                                  float(nms_thresh), int(topk), _ptr(ws), ws.numel(), _ptr(out_boxes), _ptr(out_scores),
                                                  _ptr(out_classes), _ptr(out_rows), _ptr(counts), _stream(probs)),
                  "locov_detect_postprocess_cs")
        elif box_classes > 1:
            check(lib.locov_detect_postprocess_wide_cs(_ptr(probs), probs.stride(0), K, _ptr(deltas), deltas.stride(0), box_classes,
                                                       _ptr(proposal_boxes), offs, hw, B, wx, wy, ww, wh, float(scale_clamp),
                                                       float(score_thresh), float(nms_thresh), int(topk), per_class_above, _ptr(ws),
                                                       ws.numel(), _ptr(out_boxes), _ptr(out_scores), _ptr(out_classes), _ptr(out_rows),
                                                       _ptr(counts), _stream(probs)), "locov_detect_postprocess_wide_cs")
        elif per_class_above is None:
            check(lib.locov_detect_postprocess(_ptr(probs), probs.stride(0), K, _ptr(deltas), _ptr(proposal_boxes), offs, hw, B, wx, wy, ww,
                                               wh, float(scale_clamp), float(score_thresh), float(nms_thresh), int(topk), _ptr(ws),
                                               ws.numel(), _ptr(out_boxes), _ptr(out_scores), _ptr(out_classes), _ptr(out_rows),
                                               _ptr(counts), _stream(probs)), "locov_detect_postprocess")
        else:
            check(lib.locov_detect_postprocess_wide(_ptr(probs), probs.stride(0), K, _ptr(deltas), _ptr(proposal_boxes), offs, hw, B, wx,
                                                    wy, ww, wh, float(scale_clamp), float(score_thresh), float(nms_thresh), int(topk),
                                                    per_class_above, _ptr(ws), ws.numel(), _ptr(out_boxes), _ptr(out_scores),
                                                    _ptr(out_classes), _ptr(out_rows), _ptr(counts), _stream(probs)),
                  "locov_detect_postprocess_wide")
    vals = _read_counts_and_flags(counts)
    return (out_boxes, out_scores, out_classes, out_rows, vals[:B]), vals[B]


def _read_counts_and_flags(counts: torch.Tensor) -> list:
    """The ONE host read of a post-processing call: its B + 1 ints to pinned memory behind an event (the stream's later work
    stays queued)."""
    dev, n = counts.device, counts.numel()
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    host = _DETECT_PINNED.get(key)
    if host is None or host.numel() < n:
        host = _DETECT_PINNED[key] = torch.empty(max(n, DETECT_MAX_IMAGES + 1), dtype=torch.int32).pin_memory()
    host[:n].copy_(counts, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    ev.synchronize()
    return host[:n].tolist()


def detect_postprocess_wide(probs: torch.Tensor, deltas: torch.Tensor, proposal_boxes: torch.Tensor, sizes, image_shapes, weights,
                            scale_clamp: float, score_thresh: float, nms_thresh: float, topk: int, per_class_above: int):
    """detect_postprocess for ANY candidate count (csrc/detect_wide.hip): LVIS-style thresholds (1e-4 over 1 203 classes: up to
    1.2e6 candidates per image) stay on the device with ONE host read.  per_class_above: batched_nms's switch -- an image with that
    many candidates or more runs one NMS per class on the unshifted boxes, below it one NMS on the class-shifted boxes.
    Returns what detect_postprocess returns; None only when the kernels flagged non-finite values (the caller runs the torch chain)."""
    out, flags = _detect_postprocess_flags(probs, deltas, proposal_boxes, sizes, image_shapes, weights, scale_clamp, score_thresh,
                                           nms_thresh, topk, per_class_above=per_class_above)
    return None if flags else out


RPN_MAX_IMAGES, RPN_MAX_PRE_NMS_TOPK, RPN_MAX_ANCHORS = _lib.LABEL_MAX_IMAGES, _lib.RPN_MAX_PRE_NMS_TOPK, _lib.RPN_MAX_ANCHORS


def rpn_proposals(logits: torch.Tensor, deltas: torch.Tensor, anchors: torch.Tensor, image_shapes, weights, scale_clamp: float,
                  pre_nms_topk: int, post_nms_topk: int, min_box_size: float, nms_thresh: float):
    """The RPN's proposal generation of one feature level on the device (csrc/rpn.hip): the pre_nms_topk best anchors per image
    (descending logit, ties by anchor index), box decoding, the finite test, clipping, the size filter, greedy NMS and the first
    post_nms_topk survivors -- three launches and ONE host read (the proposals per image + the flag word).
    logits [N, HWA], deltas [N, HWA, 4], anchors [HWA, 4] in the (y, x, a) order of an NHWC head output; image_shapes: (height,
    width) per image; weights: Box2BoxTransform's.
    Returns (boxes [N, post, 4], logits [N, post], index [N, post] int64, counts: list of N ints); rows at or beyond an image's
    count are zero (index -1).  None when the kernels flagged non-finite values: the caller then runs the torch chain."""
    out, flags = _rpn_proposals_flags(logits, deltas, anchors, image_shapes, weights, scale_clamp, pre_nms_topk, post_nms_topk,
                                      min_box_size, nms_thresh)
    return None if flags else out


def _rpn_proposals_flags(logits, deltas, anchors, image_shapes, weights, scale_clamp, pre_nms_topk, post_nms_topk, min_box_size,
                         nms_thresh):
    """rpn_proposals's work, with the flag word (RPN_FLAG_NONFINITE) returned next to the outputs instead of folded into None."""
    logits, deltas, anchors = _dev(logits, "logits"), _dev(deltas, "deltas"), _dev(anchors, "anchors")
    if logits.dim() != 2 or tuple(deltas.shape) != (*logits.shape, 4) or tuple(anchors.shape) != (logits.shape[1], 4) \
            or len(image_shapes) != logits.shape[0]:
        raise ValueError("rpn_proposals: inconsistent shapes (logits [N, HWA], deltas [N, HWA, 4], anchors [HWA, 4], N image shapes)")
    N, HWA = logits.shape
    pre, post = int(pre_nms_topk), int(post_nms_topk)
    if not (N <= RPN_MAX_IMAGES and HWA <= RPN_MAX_ANCHORS and 1 <= post <= pre <= RPN_MAX_PRE_NMS_TOPK):
        raise ValueError("rpn_proposals: outside the kernels' limits (images, anchors per image, 1 <= post <= pre <= 16 384)")
    dev = logits.device
    if N == 0 or HWA == 0:                  # (the C call is a no-op then: the empty rows are written here)
        return (torch.zeros((N, post, 4), dtype=torch.float32, device=dev), torch.zeros((N, post), dtype=torch.float32, device=dev),
                torch.full((N, post), -1, dtype=torch.int64, device=dev), [0] * N), 0
    out_boxes = torch.empty((N, post, 4), dtype=torch.float32, device=dev)
    out_logits = torch.empty((N, post), dtype=torch.float32, device=dev)
    out_index = torch.empty((N, post), dtype=torch.int64, device=dev)
    lib = _lib.load()
    hw = (ctypes.c_float * (2 * N))(*[float(v) for shape in image_shapes for v in shape[:2]])
    nbytes = int(lib.locov_rpn_proposals_workspace_bytes(N, HWA, pre))
    if nbytes < 0:
        check(nbytes, "locov_rpn_proposals_workspace_bytes")
    ws = _workspace("rpn", logits, nbytes)
    counts = torch.empty((N + 1,), dtype=torch.int32, device=dev)
    wx, wy, ww, wh = (float(w) for w in weights)
    with torch.cuda.device(dev):
        check(lib.locov_rpn_proposals(_ptr(logits), _ptr(deltas), _ptr(anchors), HWA, hw, N, wx, wy, ww, wh, float(scale_clamp), pre, post,
                                      float(min_box_size), float(nms_thresh), _ptr(ws), ws.numel(), _ptr(out_boxes), _ptr(out_logits),
                                      _ptr(out_index), _ptr(counts), _stream(logits)), "locov_rpn_proposals")
    vals = _read_counts_and_flags(counts)
    return (out_boxes, out_logits, out_index, vals[:N]), vals[N]


# --------------------------------------------------------------------------------------
# Backward-pass building blocks of the Res5 stage (csrc/gemm_tn.hip, res5_bwd.hip, the mask epilogue of gemm_nt.hip and
# the gradient transforms of winograd.hip); composed by locov_amd/res5_train.py.
_WS = {}


def _workspace(tag: str, ref: torch.Tensor, nbytes: int) -> torch.Tensor:
    """Cached device scratch (grows to the largest request), one per (tag, device, stream)."""
    key = (tag, ref.device, torch.cuda.current_stream(ref.device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        _WS.pop(key, None)
        ws = _WS[key] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=ref.device)
    return ws


def linear_ex(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, scale=None, residual=None,
              mask=None, relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear() with the weight rows optionally strided (a column block of a wider matrix) and an optional `mask` [M,N]:
    the finished value is kept where mask > 0 and zeroed elsewhere (ReLU backward fused into a data-gradient GEMM)."""
    x = _rows(x, "x")
    weight = _rows(weight, "weight")
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K or K % 4:
        raise ValueError(f"linear_ex: x {tuple(x.shape)} weight {tuple(weight.shape)} (K must be a multiple of 4)")
    bias = _dev(bias, "bias") if bias is not None else None
    scale = _dev(scale, "scale") if scale is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    mask = _dev(mask, "mask") if mask is not None else None
    for t, name in ((residual, "residual"), (mask, "mask")):
        if t is not None and tuple(t.shape) != (M, N):
            raise ValueError(f"linear_ex: {name} must be [M,N]")
    y = torch.empty((M, N), dtype=torch.float32, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or not y.is_contiguous():
        raise ValueError("linear_ex: out must be a contiguous [M,N] tensor")
    with torch.cuda.device(x.device):
        check(_lib.load().locov_gemm_nt_f32_ex(_ptr(x), x.stride(0) if M else K, _ptr(weight), weight.stride(0), _ptr(scale),
                                               _ptr(bias), _ptr(residual), _ptr(mask), _ptr(y), N, M, N, K,
                                               _lib.EPI_RELU if relu else 0, _stream(x)), "locov_gemm_nt_f32_ex")
    return y


def conv3x3_nhwc_ex(x: torch.Tensor, w_packed: torch.Tensor, H: int, W: int, *, scale=None, shift=None, residual=None,
                    mask=None, relu: bool = False, pos_major: bool = False) -> torch.Tensor:
    """conv3x3_nhwc() with the optional epilogue mask of linear_ex."""
    x = _dev(x, "x")
    w_packed = _dev(w_packed, "w_packed")
    M, Cin = x.shape
    N = w_packed.shape[0]
    if w_packed.shape[1] != 9 * Cin or M % (H * W) != 0:
        raise ValueError("conv3x3_nhwc_ex: inconsistent shapes")
    scale = _dev(scale, "scale") if scale is not None else None
    shift = _dev(shift, "shift") if shift is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    mask = _dev(mask, "mask") if mask is not None else None
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_conv3x3_nhwc_f32_ex(_ptr(x), M // (H * W), H, W, Cin, int(pos_major), _ptr(w_packed), _ptr(scale),
                                                    _ptr(shift), _ptr(residual), _ptr(mask), _ptr(y), N,
                                                    _lib.EPI_RELU if relu else 0, _stream(x)), "locov_conv3x3_nhwc_f32_ex")
    return y


def winograd_conv3x3_ex(x: torch.Tensor, U: torch.Tensor, *, scale=None, shift=None, mask=None, relu: bool = False,
                        roi_major: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """winograd_conv3x3() on the f32 MFMA with the optional output mask (rows of x, mask and the result in one order:
    ROI-major by default)."""
    x = _dev(x, "x")
    U = _dev(U, "U")
    M, Cin = x.shape
    if U.dim() != 3 or U.shape[0] != 121 or U.shape[2] != Cin or M % 49 != 0:
        raise ValueError("winograd_conv3x3_ex: inconsistent shapes")
    N, R = U.shape[1], M // 49
    scale = _dev(scale, "scale") if scale is not None else None
    shift = _dev(shift, "shift") if shift is not None else None
    mask = _dev(mask, "mask") if mask is not None else None
    if mask is not None and tuple(mask.shape) != (M, N):
        raise ValueError("winograd_conv3x3_ex: mask must be [49*R, N]")
    y = _out(out, (M, N), x, "winograd_conv3x3_ex")
    lib = _lib.load()
    ws = _workspace("wino", x, int(lib.locov_winograd_workspace_bytes(R, Cin, N)))
    flags = (_lib.EPI_RELU if relu else 0) | ((_lib.WINO_OUT_ROI_MAJOR | _lib.WINO_IN_ROI_MAJOR) if roi_major else 0)
    with torch.cuda.device(x.device):
        check(lib.locov_winograd_conv3x3_f32_ex(_ptr(x), R, Cin, _ptr(U), _ptr(scale), _ptr(shift), _ptr(mask), _ptr(y), N, N,
                                                flags, _ptr(ws), ws.numel(), _stream(x)), "locov_winograd_conv3x3_f32_ex")
    return y


def gemm_tn(a: torch.Tensor, b: torch.Tensor, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[N,K] = row_scale[n] * sum_m a[m,n] * b[m,k]  (a [M,N], b [M,K], rows may be strided): the weight gradient
    of a 1x1 convolution, dW = s * g^T x.  Deterministic (fixed-order reduction of the M chunks)."""
    a, b = _rows(a, "a"), _rows(b, "b")
    M, N = a.shape
    K = b.shape[1]
    if b.shape[0] != M or N % 4 or K % 4:
        raise ValueError(f"gemm_tn: a {tuple(a.shape)} b {tuple(b.shape)} (N, K must be multiples of 4)")
    row_scale = _dev(row_scale, "row_scale") if row_scale is not None else None
    out = torch.empty((N, K), dtype=torch.float32, device=a.device)
    lib = _lib.load()
    ws = _workspace("tn", a, int(lib.locov_gemm_tn_workspace_bytes(M, N, K, 1)))
    with torch.cuda.device(a.device):
        check(lib.locov_gemm_tn_f32(_ptr(a), a.stride(0) if M else N, 0, _ptr(b), b.stride(0) if M else K, 0, _ptr(out), K, 0,
                                    M, N, K, 1, _ptr(row_scale), _ptr(ws), ws.numel(), _stream(a)), "locov_gemm_tn_f32")
    return out


def winograd_wgrad(x: torch.Tensor, g: torch.Tensor, row_scale: Optional[torch.Tensor] = None,
                   roi_major: bool = True, split: bool = False, v_split: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dw [N,Cin,3,3] = row_scale[n] * d/dw of conv3x3(x) . g over R 7x7 tiles, in the Winograd domain.
    x [49*R, Cin], g [49*R, N], both in the same row order.  split: the 121 TN GEMMs in split-operand arithmetic.
    v_split (split only): the workspace winograd_conv3x3(x, SplitWeight, workspace=...) was given in the forward -- it starts with
    the transformed x in the split layout, which is then not computed again (same bits)."""
    x, g = _dev(x, "x"), _dev(g, "g")
    M, Cin = x.shape
    N = g.shape[1]
    if g.shape[0] != M or M % 49 or Cin % 4 or N % 4:
        raise ValueError("winograd_wgrad: inconsistent shapes")
    R = M // 49
    if v_split is not None and not (split and R > 0 and Cin % 8 == 0 and v_split.is_cuda and v_split.device == x.device
                                    and v_split.numel() * v_split.element_size() >= 121 * R * Cin * 4 and v_split.data_ptr() % 16 == 0):
        raise ValueError("winograd_wgrad: v_split needs the split arithmetic, Cin % 8 == 0 and the forward's workspace of the same x")
    row_scale = _dev(row_scale, "row_scale") if row_scale is not None else None
    dw = torch.empty((N, Cin, 3, 3), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    ws = _workspace("wino_wgrad", x, int(lib.locov_winograd_wgrad_workspace_bytes(R, Cin, N)))
    with torch.cuda.device(x.device):
        if v_split is not None:
            check(lib.locov_winograd_wgrad_f32_split_v(_ptr(v_split), _ptr(g), R, Cin, N, _lib.WINO_IN_ROI_MAJOR if roi_major else 0,
                                                       _ptr(row_scale), _ptr(dw), _ptr(_overflow_word(x)), _ptr(ws), ws.numel(),
                                                       _stream(x)), "locov_winograd_wgrad_f32_split_v")
        elif split and R > 0:
            check(lib.locov_winograd_wgrad_f32_split(_ptr(x), _ptr(g), R, Cin, N, _lib.WINO_IN_ROI_MAJOR if roi_major else 0,
                                                     _ptr(row_scale), _ptr(dw), _ptr(_overflow_word(x)), _ptr(ws), ws.numel(),
                                                     _stream(x)), "locov_winograd_wgrad_f32_split")
        else:
            check(lib.locov_winograd_wgrad_f32(_ptr(x), _ptr(g), R, Cin, N, _lib.WINO_IN_ROI_MAJOR if roi_major else 0,
                                               _ptr(row_scale), _ptr(dw), _ptr(ws), ws.numel(), _stream(x)),
                  "locov_winograd_wgrad_f32")
    return dw


def split_scale_from_amax(x: torch.Tensor, target_log2: float = 13.0) -> torch.Tensor:
    """Device-side operand scale of a tensor whose range is only known on the device (a gradient): a 4-float device tensor
    {s, 1/s, bits of max|x|, -} with s the power of two that puts max |s x| in [2^(target-1), 2^target).  No host read."""
    x = _dev(x, "x")
    if x.numel() % 4:
        raise ValueError("split_scale_from_amax: numel must be a multiple of 4")
    out = _scale_slot(x)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_split_scale_from_amax_zeroed(_ptr(x), x.numel(), float(target_log2), _ptr(out), _stream(x)),
              "locov_split_scale_from_amax_zeroed")
    return out


def amax_bound(tensors, muls, slot: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A zeroed operand-scale slot (scale_slot) whose max word holds max_i (muls[i] * max |tensors[i]|): the range of a LARGE
    tensor about to be derived from these small ones (a broadcast / masked copy), without a pass over it.  No host read.
    slot: fold into this existing (lazy) slot instead of a fresh one."""
    ts = [(_dev(t, "tensor"), float(m)) for t, m in zip(tensors, muls) if t is not None and t.numel() > 0]
    if not ts:
        raise ValueError("amax_bound: no tensor")
    if len(ts) > _lib.AMAX_BOUND_MAX or any(t.numel() % 4 for t, _ in ts):
        raise ValueError(f"amax_bound: at most {_lib.AMAX_BOUND_MAX} tensors, numel % 4 == 0")
    if slot is None:
        slot = _scale_slot(ts[0][0], lazy=True)
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t, _ in ts])
    ns = (ctypes.c_int64 * len(ts))(*[t.numel() for t, _ in ts])
    ms = (ctypes.c_float * len(ts))(*[m for _, m in ts])
    with torch.cuda.device(slot.device):
        check(_lib.load().locov_amax_bound(ptrs, ns, ms, len(ts), _ptr(slot), _stream(slot)), "locov_amax_bound")
    return slot


_SCALE_SLOTS = {}


def _scale_slot(ref: torch.Tensor, lazy: bool = False) -> torch.Tensor:
    """16 bytes for a device-chosen operand scale, from a per-(device, stream) ring of 2048 zeroed slots.  The reduction kernel
    (split_scale_from_amax) leaves {s, 1/s, 0, 0} behind; a `lazy` slot (scale_slot: producers fold their max into
    word 2, consumers derive the scale while word 0 is zero) stays dirty too, so the ring is zeroed every time it wraps -- one
    fill per 2048 uses, enqueued behind every GEMM that read the old contents (same stream; a training step takes ~40 slots)."""
    key = (ref.device, torch.cuda.current_stream(ref.device).cuda_stream)
    ring = _SCALE_SLOTS.get(key)
    if ring is None:
        ring = _SCALE_SLOTS[key] = [torch.zeros(2048, 4, dtype=torch.float32, device=ref.device), 0, False]
    i = ring[1]
    if i == 0 and ring[2]:
        ring[0].zero_()
        ring[2] = False
    ring[1] = (i + 1) % ring[0].shape[0]
    # every hand-out dirties the ring: the reduction kernel leaves {s, 1/s, 0, 0} behind, and a LAZY consumer derives the scale
    # from word 2 only while word 0 is zero -- a slot that carried a reduced scale in the previous cycle must not be handed out
    # lazily with that stale s in it
    ring[2] = True
    return ring[0][i]


def scale_slot(ref: torch.Tensor) -> torch.Tensor:
    """A zeroed 16-byte operand-scale slot (device) for `amax_out=`: the kernel that writes a gradient folds max |.| into it,
    the split GEMMs that read the gradient (`x_scale_dev=` / `a_scale_dev=`) derive its power-of-two scale from that."""
    return _scale_slot(_dev(ref, "ref"), lazy=True)


def linear_split_ex(x: torch.Tensor, weight: SplitWeight, bias: Optional[torch.Tensor] = None, *, scale=None, residual=None,
                    mask=None, relu: bool = False, x_scale: float = 16.0, x_scale_dev: Optional[torch.Tensor] = None,
                    amax_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_split() with the epilogue mask of linear_ex and, optionally, the operand scale of x taken from device
    memory (split_scale_from_amax / scale_slot): the data-gradient GEMMs of the training step in split arithmetic.
    amax_out: scale_slot() that receives max |y|."""
    x = _rows(x, "x")
    wd = _dev(weight.data, "weight")
    M, K = x.shape
    N = wd.shape[0]
    if wd.shape[1] != K or K % 32 or N % 4:
        raise ValueError(f"linear_split_ex: x {tuple(x.shape)} weight {tuple(wd.shape)} (K % 32 == 0, N % 4 == 0)")
    bias = _dev(bias, "bias") if bias is not None else None
    scale = _dev(scale, "scale") if scale is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    mask = _dev(mask, "mask") if mask is not None else None
    for t_, name in ((residual, "residual"), (mask, "mask")):
        if t_ is not None and tuple(t_.shape) != (M, N):
            raise ValueError(f"linear_split_ex: {name} must be [M,N]")
    y = _out(out, (M, N), x, "linear_split_ex")
    with torch.cuda.device(x.device):
        check(_lib.load().locov_gemm_nt_f32_split_ex(_ptr(x), x.stride(0) if M else K, _ptr(wd), _ptr(scale), _ptr(bias), _ptr(residual),
                                                     _ptr(mask), _ptr(y), N, M, N, K, _lib.EPI_RELU if relu else 0, float(x_scale),
                                                     _ptr(x_scale_dev), weight.scale, _ptr(_overflow_word(x)), _ptr(amax_out), _stream(x)),
              "locov_gemm_nt_f32_split_ex")
    return y


def gemm_tn_split(a: torch.Tensor, b: torch.Tensor, row_scale: Optional[torch.Tensor], a_scale_dev: torch.Tensor,
                  b_scale: float = 16.0, b_is_split: bool = False) -> torch.Tensor:
    """gemm_tn() in split-operand arithmetic: a (gradient) scaled by a_scale_dev[0] (split_scale_from_amax), b (activation)
    by b_scale.  b_is_split: b is float32-typed storage of the split layout at that scale (split_pack / out_split), K % 8 == 0:
    transposed on its way into LDS instead of converted -- the same bits."""
    a, b = _rows(a, "a"), _rows(b, "b")
    M, N = a.shape
    K = b.shape[1]
    if b.shape[0] != M or N % 4 or K % 4 or M == 0 or (b_is_split and (K % 8 or b.stride(0) % 8)):
        raise ValueError(f"gemm_tn_split: a {tuple(a.shape)} b {tuple(b.shape)} (N, K multiples of 4 -- 8 for a pre-split b --, M > 0)")
    row_scale = _dev(row_scale, "row_scale") if row_scale is not None else None
    out = torch.empty((N, K), dtype=torch.float32, device=a.device)
    lib = _lib.load()
    ws = _workspace("tn", a, int(lib.locov_gemm_tn_workspace_bytes(M, N, K, 1)))
    with torch.cuda.device(a.device):
        fn = lib.locov_gemm_tn_f32_split_b if b_is_split else lib.locov_gemm_tn_f32_split
        check(fn(_ptr(a), a.stride(0), 0, _ptr(b), b.stride(0), 0, _ptr(out), K, 0, M, N, K, 1, _ptr(row_scale),
                 _ptr(a_scale_dev), float(b_scale), _ptr(_overflow_word(a)), _ptr(ws), ws.numel(), _stream(a)),
              "locov_gemm_tn_f32_split_b" if b_is_split else "locov_gemm_tn_f32_split")
    return out


def winograd_conv3x3_split_ex(x: torch.Tensor, U: SplitWeight, *, scale=None, shift=None, mask=None, relu: bool = False,
                              roi_major: bool = True, v_scale: Optional[float] = None,
                              amax_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """winograd_conv3x3() in split arithmetic with the output mask; v_scale None = chosen on the device from max |V| (the input
    is a gradient)."""
    x = _dev(x, "x")
    Ud = _dev(U.data, "U")
    M, Cin = x.shape
    if Ud.dim() != 3 or Ud.shape[0] != 121 or Ud.shape[2] != Cin or M % 49 != 0:
        raise ValueError("winograd_conv3x3_split_ex: inconsistent shapes")
    N, R = Ud.shape[1], M // 49
    scale = _dev(scale, "scale") if scale is not None else None
    shift = _dev(shift, "shift") if shift is not None else None
    mask = _dev(mask, "mask") if mask is not None else None
    if mask is not None and tuple(mask.shape) != (M, N):
        raise ValueError("winograd_conv3x3_split_ex: mask must be [49*R, N]")
    y = _out(out, (M, N), x, "winograd_conv3x3_split_ex")
    lib = _lib.load()
    ws = _workspace("wino", x, int(lib.locov_winograd_workspace_bytes(R, Cin, N)))
    flags = (_lib.EPI_RELU if relu else 0) | ((_lib.WINO_OUT_ROI_MAJOR | _lib.WINO_IN_ROI_MAJOR) if roi_major else 0)
    with torch.cuda.device(x.device):
        check(lib.locov_winograd_conv3x3_f32_split_ex(_ptr(x), R, Cin, _ptr(Ud), U.scale, float(v_scale or 1.0), int(v_scale is None),
                                                      _ptr(scale), _ptr(shift), _ptr(mask), _ptr(y), N, N, flags, 0.0, _ptr(ws), ws.numel(),
                                                      _ptr(_overflow_word(x)), _ptr(amax_out), _stream(x)), "locov_winograd_conv3x3_f32_split_ex")
    return y


def winograd_scale_slot(x: torch.Tensor, R: int, Cin: int, N: int, wgrad: bool = False) -> torch.Tensor:
    """The 16-byte operand-scale slot {s, 1/s, bits of max |.|, -} that the last winograd_conv3x3_split_ex(v_scale=None) (V's scale) or,
    with wgrad, winograd_wgrad(split=True) (dM's scale) on x's device and current stream filled: winograd.hip keeps it in the last 16
    bytes of the workspace it is given, here the cached one of that call.  Test / debug aid (a view, valid until the next such call)."""
    lib = _lib.load()
    if wgrad:
        ws = _workspace("wino_wgrad", x, int(lib.locov_winograd_wgrad_workspace_bytes(R, Cin, N)))
    else:
        ws = _workspace("wino", x, int(lib.locov_winograd_workspace_bytes(R, Cin, N)))
    return ws[ws.numel() - 16:].view(torch.float32)


PREP_KINDS = {"plain": _lib.PREP_PLAIN, "t": _lib.PREP_TRANSPOSE, "col": _lib.PREP_IM2COL, "flip9": _lib.PREP_IM2COL_FLIP,
              "wino": _lib.PREP_WINO, "uflip": _lib.PREP_WINO_FLIP}


def prep_shape(kind: str, w: torch.Tensor) -> Tuple[int, ...]:
    """Shape of the operand locov_res5_weight_prep derives from the convolution weight w for `kind`."""
    N, C = w.shape[0], w.shape[1]
    return {"plain": (N, C), "t": (C, N), "col": (N, 9 * C), "flip9": (C, 9 * N), "wino": (121, N, C), "uflip": (121, C, N)}[kind]


def res5_weight_prep(jobs) -> None:
    """jobs: [(kind, weight [N,K] | [N,Cin,3,3], FrozenBN row scale | None, out, split scale)] -- every split-layout operand of a
    training step in ONE launch (locov_res5_weight_prep); `out` are float32-typed tensors of prep_shape(kind, weight)."""
    if not jobs:
        return
    lib = _lib.load()
    ref = jobs[0][1]
    for i in range(0, len(jobs), _lib.WEIGHT_PREP_MAX_JOBS):
        chunk = jobs[i:i + _lib.WEIGHT_PREP_MAX_JOBS]
        arr = (_lib.WeightPrepJob * len(chunk))()
        for a, (kind, w, rs, out, scale) in zip(arr, chunk):
            w = _dev(w, "weight")
            if tuple(out.shape) != prep_shape(kind, w) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != w.device:
                raise ValueError(f"res5_weight_prep: out of a {kind!r} job must be a contiguous fp32 {prep_shape(kind, w)} tensor")
            a.w, a.row_scale, a.out = w.data_ptr(), (_dev(rs, "row_scale").data_ptr() if rs is not None else None), out.data_ptr()
            a.scale, a.kind, a.N, a.K = float(scale), PREP_KINDS[kind], int(w.shape[0]), int(w.shape[1])
        with torch.cuda.device(ref.device):
            check(lib.locov_res5_weight_prep(arr, len(chunk), _ptr(_overflow_word(ref)), _stream(ref)), "locov_res5_weight_prep")


def weight_transpose_scale(w: torch.Tensor, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w [N,K] -> [K,N] with out[k,n] = row_scale[n] * w[n,k]."""
    w = _dev(w, "w")
    N, K = w.shape
    row_scale = _dev(row_scale, "row_scale") if row_scale is not None else None
    out = torch.empty((K, N), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        check(_lib.load().locov_weight_transpose_scale(_ptr(w), N, K, _ptr(row_scale), _ptr(out), _stream(w)),
              "locov_weight_transpose_scale")
    return out


def conv3x3_weight_flip(w: torch.Tensor, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w [N,Cin,3,3] -> [Cin,N,3,3] with out[c,n,a,b] = row_scale[n] * w[n,c,2-a,2-b]: the filter of the data gradient."""
    w = _dev(w, "w")
    N, Cin = w.shape[:2]
    row_scale = _dev(row_scale, "row_scale") if row_scale is not None else None
    out = torch.empty((Cin, N, 3, 3), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        check(_lib.load().locov_conv3x3_weight_flip(_ptr(w), N, Cin, _ptr(row_scale), _ptr(out), _stream(w)),
              "locov_conv3x3_weight_flip")
    return out


def im2col3x3(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """x [R*H*W, C] ROI-major pixel rows -> [R*H*W, 9*C] 3x3 / pad 1 patches (column = tap*C + c)."""
    x = _dev(x, "x")
    M, C = x.shape
    if M % (H * W) or C % 4:
        raise ValueError("im2col3x3: inconsistent shapes")
    col = torch.empty((M, 9 * C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_im2col3x3_nhwc(_ptr(x), M // (H * W), H, W, C, _ptr(col), _stream(x)), "locov_im2col3x3_nhwc")
    return col


def conv3x3_wgrad_unpack(dw_packed: torch.Tensor, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, 9*Cin] (column = tap*Cin + c) -> [N,Cin,3,3], rows scaled."""
    dw_packed = _dev(dw_packed, "dw_packed")
    N, K9 = dw_packed.shape
    Cin = K9 // 9
    row_scale = _dev(row_scale, "row_scale") if row_scale is not None else None
    dw = torch.empty((N, Cin, 3, 3), dtype=torch.float32, device=dw_packed.device)
    with torch.cuda.device(dw.device):
        check(_lib.load().locov_conv3x3_wgrad_unpack(_ptr(dw_packed), N, Cin, _ptr(row_scale), _ptr(dw), _stream(dw)),
              "locov_conv3x3_wgrad_unpack")
    return dw


def relu_mask(g: torch.Tensor, act: torch.Tensor, amax_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g where act > 0, else 0.  amax_out: scale_slot() that receives max |result|."""
    g, act = _dev(g, "g"), _dev(act, "act")
    if g.shape != act.shape or g.numel() % 4:
        raise ValueError("relu_mask: shapes must match, numel % 4 == 0")
    out = _out(out, tuple(g.shape), g, "relu_mask")
    with torch.cuda.device(g.device):
        check(_lib.load().locov_relu_mask(_ptr(g), _ptr(act), g.numel(), _ptr(out), _ptr(amax_out), _stream(g)), "locov_relu_mask")
    return out


LABEL_MAX_IMAGES, LABEL_MAX_THRESHOLDS = _lib.LABEL_MAX_IMAGES, _lib.LABEL_MAX_THRESHOLDS
AMAX_BOUND_MAX = _lib.AMAX_BOUND_MAX


def label_proposals(boxes: torch.Tensor, n_props, gt_boxes: torch.Tensor, gt_classes: torch.Tensor, n_gt, thresholds, labels_of,
                    num_classes: int, rnd: torch.Tensor):
    """Labelling of a whole batch in one launch (locov_label_proposals; roi_emb_heads.py:25-118's device half).
    boxes [sum R, 4] / gt_boxes [sum M, 4] fp32 and gt_classes [sum M] int64, concatenated over the images; n_props / n_gt: per-image
    counts (host ints); thresholds: the Matcher's [-inf, t1, ..., inf]; labels_of: its interval labels; rnd [2, sum R] float64 in [0, 1).
    Returns (gt_index, labels, key_pos, key_neg, rows [B, 4] int64) -- see include/locov_hip.h."""
    boxes = _dev(boxes, "boxes")
    B, total = len(n_props), int(sum(n_props))
    if B > _lib.LABEL_MAX_IMAGES or len(labels_of) > _lib.LABEL_MAX_THRESHOLDS or boxes.shape[0] != total:
        raise ValueError("label_proposals: too many images / matcher intervals, or counts that do not add up")
    dev = boxes.device
    gt_boxes = _dev(gt_boxes, "gt_boxes") if sum(n_gt) else None
    gt_classes = _dev(gt_classes, "gt_classes", torch.int64) if sum(n_gt) else None
    rnd = _dev(rnd, "rnd", torch.float64)
    gt_index = torch.empty(total, dtype=torch.int64, device=dev)
    labels = torch.empty(total, dtype=torch.int64, device=dev)
    keys = torch.empty((2, total), dtype=torch.float64, device=dev)
    rows = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    roff = (ctypes.c_int * (B + 1))(*([0] + list(itertools.accumulate(int(n) for n in n_props))))
    goff = (ctypes.c_int * (B + 1))(*([0] + list(itertools.accumulate(int(n) for n in n_gt))))
    nt = len(labels_of)
    lo = (ctypes.c_float * max(nt, 1))(*[float(v) for v in thresholds[:-1]])
    hi = (ctypes.c_float * max(nt, 1))(*[float(v) for v in thresholds[1:]])
    lab = (ctypes.c_int * max(nt, 1))(*[int(v) for v in labels_of])
    with torch.cuda.device(dev):
        check(_lib.load().locov_label_proposals(_ptr(boxes), roff, _ptr(gt_boxes), _ptr(gt_classes), goff, B, lo, hi, lab, nt,
                                                int(num_classes), _ptr(rnd), _ptr(gt_index), _ptr(labels), _ptr(keys[0]), _ptr(keys[1]),
                                                _ptr(rows), _stream(boxes)), "locov_label_proposals")
    return gt_index, labels, keys[0], keys[1], rows


SAMPLE_MAX_PROPOSALS = _lib.SAMPLE_MAX_PROPOSALS


def sample_proposals(key_pos: torch.Tensor, key_neg: torch.Tensor, labels: torch.Tensor, gt_index: torch.Tensor, rows: torch.Tensor,
                     boxes: torch.Tensor, gt_boxes: Optional[torch.Tensor], n_props, n_gt, budget: int, max_pos: int, num_classes: int,
                     field: Optional[torch.Tensor] = None):
    """The sampler behind label_proposals for a batch whose every image fills its budget, every field of the sampled Instances
    from one launch and no host read (locov_sample_proposals; roi_emb_heads.py:79-106).  Inputs: label_proposals' outputs and inputs
    of the same batch; field: one more fp32 per-proposal field (objectness_logits).  Returns (picked, boxes [B*budget, 4], classes,
    matched gt boxes [B*budget, 4], fg flags, rois [B*budget, 5], field[picked] | None), image-major."""
    boxes = _dev(boxes, "boxes")
    B, total = len(n_props), int(sum(n_props))
    if B > _lib.LABEL_MAX_IMAGES or boxes.shape[0] != total or not n_props or max(n_props) > SAMPLE_MAX_PROPOSALS or min(n_props) < 1:
        raise ValueError("sample_proposals: 1..64 images of 1..4096 proposals each, counts that add up")
    dev = boxes.device
    key_pos, key_neg = _dev(key_pos, "key_pos", torch.float64), _dev(key_neg, "key_neg", torch.float64)
    labels, gt_index, rows = _dev(labels, "labels", torch.int64), _dev(gt_index, "gt_index", torch.int64), _dev(rows, "rows", torch.int64)
    gt_boxes = _dev(gt_boxes, "gt_boxes") if sum(n_gt) else None
    field = _dev(field, "field") if field is not None else None
    n = B * int(budget)
    picked = torch.empty(n, dtype=torch.int64, device=dev)
    out_boxes = torch.empty((n, 4), dtype=torch.float32, device=dev)
    classes = torch.empty(n, dtype=torch.int64, device=dev)
    out_gt = torch.empty((n, 4), dtype=torch.float32, device=dev)
    fg = torch.empty(n, dtype=torch.int64, device=dev)
    rois = torch.empty((n, 5), dtype=torch.float32, device=dev)
    field_out = torch.empty(n, dtype=torch.float32, device=dev) if field is not None else None
    roff = (ctypes.c_int * (B + 1))(*([0] + list(itertools.accumulate(int(v) for v in n_props))))
    goff = (ctypes.c_int * (B + 1))(*([0] + list(itertools.accumulate(int(v) for v in n_gt))))
    with torch.cuda.device(dev):
        check(_lib.load().locov_sample_proposals(_ptr(key_pos), _ptr(key_neg), _ptr(labels), _ptr(gt_index), _ptr(rows), _ptr(boxes),
                                                 _ptr(gt_boxes), _ptr(field), roff, goff, B, int(budget), int(max_pos), int(num_classes),
                                                 _ptr(picked), _ptr(out_boxes), _ptr(classes), _ptr(out_gt), _ptr(fg), _ptr(rois),
                                                 _ptr(field_out), _stream(boxes)), "locov_sample_proposals")
    return picked, out_boxes, classes, out_gt, fg, rois, field_out


RPN_LOSS_FLAG_DEGENERATE = _lib.RPN_LOSS_FLAG_DEGENERATE


def _check_rpn_train_limits(fn: str, N: int, HWA: int) -> None:
    if N > RPN_MAX_IMAGES or HWA > RPN_MAX_ANCHORS:
        raise ValueError(f"{fn}: outside the kernels' limits (at most {RPN_MAX_IMAGES} images, fewer than 2^22 anchors per image)")


def rpn_label_anchors(anchors: torch.Tensor, gt_boxes: Optional[torch.Tensor], n_gt, image_shapes, thresholds, labels_of,
                      allow_low_quality: bool = True, boundary_thresh: float = -1.0):
    """The RPN's anchor labelling of a batch on the device (locov_rpn_label_anchors, csrc/rpn_train.hip): pairwise_iou, the Matcher
    with its low-quality rule, the boundary test -- two launches, no [num_gt, HWA] matrix, no host read.
    anchors [HWA, 4] fp32 (shared by the images); gt_boxes [sum M, 4] fp32 concatenated over the images (None when there are none);
    n_gt: per-image counts (host ints); image_shapes: (height, width) per image; thresholds: the Matcher's [-inf, t1, ..., inf];
    labels_of: its interval labels.
    Returns (labels [N, HWA] int8 before the draw, matched boxes [N, HWA, 4], counts [N, 4] int32 = (#1, #0, 0, 0))."""
    anchors = _dev(anchors, "anchors")
    N, HWA, total = len(n_gt), anchors.shape[0], int(sum(n_gt))
    if anchors.dim() != 2 or anchors.shape[1] != 4 or len(image_shapes) != N:
        raise ValueError("rpn_label_anchors: anchors [HWA, 4], one (height, width) per image")
    _check_rpn_train_limits("rpn_label_anchors", N, HWA)
    if len(labels_of) > LABEL_MAX_THRESHOLDS or len(thresholds) != len(labels_of) + 1:
        raise ValueError("rpn_label_anchors: too many matcher intervals, or thresholds / labels that do not pair up")
    gt_boxes = _dev(gt_boxes, "gt_boxes") if total else None
    if total and tuple(gt_boxes.shape) != (total, 4):
        raise ValueError("rpn_label_anchors: gt_boxes must be [sum(n_gt), 4]")
    dev = anchors.device
    labels = torch.empty((N, HWA), dtype=torch.int8, device=dev)
    matched = torch.empty((N, HWA, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    if N == 0 or HWA == 0:
        return labels, matched, counts
    lib = _lib.load()
    goff = (ctypes.c_int * (N + 1))(*([0] + list(itertools.accumulate(int(n) for n in n_gt))))
    hw = (ctypes.c_float * (2 * N))(*[float(v) for shape in image_shapes for v in shape[:2]])
    nt = len(labels_of)
    lo = (ctypes.c_float * max(nt, 1))(*[float(v) for v in thresholds[:-1]])
    hi = (ctypes.c_float * max(nt, 1))(*[float(v) for v in thresholds[1:]])
    lab = (ctypes.c_int * max(nt, 1))(*[int(v) for v in labels_of])
    nbytes = int(lib.locov_rpn_label_anchors_workspace_bytes(N, HWA, total))
    if nbytes < 0:
        check(nbytes, "locov_rpn_label_anchors_workspace_bytes")
    ws = _workspace("rpn_label", anchors, nbytes)
    with torch.cuda.device(dev):
        check(lib.locov_rpn_label_anchors(_ptr(anchors), HWA, _ptr(gt_boxes), goff, hw, N, lo, hi, lab, nt, int(bool(allow_low_quality)),
                                          float(boundary_thresh), _ptr(ws), ws.numel(), _ptr(labels), _ptr(matched), _ptr(counts),
                                          _stream(anchors)), "locov_rpn_label_anchors")
    return labels, matched, counts


def rpn_sample_anchors(labels: torch.Tensor, counts: torch.Tensor, rnd: torch.Tensor, budget: int, max_pos: int) -> torch.Tensor:
    """subsample_labels behind rpn_label_anchors, on the device (locov_rpn_sample_anchors): per image the min(#1, max_pos) positives
    of smallest rnd[0] stay 1, the min(#0, budget - num_pos) negatives of smallest rnd[1] stay 0 (equal keys in anchor order),
    everything else becomes -1 -- one launch, no host read.  labels [N, HWA] int8 and counts [N, 4] int32 from rpn_label_anchors;
    rnd [2, N, HWA] float64 uniforms in [0, 1).  Returns the final labels [N, HWA] int8; counts[:, 2:] receive (num_pos, num_neg)."""
    labels, counts, rnd = _dev(labels, "labels", torch.int8), _dev(counts, "counts", torch.int32), _dev(rnd, "rnd", torch.float64)
    if labels.dim() != 2 or tuple(counts.shape) != (labels.shape[0], 4) or tuple(rnd.shape) != (2, *labels.shape):
        raise ValueError("rpn_sample_anchors: labels [N, HWA] int8, counts [N, 4] int32, rnd [2, N, HWA] float64")
    N, HWA = labels.shape
    _check_rpn_train_limits("rpn_sample_anchors", N, HWA)
    if not 0 <= int(max_pos) <= int(budget):
        raise ValueError("rpn_sample_anchors: 0 <= max_pos <= budget")
    out = torch.empty_like(labels)
    with torch.cuda.device(labels.device):
        check(_lib.load().locov_rpn_sample_anchors(_ptr(labels), _ptr(rnd), HWA, N, int(budget), int(max_pos), _ptr(counts), _ptr(out),
                                                   _stream(labels)), "locov_rpn_sample_anchors")
    return out


class _RpnLossFn(torch.autograd.Function):
    """locov_rpn_loss: both losses and both gradients from ONE pass; backward scales the saved gradients by the incoming [2]."""

    @staticmethod
    def forward(ctx, logits, deltas, labels, anchors, matched, weights, beta, cls_scale, loc_scale):
        logits, deltas = _dev(logits, "logits"), _dev(deltas, "deltas")
        labels, anchors, matched = _dev(labels, "labels", torch.int8), _dev(anchors, "anchors"), _dev(matched, "matched_boxes")
        N, HWA = logits.shape
        dev = logits.device
        loss = torch.zeros(2, dtype=torch.float32, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        dlogits, ddeltas = torch.empty_like(logits), torch.empty_like(deltas)
        lib = _lib.load()
        nbytes = int(lib.locov_rpn_loss_workspace_bytes(N, HWA))
        if nbytes < 0:
            check(nbytes, "locov_rpn_loss_workspace_bytes")
        ws = _workspace("rpn_loss", logits, nbytes)
        with torch.cuda.device(dev):
            check(lib.locov_rpn_loss(_ptr(logits), _ptr(deltas), _ptr(labels), _ptr(anchors), _ptr(matched), HWA, N,
                                     *(float(w) for w in weights), float(beta), float(cls_scale), float(loc_scale), _ptr(ws), ws.numel(),
                                     _ptr(loss), _ptr(dlogits), _ptr(ddeltas), _ptr(flags), _stream(logits)), "locov_rpn_loss")
        ctx.grads = (dlogits, ddeltas)
        ctx.mark_non_differentiable(flags)
        return loss, flags

    @staticmethod
    def backward(ctx, g, _):
        dlogits, ddeltas = ctx.grads
        return (dlogits * g[0] if ctx.needs_input_grad[0] else None, ddeltas * g[1] if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None, None)


def rpn_loss(logits: torch.Tensor, deltas: torch.Tensor, labels: torch.Tensor, anchors: torch.Tensor, matched_boxes: torch.Tensor,
             weights, smooth_l1_beta: float, cls_scale: float, loc_scale: float):
    """[D2-upstream] RPN.losses in one pass (locov_rpn_loss): loss[0] = cls_scale * sum over labels >= 0 of the objectness
    cross-entropy, loss[1] = loc_scale * sum over labels == 1 of smooth-L1(deltas - get_deltas(anchor, matched box)) -- the caller
    folds the normaliser and the loss weights into the two scales.  logits [N, HWA], deltas [N, HWA, 4], labels [N, HWA] int8 (after
    the draw), anchors [HWA, 4], matched_boxes [N, HWA, 4].  Differentiable in logits and deltas; reproducible bit for bit.
    Returns (loss [2], flags [1] int32: RPN_LOSS_FLAG_DEGENERATE when a positive anchor has no positive width and height)."""
    if logits.dim() != 2 or tuple(deltas.shape) != (*logits.shape, 4) or tuple(labels.shape) != tuple(logits.shape) \
            or tuple(anchors.shape) != (logits.shape[1], 4) or tuple(matched_boxes.shape) != tuple(deltas.shape):
        raise ValueError("rpn_loss: logits [N, HWA], deltas [N, HWA, 4], labels [N, HWA], anchors [HWA, 4], matched_boxes [N, HWA, 4]")
    _check_rpn_train_limits("rpn_loss", *logits.shape)
    return _RpnLossFn.apply(logits.float(), deltas.float(), labels, anchors, matched_boxes, tuple(weights), smooth_l1_beta, cls_scale, loc_scale)


def zero_if_raised(tensors, word: torch.Tensor) -> None:
    """Zero-fill every tensor of `tensors` (contiguous fp32 device tensors, None entries skipped) ON THE DEVICE when the
    range-guard word `word` is set; a no-op launch otherwise.  No host read (locov_zero_if_raised)."""
    ts = [t for t in tensors if t is not None and t.numel() > 0]
    if not ts:
        return
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise LocovError("zero_if_raised: contiguous fp32 device tensors only")
    lib = _lib.load()
    with torch.cuda.device(word.device):
        for i in range(0, len(ts), _lib.ZERO_LIST_MAX):
            chunk = ts[i:i + _lib.ZERO_LIST_MAX]
            ptrs = (ctypes.c_void_p * len(chunk))(*[t.data_ptr() for t in chunk])
            counts = (ctypes.c_int64 * len(chunk))(*[t.numel() for t in chunk])
            check(lib.locov_zero_if_raised(ptrs, counts, len(chunk), _ptr(word), _stream(word)), "locov_zero_if_raised")


def spatial_mean_bwd(g: torch.Tensor, act: Optional[torch.Tensor], hw: int, amax_out: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g [R,C] -> [R*hw, C] ROI-major rows: g[r]/hw broadcast over the positions, zeroed where act <= 0."""
    g = _dev(g, "g")
    R, C = g.shape
    act = _dev(act, "act") if act is not None else None
    if act is not None and tuple(act.shape) != (R * hw, C):
        raise ValueError("spatial_mean_bwd: act must be [R*hw, C]")
    out = _out(out, (R * hw, C), g, "spatial_mean_bwd")
    with torch.cuda.device(g.device):
        check(_lib.load().locov_spatial_mean_bwd(_ptr(g), _ptr(act), R, C, hw, _ptr(out), _ptr(amax_out), _stream(g)), "locov_spatial_mean_bwd")
    return out


def rows_stride2(src: torch.Tensor, N: int, H: int, W: int, forward: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """forward: channels-last map [N,H,W,C] -> rows of its even pixels [N*OH*OW, C]; else the adjoint (rows -> zero-filled map)."""
    src = _dev(src, "src")
    C = src.shape[-1]
    OH, OW = (H + 1) // 2, (W + 1) // 2
    out = _out(out, (N * OH * OW, C) if forward else (N, H, W, C), src, "rows_stride2")
    with torch.cuda.device(src.device):
        check(_lib.load().locov_rows_stride2(_ptr(src), N, H, W, C, int(forward), _ptr(out), _stream(src)), "locov_rows_stride2")
    return out


def roi_align_nhwc_bwd(grad_rows: torch.Tensor, feat_shape, rois: torch.Tensor, output_size: int, spatial_scale: float,
                       sampling_ratio: int = 0, aligned: bool = True, bin_stride: int = 1, pos_major: bool = False,
                       accumulate_into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adjoint of roi_align_nhwc: grad_rows [o*o*R, C] -> gradient of the channels-last map [N,H,W,C].
    accumulate_into: an existing [N,H,W,C] gradient the result is ADDED to (fp32 atomics, as into the zero-filled fresh one)."""
    grad_rows = _rows(grad_rows, "grad_rows")
    rois = _dev(rois, "rois")
    N, H, W, C = feat_shape
    if accumulate_into is None:
        gf = torch.zeros((N, H, W, C), dtype=torch.float32, device=grad_rows.device)
    else:
        gf = _out(accumulate_into, (N, H, W, C), grad_rows, "roi_align_nhwc_bwd")
    with torch.cuda.device(gf.device):
        check(_lib.load().locov_roi_align_nhwc_bwd(_ptr(grad_rows), grad_rows.stride(0) if grad_rows.shape[0] else C, N, H, W, C,
                                                   _ptr(rois), rois.shape[0], output_size, output_size, float(spatial_scale),
                                                   int(sampling_ratio), int(aligned), int(bin_stride), int(pos_major), _ptr(gf),
                                                   _stream(gf)), "locov_roi_align_nhwc_bwd")
    return gf


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    """[N,H,W,C] -> [N,C,H,W] (the transpose kernel of nchw_to_nhwc with the roles of HW and C swapped)."""
    x = _dev(x, "x")
    N, H, W, C = x.shape
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_nchw_to_nhwc(_ptr(x), N, H * W, C, 1, _ptr(out), F32, _stream(x)), "locov_nchw_to_nhwc")
    return out


def resnet_stem_shape(H: int, W: int) -> Tuple[int, int]:
    """(PH, PW) of the stem's pooled map for an H x W image: conv 7x7 / 2 / pad 3, then max-pool 3x3 / 2 / pad 1."""
    CH, CW = (H + 1) // 2, (W + 1) // 2
    return (CH + 1) // 2, (CW + 1) // 2


def resnet_stem(images: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[D2-upstream] BasicStem in one launch (csrc/resnet_stem.hip): max_pool(relu(conv7x7/2(images) * scale + shift)).
    images [N,3,H,W] NCHW, weight [64,3,7,7], scale / shift [64] (the FrozenBN fold) -> channels-last [N,PH,PW,64]."""
    images, weight = _dev(images, "images"), _dev(weight, "weight")
    scale, shift = _dev(scale, "scale"), _dev(shift, "shift")
    if images.dim() != 4 or images.shape[1] != 3 or min(images.shape[2:]) < 1:
        raise ValueError(f"resnet_stem: images must be [N,3,H,W], got {tuple(images.shape)}")
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, 3, 7, 7) or tuple(scale.shape) != (Cout,) or tuple(shift.shape) != (Cout,):
        raise ValueError(f"resnet_stem: weight must be [Cout,3,7,7] and scale, shift [Cout], got {tuple(weight.shape)}, "
                         f"{tuple(scale.shape)}, {tuple(shift.shape)}")
    N, _, H, W = images.shape
    PH, PW = resnet_stem_shape(H, W)
    y = _out(out, (N, PH, PW, Cout), images, "resnet_stem")
    with torch.cuda.device(images.device):
        check(_lib.load().locov_resnet_stem_fwd(_ptr(images), N, H, W, _ptr(weight), _ptr(scale), _ptr(shift), Cout, _ptr(y),
                                                _stream(images)), "locov_resnet_stem_fwd")
    return y


def resnet_stem_train(images: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                      out: Optional[torch.Tensor] = None, sel_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """resnet_stem for a training step: (y, sel) with y bit-identical to resnet_stem's and sel uint8 [N,PH,PW,64], per pooled
    element 3 di + dj of the conv position (2p - 1 + di, 2q - 1 + dj) that first attains the window maximum (torch's max-pool
    rule), 9 where y is 0 -- what resnet_stem_wgrad routes the gradient by."""
    images, weight = _dev(images, "images"), _dev(weight, "weight")
    scale, shift = _dev(scale, "scale"), _dev(shift, "shift")
    if images.dim() != 4 or images.shape[1] != 3 or min(images.shape[2:]) < 1:
        raise ValueError(f"resnet_stem_train: images must be [N,3,H,W], got {tuple(images.shape)}")
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, 3, 7, 7) or tuple(scale.shape) != (Cout,) or tuple(shift.shape) != (Cout,):
        raise ValueError(f"resnet_stem_train: weight must be [Cout,3,7,7] and scale, shift [Cout], got {tuple(weight.shape)}, "
                         f"{tuple(scale.shape)}, {tuple(shift.shape)}")
    N, _, H, W = images.shape
    PH, PW = resnet_stem_shape(H, W)
    y = _out(out, (N, PH, PW, Cout), images, "resnet_stem_train")
    if sel_out is None:
        sel = torch.empty((N, PH, PW, Cout), dtype=torch.uint8, device=images.device)
    else:
        sel = sel_out
        if tuple(sel.shape) != (N, PH, PW, Cout) or sel.dtype != torch.uint8 or sel.device != images.device or not sel.is_contiguous():
            raise ValueError(f"resnet_stem_train: sel_out must be a contiguous uint8 {(N, PH, PW, Cout)} tensor on {images.device}")
    with torch.cuda.device(images.device):
        check(_lib.load().locov_resnet_stem_fwd_sel(_ptr(images), N, H, W, _ptr(weight), _ptr(scale), _ptr(shift), Cout, _ptr(y),
                                                    _ptr(sel), _stream(images)), "locov_resnet_stem_fwd_sel")
    return y, sel


def resnet_stem_wgrad(images: torch.Tensor, g: torch.Tensor, sel: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The stem's weight gradient (csrc/resnet_stem.hip): dw [64,3,7,7] = scale[o] * sum gconv * x over the conv positions, gconv
    the gradient g [N,PH,PW,64] of the pooled map routed by resnet_stem_train's sel.  Fixed-order reduction: no atomics, two
    calls give the same bits."""
    images, g, scale = _dev(images, "images"), _dev(g, "g"), _dev(scale, "scale")
    sel = _dev(sel, "sel", dtype=torch.uint8)
    if images.dim() != 4 or images.shape[1] != 3 or min(images.shape[2:]) < 1:
        raise ValueError(f"resnet_stem_wgrad: images must be [N,3,H,W], got {tuple(images.shape)}")
    N, _, H, W = images.shape
    PH, PW = resnet_stem_shape(H, W)
    Cout = scale.shape[0]
    if tuple(g.shape) != (N, PH, PW, Cout) or tuple(sel.shape) != (N, PH, PW, Cout) or scale.dim() != 1:
        raise ValueError(f"resnet_stem_wgrad: g and sel must be [{N},{PH},{PW},Cout] and scale [Cout], got {tuple(g.shape)}, "
                         f"{tuple(sel.shape)}, {tuple(scale.shape)}")
    lib = _lib.load()
    dw = torch.empty((Cout, 3, 7, 7), dtype=torch.float32, device=images.device)
    if N == 0:
        return dw.zero_()
    nbytes = int(lib.locov_resnet_stem_wgrad_workspace_bytes(N, H, W))
    ws = _workspace("stem_wgrad", images, nbytes)
    with torch.cuda.device(images.device):
        check(lib.locov_resnet_stem_wgrad(_ptr(images), N, H, W, _ptr(g), _ptr(sel), _ptr(scale), Cout, _ptr(dw), _ptr(ws), ws.numel(),
                                          _stream(images)), "locov_resnet_stem_wgrad")
    return dw


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b on the f32 MFMA NT-GEMM kernel; backward: grad_x = g W as an NT GEMM against the transposed
    weight (one small weight-sized transpose), grad_W = g^T x on the TN kernel (no activation-sized transposes),
    grad_b = sum g."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        gx = gw = gb = None
        N, K = weight.shape
        if ctx.needs_input_grad[0]:
            gx = linear(g, weight_transpose_scale(weight.detach()))           # [M,N] . ([K,N])^T
        if ctx.needs_input_grad[1]:
            if N % 4 == 0 and K % 4 == 0:
                gw = gemm_tn(g, x)                                            # g^T x, contraction over the rows
            else:                                                             # odd sizes (e.g. an 81-way cls_score): transposed copies
                gw = linear(g.t().contiguous(), x.t().contiguous())
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum(dim=0)
        return gx, gw, gb


def linear_autograd(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable x W^T + b (both operands may require grad)."""
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        return _LinearFn.apply(x, weight, bias)
    return linear(x.detach(), weight.detach(), bias.detach() if bias is not None else None)


GROUNDING_ALIGNMENTS = {"softmax": _lib.GROUNDING_ALIGN_SOFTMAX, "hardmax": _lib.GROUNDING_ALIGN_HARDMAX}


class _GroundingAlignFn(torch.autograd.Function):
    """The alignment launch with its rule chosen and either direction optional (locov_grounding_align_fwd / _bwd): returns the costs
    of the directions that are on."""

    @staticmethod
    def forward(ctx, S, cmask, rmask, B, T, NR, temperature, alignment, words, regions):
        ctx.set_materialize_grads(False)
        S = _dev(S, "S")
        cmask, rmask = _dev(cmask, "caption_mask"), _dev(rmask, "region_mask")
        w2r = torch.empty((B, B), dtype=torch.float32, device=S.device) if words else None
        r2w = torch.empty((B, B), dtype=torch.float32, device=S.device) if regions else None
        with torch.cuda.device(S.device):
            check(_lib.load().locov_grounding_align_fwd(_ptr(S), B, T, NR, _ptr(cmask), _ptr(rmask), float(temperature), alignment,
                                                        _ptr(w2r), _ptr(r2w), _stream(S)), "locov_grounding_align_fwd")
        ctx.save_for_backward(S, cmask, rmask)
        ctx.dims = (B, T, NR, temperature, alignment, words, regions)
        return tuple(c for c in (w2r, r2w) if c is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, *g):
        S, cmask, rmask = ctx.saved_tensors
        B, T, NR, temperature, alignment, words, regions = ctx.dims
        g = list(g)
        g_w2r = g.pop(0) if words else None
        g_r2w = g.pop(0) if regions else None
        if g_w2r is None and g_r2w is None:                       # no cost was used: nothing flows
            return (torch.zeros_like(S),) + (None,) * 9
        g_w2r = _dev(g_w2r, "grad_w2r") if g_w2r is not None else None
        g_r2w = _dev(g_r2w, "grad_r2w") if g_r2w is not None else None
        dS = torch.empty_like(S)
        with torch.cuda.device(S.device):
            check(_lib.load().locov_grounding_align_bwd(_ptr(S), B, T, NR, _ptr(cmask), _ptr(rmask), float(temperature), alignment,
                                                        _ptr(g_w2r), _ptr(g_r2w), _ptr(dS), _stream(S)),
                  "locov_grounding_align_bwd")
        return (dS,) + (None,) * 9


def grounding_costs(S: torch.Tensor, caption_mask: torch.Tensor, region_mask: torch.Tensor, temperature: float,
                    alignment: str = "softmax", words: bool = True,
                    regions: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """S [B*T, B*NR] (caption tokens x region embeddings), masks [B,T] / [B,NR] fp32 ->
    (cost_w2r, cost_r2w) [B,B] with rows = captions, columns = images.  Differentiable in S.
    alignment "softmax" | "hardmax" (grounding_head.py:161-174); words / regions False turns that direction off (its cost is
    None and nothing of it is computed)."""
    B, T = caption_mask.shape
    NR = region_mask.shape[1]
    if tuple(S.shape) != (B * T, B * NR):
        raise ValueError(f"S must be [{B * T},{B * NR}], got {tuple(S.shape)}")
    if alignment not in GROUNDING_ALIGNMENTS:
        raise ValueError(f"grounding_costs: unknown alignment {alignment!r} (softmax | hardmax)")
    if not (words or regions):
        raise ValueError("grounding_costs: both alignment directions are off")
    res = list(_GroundingAlignFn.apply(S, caption_mask.to(torch.float32), region_mask.to(torch.float32), B, T, NR, float(temperature),
                                       GROUNDING_ALIGNMENTS[alignment], bool(words), bool(regions)))
    return (res.pop(0) if words else None), (res.pop(0) if regions else None)


GROUNDING_CE_MAX_B = 64        # LOCOV_GROUNDING_CE_MAX_B
TRIPLET_MINING = {"hardest": _lib.TRIPLET_HARDEST, "easiest": _lib.TRIPLET_EASIEST, "given": _lib.TRIPLET_GIVEN}


class _GroundingTailFn(torch.autograd.Function):
    """The tail of GroundingHead.forward on the [B, B] costs, one launch each way: loss "cross_entropy" without the filled costs
    (locov_grounding_ce_fwd / _bwd) or with them (locov_grounding_ce_dist_), or "triplet" (locov_grounding_triplet_; mining, margin
    and neg_idx are its alone).  Returns the 8 scalars, then with_dist the filled cost of every direction that is on."""

    @staticmethod
    def _head(ctx, c0, c1, cmask, rmask, neg_idx):
        """(the costs' reference tensor, the arguments every entry point of ctx.entry starts with)"""
        ref = c0 if c0 is not None else c1
        head = (_ptr(c0), _ptr(c1), _ptr(cmask), _ptr(rmask), ref.shape[0], cmask.shape[1], rmask.shape[1])
        return ref, head + ((*ctx.triplet, _ptr(neg_idx)) if ctx.triplet else ())

    @staticmethod
    def forward(ctx, cost_w2r, cost_r2w, cmask, rmask, loss, mining, margin, neg_idx, with_dist):
        ctx.set_materialize_grads(False)                  # unused outputs send NULL, not zero-filled upstream gradients
        c0 = _dev(cost_w2r, "cost_w2r") if cost_w2r is not None else None
        c1 = _dev(cost_r2w, "cost_r2w") if cost_r2w is not None else None
        cmask, rmask = _dev(cmask, "caption_mask"), _dev(rmask, "region_mask")
        ctx.triplet = (mining, margin) if loss == "triplet" else None
        ctx.entry = "locov_grounding_triplet" if ctx.triplet else "locov_grounding_ce_dist" if with_dist else "locov_grounding_ce"
        ctx.pw_args = ctx.entry != "locov_grounding_ce"   # (the plain cross-entropy pair has no pw / gpw arguments)
        ref, head = _GroundingTailFn._head(ctx, c0, c1, cmask, rmask, neg_idx)
        # locov_grounding_ce_fwd's caller zero-fills an absent alignment's four outputs; the other entry points' kernels do
        out = (torch.empty if ctx.pw_args or (c0 is not None and c1 is not None) else torch.zeros)(8, dtype=torch.float32, device=ref.device)
        pw0 = torch.empty_like(c0) if with_dist and c0 is not None else None
        pw1 = torch.empty_like(c1) if with_dist and c1 is not None else None
        with torch.cuda.device(ref.device):
            check(getattr(_lib.load(), ctx.entry + "_fwd")(*head, _ptr(out), *((_ptr(pw0), _ptr(pw1)) if ctx.pw_args else ()), _stream(ref)),
                  ctx.entry + "_fwd")
        ctx.save_for_backward(*(t for t in (c0, c1, neg_idx) if t is not None), cmask, rmask)
        ctx.have = (c0 is not None, c1 is not None, neg_idx is not None)
        ctx.with_dist = with_dist
        vals = out.unbind(0)
        ctx.mark_non_differentiable(vals[2], vals[3], vals[6], vals[7])
        return vals + tuple(p for p in (pw0, pw1) if p is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, *g):
        saved = list(ctx.saved_tensors)
        c0, c1, neg_idx = (saved.pop(0) if on else None for on in ctx.have)
        cmask, rmask = saved
        ref, head = _GroundingTailFn._head(ctx, c0, c1, cmask, rmask, neg_idx)
        ups = [(_dev(g[i].reshape(1), "grad") if g[i] is not None else None) for i in (0, 1, 4, 5)]
        gpw = list(g[8:])
        g0 = gpw.pop(0) if ctx.with_dist and ctx.have[0] else None
        g1 = gpw.pop(0) if ctx.with_dist and ctx.have[1] else None
        g0 = _dev(g0, "grad_pw_w2r") if g0 is not None else None
        g1 = _dev(g1, "grad_pw_r2w") if g1 is not None else None
        d0 = torch.empty_like(c0) if c0 is not None else None
        d1 = torch.empty_like(c1) if c1 is not None else None
        with torch.cuda.device(ref.device):
            check(getattr(_lib.load(), ctx.entry + "_bwd")(*head, *(_ptr(u) for u in ups), *((_ptr(g0), _ptr(g1)) if ctx.pw_args else ()),
                                                          _ptr(d0), _ptr(d1), _stream(ref)), ctx.entry + "_bwd")
        return (d0, d1) + (None,) * 7


def _grounding_tail(cost_w2r, cost_r2w, caption_mask, region_mask, loss, mining=0, margin=0.0, neg_idx=None, with_dist=False):
    """What grounding_ce, grounding_ce_dist and grounding_triplet share: (the 8 scalars, pw_w2r, pw_r2w), the two None without
    with_dist or for an absent alignment."""
    res = _GroundingTailFn.apply(cost_w2r, cost_r2w, caption_mask.to(torch.float32), region_mask.to(torch.float32), loss, mining, margin,
                                 neg_idx, with_dist)
    pw = list(res[8:])
    pw0 = pw.pop(0) if with_dist and cost_w2r is not None else None
    pw1 = pw.pop(0) if with_dist and cost_r2w is not None else None
    return tuple(res[:8]), pw0, pw1


def _tail_costs(fn: str, cost_w2r: Optional[torch.Tensor], cost_r2w: Optional[torch.Tensor]) -> torch.Tensor:
    """The cost that is there, after the check the three tail functions share."""
    ref = cost_w2r if cost_w2r is not None else cost_r2w
    if ref is None or ref.dim() != 2 or ref.shape[0] != ref.shape[1] or ref.shape[0] > GROUNDING_CE_MAX_B:
        raise ValueError(f"{fn}: costs must be [B, B] with B <= {GROUNDING_CE_MAX_B}")
    return ref


def grounding_ce(cost_w2r: Optional[torch.Tensor], cost_r2w: Optional[torch.Tensor], caption_mask: torch.Tensor,
                 region_mask: torch.Tensor) -> Tuple[torch.Tensor, ...]:
    """The cross-entropy tail of GroundingHead.forward (grounding_head.py:239-290,357-377) on the [B, B] costs of grounding_costs, one
    launch (and one in backward): returns 8 scalars -- for w2r, then r2w: CE choose caption, CE choose image, batch accuracy choose
    caption, batch accuracy choose image (zeros for a cost that is None).  Differentiable in the costs."""
    _tail_costs("grounding_ce", cost_w2r, cost_r2w)
    return _grounding_tail(cost_w2r, cost_r2w, caption_mask, region_mask, "cross_entropy")[0]


def grounding_ce_dist(cost_w2r: Optional[torch.Tensor], cost_r2w: Optional[torch.Tensor], caption_mask: torch.Tensor,
                      region_mask: torch.Tensor) -> Tuple[Tuple[torch.Tensor, ...], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """grounding_ce for a GroundingHead that also returns its distributions (MMSS_HEAD.DISTILLATION_LOSS): one launch each way
    (locov_grounding_ce_dist_fwd / _bwd).  Returns (the 8 scalars of grounding_ce, pw_w2r, pw_r2w): the filled [B, B] costs
    (grounding_head.py:239-251, None for an absent alignment), differentiable in the costs on the pairs that are not filled."""
    _tail_costs("grounding_ce_dist", cost_w2r, cost_r2w)
    return _grounding_tail(cost_w2r, cost_r2w, caption_mask, region_mask, "cross_entropy", with_dist=True)


def grounding_triplet(cost_w2r: Optional[torch.Tensor], cost_r2w: Optional[torch.Tensor], caption_mask: torch.Tensor,
                      region_mask: torch.Tensor, mining: str, margin: float, neg_idx: Optional[torch.Tensor] = None,
                      with_dist: bool = False):
    """The triplet tail of GroundingHead.forward (grounding_head.py:239-251,279-343,357-377) on the [B, B] costs of grounding_costs,
    one launch each way (locov_grounding_triplet_fwd / _bwd).  mining "hardest" | "easiest" | "given"; "given" takes neg_idx, int64
    [2 (w2r, r2w), 2 (choose caption, choose image), B] with values in [0, B - 1): indices into the matrix without its diagonal, as
    NEGATIVE_MINING "random" draws them (the values stay on the device and are not inspected here).  Returns the 8 scalars in
    grounding_ce's layout (the hinge means in the CE slots); with_dist: (the 8 scalars, pw_w2r, pw_r2w) as grounding_ce_dist."""
    ref = _tail_costs("grounding_triplet", cost_w2r, cost_r2w)
    if mining not in TRIPLET_MINING:
        raise ValueError(f"grounding_triplet: unknown mining {mining!r} (hardest | easiest | given)")
    B = ref.shape[0]
    if mining == "given":
        if neg_idx is None or neg_idx.dtype != torch.int64 or tuple(neg_idx.shape) != (2, 2, B) or neg_idx.device != ref.device:
            raise ValueError(f"grounding_triplet: given negatives need neg_idx int64 [2, 2, {B}] on the costs' device")
        neg_idx = neg_idx.contiguous()
    else:
        neg_idx = None
    res = _grounding_tail(cost_w2r, cost_r2w, caption_mask, region_mask, "triplet", TRIPLET_MINING[mining], float(margin), neg_idx,
                          bool(with_dist))
    return res if with_dist else res[0]



DISTILL_MAX_B = _lib.DISTILL_MAX_B   # LOCOV_DISTILL_MAX_B
DISTILL_KINDS = {"kd": _lib.DISTILL_KD, "js": _lib.DISTILL_JS, "mse": _lib.DISTILL_MSE}


class _DistillLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, trans, w2r, r2w, kind, transformer_teacher, temperature, loss_weight):
        trans, w2r, r2w = _dev(trans, "trans_pw_cost"), _dev(w2r, "pw_cost_w2r"), _dev(r2w, "pw_cost_r2w")
        loss = torch.empty((), dtype=torch.float32, device=trans.device)
        with torch.cuda.device(trans.device):
            check(_lib.load().locov_distill_loss_fwd(_ptr(trans), _ptr(w2r), _ptr(r2w), trans.shape[0], kind, int(transformer_teacher),
                                                     temperature, loss_weight, _ptr(loss), _stream(trans)), "locov_distill_loss_fwd")
        ctx.save_for_backward(trans, w2r, r2w)
        ctx.args = (kind, int(transformer_teacher), temperature, loss_weight)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        trans, w2r, r2w = ctx.saved_tensors
        d = [torch.empty_like(x) if ctx.needs_input_grad[i] else None for i, x in enumerate((trans, w2r, r2w))]
        if any(x is not None for x in d):
            gl = _dev(grad_loss.reshape(1), "grad_loss")
            with torch.cuda.device(trans.device):
                check(_lib.load().locov_distill_loss_bwd(_ptr(trans), _ptr(w2r), _ptr(r2w), trans.shape[0], *ctx.args, _ptr(gl),
                                                         *(_ptr(x) for x in d), _stream(trans)), "locov_distill_loss_bwd")
        return d[0], d[1], d[2], None, None, None, None


def distill_loss(kind: str, trans_pw_cost: torch.Tensor, pw_cost_w2r: torch.Tensor, pw_cost_r2w: torch.Tensor, temperature: float,
                 loss_weight: float = 1.0, transformer_teacher: bool = True) -> torch.Tensor:
    """MultiDistillLoss ("kd") / MultiDistillLossJS ("js") / MultiDistillLossL2 ("mse") of distill_mmss_gcnn.py:211-433 on three
    [B, B] fp32 device cost matrices (B <= DISTILL_MAX_B): one launch forward (locov_distill_loss_fwd) and one backward
    (locov_distill_loss_bwd).  A detached input -- the caller's DETACH_TEACHER -- gets no gradient.  Returns the 0-dim loss."""
    if kind not in DISTILL_KINDS:
        raise ValueError(f"distill_loss: unknown kind {kind!r} (one of {sorted(DISTILL_KINDS)})")
    B = trans_pw_cost.shape[0] if trans_pw_cost.dim() == 2 else -1
    if not 1 <= B <= DISTILL_MAX_B or any(tuple(x.shape) != (B, B) for x in (trans_pw_cost, pw_cost_w2r, pw_cost_r2w)):
        raise ValueError(f"distill_loss: the three costs must be [B, B] with 1 <= B <= {DISTILL_MAX_B}")
    if not temperature > 0:
        raise ValueError("distill_loss: temperature must be > 0")
    return _DistillLossFn.apply(trans_pw_cost, pw_cost_w2r, pw_cost_r2w, DISTILL_KINDS[kind], bool(transformer_teacher),
                                float(temperature), float(loss_weight))

class _BoxRegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, proposal_boxes, gt_boxes, gt_classes, num_classes, weights, beta):
        pred = _dev(pred, "pred_deltas")
        pb, gb = _dev(proposal_boxes.detach().float(), "proposal_boxes"), _dev(gt_boxes.detach().float(), "gt_boxes")
        cls = _dev(gt_classes, "gt_classes", torch.int64)
        R, ld = pred.shape
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        need = ctx.needs_input_grad[0]
        dpred = None
        if need:
            dpred = torch.empty_like(pred) if ld == 4 else torch.zeros_like(pred)
        with torch.cuda.device(pred.device):
            check(_lib.load().locov_box_reg_loss(_ptr(pb), _ptr(gb), _ptr(pred), ld, _ptr(cls), R, int(num_classes),
                                                 *(float(w) for w in weights), float(beta), _ptr(loss), _ptr(dpred), _stream(pred)),
                  "locov_box_reg_loss")
        ctx.dpred = dpred
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        return (ctx.dpred * g if ctx.dpred is not None else None), None, None, None, None, None, None


def box_reg_loss(pred_deltas: torch.Tensor, proposal_boxes: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor,
                 num_classes: int, weights, smooth_l1_beta: float) -> torch.Tensor:
    """[D2-upstream] FastRCNNOutputLayers.box_reg_loss ("smooth_l1") in one launch: get_deltas of the foreground rows
    (0 <= gt_classes < num_classes), smooth-L1 against pred_deltas [R, 4] or [R, 4 * num_classes], sum / max(R, 1).  The foreground
    boxes must already be known to have positive width and height.  Differentiable in pred_deltas."""
    R = pred_deltas.shape[0]
    if pred_deltas.dim() != 2 or pred_deltas.shape[1] not in (4, 4 * num_classes) or tuple(proposal_boxes.shape) != (R, 4) \
            or tuple(gt_boxes.shape) != (R, 4) or tuple(gt_classes.shape) != (R,) or gt_classes.dtype != torch.int64:
        raise ValueError("box_reg_loss: pred_deltas [R, 4 | 4K], boxes [R, 4], gt_classes [R] int64")
    return _BoxRegLossFn.apply(pred_deltas.float(), proposal_boxes, gt_boxes, gt_classes, num_classes, tuple(weights), smooth_l1_beta)


BOX_IOU_KINDS = {"giou": _lib.BOX_IOU_GIOU, "diou": _lib.BOX_IOU_DIOU, "ciou": _lib.BOX_IOU_CIOU}


class _BoxIouLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, proposal_boxes, gt_boxes, gt_classes, num_classes, weights, scale_clamp, kind):
        pred = _dev(pred, "pred_deltas")
        pb, gb = _dev(proposal_boxes.detach().float(), "proposal_boxes"), _dev(gt_boxes.detach().float(), "gt_boxes")
        cls = _dev(gt_classes, "gt_classes", torch.int64)
        R, ld = pred.shape
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        need = ctx.needs_input_grad[0]
        dpred = None
        if need:
            dpred = torch.empty_like(pred) if ld == 4 else torch.zeros_like(pred)
        with torch.cuda.device(pred.device):
            check(_lib.load().locov_box_iou_loss(_ptr(pb), _ptr(gb), _ptr(pred), ld, _ptr(cls), R, int(num_classes),
                                                 *(float(w) for w in weights), float(scale_clamp), kind, _ptr(loss), _ptr(dpred),
                                                 _stream(pred)),
                  "locov_box_iou_loss")
        ctx.dpred = dpred
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        return (ctx.dpred * g if ctx.dpred is not None else None), None, None, None, None, None, None, None


def box_iou_loss(pred_deltas: torch.Tensor, proposal_boxes: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor,
                 num_classes: int, weights, scale_clamp: float, kind: str) -> torch.Tensor:
    """[D2-upstream] FastRCNNOutputLayers.box_reg_loss ("giou" / "diou" / "ciou") in one launch: apply_deltas (weights, scale_clamp) of
    the foreground rows' (0 <= gt_classes < num_classes) predictions pred_deltas [R, 4] or [R, 4 * num_classes] onto their proposals,
    [fvcore, unverified] giou_loss / diou_loss / ciou_loss against gt_boxes, sum / max(R, 1).  The foreground boxes must already be
    known to have positive width and height.  Differentiable in pred_deltas."""
    if kind not in BOX_IOU_KINDS:
        raise ValueError(f"box_iou_loss: unknown kind {kind!r} (one of {sorted(BOX_IOU_KINDS)})")
    R = pred_deltas.shape[0]
    if pred_deltas.dim() != 2 or pred_deltas.shape[1] not in (4, 4 * num_classes) or tuple(proposal_boxes.shape) != (R, 4) \
            or tuple(gt_boxes.shape) != (R, 4) or tuple(gt_classes.shape) != (R,) or gt_classes.dtype != torch.int64:
        raise ValueError("box_iou_loss: pred_deltas [R, 4 | 4K], boxes [R, 4], gt_classes [R] int64")
    return _BoxIouLossFn.apply(pred_deltas.float(), proposal_boxes, gt_boxes, gt_classes, num_classes, tuple(weights), float(scale_clamp),
                               BOX_IOU_KINDS[kind])


CLS_STATS = ("num_instances", "num_fg", "num_accurate", "fg_num_accurate", "num_false_negative", "num_invalid")


class _ClsLossFn(torch.autograd.Function):
    """locov_<name> for name in ("cls_loss", "sigmoid_cls_loss"): before_rc and after_rc are the entry's own arguments, which sit between
    gt_classes and R and between C and the workspace."""

    @staticmethod
    def forward(ctx, scores, gt_classes, want_stats, name, before_rc, after_rc):
        R, C = scores.shape
        # a column block of a wider matrix is read in place (any row stride, any base alignment)
        if not (scores.stride(1) == 1 and scores.stride(0) >= C):
            scores = scores.contiguous()
        cls = gt_classes if gt_classes.is_contiguous() else gt_classes.contiguous()
        dev = scores.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(len(CLS_STATS), dtype=torch.int64, device=dev) if want_stats else None
        dscores = torch.empty((R, C), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        lib = _lib.load()
        ws = _workspace(name, scores, getattr(lib, f"locov_{name}_workspace_bytes")(R))
        with torch.cuda.device(dev):
            check(getattr(lib, f"locov_{name}")(scores.data_ptr(), scores.stride(0), cls.data_ptr(), *before_rc, R, C, *after_rc,
                                                ws.data_ptr(), ws.numel(), loss.data_ptr(), _ptr(dscores), _ptr(stats),
                                                _stream(scores)), f"locov_{name}")
        ctx.dscores = dscores
        ctx.set_materialize_grads(False)                     # (no zeros for the statistics' "gradient")
        if stats is None:
            return loss
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g, *_):
        return (ctx.dscores * g if ctx.dscores is not None and g is not None else None), None, None, None, None, None


def _check_cls_loss_args(fn: str, shapes: str, min_classes: int, scores, gt_classes, class_mask=None) -> None:
    """The argument checks of cls_loss and sigmoid_cls_loss (class_mask [C - 1] uint8: the latter's, where given)."""
    given = {"scores": scores, "gt_classes": gt_classes}
    if class_mask is not None:
        given["class_mask"] = class_mask
    if not all(isinstance(t, torch.Tensor) for t in given.values()):
        raise TypeError(f"{fn}: {', '.join(given)} must be torch.Tensors")
    if not scores.is_cuda or any(t.device != scores.device for t in given.values()):
        raise LocovError(f"{fn}: " + ", ".join(f"{n} on {t.device}" for n, t in given.items())
                         + ": the kernel only runs on a ROCm GPU (there is no CPU fallback)")
    dtypes = dict(zip(given, (torch.float32, torch.int64, torch.uint8)))
    if any(t.dtype != dtypes[n] for n, t in given.items()):
        raise TypeError(f"{fn}: " + ", ".join(f"{n} must be {dtypes[n]} (got {t.dtype})" for n, t in given.items()))
    if scores.dim() != 2 or scores.shape[0] < 1 or scores.shape[1] < min_classes or tuple(gt_classes.shape) != (scores.shape[0],) \
            or (class_mask is not None and tuple(class_mask.shape) != (scores.shape[1] - 1,)):
        raise ValueError(f"{fn}: {shapes}, got " + ", ".join(str(tuple(t.shape)) for t in given.values()))


def cls_loss(scores: torch.Tensor, gt_classes: torch.Tensor, ignore_index: int = -100,
             want_stats: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """[D2-upstream] FastRCNNOutputLayers.losses' cross_entropy(scores, gt_classes, reduction="mean") and the counts of
    _log_classification_stats from one pass over the logits (locov_cls_loss: a row kernel and a small finishing launch).
    scores [R, C] fp32 on the device (R > 0; rows may be a column block of a wider matrix), gt_classes [R] int64.  Returns
    (loss, stats): the 0-dim loss, differentiable in scores -- the gradient is made by the same pass, backward only multiplies it by
    the incoming gradient -- and the int64 [6] device tensor of CLS_STATS (None without want_stats).  Nothing is read to the host."""
    _check_cls_loss_args("cls_loss", "scores [R, C] with R, C >= 1 and gt_classes [R]", 1, scores, gt_classes)
    if not torch.is_grad_enabled():
        scores = scores.detach()                             # (no gradient buffer under no_grad)
    res = _ClsLossFn.apply(scores, gt_classes, bool(want_stats), "cls_loss", (), (int(ignore_index),))
    return res if want_stats else (res, None)


FED_LOSS_MAX_CLASSES = _lib.FED_LOSS_MAX_CLASSES


def fed_loss_classes(gt_classes: torch.Tensor, weights: torch.Tensor, num_fed: int,
                     rnd: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """[D2-upstream, unverified] FastRCNNOutputLayers.get_fed_loss_classes on the device (locov_fed_loss_classes: one launch, no host
    read): the classes present among gt_classes [R] int64 plus, up to num_fed in all, classes sampled without replacement by
    weights [K] fp32 -- the top keys weights / rnd with rnd [K] strictly positive Exp(1) draws.  Without rnd they are drawn here from
    the device's default generator (one launch, no wait, reproducible under torch.manual_seed).  Returns (mask [K] uint8,
    counts [2] int32 = {labels present, classes sampled}), both on the device."""
    if not isinstance(gt_classes, torch.Tensor) or not isinstance(weights, torch.Tensor) or not isinstance(rnd, (torch.Tensor, type(None))):
        raise TypeError("fed_loss_classes: gt_classes, weights and rnd must be torch.Tensors")
    if not weights.is_cuda or gt_classes.device != weights.device or (rnd is not None and rnd.device != weights.device):
        raise LocovError(f"fed_loss_classes: weights are on {weights.device}, gt_classes on {gt_classes.device}"
                         + (f", rnd on {rnd.device}" if rnd is not None else "") + ": the kernel only runs on a ROCm GPU "
                         "(there is no CPU fallback)")
    if weights.dtype != torch.float32 or gt_classes.dtype != torch.int64 or (rnd is not None and rnd.dtype != torch.float32):
        raise TypeError(f"fed_loss_classes: weights (and rnd) must be torch.float32 and gt_classes torch.int64, got {weights.dtype} and "
                        f"{gt_classes.dtype}")
    K = weights.shape[0] if weights.dim() == 1 else -1
    if not 1 <= K <= FED_LOSS_MAX_CLASSES or gt_classes.dim() != 1 or (rnd is not None and tuple(rnd.shape) != (K,)):
        raise ValueError(f"fed_loss_classes: weights [K] with 1 <= K <= {FED_LOSS_MAX_CLASSES}, rnd [K] and gt_classes [R], got "
                         f"{tuple(weights.shape)}, {None if rnd is None else tuple(rnd.shape)} and {tuple(gt_classes.shape)}")
    if int(num_fed) < 0:
        raise ValueError(f"fed_loss_classes: num_fed must be >= 0, got {num_fed}")
    dev = weights.device
    if rnd is None:
        rnd = torch.empty(K, dtype=torch.float32, device=dev).exponential_()
    weights, rnd, cls = weights.detach().contiguous(), rnd.detach().contiguous(), gt_classes.contiguous()
    mask = torch.empty(K, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().locov_fed_loss_classes(_ptr(cls), cls.shape[0], _ptr(weights), _ptr(rnd), K, int(num_fed), _ptr(mask),
                                                 _ptr(counts), _stream(weights)), "locov_fed_loss_classes")
    return mask, counts


def sigmoid_cls_loss(scores: torch.Tensor, gt_classes: torch.Tensor, class_mask: Optional[torch.Tensor] = None,
                     want_stats: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """[D2-upstream, unverified] FastRCNNOutputLayers.sigmoid_cross_entropy_loss and the counts of _log_classification_stats from one
    pass over the logits (locov_sigmoid_cls_loss: a row kernel and a small finishing launch).  scores [R, K + 1] fp32 on the device
    (R > 0; rows may be a column block of a wider matrix), gt_classes [R] int64 in [0, K], class_mask [K] uint8 (fed_loss_classes'
    mask) or None for every class.  Returns (loss, stats): the 0-dim sum of the masked per-class binary cross-entropies over R,
    differentiable in scores -- the gradient is made by the same pass, backward only multiplies it by the incoming gradient -- and the
    int64 [6] device tensor of CLS_STATS (None without want_stats).  Nothing is read to the host."""
    _check_cls_loss_args("sigmoid_cls_loss", "scores [R, K + 1] with R, K >= 1, gt_classes [R] and class_mask [K]", 2, scores, gt_classes,
                         class_mask)
    if not torch.is_grad_enabled():
        scores = scores.detach()                             # (no gradient buffer under no_grad)
    mask = class_mask if class_mask is None or class_mask.is_contiguous() else class_mask.contiguous()
    res = _ClsLossFn.apply(scores, gt_classes, bool(want_stats), "sigmoid_cls_loss", (_ptr(mask),), ())
    return res if want_stats else (res, None)


def rownorm(x: torch.Tensor, mode: int, eps: float = 1e-12) -> torch.Tensor:
    x = _dev(x, "x")
    R, D = x.shape
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_rownorm_fwd(_ptr(x), R, D, int(mode), float(eps), _ptr(y), _stream(x)),
              "locov_rownorm_fwd")
    return y


class _RowNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode, eps):
        x = _dev(x.detach(), "x")
        ctx.save_for_backward(x)
        ctx.args = (mode, eps)
        return rownorm(x, mode, eps)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        mode, eps = ctx.args
        g = _dev(g, "grad")
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            check(_lib.load().locov_rownorm_bwd(_ptr(x), _ptr(g), x.shape[0], x.shape[1], int(mode), float(eps), _ptr(dx),
                                                _stream(x)), "locov_rownorm_bwd")
        return dx, None, None


def rownorm_autograd(x: torch.Tensor, mode: int, eps: float = 1e-12) -> torch.Tensor:
    """rownorm(), differentiable in x (forward and backward on the HIP kernels)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _RowNormFn.apply(x, int(mode), float(eps))
    return rownorm(x.detach(), mode, eps)


class _PoolFcFn(torch.autograd.Function):
    """(emb, deltas) = (x W_emb^T + b_emb, x W_box^T + b_box): the predictor's two FCs on one input (box_emb_head.py:196,206)
    with their backward in ONE C call (locov_pool_fc_bwd: grad_x accumulated across both layers in the GEMM epilogue, weight
    gradients as TN GEMMs, bias gradients as column sums)."""

    @staticmethod
    def forward(ctx, x, emb_w, emb_b, box_w, box_b):
        x = _rows(x.detach(), "x").contiguous()
        ctx.save_for_backward(x, emb_w.detach(), box_w.detach())
        ctx.set_materialize_grads(False)                     # an unused output (detached class predictor) sends None, not zeros
        ctx.has_bias = (emb_b is not None, box_b is not None)
        return linear(x, emb_w.detach(), None if emb_b is None else emb_b.detach()), \
            linear(x, box_w.detach(), None if box_b is None else box_b.detach())

    @staticmethod
    def backward(ctx, g_emb, g_box):
        x, emb_w, box_w = ctx.saved_tensors
        R, C5 = x.shape
        D = emb_w.shape[0]
        need = ctx.needs_input_grad
        if g_emb is None and g_box is None:
            return None, None, None, None, None
        g_emb = _dev(g_emb, "grad_emb") if g_emb is not None else None
        g_box = _dev(g_box, "grad_deltas") if g_box is not None else None
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        gx = new(R, C5) if need[0] else None
        gew = new(D, C5) if need[1] and g_emb is not None else None
        geb = new(D) if need[2] and ctx.has_bias[0] and g_emb is not None else None
        gbw = new(4, C5) if need[3] and g_box is not None else None
        gbb = new(4) if need[4] and ctx.has_bias[1] and g_box is not None else None
        lib = _lib.load()
        nbytes = lib.locov_pool_fc_bwd_workspace_bytes(R, C5, D)
        ws = _workspace("pool_fc_bwd", x, nbytes)
        with torch.cuda.device(x.device):
            check(lib.locov_pool_fc_bwd(_ptr(x), R, C5, _ptr(emb_w), D, _ptr(box_w), _ptr(g_emb), _ptr(g_box), _ptr(gx), _ptr(gew),
                                        _ptr(geb), _ptr(gbw), _ptr(gbb), _ptr(ws), ws.numel(), _stream(x)), "locov_pool_fc_bwd")
        return gx, gew, geb, gbw, gbb


def pool_fc_autograd(x, emb_w, emb_b, box_w, box_b):
    """Differentiable (emb_pred(x), bbox_pred(x)); x [R,C5], C5 and D multiples of 4, bbox_pred class-agnostic ([4,C5])."""
    if box_w.shape[0] != 4 or x.shape[1] % 4 or emb_w.shape[0] % 4:
        return linear_autograd(x, emb_w, emb_b), linear_autograd(x, box_w, box_b)
    return _PoolFcFn.apply(x, emb_w, emb_b, box_w, box_b)


class _SimGemmFn(torch.autograd.Function):
    """logits = emb . bank^T (+ bias) (box_emb_head.py:211) with locov_sim_gemm_bwd as its backward."""

    @staticmethod
    def forward(ctx, emb, bank, bias):
        emb = _rows(emb.detach(), "emb").contiguous()
        ctx.save_for_backward(emb, bank.detach())
        ctx.has_bias = bias is not None
        return linear(emb, bank.detach(), None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, g):
        emb, bank = ctx.saved_tensors
        g = _dev(g, "grad_logits")
        R, D = emb.shape
        K1 = bank.shape[0]
        need = ctx.needs_input_grad
        ge = torch.empty_like(emb) if need[0] else None
        gb = torch.empty_like(bank) if need[1] and K1 % 4 == 0 else None
        lib = _lib.load()
        ws = _workspace("sim_gemm_bwd", emb, lib.locov_sim_gemm_bwd_workspace_bytes(R, D, K1))
        with torch.cuda.device(emb.device):
            check(lib.locov_sim_gemm_bwd(_ptr(g), _ptr(emb), _ptr(bank), R, D, K1, _ptr(ge), _ptr(gb), _ptr(ws), ws.numel(),
                                         _stream(emb)), "locov_sim_gemm_bwd")
        if need[1] and gb is None:                           # a trainable bank whose row count is not a multiple of 4
            gb = linear(g.t().contiguous(), emb.t().contiguous())
        return ge, gb, (g.sum(dim=0) if ctx.has_bias and need[2] else None)


def sim_gemm_autograd(emb: torch.Tensor, bank: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable fp32 similarity GEMM emb [R,D] x bank [K1,D]^T."""
    if emb.shape[1] % 4 or not (torch.is_grad_enabled() and (emb.requires_grad or bank.requires_grad)):
        return linear_autograd(emb, bank, bias)
    return _SimGemmFn.apply(emb, bank, bias)


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16, round to nearest even (torch's conversion).  The kernel reads 16 bytes per lane: a contiguous view
    that does not start on a 16-byte boundary (x[1:]) is converted from an aligned copy."""
    x = _dev(x, "x")
    if x.data_ptr() % 16:
        x = x.clone()
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_f32_to_bf16(_ptr(x), x.numel(), _ptr(y), _stream(x)), "locov_f32_to_bf16")
    return y


def linear_bf16(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                scale: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                relu: bool = False) -> torch.Tensor:
    """y = epi(x . weight^T) with bf16 operands on the bf16 MFMA pipe, fp32 accumulate, fp32 epilogue and
    output (the opt-in reduced-precision form of the Res5 GEMMs).  x [M,K] bf16, weight [N,K] bf16."""
    x = _dev(x, "x", torch.bfloat16)
    weight = _dev(weight, "weight", torch.bfloat16)
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K or K % 8:
        raise ValueError(f"linear_bf16: x {tuple(x.shape)} weight {tuple(weight.shape)} (K must be a multiple of 8)")
    bias = _dev(bias, "bias") if bias is not None else None
    scale = _dev(scale, "scale") if scale is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_gemm_nt_bf16(_ptr(x), K, _ptr(weight), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), N,
                                             M, N, K, _lib.EPI_RELU if relu else 0, _stream(x)), "locov_gemm_nt_bf16")
    return y


def conv3x3_nhwc_bf16(x: torch.Tensor, w_packed: torch.Tensor, H: int, W: int, *, scale=None, shift=None,
                      residual=None, relu: bool = False, pos_major: bool = False) -> torch.Tensor:
    """conv3x3_nhwc with bf16 operands (x [R*H*W, Cin] bf16, w_packed [N, 9*Cin] bf16), fp32 output."""
    x = _dev(x, "x", torch.bfloat16)
    w_packed = _dev(w_packed, "w_packed", torch.bfloat16)
    M, Cin = x.shape
    N = w_packed.shape[0]
    if w_packed.shape[1] != 9 * Cin or M % (H * W) != 0:
        raise ValueError("conv3x3_nhwc_bf16: inconsistent shapes")
    scale = _dev(scale, "scale") if scale is not None else None
    shift = _dev(shift, "shift") if shift is not None else None
    residual = _dev(residual, "residual") if residual is not None else None
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.load().locov_conv3x3_nhwc_bf16(_ptr(x), M // (H * W), H, W, Cin, int(pos_major), _ptr(w_packed),
                                                  _ptr(scale), _ptr(shift), _ptr(residual), _ptr(y), N,
                                                  _lib.EPI_RELU if relu else 0, _stream(x)), "locov_conv3x3_nhwc_bf16")
    return y


def sim_gemm_bf16(emb: torch.Tensor, bank: torch.Tensor) -> torch.Tensor:
    """logits[R,K1] = emb[R,D] . bank[K1,D]^T, bf16 operands, fp32 accumulate / output."""
    emb = _dev(emb, "emb", torch.bfloat16)
    bank = _dev(bank, "bank", torch.bfloat16)
    R, D = emb.shape
    K1 = bank.shape[0]
    if bank.shape[1] != D:
        raise ValueError("emb / bank embedding dims differ")
    out = torch.empty((R, K1), dtype=torch.float32, device=emb.device)
    with torch.cuda.device(emb.device):
        check(_lib.load().locov_sim_gemm_bf16(_ptr(emb), _ptr(bank), R, D, K1, _ptr(out), K1, _stream(emb)),
              "locov_sim_gemm_bf16")
    return out


def box_head(x: torch.Tensor, emb_w: torch.Tensor, emb_b: torch.Tensor, bbox_w: torch.Tensor,
             bbox_b: torch.Tensor, bank: torch.Tensor, bank_bf16: Optional[torch.Tensor] = None,
             norm_mode: int = NORM_NONE, sim_dtype: int = F32, channels_last=False
             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Spatial mean + EmbeddingFastRCNNOutputLayers.forward in one C call.
    x: [R,C5] | [R,C5,h,w] | channels_last=1: [R,h,w,C5] | channels_last=2: position-major [h,w,R,C5].
    Returns (pooled [R,C5], deltas [R,4], emb [R,D], logits [R,K1])."""
    x = _dev(x, "x")
    R, C5, HW, channels_last = _layout_dims(x, channels_last)
    emb_w, emb_b = _dev(emb_w, "emb_w"), _dev(emb_b, "emb_b")
    bbox_w, bbox_b = _dev(bbox_w, "bbox_w"), _dev(bbox_b, "bbox_b")
    bank = _dev(bank, "bank")
    D, K1 = emb_w.shape[0], bank.shape[0]
    if emb_w.shape[1] != C5 or bbox_w.shape != (4, C5) or bank.shape[1] != D:
        raise ValueError("box_head: inconsistent weight shapes")
    dev = x.device
    # HW == 1: the mean is the identity and the C side skips the copy when pooled aliases x
    pooled = x.reshape(R, C5) if HW == 1 else torch.empty((R, C5), dtype=torch.float32, device=dev)
    deltas = torch.empty((R, 4), dtype=torch.float32, device=dev)
    emb = torch.empty((R, D), dtype=torch.float32, device=dev)
    logits = torch.empty((R, K1), dtype=torch.float32, device=dev)
    emb_bf16 = None
    if sim_dtype == BF16:
        if bank_bf16 is None:
            bank_bf16 = to_bf16(bank)
        bank_bf16 = _dev(bank_bf16, "bank_bf16", torch.bfloat16)
        emb_bf16 = torch.empty((R, D), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().locov_box_head_fwd(_ptr(x), R, C5, max(HW, 1), int(channels_last), _ptr(emb_w), _ptr(emb_b),
                                             _ptr(bbox_w), _ptr(bbox_b), _ptr(bank), _ptr(bank_bf16), D, K1,
                                             int(norm_mode), int(sim_dtype), _ptr(pooled), _ptr(deltas), _ptr(emb),
                                             _ptr(emb_bf16), _ptr(logits), _stream(x)), "locov_box_head_fwd")
    return pooled, deltas, emb, logits


def token_attention(sim: torch.Tensor, tok_off: torch.Tensor, num_tok: torch.Tensor, tmax: int, temperature: float,
                    gmin: torch.Tensor, cosine: bool = False, hardmax: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Multi-token class scores of the grounding predictor (box_emb_grounding_head.py:163-225).
    sim [R,Ttot] raw token similarities; tok_off / num_tok [K1] int32; gmin: 1-element device tensor.
    Returns (scores [R,K1], attention [R,K1,tmax])."""
    sim = _dev(sim, "sim")
    tok_off, num_tok = _dev(tok_off, "tok_off", torch.int32), _dev(num_tok, "num_tok", torch.int32)
    gmin = _dev(gmin.reshape(1), "gmin")
    R, Ttot = sim.shape
    K1 = num_tok.numel()
    scores = torch.empty((R, K1), dtype=torch.float32, device=sim.device)
    att = torch.empty((R, K1, tmax), dtype=torch.float32, device=sim.device)
    with torch.cuda.device(sim.device):
        check(_lib.load().locov_token_attention_fwd(_ptr(sim), R, Ttot, _ptr(tok_off), _ptr(num_tok), K1, int(tmax),
                                                    float(temperature), int(cosine), int(hardmax), _ptr(gmin),
                                                    _ptr(scores), _ptr(att), _stream(sim)), "locov_token_attention_fwd")
    return scores, att


class _TokenAttentionFn(torch.autograd.Function):
    """token_attention() with locov_token_attention_bwd as its backward: the attention is recomputed from sim and gmin."""

    @staticmethod
    def forward(ctx, sim, tok_off, num_tok, tmax, temperature, gmin, cosine, hardmax):
        sim = _dev(sim.detach(), "sim")
        gmin = _dev(gmin.detach().reshape(1), "gmin")
        ctx.save_for_backward(sim, tok_off, num_tok, gmin)
        ctx.set_materialize_grads(False)                     # an unused attention sends None -> a null pointer, not zeros
        ctx.args = (int(tmax), float(temperature), bool(cosine), bool(hardmax))
        return token_attention(sim, tok_off, num_tok, tmax, temperature, gmin, cosine=cosine, hardmax=hardmax)

    @staticmethod
    def backward(ctx, g_scores, g_att):
        sim, tok_off, num_tok, gmin = ctx.saved_tensors
        tmax, temperature, cosine, hardmax = ctx.args
        none = (None,) * 8
        if g_scores is None and g_att is None:
            return none
        R, Ttot = sim.shape
        K1 = num_tok.numel()
        g_scores = _dev(g_scores, "grad_scores") if g_scores is not None else sim.new_zeros((R, K1))
        g_att = _dev(g_att, "grad_att") if g_att is not None else None
        tok_off, num_tok = _dev(tok_off, "tok_off", torch.int32), _dev(num_tok, "num_tok", torch.int32)
        g_sim = torch.empty_like(sim)
        with torch.cuda.device(sim.device):
            check(_lib.load().locov_token_attention_bwd(_ptr(sim), R, Ttot, _ptr(tok_off), _ptr(num_tok), K1, tmax, temperature,
                                                        int(cosine), int(hardmax), _ptr(gmin), _ptr(g_scores), _ptr(g_att),
                                                        _ptr(g_sim), _stream(sim)), "locov_token_attention_bwd")
        return (g_sim,) + none[1:]


def token_attention_autograd(sim: torch.Tensor, tok_off: torch.Tensor, num_tok: torch.Tensor, tmax: int, temperature: float,
                             gmin: torch.Tensor, cosine: bool = False, hardmax: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """token_attention(), differentiable in sim: scores and attention are both differentiable outputs, gmin is a constant
    (the reference detaches it).  The classes' column ranges [tok_off[k], tok_off[k] + max(num_tok[k], 1)) must partition
    [0, Ttot) -- GroundingModule.set_class_embeddings builds them so."""
    if torch.is_grad_enabled() and sim.requires_grad:
        return _TokenAttentionFn.apply(sim, tok_off, num_tok, tmax, temperature, gmin, cosine, hardmax)
    return token_attention(sim.detach(), tok_off, num_tok, tmax, temperature, gmin.detach(), cosine=cosine, hardmax=hardmax)


# -------------------------------------------------------------------------------------- grounding branches' regions
REGIONS_MAX_B = _lib.REGIONS_MAX_B                        # LOCOV_REGIONS_MAX_B
REGIONS_MAX_CANDIDATES = _lib.REGIONS_MAX_CANDIDATES      # LOCOV_REGIONS_MAX_CANDIDATES


class RegionSelection(NamedTuple):
    """What locov_regions_select wrote (see include/locov_hip.h)."""
    indices: Optional[torch.Tensor]      # [B, n] int64: candidate of each slot within its image, -1 = padding
    src_row: Optional[torch.Tensor]      # [B, n] int32: the same as a row of the concatenated candidates
    inv: Optional[torch.Tensor]          # [sum count] int32: candidate -> output row, -1 = not selected
    mask: torch.Tensor                   # [B, mask_w] uint8
    loc: torch.Tensor                    # [B, n, 2] fp32
    mvm: torch.Tensor                    # [B, mvm_w] fp32 zeros


def regions_select(mode: str, keys: Optional[torch.Tensor], counts, ext_a, ext_b, n: int, limit: int, mask_w: int, mvm_w: int, *,
                   grid_w: int = 1, boxes: Optional[Sequence[torch.Tensor]] = None, device=None) -> RegionSelection:
    """distill_prop_mmss_gcnn.py:285-320 (mode "grid"; "grid_all" when :302 is not taken) / :349-391 (mode "boxes"): which candidate
    fills which slot, the mask, the loc rows and the zero mvm_mask, in one launch (locov_regions_select).  counts / ext_a / ext_b
    are host integers per image and travel as launch arguments; `keys` is one float64 per candidate on the device."""
    modes = {"grid": _lib.REGIONS_GRID, "grid_all": _lib.REGIONS_GRID_ALL, "boxes": _lib.REGIONS_BOXES}
    if mode not in modes:
        raise ValueError(f"regions_select: unknown mode {mode!r} (one of {sorted(modes)})")
    B = len(counts)
    if not 1 <= B <= REGIONS_MAX_B:
        raise ValueError(f"regions_select: 1 <= B <= {REGIONS_MAX_B}, got {B}")
    if len(ext_a) != B or len(ext_b) != B:
        raise ValueError("regions_select: counts, ext_a and ext_b must have one entry per image")
    total = int(sum(int(c) for c in counts))
    if mode != "grid_all":
        keys = _dev(keys, "keys", torch.float64)
        if keys.numel() != total:
            raise ValueError(f"regions_select: keys must hold one value per candidate ({total}), got {tuple(keys.shape)}")
        device = keys.device
    elif device is None:
        raise ValueError("regions_select: mode 'grid_all' needs the device")
    device = torch.device(device)
    ptrs = None
    if mode == "boxes":
        if boxes is None or len(boxes) != B:
            raise ValueError("regions_select: mode 'boxes' needs one [Ri, 4] box tensor per image")
        boxes = [_dev(b, "boxes") for b in boxes]
        for b, c in zip(boxes, counts):
            if tuple(b.shape) != (int(c), 4):
                raise ValueError(f"regions_select: boxes must be [{int(c)}, 4], got {tuple(b.shape)}")
        ptrs = (ctypes.c_void_p * B)(*[b.data_ptr() for b in boxes])
    ints = lambda v: (ctypes.c_int * B)(*[int(x) for x in v])
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
    sel = mode != "grid_all"
    out = RegionSelection(new((B, n), torch.int64) if sel else None, new((B, n), torch.int32) if sel else None,
                          new((total,), torch.int32) if sel else None, new((B, mask_w), torch.uint8), new((B, n, 2), torch.float32),
                          new((B, mvm_w), torch.float32))
    with torch.cuda.device(device):
        check(_lib.load().locov_regions_select(_ptr(keys) if sel else None, modes[mode], B, ints(counts), ints(ext_a), ints(ext_b), int(grid_w),
                                               ptrs, int(n), int(limit), int(mask_w), int(mvm_w), _ptr(out.indices), _ptr(out.src_row),
                                               _ptr(out.inv), _ptr(out.mask), _ptr(out.loc), _ptr(out.mvm), _stream(out.loc)),
              "locov_regions_select")
    return out


def _regions_layout(src: torch.Tensor):
    """How locov_regions_gather_* address `src`: ("rows", ld) for a [R, C] matrix (stride(1) == 1) or a logical [B, C, gh, gw] tensor
    in channels-last memory; ("nchw", hw) for a contiguous [B, C, gh, gw]; None otherwise."""
    if src.dim() == 2:
        return ("rows", src.stride(0)) if src.stride(1) == 1 and src.stride(0) >= src.shape[1] else None
    if src.dim() == 4:
        if src.is_contiguous():
            return ("nchw", src.shape[2] * src.shape[3])
        if src.permute(0, 2, 3, 1).is_contiguous():
            return ("rows", src.shape[1])
    return None


class _RegionsGatherFn(torch.autograd.Function):
    """out [B, n, C] = the source rows locov_regions_select chose, zeros in the padding slots (the fancy-index + pad_sequence of
    distill_prop_mmss_gcnn.py:311-316 / :361,:385); backward: the source-shaped gradient in the source's own memory layout, every
    element written once (the selected slot's gradient or zero)."""

    @staticmethod
    def forward(ctx, src, src_row, inv):
        if not (src.is_cuda and src.dtype == torch.float32 and _regions_layout(src) is not None):
            src = _dev(src, "features")                      # (raises off the device; else a contiguous copy)
        layout, arg = _regions_layout(src) or (("rows", src.shape[1]) if src.dim() == 2 else ("nchw", src.shape[2] * src.shape[3]))
        B, n = src_row.shape
        C = src.shape[1]
        out = torch.empty((B, n, C), dtype=torch.float32, device=src.device)
        nchw = layout == "nchw"
        with torch.cuda.device(src.device):
            check(_lib.load().locov_regions_gather_fwd(_ptr(src), _lib.REGIONS_NCHW if nchw else _lib.REGIONS_ROWS, 0 if nchw else arg, B, n, C,
                                                       arg if nchw else 0, _ptr(src_row), _ptr(out), _stream(src)), "locov_regions_gather_fwd")
        ctx.save_for_backward(inv)
        ctx.src = (tuple(src.shape), nchw)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (inv,) = ctx.saved_tensors
        shape, nchw = ctx.src
        g = _dev(g, "grad_region_features")
        C = shape[1]
        if len(shape) == 2:
            gs = out = torch.empty(shape, dtype=torch.float32, device=g.device)
        elif nchw:
            gs = out = torch.empty(shape, dtype=torch.float32, device=g.device)
        else:                                                  # channels-last memory, handed back as the same logical NCHW view
            gs = torch.empty((shape[0], shape[2], shape[3], C), dtype=torch.float32, device=g.device)
            out = gs.permute(0, 3, 1, 2)
        with torch.cuda.device(g.device):
            check(_lib.load().locov_regions_gather_bwd(_ptr(g), _lib.REGIONS_NCHW if nchw else _lib.REGIONS_ROWS, 0 if nchw else C, inv.numel(), C,
                                                       shape[2] * shape[3] if nchw else 0, _ptr(inv), _ptr(gs), _stream(g)),
                  "locov_regions_gather_bwd")
        return out, None, None


def regions_gather(src: torch.Tensor, selection: RegionSelection) -> torch.Tensor:
    """The selected rows of `src` -- [R, C] box features, or the logical [B, C, gh, gw] grid features in NCHW-contiguous or
    channels-last memory -- as [B, n, C], padding slots zero.  Differentiable in `src` (locov_regions_gather_fwd / _bwd)."""
    rows = src.shape[0] if src.dim() == 2 else src.shape[0] * src.shape[2] * src.shape[3] if src.dim() == 4 else -1
    if rows != selection.inv.numel():
        raise ValueError(f"regions_gather: the selection is over {selection.inv.numel()} candidates, the features hold {rows}")
    return _RegionsGatherFn.apply(src, selection.src_row, selection.inv)


# --------------------------------------------------------------------------------------
# fused multi-head self-attention core (csrc/mha.hip)
MHA_MAX_S = _lib.MHA_MAX_S            # LOCOV_MHA_MAX_S
MHA_HEAD_DIMS = _lib.MHA_HEAD_DIMS    # the head dims locov_mha_fwd / _bwd are built for


def _check_mha_args(fn: str, given: dict, key_bias, num_heads: int, keep, p_drop: float) -> None:
    """The argument checks of mha and mha_packed.  given: the row operands ({"q": .., "k": .., "v": ..} | {"qkv": ..})."""
    every = {**given, "key_bias": key_bias, **({"keep": keep} if keep is not None else {})}
    if not all(isinstance(t, torch.Tensor) for t in every.values()):
        raise TypeError(f"{fn}: {', '.join(every)} must be torch.Tensors")
    first = next(iter(given.values()))
    if not first.is_cuda or any(t.device != first.device for t in every.values()):
        raise LocovError(f"{fn}: " + ", ".join(f"{n} on {t.device}" for n, t in every.items())
                         + ": the kernel only runs on a ROCm GPU (there is no CPU fallback)")
    want = {n: (torch.uint8 if n == "keep" else torch.float32) for n in every}
    if any(t.dtype != want[n] for n, t in every.items()):
        raise TypeError(f"{fn}: " + ", ".join(f"{n} must be {want[n]} (got {t.dtype})" for n, t in every.items()))
    shapes = ", ".join(f"{n} {tuple(t.shape)}" for n, t in every.items())
    parts = 3 if "qkv" in given else 1
    H = int(num_heads)
    if any(t.dim() != 2 for t in given.values()) or len({tuple(t.shape) for t in given.values()}) != 1 or key_bias.dim() != 2 or H < 1:
        raise ValueError(f"{fn}: row operands [Nseq * S, {parts if parts > 1 else ''}{' * ' if parts > 1 else ''}H * d] and key_bias "
                         f"[Nseq, S] with num_heads >= 1, got {shapes}, num_heads {num_heads}")
    R, E = first.shape
    nseq, S = key_bias.shape
    if R != nseq * S or E % (parts * H) != 0:
        raise ValueError(f"{fn}: {R} rows of {E} columns do not match key_bias [Nseq, S] = {tuple(key_bias.shape)} and num_heads {H}: "
                         f"got {shapes}")
    d = E // (parts * H)
    if d not in MHA_HEAD_DIMS:
        raise ValueError(f"{fn}: head dim must be one of {MHA_HEAD_DIMS}, got {d} ({shapes}, num_heads {H})")
    if not 1 <= S <= MHA_MAX_S:
        raise ValueError(f"{fn}: sequence length S must be in [1, {MHA_MAX_S}], got {S}")
    if keep is not None and tuple(keep.shape) != (nseq, H, S, S):
        raise ValueError(f"{fn}: keep must be uint8 [Nseq, H, S, S] = {(nseq, H, S, S)}, got {tuple(keep.shape)}")
    if keep is not None and not 0.0 <= float(p_drop) < 1.0:
        raise ValueError(f"{fn}: p_drop must be in [0, 1), got {p_drop}")


class _MhaFn(torch.autograd.Function):
    """locov_mha_fwd / locov_mha_bwd.  packed: `a` is one [R, 3 H d] matrix whose column blocks are Q, K, V (b, c are None) and the
    backward returns ONE [R, 3 H d] gradient, written in place by the kernels."""

    @staticmethod
    def forward(ctx, a, b, c, key_bias, keep, H, scale, p_drop, packed):
        a = _rows(a, "qkv" if packed else "q")
        if packed:
            E = a.shape[1] // 3
            q, k, v = a[:, :E], a[:, E:2 * E], a[:, 2 * E:]
        else:
            q, k, v = a, _rows(b, "k"), _rows(c, "v")
            E = q.shape[1]
        bias = _dev(key_bias, "key_bias")
        keep = _dev(keep, "keep", torch.uint8) if keep is not None else None
        nseq, S = bias.shape
        d = E // H
        out = torch.empty((nseq * S, E), dtype=torch.float32, device=q.device)
        lse = torch.empty((nseq, H, S), dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            check(_lib.load().locov_mha_fwd(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(bias), _ptr(keep),
                                            float(p_drop), float(scale), nseq, S, H, d, _ptr(out), out.stride(0), _ptr(lse),
                                            _stream(q)), "locov_mha_fwd")
        ctx.save_for_backward(a if packed else q, k if not packed else None, v if not packed else None, bias, keep, lse)
        ctx.args = (H, float(scale), float(p_drop), packed, nseq, S, d, E)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, k, v, bias, keep, lse = ctx.saved_tensors
        H, scale, p_drop, packed, nseq, S, d, E = ctx.args
        g = g if g.is_contiguous() else g.contiguous()
        if packed:
            q, k, v = a[:, :E], a[:, E:2 * E], a[:, 2 * E:]
            grad = torch.empty_like(a, memory_format=torch.contiguous_format)
            dq, dk, dv = grad[:, :E], grad[:, E:2 * E], grad[:, 2 * E:]
        else:
            q = a
            dq, dk, dv = (torch.empty((nseq * S, E), dtype=torch.float32, device=q.device) for _ in range(3))
        delta = torch.empty_like(lse)
        with torch.cuda.device(q.device):
            check(_lib.load().locov_mha_bwd(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(bias), _ptr(keep),
                                            p_drop, scale, nseq, S, H, d, _ptr(g), g.stride(0), _ptr(lse), _ptr(delta),
                                            _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), _stream(q)),
                  "locov_mha_bwd")
        if packed:
            return grad, None, None, None, None, None, None, None, None
        return dq, dk, dv, None, None, None, None, None, None


def mha(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_bias: torch.Tensor, num_heads: int, *, scale: Optional[float] = None,
        keep: Optional[torch.Tensor] = None, p_drop: float = 0.0) -> torch.Tensor:
    """ctx = dropout(softmax(Q K^T * scale + key_bias[n, key])) V per (sequence, head), in one launch (locov_mha_fwd); differentiable
    in q, k, v (locov_mha_bwd: two launches, no atomics, bitwise reproducible).  q, k, v [Nseq * S, H * d] fp32 on the device --
    column blocks of a wider matrix are read in place (unit column stride, row pitch a multiple of 4, 16-byte aligned) -- key_bias
    [Nseq, S] fp32 (finite, no gradient), d in MHA_HEAD_DIMS, S <= MHA_MAX_S, scale defaults to 1 / sqrt(d).  keep: optional uint8
    [Nseq, H, S, S] dropout keep mask drawn by the caller; kept probabilities are multiplied by 1 / (1 - p_drop).  No S x S tensor is
    allocated and nothing is read to the host."""
    _check_mha_args("mha", {"q": q, "k": k, "v": v}, key_bias, num_heads, keep, p_drop)
    H = int(num_heads)
    scale = 1.0 / math.sqrt(q.shape[1] // H) if scale is None else float(scale)
    return _MhaFn.apply(q, k, v, key_bias, keep, H, scale, float(p_drop), False)


def mha_packed(qkv: torch.Tensor, key_bias: torch.Tensor, num_heads: int, *, scale: Optional[float] = None,
               keep: Optional[torch.Tensor] = None, p_drop: float = 0.0) -> torch.Tensor:
    """mha for Q, K, V that are the three column blocks of ONE [Nseq * S, 3 H d] matrix (one GEMM against the concatenated weight):
    the blocks are read in place and the backward writes one [Nseq * S, 3 H d] gradient in place, with no slicing or summing."""
    _check_mha_args("mha_packed", {"qkv": qkv}, key_bias, num_heads, keep, p_drop)
    H = int(num_heads)
    scale = 1.0 / math.sqrt(qkv.shape[1] // (3 * H)) if scale is None else float(scale)
    return _MhaFn.apply(qkv, None, None, key_bias, keep, H, scale, float(p_drop), True)


# --------------------------------------------------------------------------------------
# The two ends of the detector call (csrc/image_batch.hip; meta_arch.py: preprocess_image / _postprocess)
IMAGE_BATCH_MAX_IMAGES, IMAGE_BATCH_MAX_CHANNELS = _lib.LABEL_MAX_IMAGES, _lib.IMAGE_MAX_CHANNELS


def preprocess_images(images: Sequence[torch.Tensor], mean: Sequence[float], std: Sequence[float], size_divisibility: int = 0,
                      pad_value: float = 0.0, padding_constraints: Optional[dict] = None, out: Optional[torch.Tensor] = None):
    """(x - mean[c]) / std[c] of N [C, h_i, w_i] device images (all uint8 or all fp32) padded with pad_value into ONE fp32
    [N, C, Hb, Wb] batch, in one launch (locov_preprocess_images): the bits of the CPU torch expression followed by
    ImageList.from_tensors, whose batch-shape rule (largest sizes, square_size, rounded up to size_divisibility) this follows.
    Returns (tensor, image_sizes).  out: the caller's [N, C, Hb, Wb] tensor instead of a fresh one; every element of it is written.
    No H2D copy, no workspace, nothing read by the host."""
    from .structures import padded_batch_size
    images = list(images)
    if not images:
        raise ValueError("preprocess_images: no image")
    ims, C = _images(images, 0, dtype=None)
    dt = ims[0].dtype
    if dt not in (torch.uint8, torch.float32) or any(t.dtype != dt for t in ims):
        raise TypeError("preprocess_images: the images must all be uint8 or all be fp32")
    if C < 0:
        raise ValueError("preprocess_images: the images must be [C, H, W] with one channel count, on one device")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if not (1 <= C <= IMAGE_BATCH_MAX_CHANNELS) or len(mean) != C or len(std) != C or len(ims) > IMAGE_BATCH_MAX_IMAGES:
        raise ValueError(f"preprocess_images: outside the kernel's limits (1..{IMAGE_BATCH_MAX_CHANNELS} channels with one mean and "
                         f"std each, at most {IMAGE_BATCH_MAX_IMAGES} images)")
    image_sizes = [(int(t.shape[-2]), int(t.shape[-1])) for t in ims]
    Hb, Wb = padded_batch_size(image_sizes, size_divisibility, padding_constraints)
    n = len(ims)
    out = _out(out, (n, C, Hb, Wb), ims[0], "preprocess_images")
    hs, ws = _ints([s[0] for s in image_sizes]), _ints([s[1] for s in image_sizes])
    with torch.cuda.device(out.device):
        check(_lib.load().locov_preprocess_images(_ptrs(ims), hs, ws, n, _lib.IMAGE_U8 if dt == torch.uint8 else _lib.IMAGE_F32, C,
                                                  (ctypes.c_float * C)(*mean), (ctypes.c_float * C)(*std), float(pad_value),
                                                  _ptr(out), Hb, Wb, _stream(out)), "locov_preprocess_images")
    return out, image_sizes


def detector_rescale(boxes: torch.Tensor, sizes: Sequence[int], image_sizes, output_sizes):
    """detector_postprocess' box part for a batch in one launch (locov_detector_rescale) and ONE host read (the N counts).
    boxes [T, 4] fp32: the images' results concatenated, sizes[i] rows of image i predicted at image_sizes[i] = (h, w) and wanted
    at output_sizes[i] = (height, width).  Returns (out_boxes [T, 4], src int64 [T], counts): image i's kept boxes -- scaled by
    fp32(width / w), fp32(height / h) as `tensor *= python_float` scales, clipped, non-empty -- are the first counts[i] rows of its
    segment in their original order, src the row within the image each came from; the rest of the segment is 0 / -1."""
    boxes = _dev(boxes, "boxes")
    sizes = [int(s) for s in sizes]
    n = len(sizes)
    if boxes.dim() != 2 or boxes.shape[1] != 4 or sum(sizes) != boxes.shape[0] or min(sizes, default=0) < 0:
        raise ValueError("detector_rescale: boxes must be [sum(sizes), 4]")
    if not (len(image_sizes) == len(output_sizes) == n) or n > IMAGE_BATCH_MAX_IMAGES:
        raise ValueError(f"detector_rescale: one image size and one output size per image, at most {IMAGE_BATCH_MAX_IMAGES} images")
    T = boxes.shape[0]
    out = torch.empty((T, 4), dtype=torch.float32, device=boxes.device)
    src = torch.empty((T,), dtype=torch.int64, device=boxes.device)
    if n == 0:
        return out, src, []
    if boxes.data_ptr() % 16:
        boxes = boxes.clone()
    counts = torch.empty((n,), dtype=torch.int32, device=boxes.device)
    roff = (ctypes.c_int * (n + 1))(0, *itertools.accumulate(sizes))
    sx = (ctypes.c_float * n)(*[float(o[1]) / float(s[1]) for o, s in zip(output_sizes, image_sizes)])    # (double, then ONE rounding)
    sy = (ctypes.c_float * n)(*[float(o[0]) / float(s[0]) for o, s in zip(output_sizes, image_sizes)])
    oh, ow = (ctypes.c_int * n)(*[int(o[0]) for o in output_sizes]), (ctypes.c_int * n)(*[int(o[1]) for o in output_sizes])
    with torch.cuda.device(boxes.device):
        check(_lib.load().locov_detector_rescale(_ptr(boxes), roff, sx, sy, oh, ow, n, _ptr(out), _ptr(src), _ptr(counts), _stream(boxes)),
              "locov_detector_rescale")
    return out, src, counts.tolist()


# --------------------------------------------------------------------------------------
# The image side of the dataset mapper (csrc/image_resize.hip; data.py: DatasetMapper.map_batch)
RESIZE_MAX_TAPS = _lib.RESIZE_MAX_TAPS            # LOCOV_RESIZE_MAX_TAPS
FLIP_NONE, FLIP_HORIZONTAL, FLIP_VERTICAL = _lib.FLIP_NONE, _lib.FLIP_HORIZONTAL, _lib.FLIP_VERTICAL


def resize_supported(in_size, out_size, channels: int = 3) -> bool:
    """Whether locov_resize_flip_images takes an (h, w) -> (new_h, new_w) image of `channels` channels: every upscale, and a
    downscale of at most RESIZE_MAX_TAPS taps per axis (ceil(in / out) <= 8).  No launch; the library's own rule."""
    return bool(_lib.load().locov_resize_supported(int(in_size[0]), int(in_size[1]), int(out_size[0]), int(out_size[1]), int(channels)))


def resize_flip_images(images: Sequence[torch.Tensor], out_sizes, flips: Optional[Sequence[int]] = None,
                       out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """Pillow's 8-bit bilinear resize, a flip and the HWC -> CHW transposition of N uint8 [h_i, w_i, C] device images, each to its own
    out_sizes[i] = (new_h, new_w), in one launch (locov_resize_flip_images): the bytes of
    np.asarray(Image.fromarray(img).resize((new_w, new_h), Image.BILINEAR)), flipped (FLIP_NONE / FLIP_HORIZONTAL / FLIP_VERTICAL
    per image, default none), transposed.  Returns N uint8 [C, new_h, new_w] tensors; out: the caller's tensors instead of fresh ones,
    every byte of which is written.  Sizes outside resize_supported raise: the caller takes data.resize_bilinear_host for those."""
    images = list(images)
    n = len(images)
    if n == 0:
        return []
    ims, C = _images(images, 2)
    if C < 0:
        raise ValueError("resize_flip_images: the images must be [H, W, C] with one channel count, on one device")
    flips = [FLIP_NONE] * n if flips is None else [int(f) for f in flips]
    out_sizes = [(int(s[0]), int(s[1])) for s in out_sizes]
    if len(out_sizes) != n or len(flips) != n or n > IMAGE_BATCH_MAX_IMAGES or not (1 <= C <= IMAGE_BATCH_MAX_CHANNELS):
        raise ValueError(f"resize_flip_images: one size and one flip per image, at most {IMAGE_BATCH_MAX_IMAGES} images of "
                         f"1..{IMAGE_BATCH_MAX_CHANNELS} channels")
    for t, s in zip(ims, out_sizes):
        if min(t.shape[0], t.shape[1]) < 1 or min(s) < 1 or not resize_supported(t.shape[:2], s, C):
            raise ValueError(f"resize_flip_images: {tuple(t.shape[:2])} -> {s} is outside the kernel's limits (positive sizes, at most "
                             f"{RESIZE_MAX_TAPS} taps per axis)")
    shapes = [(C, s[0], s[1]) for s in out_sizes]
    outs = [torch.empty(s, dtype=torch.uint8, device=ims[0].device) for s in shapes] if out is None else _out_images(
        out, shapes, ims[0].device, "resize_flip_images: out must hold one contiguous uint8 [C, new_h, new_w] tensor per image, on the images' device")
    with torch.cuda.device(ims[0].device):
        check(_lib.load().locov_resize_flip_images(
            _ptrs(ims), _ints([t.shape[0] for t in ims]), _ints([t.shape[1] for t in ims]), _ptrs(outs), _ints([s[0] for s in out_sizes]),
            _ints([s[1] for s in out_sizes]), _ints(flips), n, C, _stream(ims[0])), "locov_resize_flip_images")
    return outs


# --------------------------------------------------------------------------------------
# The strong augmentation of the dataset mapper (csrc/image_augment.hip; strong_augment.py: apply_host is the definition)
AUG_MAX_ERASERS = _lib.AUG_MAX_ERASERS            # LOCOV_AUG_MAX_ERASERS


def augment_supported(sigma: float) -> bool:
    """Whether locov_augment_images takes a blur of this sigma: a box pass may reach two pixels, which holds for 0 < sigma up to
    about 2.449 and so for the reference's [0.1, 2.0].  No launch; the library's own rule."""
    sigma = float(sigma)
    return sigma == sigma and bool(_lib.load().locov_augment_supported(sigma))


def _augment_desc(desc, draws: dict, h: int, w: int, noise_offset: int) -> int:
    """Fills one locov_augment_desc from StrongAugmentation.draw's dict; returns the noise elements the image takes."""
    from . import strong_augment as sa
    chain = sa.jitter_chain(draws)
    if len(chain) > 4 or len(draws["erase"]) > AUG_MAX_ERASERS:
        raise ValueError(f"augment_images: at most 4 jitter operations and {AUG_MAX_ERASERS} erasers per image")
    desc.height, desc.width, desc.n_ops = h, w, len(chain)
    for k, (op, _) in enumerate(chain):
        desc.ops[k] = op
    desc.brightness, desc.contrast, desc.saturation = float(draws["brightness"]), float(draws["contrast"]), float(draws["saturation"])
    desc.hue_shift = sa.hue_shift(draws["hue"])
    desc.gray = int(bool(draws["gray"]))
    desc.sigma = float(draws["sigma"]) if draws["blur"] else 0.0
    if draws["blur"] and not augment_supported(draws["sigma"]):
        raise ValueError(f"augment_images: sigma {draws['sigma']} is outside augment_supported: the caller takes strong_augment.apply_host")
    rects = [e for e in draws["erase"] if e is not None]
    desc.n_erase, desc.noise_offset = len(rects), noise_offset
    for k, rect in enumerate(rects):
        for m in range(4):
            desc.erase[k][m] = int(rect[m])
    return sa.noise_count(draws)


def augment_images(images: Sequence[torch.Tensor], draws: Sequence[dict], noise: Optional[torch.Tensor] = None,
                   noise_offsets: Optional[Sequence[int]] = None, out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """The strong augmentation of N uint8 [3, h_i, w_i] device images (what resize_flip_images returns), image i by draws[i] =
    StrongAugmentation.draw's dict, in at most two launches (locov_augment_images) and no host read: the bytes of
    strong_augment.apply_host, i.e. of torchvision's ColorJitter / RandomGrayscale / RandomErasing over Pillow and Pillow's
    GaussianBlur.  noise: device fp32 [n], the erasers' normal draws; image i reads from noise_offsets[i] (default: the images'
    blocks one after the other).  Returns N fresh uint8 [3, h_i, w_i] tensors, or `out` (distinct from the inputs), every byte of
    which is written.  A sigma outside augment_supported raises: the caller takes apply_host for that image."""
    images, draws = list(images), list(draws)
    n = len(images)
    if n == 0:
        return []
    ims, C = _images(images, 0)
    if C != 3 or any(min(t.shape[1:]) < 1 for t in ims):
        raise ValueError("augment_images: the images must be non-empty [3, H, W], on one device")
    if len(draws) != n or n > IMAGE_BATCH_MAX_IMAGES or (noise_offsets is not None and len(noise_offsets) != n):
        raise ValueError(f"augment_images: one dict of draws (and one noise offset) per image, at most {IMAGE_BATCH_MAX_IMAGES} images")
    descs = (_lib.AugmentDesc * n)()
    at, end = 0, 0                                                 # end: one past the last noise element an eraser reads
    for i, (t, d) in enumerate(zip(ims, draws)):
        if noise_offsets is not None:
            at = int(noise_offsets[i])
        took = _augment_desc(descs[i], d, int(t.shape[1]), int(t.shape[2]), at)
        if took and at < 0:
            raise ValueError(f"augment_images: noise_offsets[{i}] is negative")
        end = max(end, at + took) if took else end
        at += took
    n_noise = 0
    if end:
        noise = _dev(noise, "noise", dtype=torch.float32) if noise is not None else None
        if noise is None or noise.dim() != 1 or noise.device != ims[0].device or end > noise.numel():
            raise ValueError(f"augment_images: noise must be a device fp32 [>= {end}] vector holding every eraser's block")
        n_noise = int(noise.numel())
    outs = [torch.empty_like(t) for t in ims] if out is None else _out_images(out, [t.shape for t in ims], ims[0].device, apart_from=ims, what=(
        "augment_images: out must hold one contiguous uint8 tensor of each image's shape, on its device, not the image itself"))
    lib = _lib.load()
    ws_bytes = int(lib.locov_augment_images_workspace_bytes(descs, n))
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=ims[0].device)
    with torch.cuda.device(ims[0].device):
        check(lib.locov_augment_images(_ptrs(ims), _ptrs(outs), descs, n, _ptr(noise) if n_noise else None, n_noise, _ptr(workspace), ws_bytes,
                                       _stream(ims[0])), "locov_augment_images")
    return outs


# --------------------------------------------------------------------------------------
# The proposal side of the dataset mapper (csrc/proposal_map.hip; data.py: transform_proposals + change_proposals_as_gt)
PROPOSAL_DTYPES = (torch.float32, torch.float64)  # the row dtypes locov_map_proposals takes; any other goes to data.py's host definition


class ProposalBuffers(NamedTuple):
    """locov_map_proposals' outputs over T = sum(n_rows) rows and N images; every element is written by a call."""
    prop_boxes: torch.Tensor     # fp32 [T, 4]
    prop_logits: torch.Tensor    # fp32 [T]
    prop_src: torch.Tensor       # int64 [T]
    gt_boxes: torch.Tensor       # fp32 [T, 4]
    gt_logits: torch.Tensor      # fp32 [T]
    gt_classes: torch.Tensor     # int64 [T]
    gt_src: torch.Tensor         # int64 [T]
    counts: torch.Tensor         # int32 [N, 2]


class MappedProposals(NamedTuple):
    """One image's lists, views of the ProposalBuffers cut at its counts."""
    prop_boxes: torch.Tensor
    prop_logits: torch.Tensor
    prop_src: torch.Tensor
    gt_boxes: torch.Tensor
    gt_logits: torch.Tensor
    gt_classes: torch.Tensor
    gt_src: torch.Tensor


def proposal_buffers(total_rows: int, n_images: int, device) -> ProposalBuffers:
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
    i = lambda *shape: torch.empty(shape, dtype=torch.int64, device=device)
    T = int(total_rows)
    return ProposalBuffers(f(T, 4), f(T), i(T), f(T, 4), f(T), i(T), i(T), torch.empty((int(n_images), 2), dtype=torch.int32, device=device))


def map_proposals(store_rows: torch.Tensor, row_start: Sequence[int], n_rows: Sequence[int], factors, flips: Sequence[int], sizes,
                  topk: int, thr: float, out: Optional[ProposalBuffers] = None) -> List[MappedProposals]:
    """transform_proposals and change_proposals_as_gt of a batch (locov_map_proposals: one launch per 64 images) and ONE host read,
    of the counts.  store_rows [R, 5] fp32 or fp64 on the device, XYXY + logit; image i owns rows [row_start[i], row_start[i] +
    n_rows[i]), is resized by factors[i] = (fx, fy) -- Python floats, rounded to the rows' dtype in the kernel --, flipped by
    flips[i] in sizes[i] = (new_h, new_w) and clipped to it.  Per image: the first topk non-empty boxes in their order with their
    fp32 logits and source rows, and of those the ones with logit > fp32(thr) with gt_classes 1.  out: the caller's
    ProposalBuffers instead of fresh ones."""
    store_rows = _dev(store_rows, "store_rows", dtype=None)
    if store_rows.dtype not in PROPOSAL_DTYPES or store_rows.dim() != 2 or store_rows.shape[1] != 5:
        raise TypeError(f"map_proposals: store_rows must be fp32 or fp64 [R, 5], got {store_rows.dtype} {tuple(store_rows.shape)}")
    starts, counts, flips = [int(s) for s in row_start], [int(c) for c in n_rows], [int(f) for f in flips]
    n = len(counts)
    if not (len(starts) == len(factors) == len(flips) == len(sizes) == n):
        raise ValueError("map_proposals: one row_start, n_rows, factor pair, flip and size per image")
    R = int(store_rows.shape[0])
    if int(topk) < 0 or any(c < 0 or s < 0 or s + c > R for s, c in zip(starts, counts)):
        raise ValueError(f"map_proposals: topk and the counts must not be negative and the rows must lie in the store's {R}")
    offs = [0, *itertools.accumulate(counts)]
    T = offs[-1]
    if T > 2 ** 31 - 1:
        raise ValueError(f"map_proposals: {T} rows leave int32")
    bufs = proposal_buffers(T, n, store_rows.device) if out is None else out
    if out is not None:
        f, i = torch.float32, torch.int64
        want = (((T, 4), f), ((T,), f), ((T,), i), ((T, 4), f), ((T,), f), ((T,), i), ((T,), i), ((n, 2), torch.int32))
        if any(not b.is_contiguous() or b.device != store_rows.device or (tuple(b.shape), b.dtype) != w for b, w in zip(bufs, want)):
            raise ValueError("map_proposals: out must be contiguous ProposalBuffers of this batch's sizes on the rows' device")
    lib = _lib.load()
    dtype = _lib.PROPOSAL_F32 if store_rows.dtype == torch.float32 else _lib.PROPOSAL_F64
    with torch.cuda.device(store_rows.device):
        for lo in range(0, n, IMAGE_BATCH_MAX_IMAGES):
            hi = min(lo + IMAGE_BATCH_MAX_IMAGES, n)
            m, part = hi - lo, slice(offs[lo], offs[hi])
            check(lib.locov_map_proposals(
                _ptr(store_rows), R, dtype, (ctypes.c_int64 * m)(*starts[lo:hi]), _ints(counts[lo:hi]),
                (ctypes.c_double * m)(*[float(f[0]) for f in factors[lo:hi]]), (ctypes.c_double * m)(*[float(f[1]) for f in factors[lo:hi]]),
                _ints(flips[lo:hi]), _ints([int(s[0]) for s in sizes[lo:hi]]), _ints([int(s[1]) for s in sizes[lo:hi]]), m, int(topk), float(thr),
                *[_ptr(b[part]) for b in bufs[:7]], _ptr(bufs.counts[lo:hi]), _stream(store_rows)), "locov_map_proposals")
    kept = bufs.counts.tolist() if n else []                       # the call's ONE host read
    return [MappedProposals(*[b[o:o + c[0]] for b in bufs[:3]], *[b[o:o + c[1]] for b in bufs[3:7]]) for o, c in zip(offs, kept)]


# --------------------------------------------------------------------------------------
# The caption path of the LSM step (csrc/caption.hip; language_backbone.py: BertEmbedding.forward_tokenized)
CAPTION_MAX_TOKENS = _lib.CAPTION_MAX_TOKENS      # LOCOV_CAPTION_MAX_TOKENS
CAPTION_MAX_HIDDEN = _lib.CAPTION_MAX_HIDDEN      # LOCOV_CAPTION_MAX_HIDDEN


class CaptionMlm(NamedTuple):
    """The masked-language-modelling rule's host numbers (transf_models.py:126-134): p = ..._PROB, p_mask = ..._PROB_MASK,
    p_mask_noise = ..._PROB_MASK + ..._PROB_NOISE summed in double, the [MASK] id and len(tokenizer)."""
    p: float
    p_mask: float
    p_mask_noise: float
    mask_id: int
    len_tok: int


class _CaptionEmbedFn(torch.autograd.Function):
    """locov_caption_embed_fwd / _bwd.  Returns (ints [rows, N] int64, input_emb [N, H], encoded [N, H] or None); differentiable
    in `weight` only (BertEmbedding.freeze, transf_models.py:156-164)."""

    @staticmethod
    def forward(ctx, weight, packed, draws, T, mlm, int_rows, position, token_type, ln_weight, ln_bias, eps, keep, p_drop):
        N, (V, H) = packed.shape[1], weight.shape
        dev = weight.device
        ints = torch.empty((int_rows, N), dtype=torch.int64, device=dev)
        input_emb = torch.empty((N, H), dtype=torch.float32, device=dev)
        layer_norm = position is not None
        encoded = torch.empty((N, H), dtype=torch.float32, device=dev) if layer_norm else None
        mean = torch.empty((N,), dtype=torch.float32, device=dev) if layer_norm else None
        rstd = torch.empty((N,), dtype=torch.float32, device=dev) if layer_norm else None
        m = mlm if draws is not None else CaptionMlm(1.0, 0.0, 0.0, 0, 1)
        with torch.cuda.device(dev):
            check(_lib.load().locov_caption_embed_fwd(
                _ptr(packed), _ptr(draws), N, int(T), H, V, _ptr(weight), _ptr(position), position.shape[0] if layer_norm else 0,
                _ptr(token_type), token_type.shape[0] if layer_norm else 0, _ptr(ln_weight), _ptr(ln_bias), float(eps), _ptr(keep),
                float(p_drop), float(m.p), float(m.p_mask), float(m.p_mask_noise), int(m.mask_id), int(m.len_tok), int(int_rows),
                _ptr(ints), _ptr(input_emb), _ptr(encoded), _ptr(mean), _ptr(rstd), _stream(weight)), "locov_caption_embed_fwd")
        ctx.mark_non_differentiable(ints)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(weight, ints, position, token_type, ln_weight, mean, rstd, keep)
            ctx.args = (int(T), float(p_drop))
        return ints, input_emb, encoded

    @staticmethod
    @once_differentiable
    def backward(ctx, _, g_in, g_enc):
        weight, ints, position, token_type, ln_weight, mean, rstd, keep = ctx.saved_tensors
        T, p_drop = ctx.args
        N, (V, H) = ints.shape[1], weight.shape
        layer_norm = position is not None
        g_in = _dev(g_in, "grad_input_embeddings") if g_in is not None else None
        g_enc = _dev(g_enc, "grad_encoded_tokens") if g_enc is not None else None
        lib = _lib.load()
        dW = torch.empty((V, H), dtype=torch.float32, device=weight.device)
        nbytes = int(lib.locov_caption_embed_bwd_workspace_bytes(N, H, int(layer_norm)))
        ws = _workspace("caption_bwd", weight, nbytes)
        with torch.cuda.device(weight.device):
            check(lib.locov_caption_embed_bwd(_ptr(ints), N, T, H, V, _ptr(weight), _ptr(position), _ptr(token_type), _ptr(ln_weight),
                                              _ptr(mean), _ptr(rstd), _ptr(keep), p_drop, _ptr(g_enc), _ptr(g_in), _ptr(dW), _ptr(ws),
                                              ws.numel(), _stream(weight)), "locov_caption_embed_bwd")
        return (dW,) + (None,) * 12


def caption_embed(packed: torch.Tensor, draws: Optional[torch.Tensor], T: int, weight: torch.Tensor, *, mlm: Optional[CaptionMlm] = None,
                  with_targets: bool = True, position: Optional[torch.Tensor] = None, token_type: Optional[torch.Tensor] = None,
                  ln_weight: Optional[torch.Tensor] = None, ln_bias: Optional[torch.Tensor] = None, eps: float = 1e-12,
                  keep: Optional[torch.Tensor] = None, p_drop: float = 0.0):
    """BertEmbedding's forward after the tokenizer (transf_models.py:114-152) in one launch (locov_caption_embed_fwd).

    packed int32 [4, N] on the device: input_ids, token_type_ids, attention_mask, special_tokens_mask, N = B * T tokens, whose ids
    and types the CALLER has validated against the tables on the host.  draws float64 [2, N] or None (masked language modelling
    inactive); mlm: the rule's numbers, required with draws.  weight fp32 [V, H].  with_targets: also produce target_ids and
    mlm_mask (MASKED_LANGUAGE_MODELING configured on).  position [max_pos, H], token_type [types, H], ln_weight / ln_bias [H], eps:
    the ADD_POSITION_EMBEDDING path, dropout(LayerNorm((W[id] + Tt[type]) + P[j])); keep: optional uint8 [N, H] keep mask drawn by
    the caller, kept values are multiplied by 1 / (1 - p_drop).

    Returns (ints int64 [4 | 6, N], input_embeddings [N, H], encoded_tokens [N, H] or None without the position path).
    Differentiable in `weight` only (locov_caption_embed_bwd: no atomics, bitwise reproducible).  N > CAPTION_MAX_TOKENS or
    H > CAPTION_MAX_HIDDEN raises LocovError (LOCOV_ERR_UNSUPPORTED): a caller with a torch expression checks the limits first."""
    packed = _dev(packed, "packed", torch.int32)
    weight = _dev(weight, "weight")
    if packed.dim() != 2 or packed.shape[0] != 4 or weight.dim() != 2:
        raise ValueError("caption_embed: packed must be [4, N] and weight [V, H]")
    N, (V, H) = packed.shape[1], weight.shape
    if T < 1 or N % T:
        raise ValueError(f"caption_embed: N = {N} tokens is not a multiple of T = {T}")
    if draws is not None:
        draws = _dev(draws, "draws", torch.float64)
        if tuple(draws.shape) != (2, N) or mlm is None or not with_targets:
            raise ValueError(f"caption_embed: draws must be [2, {N}] and come with `mlm` and with_targets")
        if not (0 <= mlm.mask_id < V and 1 <= mlm.len_tok <= V):
            raise ValueError(f"caption_embed: mask_id {mlm.mask_id} / len(tokenizer) {mlm.len_tok} outside the {V}-row word table")
    ln = (position, token_type, ln_weight, ln_bias)
    if any(t is not None for t in ln):
        if any(t is None for t in ln):
            raise ValueError("caption_embed: the position path needs position, token_type, ln_weight and ln_bias")
        position, token_type, ln_weight, ln_bias = (_dev(t.detach(), n) for t, n in zip(ln, ("position", "token_type", "ln_weight", "ln_bias")))
        if position.dim() != 2 or token_type.dim() != 2 or position.shape[1] != H or token_type.shape[1] != H or \
                tuple(ln_weight.shape) != (H,) or tuple(ln_bias.shape) != (H,) or position.shape[0] < T:
            raise ValueError(f"caption_embed: position [>= {T}, {H}], token_type [types, {H}], ln_weight / ln_bias [{H}] expected")
        if keep is not None:
            keep = _dev(keep, "keep", torch.uint8)
            if keep.numel() != N * H or not 0.0 <= p_drop < 1.0:
                raise ValueError(f"caption_embed: keep must hold {N} x {H} values and p_drop lie in [0, 1)")
    elif keep is not None:
        raise ValueError("caption_embed: keep without the position path")
    return _CaptionEmbedFn.apply(weight, packed, draws, int(T), mlm, 6 if with_targets else 4, position, token_type, ln_weight, ln_bias,
                                 float(eps), keep, float(p_drop))


# --------------------------------------------------------------------------------------
# the optimiser step over a list of tensors (csrc/sgd.hip)
SGD_CHUNK = _lib.SGD_CHUNK                        # LOCOV_SGD_CHUNK
SGD_MAX_CLASSES = _lib.SGD_MAX_CLASSES            # LOCOV_SGD_MAX_CLASSES
_SGD_CLIP = {None: _lib.SGD_CLIP_NONE, "value": _lib.SGD_CLIP_VALUE, "norm": _lib.SGD_CLIP_NORM}


class SgdTable:
    """The descriptor table of one sgd_step call site: the device copy the kernel reads, two pinned host copies it is filled from
    (a copy in flight is never overwritten: the one before it has been waited for), and the norm-clipping workspace.  `uploads`
    counts the host-to-device copies: one per step on which a pointer, a count, a class or a FIRST flag differs from the step
    before, none otherwise."""

    def __init__(self):
        self.uploads = 0
        self._records = None        # numpy int64 [n, 6]: what the device table holds
        self._counts = None         # the element counts the chunk map was built for
        self._chunks, self._chunk_map = 0, None
        self._device = None
        self._pinned = [None, None]
        self._events = [None, None]
        self._turn = 0
        self._workspace = None

    def _fill(self, records, counts, dev):
        import numpy as np
        n = len(counts)
        words = n * 6
        remap = counts != self._counts or self._device is None or self._device.device != dev
        if remap:
            per = [-(-c // SGD_CHUNK) for c in counts]
            chunks = sum(per)
            total = words + (chunks + 1) // 2
            if self._device is None or self._device.device != dev or self._device.numel() < total:
                self._device = torch.empty((total,), dtype=torch.int64, device=dev)
                self._pinned = [torch.empty((total,), dtype=torch.int64).pin_memory() for _ in range(2)]
                self._events = [None, None]
            self._chunk_map = np.repeat(np.arange(n, dtype=np.int32), per)
            self._counts, self._chunks = counts, chunks
        elif np.array_equal(records, self._records):
            return
        turn = self._turn = self._turn ^ 1
        if self._events[turn] is not None and not self._events[turn].query():
            self._events[turn].synchronize()              # (the copy issued two uploads ago: all but always finished)
        host = self._pinned[turn].numpy()
        host[:words] = records.reshape(-1)
        upto = words
        if remap:
            upto = words + (self._chunks + 1) // 2
            host[words:upto].view(np.int32)[:self._chunks] = self._chunk_map
        self._device[:upto].copy_(self._pinned[turn][:upto], non_blocking=True)
        if self._events[turn] is None:
            self._events[turn] = torch.cuda.Event()
        self._events[turn].record(torch.cuda.current_stream(dev))
        self._records = records
        self.uploads += 1

    def _workspace_for(self, nbytes, dev):
        if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < nbytes:
            self._workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        return self._workspace


def sgd_step(table: SgdTable, params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], bufs: Sequence[Optional[torch.Tensor]],
             classes: Sequence[int], first: Sequence[bool], lr: Sequence[float], wd: Sequence[float], *, momentum: float = 0.0,
             dampening: float = 0.0, nesterov: bool = False, clip_type: Optional[str] = None, clip_value: float = 1.0) -> None:
    """One torch.optim.SGD step over a list of tensors, in place, in one launch (locov_sgd_step; three with clip_type "norm").

    params[i], grads[i] and, with momentum != 0, bufs[i]: fp32, contiguous, on ONE ROCm device, of equal element counts (empty
    tensors are not accepted: leave them out).  classes[i] indexes lr / wd (at most SGD_MAX_CLASSES of them); first[i]: bufs[i]
    holds nothing yet and receives d.  clip_type None, "value" (clamp to +- clip_value) or "norm" (scale to an L2 norm of
    clip_value, per tensor).  grads are never written.  `table` belongs to the call site and is re-uploaded only when something
    in it changed.  No host read."""
    import numpy as np
    n = len(params)
    if not (len(grads) == len(bufs) == len(classes) == len(first) == n):
        raise ValueError("sgd_step: params, grads, bufs, classes and first must have one entry per tensor")
    if clip_type not in _SGD_CLIP:
        raise ValueError(f"sgd_step: unknown clip_type {clip_type!r}")
    if not 1 <= len(lr) <= SGD_MAX_CLASSES or len(wd) != len(lr):
        raise ValueError(f"sgd_step: 1..{SGD_MAX_CLASSES} hyper-parameter classes per call, one lr and one wd each")
    if n == 0:
        return
    dev = params[0].device
    use_buf = momentum != 0
    rows, counts = [], []
    for i in range(n):
        p, g, b = params[i], grads[i], bufs[i] if use_buf else None
        cnt = p.numel()
        for t, what in ((p, "param"), (g, "grad"), (b, "momentum buffer")):
            if t is None:
                if what == "momentum buffer" and not use_buf:
                    continue
                raise ValueError(f"sgd_step: tensor {i}: missing {what}")
            if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() != cnt or t.is_sparse:
                raise ValueError(f"sgd_step: tensor {i}: {what} must be a contiguous fp32 tensor of {cnt} elements on {dev}")
        if cnt == 0:
            raise ValueError(f"sgd_step: tensor {i} is empty")
        if not 0 <= classes[i] < len(lr):
            raise ValueError(f"sgd_step: tensor {i}: class {classes[i]} outside the {len(lr)} given")
        rows.append((p.data_ptr(), g.data_ptr(), b.data_ptr() if use_buf else 0, cnt, 0, int(classes[i]) | (int(bool(first[i])) << 32)))
        counts.append(cnt)
    if dev.type != "cuda":
        raise LocovError(f"sgd_step: tensors are on {dev}: the kernel only runs on a ROCm GPU")
    records = np.array(rows, dtype=np.int64)
    per = -(-records[:, 3] // SGD_CHUNK)
    records[1:, 4] = np.cumsum(per)[:-1]
    chunks = int(per.sum())
    lib = _lib.load()
    with torch.cuda.device(dev):
        table._fill(records, tuple(counts), dev)
        ws, ws_bytes = None, 0
        if clip_type == "norm":
            ws_bytes = int(lib.locov_sgd_workspace_bytes(n, chunks))
            ws = table._workspace_for(ws_bytes, dev)
        c = len(lr)
        check(lib.locov_sgd_step(_ptr(table._device), n, chunks, (ctypes.c_float * c)(*lr), (ctypes.c_float * c)(*wd), c, float(momentum),
                                 float(dampening), int(bool(nesterov)), _SGD_CLIP[clip_type], float(clip_value), _ptr(ws), ws_bytes,
                                 _stream(params[0])), "locov_sgd_step")


# --------------------------------------------------------------------------------------
# COCO-protocol box evaluation (csrc/coco_eval.hip); composed by locov_amd/evaluation.py, whose docstring states the protocol.
class CocoOrder(NamedTuple):
    det_offsets: torch.Tensor   # int32 [C + 1]: each cell's dets in `boxes`
    boxes: torch.Tensor         # fp32 [N, 4] XYXY in cell order (cell, descending score, input order)
    cat_offsets: torch.Tensor   # int32 [K + 1] into the acc_* arrays
    acc_index: torch.Tensor     # int32 [N]: the cell-order slot of each det in (category, descending score, image, in-cell rank) order
    acc_rank: torch.Tensor      # int32 [N]: its in-cell rank
    acc_score: torch.Tensor     # fp64 [N]: its score


def _descending_key(score: torch.Tensor) -> torch.Tensor:
    """int64 keys whose ascending order is the descending order of the fp64 scores, equal scores (0.0 and -0.0 too) on equal keys."""
    b = (score + 0.0).view(torch.int64)
    return ~(b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF))


def coco_order(img_rank: torch.Tensor, cls: torch.Tensor, score: torch.Tensor, boxes: torch.Tensor, n_images: int,
               n_categories: int) -> CocoOrder:
    """The two orderings locov_coco_match / locov_coco_accumulate take, by stable sorts on integer keys (no host read).
    img_rank, cls: int64 [N]; score: fp64 [N]; boxes: fp32 [N, 4].  A class outside [0, K) goes to a trailing cell nothing reads."""
    boxes = _dev(boxes, "boxes")
    score = _dev(score, "score", torch.float64)
    img_rank, cls = _dev(img_rank, "img_rank", torch.int64), _dev(cls, "cls", torch.int64)
    I, K, N = int(n_images), int(n_categories), score.shape[0]
    C = I * K
    dev = boxes.device
    cell = torch.where((cls >= 0) & (cls < K), cls * I + img_rank, torch.full_like(cls, C))
    key = _descending_key(score)
    p1 = torch.sort(key, stable=True).indices
    cell, p2 = torch.sort(cell[p1], stable=True)
    perm = p1[p2]
    det_offsets = torch.searchsorted(cell, torch.arange(C + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    rank = (torch.arange(N, dtype=torch.int64, device=dev) - det_offsets[cell]).to(torch.int32)
    pa = torch.sort(key[perm], stable=True).indices
    cat, pb = torch.sort(torch.clamp(torch.div(cell, max(I, 1), rounding_mode="floor"), max=K)[pa], stable=True)
    acc = pa[pb]
    cat_offsets = torch.searchsorted(cat, torch.arange(K + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    return CocoOrder(det_offsets, boxes[perm].contiguous(), cat_offsets, acc.to(torch.int32), rank[acc].contiguous(),
                     score[perm][acc].contiguous())


def _match(fn: str, det_offsets, gt_offsets, cell_flags, det_boxes, gt_boxes, gt_area, gt_flag, area_ranges, iou_thresholds, max_det):
    """coco_match (cell_flags unused, gt_flag = gt_crowd) and lvis_match (gt_flag = gt_ignore_in): the checks, the outputs, the shared
    workspace and the call of the entry point.  fn is the public name: it selects the protocol and the messages carry it."""
    import numpy as np
    lvis = fn == "lvis_match"
    flag_name = "gt_ignore_in" if lvis else "gt_crowd"
    det_offsets, gt_offsets = _dev(det_offsets, "det_offsets", torch.int32), _dev(gt_offsets, "gt_offsets", torch.int32)
    if lvis:
        cell_flags = _dev(cell_flags, "cell_flags", torch.uint8)
    det_boxes = _dev(det_boxes, "det_boxes")
    gt_boxes, gt_area = _dev(gt_boxes, "gt_boxes", torch.float64), _dev(gt_area, "gt_area", torch.float64)
    gt_flag = _dev(gt_flag, flag_name, torch.uint8)
    C, N, G = det_offsets.shape[0] - 1, det_boxes.shape[0], gt_area.shape[0]
    if (gt_offsets.shape[0] != C + 1 or (lvis and cell_flags.shape[0] != C) or det_boxes.shape != (N, 4) or gt_boxes.shape != (G, 4)
            or gt_flag.shape[0] != G):
        raise ValueError(f"{fn}: offsets of C + 1 entries each, {'cell_flags [C], ' if lvis else ''}det_boxes [N,4], gt_boxes [G,4], "
                         f"gt_area [G], {flag_name} [G]")
    ar = np.ascontiguousarray(area_ranges, dtype=np.float64).reshape(-1, 2)
    th = np.ascontiguousarray(iou_thresholds, dtype=np.float64).reshape(-1)
    A, T = len(ar), len(th)
    dev = det_boxes.device
    bits = torch.empty((N, A * T), dtype=torch.uint8, device=dev)
    gt_ignore = torch.empty((A, G), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws_bytes = int(lib.locov_coco_match_workspace_bytes(G, int(max_det))) if N and G else 0
        ws = _workspace("coco_match", det_boxes, ws_bytes) if ws_bytes else None      # one cached buffer for both protocols
        dp = ctypes.POINTER(ctypes.c_double)
        entry, cells = (lib.locov_lvis_match, (_ptr(cell_flags),)) if lvis else (lib.locov_coco_match, ())
        check(entry(_ptr(det_offsets), _ptr(gt_offsets), *cells, C, N, G, int(max_det), _ptr(det_boxes), _ptr(gt_boxes), _ptr(gt_area),
                    _ptr(gt_flag), ar.ctypes.data_as(dp), A, th.ctypes.data_as(dp), T, _ptr(bits), _ptr(gt_ignore), _ptr(ws), ws_bytes,
                    _stream(det_boxes)), "locov_" + fn)
    return bits, gt_ignore


def coco_match(det_offsets: torch.Tensor, gt_offsets: torch.Tensor, det_boxes: torch.Tensor, gt_boxes: torch.Tensor,
               gt_area: torch.Tensor, gt_crowd: torch.Tensor, area_ranges, iou_thresholds, max_det: int):
    """locov_coco_match: -> det_bits uint8 [N, A * T] (bit 0 matched, bit 1 ignored), gt_ignore uint8 [A, G].  One launch, no host
    read.  det_offsets / gt_offsets: int32 [C + 1]; det_boxes fp32 [N, 4] XYXY in cell order; gt_boxes fp64 [G, 4] XYWH, gt_area
    fp64 [G], gt_crowd uint8 [G]; area_ranges [A][2] and iou_thresholds [T]: host doubles."""
    return _match("coco_match", det_offsets, gt_offsets, None, det_boxes, gt_boxes, gt_area, gt_crowd, area_ranges, iou_thresholds, max_det)


def coco_accumulate(cat_offsets: torch.Tensor, acc_index: torch.Tensor, acc_rank: torch.Tensor, acc_score: torch.Tensor,
                    det_bits: torch.Tensor, npig: torch.Tensor, n_thresholds: int, max_dets: Sequence[int], recall_thresholds,
                    with_scores: bool = True) -> torch.Tensor:
    """locov_coco_accumulate: -> ONE fp64 vector holding precision [T,R,K,A,M], then scores [T,R,K,A,M] (with_scores), then
    recall [T,K,A,M], every element written (-1 where npig == 0), so the caller downloads it in one copy.  One launch, no host read.
    cat_offsets int32 [K + 1]; acc_index / acc_rank int32 [N] and acc_score fp64 [N] in (category, descending score, image rank,
    in-cell rank) order; det_bits as coco_match leaves it; npig int32 [K, A]."""
    import numpy as np
    cat_offsets = _dev(cat_offsets, "cat_offsets", torch.int32)
    acc_index, acc_rank = _dev(acc_index, "acc_index", torch.int32), _dev(acc_rank, "acc_rank", torch.int32)
    acc_score, det_bits, npig = _dev(acc_score, "acc_score", torch.float64), _dev(det_bits, "det_bits", torch.uint8), _dev(npig, "npig", torch.int32)
    K, N, T = cat_offsets.shape[0] - 1, acc_index.shape[0], int(n_thresholds)
    if npig.dim() != 2 or npig.shape[0] != K:
        raise ValueError("coco_accumulate: npig must be [K, A]")
    A = npig.shape[1]
    if acc_rank.shape[0] != N or acc_score.shape[0] != N or det_bits.shape != (N, A * T):
        raise ValueError("coco_accumulate: acc_index, acc_rank, acc_score of N entries each and det_bits [N, A * T]")
    caps = np.ascontiguousarray(max_dets, dtype=np.int32).reshape(-1)
    rec = np.ascontiguousarray(recall_thresholds, dtype=np.float64).reshape(-1)
    M, R = len(caps), len(rec)
    n = T * R * K * A * M
    flat = torch.empty(((2 if with_scores else 1) * n + T * K * A * M,), dtype=torch.float64, device=det_bits.device)
    precision, scores, recall = flat[:n], (flat[n:2 * n] if with_scores else None), flat[-T * K * A * M:] if K else flat[:0]
    with torch.cuda.device(det_bits.device):
        check(_lib.load().locov_coco_accumulate(_ptr(cat_offsets), K, _ptr(acc_index), _ptr(acc_rank), _ptr(acc_score), N, _ptr(det_bits),
                                                _ptr(npig), A, T, caps.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), M,
                                                rec.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), R, _ptr(precision), _ptr(recall),
                                                _ptr(scores), _stream(det_bits)), "locov_coco_accumulate")
    return flat


# --------------------------------------------------------------------------------------
# LVIS-protocol box evaluation: the same kernels under the federated rules (evaluation.py's docstring states them).
def lvis_limit(img_rank: torch.Tensor, cls: torch.Tensor, score: torch.Tensor, n_images: int, n_categories: int,
               max_dets_per_image: int) -> torch.Tensor:
    """LVISResults.limit_dets_per_image without a host read: -> cls with every det past its image's first max_dets_per_image (of a
    stable sort by descending score, over all categories together) sent to class K, the trailing cell coco_order leaves unread.
    Two stable sorts on integer keys (descending score, then image rank) and the position inside the image.  A class outside
    [0, K) is left out before the cap: it takes no place among its image's dets."""
    score = _dev(score, "score", torch.float64)
    img_rank, cls = _dev(img_rank, "img_rank", torch.int64), _dev(cls, "cls", torch.int64)
    I, K, N = int(n_images), int(n_categories), score.shape[0]
    dev = score.device
    image = torch.where((cls >= 0) & (cls < K), img_rank, torch.full_like(img_rank, I))
    p1 = torch.sort(_descending_key(score), stable=True).indices
    image, p2 = torch.sort(image[p1], stable=True)
    perm = p1[p2]
    first = torch.searchsorted(image, torch.arange(I + 1, dtype=torch.int64, device=dev))
    pos = torch.arange(N, dtype=torch.int64, device=dev) - first[image]
    return cls.scatter(0, perm, torch.where(pos >= int(max_dets_per_image), torch.full_like(cls, K), cls[perm]))


def lvis_match(det_offsets: torch.Tensor, gt_offsets: torch.Tensor, cell_flags: torch.Tensor, det_boxes: torch.Tensor,
               gt_boxes: torch.Tensor, gt_area: torch.Tensor, gt_ignore_in: torch.Tensor, area_ranges, iou_thresholds, max_det: int):
    """locov_lvis_match: -> det_bits uint8 [N, A * T] (bit 0 matched, bit 1 ignored; 2 for every det of an unlisted cell),
    gt_ignore uint8 [A, G].  One launch, no host read.  As coco_match, with cell_flags uint8 [C] (_lib.LVIS_CELL_NEG |
    _lib.LVIS_CELL_NOT_EXHAUSTIVE) and gt_ignore_in uint8 [G] (the annotation's ignore field) in place of gt_crowd."""
    return _match("lvis_match", det_offsets, gt_offsets, cell_flags, det_boxes, gt_boxes, gt_area, gt_ignore_in, area_ranges, iou_thresholds,
                  max_det)


# --------------------------------------------------------------------------------------
# Class-agnostic proposal recall (csrc/proposal_recall.hip); composed by locov_amd/evaluation.py, whose docstring states the protocol.
def proposal_recall(img_rank: torch.Tensor, logits: torch.Tensor, boxes: torch.Tensor, gt_offsets: torch.Tensor, gt_boxes: torch.Tensor,
                    gt_area: torch.Tensor, gt_skip: Optional[torch.Tensor], max_gt_per_image: int, area_ranges, limits: Sequence[int],
                    iou_thresholds, mark=None):
    """locov_proposal_recall behind its ordering: -> (totals int64 [A * L, T + 1]: per (range, limit) the overlaps >= each threshold,
    then num_pos, summed over the images; gt_overlaps fp32 [A * L, G]), both on the device.  No host read.
    img_rank int64 [N], logits fp64 [N], boxes fp32 [N, 4] XYXY: the proposals of every processed image in any order; they are put
    by image rank, inside an image by descending logit with ties in input order, by two stable sorts on integer keys (as
    lvis_limit orders its dets).  gt_offsets int32 [I + 1], gt_boxes fp32 [G, 4] XYXY, gt_area fp32 [G], gt_skip uint8 [G] or None:
    the ground truth by image.  area_ranges [A][2], limits [L] (ascending) and iou_thresholds [T] are host values, rounded to
    fp32.  mark: called with "orderings", "launch" and "sum" after each step (tools/time_evaluation.py synchronises there)."""
    import numpy as np
    step = mark if mark is not None else (lambda name: None)
    boxes = _dev(boxes, "boxes")
    logits = _dev(logits, "logits", torch.float64)
    img_rank = _dev(img_rank, "img_rank", torch.int64)
    gt_offsets = _dev(gt_offsets, "gt_offsets", torch.int32)
    gt_boxes, gt_area = _dev(gt_boxes, "gt_boxes"), _dev(gt_area, "gt_area")
    if gt_skip is not None:
        gt_skip = _dev(gt_skip, "gt_skip", torch.uint8)
    I, N, G = gt_offsets.shape[0] - 1, boxes.shape[0], gt_area.shape[0]
    if (I < 0 or boxes.shape != (N, 4) or logits.shape != (N,) or img_rank.shape != (N,) or gt_boxes.shape != (G, 4)
            or (gt_skip is not None and gt_skip.shape != (G,))):
        raise ValueError("proposal_recall: img_rank [N], logits [N], boxes [N,4], gt_offsets [I + 1], gt_boxes [G,4], gt_area [G], gt_skip [G]")
    ar = np.ascontiguousarray(area_ranges, dtype=np.float32).reshape(-1, 2)
    th = np.ascontiguousarray(iou_thresholds, dtype=np.float32).reshape(-1)
    lim = np.ascontiguousarray(limits, dtype=np.int32).reshape(-1)
    A, L, T = len(ar), len(lim), len(th)
    dev = boxes.device
    p1 = torch.sort(_descending_key(logits), stable=True).indices
    image, p2 = torch.sort(img_rank[p1], stable=True)
    prop_offsets = torch.searchsorted(image, torch.arange(I + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    sorted_boxes = boxes[p1[p2]].contiguous()
    step("orderings")
    overlaps = torch.empty((A * L, G), dtype=torch.float32, device=dev)
    counts = torch.empty((I, A * L, T + 1), dtype=torch.int32, device=dev)        # (the launch writes every element; with no image,
    if I == 0 or (N == 0 and G == 0):                                             # or no proposal and no gt, nothing is launched)
        counts.zero_()
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    with torch.cuda.device(dev):
        check(_lib.load().locov_proposal_recall(_ptr(prop_offsets), _ptr(gt_offsets), I, N, G, int(max_gt_per_image), _ptr(sorted_boxes),
                                                _ptr(gt_boxes), _ptr(gt_area), _ptr(gt_skip), ar.ctypes.data_as(fp), A,
                                                lim.ctypes.data_as(ip), L, th.ctypes.data_as(fp), T, _ptr(overlaps), _ptr(counts),
                                                _stream(boxes)), "locov_proposal_recall")
    step("launch")
    totals = counts.sum(0)
    step("sum")
    return totals, overlaps


# --------------------------------------------------------------------------------------
# Baseline JPEG decoding for the dataset mapper (csrc/jpeg_entropy.h on host threads, csrc/jpeg.hip; jpeg.py is the definition)
JPEG_FORMATS = {"RGB": _lib.JPEG_RGB, "BGR": _lib.JPEG_BGR, "L": _lib.JPEG_L}


def _jpeg_bytes(data) -> bytes:
    return data if isinstance(data, bytes) else bytes(data)


def jpeg_parse(data) -> "_lib.JpegHeader":
    """The header of a JPEG stream (locov_jpeg_parse; jpeg.parse_jpeg is its definition, field by field): .supported says whether
    the device decoder takes the stream and .reason (jpeg.REASONS) why not.  Never raises on a malformed stream.  No GPU."""
    data = _jpeg_bytes(data)
    header = _lib.JpegHeader()
    check(_lib.load().locov_jpeg_parse(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), ctypes.byref(header)), "locov_jpeg_parse")
    return header


class JpegStaged(NamedTuple):
    """One stream after locov_jpeg_entropy_decode: its header, the stage's status (jpeg.STATUSES; 0: decoded), the staging buffer
    (scan order) and the bytes its record will take."""
    header: "_lib.JpegHeader"
    status: int
    staging: Optional["object"]
    record_bytes: int


class JpegBatch(NamedTuple):
    """The packed records of a batch, ready for the upload: `records` is ONE uint8 host buffer (pinned on request) holding, per
    decoded image, its quantisation tables and its record; `descs` the locov_jpeg_desc fields of the decoded images, `index` their
    places in the list the batch was made from; `headers` and `status` cover every stream of that list."""
    records: torch.Tensor
    descs: List[tuple]           # (width, height, ncomp, hs, vs, record_offset, record_bytes, qt_offset)
    index: List[int]
    headers: list
    status: List[int]

    def record(self, i: int):
        """The record of stream i (of the original list) as uint32 words, its zero padding included; None if it was not decoded."""
        if i not in self.index:
            return None
        d = self.descs[self.index.index(i)]
        return self.records.numpy()[d[5]:d[5] + d[6]].view("uint32")


def jpeg_entropy_stage(datas: Sequence, headers: Optional[Sequence] = None) -> List[JpegStaged]:
    """Huffman-decodes the scans of a list of streams on up to min(16, n) host threads (locov_jpeg_entropy_decode; the GIL is
    released).  A stream whose header is not supported is not decoded (status jpeg.STATUS_UNSUPPORTED).  No GPU."""
    import numpy as np
    datas = [_jpeg_bytes(d) for d in datas]
    n = len(datas)
    if n == 0:
        return []
    lib = _lib.load()
    heads = (_lib.JpegHeader * n)()
    for i, d in enumerate(datas):
        if headers is not None:
            heads[i] = headers[i]
        else:
            check(lib.locov_jpeg_parse(ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p), len(d), ctypes.byref(heads[i])), "locov_jpeg_parse")
    need = [int(lib.locov_jpeg_entropy_bytes(ctypes.byref(heads[i]), len(d))) if heads[i].supported else 0 for i, d in enumerate(datas)]
    staging = [np.empty(max(b, 4), dtype=np.uint8) for b in need]        # (untouched pages cost nothing: the bound is loose)
    status, sizes = (ctypes.c_int32 * n)(), (ctypes.c_int64 * n)()
    check(lib.locov_jpeg_entropy_decode(
        (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p) for d in datas]), (ctypes.c_int64 * n)(*[len(d) for d in datas]),
        heads, (ctypes.c_void_p * n)(*[s.ctypes.data for s in staging]), (ctypes.c_int64 * n)(*need), n, status, sizes), "locov_jpeg_entropy_decode")
    return [JpegStaged(_lib.JpegHeader.from_buffer_copy(heads[i]), int(status[i]), staging[i] if status[i] == 0 else None, int(sizes[i]))
            for i in range(n)]


def jpeg_pack(staged: Sequence[JpegStaged], pin_memory: bool = False) -> JpegBatch:
    """Lays the records of the decoded streams of `staged` out in one host buffer (locov_jpeg_entropy_pack), each behind its
    quantisation tables; pin_memory: a pinned buffer, for one asynchronous upload.  No GPU work."""
    import numpy as np
    staged = list(staged)
    index = [i for i, s in enumerate(staged) if s.status == 0]
    descs, at = [], 0
    for i in index:
        h = staged[i].header
        qt_offset, at = at, at + (h.ncomp * 128 + 15) // 16 * 16
        descs.append((h.width, h.height, h.ncomp, h.comp_h[0], h.comp_v[0], at, staged[i].record_bytes, qt_offset))
        at += staged[i].record_bytes
    records = torch.empty(max(at, 16), dtype=torch.uint8, pin_memory=bool(pin_memory))
    n = len(index)
    if n:
        view, base = records.numpy(), records.data_ptr()
        heads = (_lib.JpegHeader * n)()
        for k, i in enumerate(index):
            h = heads[k] = staged[i].header
            qt = np.stack([np.ctypeslib.as_array(h.qt[h.comp_tq[c]]) for c in range(h.ncomp)]).astype(np.uint16)
            view[descs[k][7]:descs[k][7] + h.ncomp * 128] = qt.reshape(-1).view(np.uint8)
            view[descs[k][7] + h.ncomp * 128:descs[k][5]] = 0
        check(_lib.load().locov_jpeg_entropy_pack(
            heads, (ctypes.c_void_p * n)(*[staged[i].staging.ctypes.data for i in index]), (ctypes.c_int64 * n)(*[d[6] for d in descs]),
            (ctypes.c_void_p * n)(*[base + d[5] for d in descs]), n), "locov_jpeg_entropy_pack")
    return JpegBatch(records, descs, index, [s.header for s in staged], [s.status for s in staged])


def jpeg_entropy_decode(datas: Sequence, pin_memory: bool = False) -> JpegBatch:
    """jpeg_entropy_stage and jpeg_pack of a list of streams: the sparse coefficient records of jpeg.entropy_decode_host, packed for
    the upload.  Needs no GPU."""
    return jpeg_pack(jpeg_entropy_stage(datas), pin_memory)


def jpeg_decode_records(records: torch.Tensor, descs: Sequence[tuple], fmt: str = "RGB") -> List[torch.Tensor]:
    """The pixel pipeline (locov_jpeg_decode: two launches, no host read) over records already on the device: `records` is a
    JpegBatch's buffer as a device tensor, `descs` its descriptors (at most IMAGE_BATCH_MAX_IMAGES).  Returns one fresh uint8
    [height, width, 3] tensor per descriptor in `fmt` order, or [height, width, 1] for "L" (grey streams only): the bytes of
    jpeg.decode_jpeg_host.  Every byte of the outputs and every byte of the workspace that is read is written by the call."""
    descs = list(descs)
    n = len(descs)
    if n == 0:
        return []
    if fmt not in JPEG_FORMATS:
        raise ValueError(f"jpeg_decode_records: format {fmt!r} is none of {sorted(JPEG_FORMATS)}")
    if n > IMAGE_BATCH_MAX_IMAGES:
        raise ValueError(f"jpeg_decode_records: at most {IMAGE_BATCH_MAX_IMAGES} images per call, got {n}")
    records = _dev(records, "records", dtype=torch.uint8)
    table = (_lib.JpegDesc * n)()
    for t, d in zip(table, descs):
        t.width, t.height, t.ncomp, t.hs, t.vs, t.record_offset, t.record_bytes, t.qt_offset = [int(v) for v in d]
        if fmt == "L" and t.ncomp != 1:
            raise ValueError("jpeg_decode_records: format 'L' takes grey streams only (a colour stream as 'L' is Pillow's conversion)")
    lib = _lib.load()
    ws_bytes = int(lib.locov_jpeg_decode_workspace_bytes(table, n))
    if ws_bytes < 0:
        raise ValueError("jpeg_decode_records: a descriptor is outside the decoder's sizes and layouts")
    C = 1 if fmt == "L" else 3
    outs = [torch.empty((t.height, t.width, C), dtype=torch.uint8, device=records.device) for t in table]
    workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=records.device)
    with torch.cuda.device(records.device):
        check(lib.locov_jpeg_decode(_ptr(records), int(records.numel()), table, n, JPEG_FORMATS[fmt], _ptrs(outs), _ptr(workspace), ws_bytes,
                                    _stream(records)), "locov_jpeg_decode")
    return outs


def decode_jpeg_images(datas: Sequence, fmt: str = "RGB", device="cuda") -> List[torch.Tensor]:
    """Baseline JPEG streams (at most IMAGE_BATCH_MAX_IMAGES, any mix of sizes and layouts) -> uint8 [height, width, 3] device
    tensors in `fmt` order ("L": [height, width, 1], grey streams only): Pillow's bytes, as jpeg.decode_jpeg_host restates them.
    The scans are Huffman-decoded on host threads into one pinned buffer, uploaded once, and the pixels made in two launches.  A
    stream the decoder does not take -- an unsupported header, an anomaly in the scan -- raises ValueError naming the reason: the
    caller takes Pillow for it, with Pillow's error semantics."""
    from . import jpeg
    datas = list(datas)
    if fmt not in JPEG_FORMATS:
        raise ValueError(f"decode_jpeg_images: format {fmt!r} is none of {sorted(JPEG_FORMATS)}")
    if len(datas) > IMAGE_BATCH_MAX_IMAGES:
        raise ValueError(f"decode_jpeg_images: at most {IMAGE_BATCH_MAX_IMAGES} images per call, got {len(datas)}")
    device = torch.device(device)
    staged = jpeg_entropy_stage(datas)
    for i, s in enumerate(staged):                                 # (the refusals come first: they need no GPU)
        if not s.header.supported:
            raise ValueError(f"decode_jpeg_images: stream {i}: {jpeg.REASONS[s.header.reason]}")
        if s.status != 0:
            raise ValueError(f"decode_jpeg_images: stream {i}: {jpeg.STATUSES[s.status]}")
        if fmt == "L" and s.header.ncomp != 1:
            raise ValueError(f"decode_jpeg_images: stream {i}: a colour stream as 'L' is Pillow's conversion, not the decoder's")
    if device.type != "cuda":
        raise LocovError(f"decode_jpeg_images: device {device}: the decoder only runs on a ROCm GPU (jpeg.decode_jpeg_host is the host definition)")
    if not staged:
        return []
    batch = jpeg_pack(staged, pin_memory=True)
    return jpeg_decode_records(batch.records.to(device, non_blocking=True), batch.descs, fmt)
