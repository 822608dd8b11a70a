"""float64 references and the error gate of the bf16 GEMM / convolution tests (tests/test_gpu_bf16.py), shared with the CPU
check that the gate rejects the bugs it is there for (tests/test_bf16_gates.py).

Every bf16 x bf16 product is exact in fp32 (8-bit significands), so a correct kernel differs from the float64 product of
the SAME bf16 operands only by its fp32 accumulation and its fp32 epilogue.  The gate bounds exactly that, per element:

    |got - ref| <= c * 2^-24 * sqrt(K) * S + 2^-22 * |ref|

S = (|A| . |B|^T) * |scale| + |shift| + |residual| (for a convolution: the convolution of |x| with |w|), K the length of
the dot product.
"""
import math

import torch
import torch.nn.functional as F

GATE_C = 2.0
U = 2.0 ** -24


def gate_ratio(got, ref, S, K, c=GATE_C):
    """max over elements of |got - ref| / bound (<= 1 passes).  An element whose bound is 0 must be exact."""
    got, ref, S = got.detach().double().cpu(), ref.double().cpu(), S.double().cpu()
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    bound = c * U * math.sqrt(K) * S + 4 * U * ref.abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    r = torch.where(torch.isnan(got) | torch.isnan(ref), math.inf, r)
    return float(r.max())


def assert_gate(got, ref, S, K, what=""):
    r = gate_ratio(got, ref, S, K)
    assert r <= 1.0, f"{what}: err / bound = {r:.3g}"
    return r


def bf16_rne(t):
    """float tensor -> float64 of its bf16 round-to-nearest-even (torch's conversion)."""
    return t.float().to(torch.bfloat16).double()


def bf16_trunc(t):
    """float tensor -> float64 of its bf16 truncation (the wrong conversion: low 16 bits dropped)."""
    bits = t.float().contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).double()


def epilogue(acc, acc_abs, scale=None, shift=None, residual=None, relu=False):
    """(ref, S) of y = relu(acc * scale + shift + residual), all float64 (scale / shift per column)."""
    y, S = acc, acc_abs
    if scale is not None:
        y, S = y * scale.double(), S * scale.double().abs()
    if shift is not None:
        y, S = y + shift.double(), S + shift.double().abs()
    if residual is not None:
        y, S = y + residual.double(), S + residual.double().abs()
    if relu:
        y = torch.relu(y)
    return y, S


def gemm_ref(x, w, scale=None, shift=None, residual=None, relu=False):
    """x [M,K], w [N,K] (bf16 or their float64 values) -> (ref, S) float64 [M,N]."""
    x, w = x.double().cpu(), w.double().cpu()
    return epilogue(x @ w.t(), x.abs() @ w.abs().t(), *(None if t is None else t.cpu() for t in (scale, shift, residual)),
                    relu=relu)


def conv_ref(x, w, scale=None, shift=None, residual=None, relu=False):
    """3x3 / pad 1 / stride 1: x [R,Cin,H,W], w [N,Cin,3,3] (values, float64 after widening); residual [R,N,H,W].
    -> (ref, S) float64 [R,N,H,W]."""
    x, w = x.double().cpu(), w.double().cpu()
    acc = F.conv2d(x, w, padding=1)
    acc_abs = F.conv2d(x.abs(), w.abs(), padding=1)
    v = lambda t: None if t is None else t.double().cpu().view(1, -1, 1, 1)
    return epilogue(acc, acc_abs, v(scale), v(shift), None if residual is None else residual.double().cpu(), relu)


def unpack_conv3x3(wp, Cin):
    """[N, 9*Cin] (k = (ky*3+kx)*Cin + c) -> [N,Cin,3,3]."""
    return wp.reshape(wp.shape[0], 3, 3, Cin).permute(0, 3, 1, 2)
