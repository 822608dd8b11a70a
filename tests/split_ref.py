"""float64 references and the per-element error gate of the fp32-in / fp32-out GEMM, Winograd and weight-gradient kernels
(f32 MFMA: gemm_nt.hip, gemm_tn.hip; f16x2 split: gemm_split.hip, gemm_split_big.hip, gemm_tn_split.hip, winograd.hip), shared by
tests/test_gpu_split_f64.py and the CPU check that the gate rejects the bugs it is there for (tests/test_split_gates.py).

Every reference is float64 of the kernel's fp32 inputs.  Next to the reference `ref` each case carries, element by element,
    S   the magnitude of the computation: |A| . |B|^T carried through the epilogue as in bf16_ref.epilogue
        (S * |scale| + |shift| + |residual|), and for a Winograd convolution the componentwise magnitude through the transforms;
    E   the error of the split operands (0 for the f32 MFMA), carried through the epilogue with |scale|;
    K   the accumulation length: the dot-product length for the f32 MFMA, 3x it for the split form (three products per pair).
The gate is, for every element (u = 2^-24, c = GATE_C = 2, as bf16_ref):

    |got - ref| <= c u (sqrt(K) + 1) S  +  4 u |ref|  +  E

  c u (sqrt(K) + 1) S   fp32 product rounding and fp32 accumulation (the f32 MFMA is a k-ordered fma chain; the split products
                        hi.hi, hi.lo, lo.hi are exact in fp32 and summed into one accumulator), plus the epilogue's scale / shift /
                        residual additions on the magnitude S.
  4 u |ref|             the fp32 epilogue's final roundings.
  E = REP_C 2^-22 S_ab  (split only) the 22-bit representation of each operand -- hi = fp16(s x), lo = fp16(s x - hi) keeps s x to
                        2^-11 * 2^-11 relative where lo is normal -- for both operands, plus the dropped lo.lo product (<= 2^-22
                        relative): REP_C = 3.  S_ab = |A| . |B|^T before the epilogue.
    + 2^-25 (sum_k |w_k| / s_a + sum_k |a_k| / s_w)
                        (split only) the subnormal floor: below |s x| = 2^-3 lo is an fp16 subnormal and below 2^-14 so is hi;
                        either way |s x - hi - lo| <= 2^-25 (half the subnormal spacing 2^-24), i.e. 2^-25 / s per operand element,
                        times the other operand.  s_a, s_w are the operand scales the launch actually used (device-chosen ones are
                        read back from their slot: slot_scale).
An element whose bound is 0 (a masked or ReLU'd zero of zero inputs) must be exact; a NaN on either side fails.

Winograd (F(4,3) | F(3,3) on a 7 x 7 tile, 11 x 11 transform domain; matrices from tools/gen_winograd_tables.build()):
    S = |A^T| [sum_c (|B^T| |d_c| |B|) (.) (|G| |g_c| |G^T|)] |A|
and K gains WINO_T = 2 * (7 + 3 + 11) = 42: one rounding per term of each 1-D pass of the input (7 taps), filter (3) and output
(11) transforms, two passes each.  The split terms are formed in the transform domain on |V| = |B^T d B| and |U| = |G g G^T| at the
operand scales v_scale and U.scale, and carried to the output with |A^T| . |A|.
Mean-fused GEMM (linear_split_segmean): the mean of the per-element bounds plus the seg-term fp32 sum, c u (sqrt(seg) + 1) mean |y|.
Weight gradients (gemm_tn, gemm_tn_split, winograd_wgrad): the contraction runs over M (ROIs x positions) in split-M chunks and a
fixed-order reduce of the chunk partials; both are fp32 sums of the same products, so K = M (3M split) covers them.
"""
import math
import os
import sys
from typing import NamedTuple

import torch
import torch.nn.functional as F

GATE_C = 2.0
U = 2.0 ** -24
REP_C = 3.0
FLOOR = 2.0 ** -25
WINO_T = 42


class Ref(NamedTuple):
    ref: torch.Tensor     # float64
    S: torch.Tensor       # float64 magnitude
    E: torch.Tensor       # float64 split-operand error (0 for the f32 MFMA)
    K: float              # accumulation length


def bound(r: Ref) -> torch.Tensor:
    return GATE_C * U * (math.sqrt(r.K) + 1) * r.S + 4 * U * r.ref.abs() + r.E


def gate_ratio(got, r: Ref) -> float:
    """max over elements of |got - ref| / bound (<= 1 passes)."""
    got = got.detach().double().cpu()
    assert got.shape == r.ref.shape, (got.shape, r.ref.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - r.ref).abs()
    b = bound(r)
    q = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    q = torch.where(torch.isnan(got) | torch.isnan(r.ref), math.inf, q)
    return float(q.max())


def assert_gate(got, r: Ref, what="") -> float:
    q = gate_ratio(got, r)
    assert q <= 1.0, f"{what}: err / bound = {q:.3g}"
    return q


def slot_scale(slot) -> float:
    """The operand scale a split launch derives from a device scale slot {s, 1/s, bits of max |x|, -} (gemm_nt.h split_scale_of)."""
    s = slot.detach().float().cpu().reshape(-1)
    if float(s[0]) != 0.0:
        return float(s[0])
    amax = float(s[2])
    if not (amax > 0 and amax < 3.0e38):
        return 1.0
    _, e = math.frexp(amax)
    return 2.0 ** (13 - e)


def _d(t):
    return None if t is None else t.detach().double().cpu()


def gemm(a, w, split=None) -> Ref:
    """a [M,K] . w [N,K]^T; split = (s_a, s_w) the operand scales of the split form, None for the f32 MFMA."""
    a, w = _d(a), _d(w)
    K = a.shape[1]
    ref, S = a @ w.t(), a.abs() @ w.abs().t()
    if split is None:
        return Ref(ref, S, torch.zeros_like(S), K)
    sa, sw = split
    fl = FLOOR * (w.abs().sum(1)[None, :] / sa + a.abs().sum(1)[:, None] / sw)
    return Ref(ref, S, REP_C * 2.0 ** -22 * S + fl, 3 * K)


def gemm_batched(a, w, split=None) -> Ref:
    """a [B,M,K] . w [B,N,K]^T per batch."""
    a, w = _d(a), _d(w)
    K = a.shape[2]
    ref, S = torch.bmm(a, w.transpose(1, 2)), torch.bmm(a.abs(), w.abs().transpose(1, 2))
    if split is None:
        return Ref(ref, S, torch.zeros_like(S), K)
    sa, sw = split
    fl = FLOOR * (w.abs().sum(2)[:, None, :] / sa + a.abs().sum(2)[:, :, None] / sw)
    return Ref(ref, S, REP_C * 2.0 ** -22 * S + fl, 3 * K)


def tn(a, b, split=None, row_scale=None) -> Ref:
    """out [N,K] = row_scale[n] * sum_m a[m,n] b[m,k]; split = (s_a, s_b)."""
    r = gemm(_d(a).t(), _d(b).t(), split)
    if row_scale is not None:
        rs = _d(row_scale).view(-1, 1)
        r = Ref(r.ref * rs, r.S * rs.abs(), r.E * rs.abs(), r.K)
    return r


def epilogue(r: Ref, scale=None, shift=None, residual=None, relu=False, mask=None) -> Ref:
    """y = relu(acc * scale + shift + residual), zeroed where mask <= 0 (scale / shift per column)."""
    y, S, E = r.ref, r.S, r.E
    if scale is not None:
        sc = _d(scale)
        y, S, E = y * sc, S * sc.abs(), E * sc.abs()
    if shift is not None:
        y, S = y + _d(shift), S + _d(shift).abs()
    if residual is not None:
        y, S = y + _d(residual), S + _d(residual).abs()
    if relu:
        y = torch.relu(y)
    if mask is not None:
        keep = _d(mask) > 0
        y, S, E = torch.where(keep, y, 0.0), torch.where(keep, S, 0.0), torch.where(keep, E, 0.0)
    return Ref(y, S, E, r.K)


def stored_split(r: Ref, s: float) -> Ref:
    """r written in the split layout at scale s (out_split) and read back as (hi + lo) / s: one more 22-bit rounding of the
    finished value, with the subnormal floor 2^-25 / s."""
    return Ref(r.ref, r.S, r.E + 2.0 ** -22 * r.ref.abs() + FLOOR / s, r.K)


def segmean(r: Ref, seg: int) -> Ref:
    """Mean over groups of `seg` consecutive (ROI-major) rows of a finished [M,N] reference -> [M/seg, N]."""
    M, N = r.ref.shape
    m = lambda t: t.view(M // seg, seg, N).mean(1)
    ymean = m(r.ref.abs())
    bnd = m(bound(r)) + GATE_C * U * (math.sqrt(seg) + 1) * ymean
    # fold everything into E so that bound() of the result is exactly that (S = 0, 4 u |ref| is part of the per-element bounds)
    ref = m(r.ref)
    return Ref(ref, torch.zeros_like(ref), (bnd - 4 * U * ref.abs()).clamp_min(0), 1)


# ------------------------------------------------------------------ Winograd
def wino_mats():
    """(BT [11,7], G [11,3], AT [7,11]) float64 of tools/gen_winograd_tables.build()."""
    tools = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_winograd_tables as T
    return tuple(torch.tensor([[float(v) for v in row] for row in m], dtype=torch.float64) for m in T.build())


def wino_transforms(d, w):
    """d [R,C,7,7], w [N,C,3,3] -> (V [R,C,11,11], Vabs, Ut [N,C,11,11], Uabs) float64: exact transforms and their magnitudes."""
    BT, G, _ = wino_mats()
    d, w = _d(d), _d(w)
    V = torch.einsum("ai,rcij,bj->rcab", BT, d, BT)
    Vabs = torch.einsum("ai,rcij,bj->rcab", BT.abs(), d.abs(), BT.abs())
    Ut = torch.einsum("ai,ncij,bj->ncab", G, w, G)
    Uabs = torch.einsum("ai,ncij,bj->ncab", G.abs(), w.abs(), G.abs())
    return V, Vabs, Ut, Uabs


def wino_conv(d, w, split=None) -> Ref:
    """3x3 / pad 1 convolution of 7x7 tiles d [R,C,7,7] with w [N,C,3,3] -> Ref over [R,N,7,7] (before the epilogue).
    split = (v_scale, u_scale): the 121 transform-domain GEMMs in split arithmetic at those operand scales."""
    _, _, AT = wino_mats()
    d, w = _d(d), _d(w)
    C = d.shape[1]
    ref = F.conv2d(d, w, padding=1)
    V, Vabs, Ut, Uabs = wino_transforms(d, w)
    out = lambda M: torch.einsum("ya,rnab,xb->rnyx", AT.abs(), M, AT.abs())
    S = out(torch.einsum("rcab,ncab->rnab", Vabs, Uabs))
    if split is None:
        return Ref(ref, S, torch.zeros_like(S), C + WINO_T)
    sv, su = split
    Va, Ua = V.abs(), Ut.abs()
    Edom = (REP_C * 2.0 ** -22 * torch.einsum("rcab,ncab->rnab", Va, Ua)
            + FLOOR * (Ua.sum(1)[None] / sv + Va.sum(1)[:, None] / su))
    return Ref(ref, S, out(Edom), 3 * C + WINO_T)


def wino_wgrad(d, g, split=None, row_scale=None) -> Ref:
    """dw [N,C,3,3] = row_scale[n] * sum_r corr(d_r, g_r) (the weight gradient of conv3x3 over R 7x7 tiles) from d [R,C,7,7],
    g [R,N,7,7].  In the Winograd domain dU = sum_r dM_r (.) V_r with dM = A g A^T, then dw = G^T dU G.
    split = (s_dM, s_V): the operand scales of the transform-domain TN GEMMs."""
    BT, G, AT = wino_mats()
    d, g = _d(d), _d(g)
    R = d.shape[0]
    ref = torch.nn.grad.conv2d_weight(d, (g.shape[1], d.shape[1], 3, 3), g, padding=1)
    V = torch.einsum("ai,rcij,bj->rcab", BT, d, BT)
    Vabs = torch.einsum("ai,rcij,bj->rcab", BT.abs(), d.abs(), BT.abs())
    dM = torch.einsum("ya,rnyx,xb->rnab", AT, g, AT)
    dMabs = torch.einsum("ya,rnyx,xb->rnab", AT.abs(), g.abs(), AT.abs())
    back = lambda T: torch.einsum("ai,ncab,bj->ncij", G.abs(), T, G.abs())
    S = back(torch.einsum("rnab,rcab->ncab", dMabs, Vabs))
    if split is None:
        E, K = torch.zeros_like(S), R + WINO_T
    else:
        sm, sv = split
        Va, Ma = V.abs(), dM.abs()
        Edom = (REP_C * 2.0 ** -22 * torch.einsum("rnab,rcab->ncab", Ma, Va)
                + FLOOR * (Va.sum(0)[None] / sm + Ma.sum(0)[:, None] / sv))
        E, K = back(Edom), 3 * R + WINO_T
    if row_scale is not None:
        rs = _d(row_scale).view(-1, 1, 1, 1)
        ref, S, E = ref * rs, S * rs.abs(), E * rs.abs()
    return Ref(ref, S, E, K)


# ------------------------------------------------------------------ CPU emulation of the split arithmetic (test_split_gates.py)
def split_halves(x, s):
    """(hi, lo) fp16 of s x: hi = fp16(s x), lo = fp16(s x - hi), subnormals kept (torch's CPU conversion)."""
    sx = x.float() * s
    hi = sx.half()
    lo = (sx - hi.float()).half()
    return hi, lo


def emulate_split_gemm(a, w, sa, sw, BK=32, products=("hh", "hl", "lh"), flush_lo=False, skip_tile=None):
    """fp32 [M,N] of the split GEMM: the three products of each 32-column K-tile summed in fp32, tile after tile, then / (sa sw).
    Bug switches: products (a subset drops hi.lo or lo.hi), flush_lo (subnormal lo halves -> 0), skip_tile (a K-tile index
    not accumulated)."""
    ah, al = split_halves(a, sa)
    wh, wl = split_halves(w, sw)
    if flush_lo:
        al = torch.where(al.float().abs() < 2.0 ** -14, torch.zeros_like(al), al)
        wl = torch.where(wl.float().abs() < 2.0 ** -14, torch.zeros_like(wl), wl)
    ah, al, wh, wl = ah.float(), al.float(), wh.float(), wl.float()
    acc = torch.zeros(a.shape[0], w.shape[0])
    for t, k0 in enumerate(range(0, a.shape[1], BK)):
        if t == skip_tile:
            continue
        k = slice(k0, k0 + BK)
        part = torch.zeros_like(acc)
        if "hh" in products:
            part = part + ah[:, k] @ wh[:, k].t()
        if "hl" in products:
            part = part + ah[:, k] @ wl[:, k].t()
        if "lh" in products:
            part = part + al[:, k] @ wh[:, k].t()
        acc = acc + part
    return acc * (1.0 / (sa * sw))
