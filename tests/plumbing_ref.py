"""Plain-torch references of the small HBM-bound kernels around the heavy ones (csrc/res5_bwd.hip, the transpose of
csrc/roi_align_nhwc.hip, the means and row norms of csrc/head.hip, the weight pack and FrozenBN fold of csrc/gemm_nt.hip), the
case lists and inputs of tests/test_gpu_plumbing.py, and the assertions that keep the edge cases in those inputs.

Every function is a direct statement of the definition and runs unchanged on CPU and device tensors.  All but the three *_f64
functions are exact by construction -- a copy, a select or ONE correctly rounded fp32 operation -- so their gate is bit equality
(assert_bits: int32 / int16 patterns, so -0.0 against +0.0 and NaN payloads count).  tests/test_plumbing_ref.py pins them to
autograd and shows that each comparison rejects the bug it exists to catch."""
import math

import numpy as np
import torch
import torch.nn.functional as F

NORM_L2, NORM_STANDARDIZE = 1, 2                      # locov_amd._lib.NORM_*
U = 2.0 ** -24                                        # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ bit patterns
def bits(t: torch.Tensor) -> torch.Tensor:
    """The integer patterns of a float32 / bfloat16 tensor."""
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def bits_equal(got: torch.Tensor, want: torch.Tensor) -> bool:
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits(got), bits(want))


def assert_bits(got: torch.Tensor, want: torch.Tensor, tag="") -> None:
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    gb, wb = bits(got).flatten(), bits(want).flatten()
    if torch.equal(gb, wb):
        return
    bad = torch.nonzero(gb != wb).flatten()
    mask = 0xFFFFFFFF if got.dtype == torch.float32 else 0xFFFF
    first = [(int(i), hex(int(gb[i]) & mask), hex(int(wb[i]) & mask)) for i in bad[:6]]
    raise AssertionError(f"{tag}: {bad.numel()} of {gb.numel()} elements differ; (flat index, got, want): {first}")


def amax_bits(t: torch.Tensor) -> int:
    """The int32 pattern of max |t| (what a kernel folds into word 2 of an operand-scale slot)."""
    return int(t.abs().max().reshape(1).float().view(torch.int32))


def f32(bit_pattern: int) -> float:
    return float(np.array([bit_pattern], dtype=np.uint32).view(np.float32)[0])


# ------------------------------------------------------------------------------------------------ res5_bwd.hip
def transpose_scale(w, s=None):
    """[N,K] -> [K,N], out[k,n] = s[n] * w[n,k]."""
    return (w if s is None else w * s[:, None]).t().contiguous()


def weight_flip(w, s=None):
    """[N,Cin,3,3] -> [Cin,N,3,3], out[c,n,a,b] = s[n] * w[n,c,2-a,2-b]."""
    v = w if s is None else w * s[:, None, None, None]
    return v.flip(2, 3).permute(1, 0, 2, 3).contiguous()


def wgrad_unpack(p, s=None):
    """[N, 9*Cin] (column = tap*Cin + c) -> [N,Cin,3,3], rows scaled."""
    N, Cin = p.shape[0], p.shape[1] // 9
    v = p.view(N, 9, Cin).permute(0, 2, 1).reshape(N, Cin, 3, 3)
    return (v if s is None else v * s[:, None, None, None]).contiguous()


def pack3x3(w, dtype=torch.float32):
    """[N,Cin,3,3] -> [N, 9*Cin] with column = (ky*3+kx)*Cin + c (the inverse of wgrad_unpack)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().to(dtype)


def im2col(rows, H, W):
    """ROI-major pixel rows [R*H*W, C] -> 3x3 / pad 1 patches [R*H*W, 9*C] (column = tap*C + c)."""
    C = rows.shape[1]
    R = rows.shape[0] // (H * W)
    x = rows.view(R, H, W, C).permute(0, 3, 1, 2)
    return F.unfold(x, 3, padding=1).view(R, C, 9, H * W).permute(0, 3, 2, 1).reshape(R * H * W, 9 * C).contiguous()


def relu_mask(g, act):
    return torch.where(act > 0, g, torch.zeros_like(g))


def mean_bwd(g, act, hw):
    """g [R,C] -> [R*hw, C]: g[r] * (1/hw) on every position of r (ONE fp32 multiply), +0.0 where act <= 0 or NaN."""
    inv = torch.tensor(np.float32(1) / np.float32(hw), dtype=torch.float32, device=g.device)
    v = (g * inv).repeat_interleave(hw, 0)
    return v if act is None else torch.where(act > 0, v, torch.zeros_like(v))


def stride2(m):
    """[N,H,W,C] -> rows of the even pixels [N*OH*OW, C], OH = (H+1)//2."""
    return m[:, ::2, ::2].reshape(-1, m.shape[-1]).contiguous()


def stride2_adjoint(rows, N, H, W):
    out = torch.zeros(N, H, W, rows.shape[-1], dtype=rows.dtype, device=rows.device)
    out[:, ::2, ::2] = rows.view(N, (H + 1) // 2, (W + 1) // 2, -1)
    return out


# ------------------------------------------------------------------------------------------------ layouts, means, norms, BN
def to_nhwc(x, dtype=torch.float32):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype)


def to_nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def mean_rows_sequential(x):
    """Mean over the LAST axis as the rows and channels-last kernels define it: fp32 adds in index order, one fp32 division."""
    s = torch.zeros(x.shape[:-1], dtype=torch.float32, device=x.device)
    for k in range(x.shape[-1]):
        s = s + x[..., k]
    return s / torch.tensor(np.float32(x.shape[-1]), dtype=torch.float32, device=x.device)


def mean_f64(x):
    return x.double().mean(-1)


def rownorm_chain(x, mode, eps):
    """The row norm in x's own precision: L2 is F.normalize (x / max(|x|, eps)), standardise (x - mean) / (unbiased std + eps)."""
    if mode == NORM_L2:
        return x / torch.linalg.vector_norm(x, dim=1, keepdim=True).clamp_min(eps)
    return (x - x.mean(1, keepdim=True)) / (x.std(1, unbiased=True, keepdim=True) + eps)


def rownorm_f64(x, mode, eps, g=None):
    """float64 value of the row norm and, with g, its autograd gradient."""
    return _rownorm_with_grad(rownorm_chain, x.double(), mode, eps, None if g is None else g.double())


def rownorm_f32(x, mode, eps, g=None, chain=rownorm_chain):
    """The same chain in fp32 on the CPU: the yardstick whose error against float64 sizes the gate."""
    return _rownorm_with_grad(chain, x.float().cpu(), mode, eps, None if g is None else g.float().cpu())


def _rownorm_with_grad(chain, x, mode, eps, g):
    if g is None:
        return chain(x, mode, eps), None
    x = x.detach().clone().requires_grad_(True)
    y = chain(x, mode, eps)
    (dx,) = torch.autograd.grad(y, x, g)
    return y.detach(), dx


def bn_fold_f64(w, b, m, v, eps):
    """FrozenBatchNorm2d fold in float64; eps is the np.float32 the kernel receives."""
    assert isinstance(eps, np.float32)
    scale = w.double() / torch.sqrt(v.double() + float(eps))
    return scale, b.double() - m.double() * scale


# ------------------------------------------------------------------------------------------------ gates of the toleranced ones
def rownorm_gate(got, want, cpu32):
    """Per row: max |got - float64| against 2 x max |fp32 CPU chain - float64| + 1e-6 x max |float64| (the yardstick of
    tests/test_gpu_mha.py, held row by row because the rows' magnitudes differ by 24 orders).  Returns the ratios [R]; a row
    whose float64 value is not finite gives NaN."""
    err = (got.double().cpu() - want).abs().amax(1)
    bound = 2.0 * (cpu32.double() - want).abs().amax(1) + 1e-6 * want.abs().amax(1)
    return err / bound.clamp_min(1e-300)


def wave_mean_bound(x, ref):
    """spatial_mean_wave_kernel: ceil(hw/64) adds per lane, six butterfly levels, one division."""
    hw = x.shape[-1]
    return (math.ceil(hw / 64) + 7) * U * x.double().abs().sum(-1) / hw + U * ref.abs()


def bn_fold_bounds(b, m, scale_ref):
    """add, sqrt, reciprocal, multiply for the scale; then multiply, subtract for the shift."""
    return 4 * U * scale_ref.abs(), U * (b.double().abs() + 6 * (m.double() * scale_ref).abs())


# ------------------------------------------------------------------------------------------------ cases and inputs
TRANSPOSE_CASES = [(1, 1), (63, 65), (64, 64), (65, 63), (130, 129), (2048, 512)]                      # (N, K)
LAYOUT_CASES = [(1, 1, 1), (2, 63, 65), (1, 64, 64), (3, 65, 129), (2, 130, 4200)]                     # (N, C, HW)
CONV_W_CASES = [(1, 1), (3, 5), (24, 40), (64, 32)]                                                    # (N, Cin)
IM2COL_CASES = [(1, 1, 1, 4), (2, 1, 5, 8), (2, 5, 1, 8), (3, 2, 2, 4), (3, 7, 7, 32), (2, 13, 21, 64)]   # (R, H, W, C)
STRIDE2_CASES = [(1, 1, 1, 4), (2, 1, 6, 8), (2, 6, 1, 8), (1, 2, 2, 4), (2, 5, 7, 8), (3, 50, 84, 64)]   # (N, H, W, C)
MASK_HW = (1, 9, 49, 64, 65)
ROWNORM_CASES = [(1, 1), (3, 2), (5, 63), (37, 65), (6, 100), (37, 768), (9, 2048)]                    # (R, D); (1, 1): L2 only
BN_CASES = (1, 255, 256, 257, 2048)
MEAN_ROWS, MEAN_HW, WAVE_HW = (1, 255, 257, 513), (2, 7, 49, 63, 64), (65, 100, 2400)
ROWNORM_EPS = 1e-12

# past the grid cap: the smallest case of each kernel with a partial second grid-stride trip
CAP = 16384 * 256                                     # grid_for(): workgroups x threads
CAP_RELU_N = 4 * (CAP + 259)
CAP_MEAN_BWD = (343, 49, 1000)                        # (R, hw, C)
CAP_IM2COL = (67, 7, 7, 572)
CAP_STRIDE2_FWD = (3, 101, 167, 1312)
CAP_STRIDE2_ADJ = (3, 51, 85, 1312)
CAP_FLIP = (683, 683)
CAP_PACK, PACK_CAP = (342, 342), 4096 * 256
CAP_MEAN_NHWC, MEAN_NHWC_CAP = (1025, 2048, 2), 2048 * 256      # (R, C, hw)


def work_items(kernel: str, case) -> int:
    """Loop iterations of the whole grid (what the cap is compared with)."""
    if kernel == "relu_mask":
        return case // 4
    if kernel == "mean_bwd":
        return case[0] * case[1] * (case[2] // 4)
    if kernel == "im2col":
        R, H, W, C = case
        return R * H * W * 9 * (C // 4)
    if kernel == "stride2_fwd":
        N, H, W, C = case
        return N * ((H + 1) // 2) * ((W + 1) // 2) * (C // 4)
    if kernel == "stride2_adj":
        N, H, W, C = case
        return N * H * W * (C // 4)
    if kernel in ("flip", "pack"):
        return case[0] * case[1] * 9
    if kernel == "mean_nhwc":
        return case[0] * (case[1] // 4)
    raise KeyError(kernel)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def special_scale(n, g):
    """A per-row scale with negative entries and, from three rows on, an exact zero."""
    s = torch.randn(n, generator=g)
    s[0] = -abs(float(s[0])) - 0.25
    if n >= 3:
        s[1] = 0.0
    return s


def assert_scale_specials(s):
    assert bool((s < 0).any()) and (s.numel() < 3 or bool((s == 0).any())), "the scale lost its negative / zero entries"


def transpose_inputs(N, K):
    g = gen(1000 * N + K)
    return torch.randn(N, K, generator=g), special_scale(N, g)


def layout_inputs(N, C, HW):
    """x [N,C,H,W] with H*W = HW, the bf16 rounding edge values of tests/test_gpu_bf16.py over its first elements."""
    from test_gpu_bf16 import _special_fp32_bits, _to_f32
    H = 50 if HW == 4200 else 1
    x = torch.randn(N, C, H, HW // H, generator=gen(N * 7 + C * 3 + HW))
    sp = _to_f32(_special_fp32_bits())
    n = min(sp.numel(), x.numel())
    x.view(-1)[:n] = sp[:n]
    return x


def conv_w_inputs(N, Cin):
    """(w [N,Cin,3,3], row scale [N], packed gradient [N, 9*Cin])."""
    g = gen(100 * N + Cin)
    return torch.randn(N, Cin, 3, 3, generator=g), special_scale(N, g), torch.randn(N, 9 * Cin, generator=g)


def im2col_inputs(R, H, W, C):
    return torch.randn(R * H * W, C, generator=gen(R + 10 * H + 100 * W + C))


def stride2_inputs(N, H, W, C):
    """(map [N,H,W,C], rows [N*OH*OW, C])."""
    g = gen(N + 10 * H + 100 * W + C)
    return torch.randn(N, H, W, C, generator=g), torch.randn(N * ((H + 1) // 2) * ((W + 1) // 2), C, generator=g)


ACT_SPECIAL_BITS = {"+0.0": 0x00000000, "-0.0": 0x80000000, "NaN": 0x7FC00000, "subnormal": 0x00000001, "+inf": 0x7F800000}


def mask_inputs(rows, C, g):
    """act [rows, C] of a ReLU mask: randn with the special values written over its first five elements (the subnormal and +inf
    keep, +-0 and NaN mask)."""
    act = torch.randn(rows, C, generator=g)
    flat = act.view(-1)
    vals = torch.from_numpy(np.array(list(ACT_SPECIAL_BITS.values()), dtype=np.uint32).view(np.float32).copy())
    n = min(flat.numel(), vals.numel())
    flat[:n] = vals[:n]
    return act


def assert_act_specials(act):
    """The ReLU mask's edge values are all still in the input (by bit pattern)."""
    have = set((bits(act.cpu()).flatten()[:64].to(torch.int64) & 0xFFFFFFFF).tolist())
    missing = [k for k, v in ACT_SPECIAL_BITS.items() if v not in have]
    assert not missing, f"act lost its special values: {missing}"


def poison_masked(gfull, act):
    """NaN and inf at every masked position of a gradient (alternating): they must come out +0.0."""
    masked = ~(act > 0)
    idx = torch.nonzero(masked.flatten()).flatten()
    out = gfull.clone().flatten()
    out[idx[0::2]] = float("nan")
    out[idx[1::2]] = float("inf")
    return out.view_as(gfull)


def mean_bwd_inputs(R, hw, C, g):
    """(g [R,C], act [R*hw, C]) of the mean's backward (C >= 8): act carries the special values at position 0 of ROI 0; channels
    0..2 of that ROI (+0.0, -0.0, NaN there) are masked at EVERY position and their gradients are NaN, +inf and -inf."""
    act = mask_inputs(R * hw, C, g)
    a3 = act.view(R, hw, C)
    a3[0, 1:, 0:3] = -a3[0, 1:, 0:3].abs()
    gp = torch.randn(R, C, generator=g)
    gp[0, 0], gp[0, 1], gp[0, 2] = float("nan"), float("inf"), float("-inf")
    return gp, act


def assert_amax_at(out, where):
    """max |out| is taken once, at the first element or at the last (the end of the grid-stride tail)."""
    a = out.abs().flatten()
    i = int(a.argmax())
    assert i == (0 if where == "first" else a.numel() - 1), (where, i)
    assert int((a == a[i]).sum()) == 1, "the maximum must be unique"


def rownorm_inputs(R, D, g, eps=ROWNORM_EPS):
    """x [R,D], grad [R,D] and the named special rows.  From three rows on: row 0 all zero, row 1 with |x| < eps (the L2 clamp is
    active), row 2 with |x| just above eps; from five rows on row 3 constant.  Every other row is randn."""
    x = torch.randn(R, D, generator=g)
    gr = torch.randn(R, D, generator=g)
    rows = {}
    if R >= 3:
        unit = x[1:3] / torch.linalg.vector_norm(x[1:3].double(), dim=1, keepdim=True).float()
        x[0] = 0.0
        x[1] = unit[0] * (0.25 * eps)
        x[2] = unit[1] * (1.5 * eps)
        rows.update(zero=0, clamped=1, above=2)
    if R >= 5:
        x[3] = 0.75
        rows["constant"] = 3
    return x, gr, rows


def assert_rownorm_rows(x, rows, eps=ROWNORM_EPS):
    n = torch.linalg.vector_norm(x.double(), dim=1)
    if "zero" in rows:
        assert float(n[rows["zero"]]) == 0.0
        assert 0.0 < float(n[rows["clamped"]]) < eps < float(n[rows["above"]]) < 2 * eps
    if "constant" in rows:
        r = x[rows["constant"]]
        assert bool((r == r[0]).all()) and float(r[0]) != 0.0


def rownorm_excluded(rows, mode, backward):
    """Rows whose float64 value is undefined, by construction: standardise of the zero row (forward and backward), and the
    backward of standardise on the constant row."""
    if mode != NORM_STANDARDIZE:
        return []
    names = ["zero", "constant"] if backward else ["zero"]
    return sorted(rows[k] for k in names if k in rows)


def bn_inputs(C, g):
    """FrozenBN statistics with negative weights, var == 0 and large means."""
    w = torch.randn(C, generator=g)
    b = torch.randn(C, generator=g)
    m = torch.randn(C, generator=g) * 3.0
    v = torch.rand(C, generator=g) * 2.0 + 1e-3
    w[0] = -abs(float(w[0])) - 0.1
    m[0] = 3.0e4
    v[C // 2] = 0.0
    m[C - 1] = -7.5e5
    return w, b, m, v


def assert_bn_specials(w, b, m, v):
    assert bool((w < 0).any()) and bool((v == 0).any()) and float(m.abs().max()) >= 1e4
