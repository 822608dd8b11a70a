"""ops.mha (csrc/mha.hip: locov_mha_fwd / locov_mha_bwd) against float64 (tests/transformer_ref.py's attention core).

The gate is sized by a yardstick that is never the code under test: the same arithmetic as an fp32 torch chain on the CPU, and ITS
error against float64.  The kernel's max error may be at most 2 x that plus 1e-6 x max |value| -- the factor 2 for another summation
order at the same precision (the MFMA result is a k-ordered fp32 fma chain, the CPU sums in blocks)."""
import functools
import math

import numpy as np
import pytest
import torch

import transformer_ref as tr

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 1, 32),          # S = 1
          (3, 2, 17, 32),         # under one tile, odd
          (2, 3, 65, 96),         # one past a 64 boundary, at the LSM head dim
          (4, 8, 170, 96),        # the LSM sequence at B = 2
          (1, 12, 170, 64),       # BERT-base head dim
          (1, 2, 257, 128)]       # several tiles, largest d
BIASES = ["mask01", "minus1e4", "zero"]
P_DROP = 0.1


@functools.lru_cache(maxsize=None)
def _inputs(shape, bias_kind):
    nseq, H, S, d = shape
    g = torch.Generator().manual_seed(1000 * S + 10 * d + nseq + BIASES.index(bias_kind))
    E = H * d
    qkv = torch.randn(nseq * S, 3 * E, generator=g)
    qkv[:, :E] *= 2.0                                           # scores q.k / sqrt(d): sigma about 2
    gout = torch.randn(nseq * S, E, generator=g)
    lengths = torch.randint(1, S + 1, (nseq,), generator=g)
    lengths[0] = 1                                              # a sequence with a single real key
    real = (torch.arange(S)[None, :] < lengths[:, None]).float()
    bias = {"mask01": real, "minus1e4": (1.0 - real) * -1e4, "zero": torch.zeros(nseq, S)}[bias_kind]
    keep = (torch.rand(nseq, H, S, S, generator=g) >= P_DROP).to(torch.uint8)
    return qkv, gout, bias, keep


def _chain(shape, bias_kind, dropout, dtype):
    """ctx, dQ, dK, dV of the torch chain on the CPU in `dtype`."""
    nseq, H, S, d = shape
    qkv, gout, bias, keep = _inputs(shape, bias_kind)
    E = H * d
    q, k, v = (qkv[:, i * E:(i + 1) * E].to(dtype).clone().requires_grad_(True) for i in range(3))
    ctx = tr.attention(q, k, v, bias.to(dtype), H, keep=keep if dropout else None, p_drop=P_DROP if dropout else 0.0)
    ctx.backward(gout.to(dtype))
    return [t.detach() for t in (ctx, q.grad, k.grad, v.grad)]


@functools.lru_cache(maxsize=None)
def _yardstick(shape, bias_kind, dropout):
    """(float64 values, per quantity the bound 2 x max |fp32 CPU chain - float64| + 1e-6 x max |float64|)."""
    want = _chain(shape, bias_kind, dropout, torch.float64)
    cpu32 = _chain(shape, bias_kind, dropout, torch.float32)
    ref_err = [float((a.double() - w).abs().max()) for a, w in zip(cpu32, want)]
    bound = [2.0 * e + 1e-6 * float(w.abs().max()) for e, w in zip(ref_err, want)]
    return want, ref_err, bound


def _run(fn, shape, bias_kind, dropout, blocks):
    nseq, H, S, d = shape
    qkv, gout, bias, keep = _inputs(shape, bias_kind)
    E = H * d
    dev = torch.device("cuda")
    if blocks:                                                  # column blocks of one matrix, read in place
        base = qkv.to(dev).requires_grad_(True)
        q, k, v = base[:, :E], base[:, E:2 * E], base[:, 2 * E:]
    else:
        q, k, v = (qkv[:, i * E:(i + 1) * E].contiguous().to(dev).requires_grad_(True) for i in range(3))
    ctx = fn(q, k, v, bias.to(dev), H, keep=keep.to(dev) if dropout else None, p_drop=P_DROP if dropout else 0.0)
    ctx.backward(gout.to(dev))
    grads = [base.grad[:, i * E:(i + 1) * E] for i in range(3)] if blocks else [q.grad, k.grad, v.grad]
    return [t.detach().cpu() for t in (ctx, *grads)]


def _gate(got, shape, bias_kind, dropout, tag):
    want, ref_err, bound = _yardstick(shape, bias_kind, dropout)
    errs = [float((g.double() - w).abs().max()) for g, w in zip(got, want)]
    for name, e, r, b in zip(("ctx", "dq", "dk", "dv"), errs, ref_err, bound):
        print(f"{tag} {shape} {bias_kind} dropout={dropout} {name}: err {e:.3e}  cpu-fp32 err {r:.3e}  bound {b:.3e}")
    for name, g, e, b in zip(("ctx", "dq", "dk", "dv"), got, errs, bound):
        assert torch.isfinite(g).all(), (tag, name)
        assert e <= b, (tag, shape, bias_kind, dropout, name, e, b)


@pytest.mark.parametrize("bias_kind", BIASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mha_matches_float64(shape, bias_kind):
    from locov_amd import ops
    for dropout in (False, True):
        for blocks in (True, False):
            got = _run(ops.mha, shape, bias_kind, dropout, blocks)
            _gate(got, shape, bias_kind, dropout, "fused/blocks" if blocks else "fused/three")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mha_packed_matches_float64(shape):
    from locov_amd import ops

    def packed(q, k, v, bias, H, **kw):
        return ops.mha_packed(q._base, bias, H, **kw)
    for dropout in (False, True):
        _gate(_run(packed, shape, "mask01", dropout, True), shape, "mask01", dropout, "fused/packed")


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[5]], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bitwise_equal(shape):
    from locov_amd import ops
    a = _run(ops.mha, shape, "mask01", True, True)
    b = _run(ops.mha, shape, "mask01", True, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("bias_kind", BIASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_composed_path_passes_the_same_gate(shape, bias_kind, monkeypatch):
    from locov_amd import transformer_head as th
    monkeypatch.setenv("LOCOV_FUSED_ATTENTION", "0")
    before = _launches()
    for dropout in (False, True):
        _gate(_run(th.attention_core, shape, bias_kind, dropout, True), shape, bias_kind, dropout, "composed")
    assert _launches() == before                                # the opt-out really is the torch chain


def _launches():
    from locov_amd import _lib
    return _lib.load().locov_launch_count()


def test_default_is_the_fused_kernel(monkeypatch):
    """attention_core without the opt-out is one launch forward and two backward, and a missing device is an error."""
    from locov_amd import transformer_head as th
    from locov_amd._lib import LocovError
    monkeypatch.delenv("LOCOV_FUSED_ATTENTION", raising=False)
    before = _launches()
    _run(th.attention_core, SHAPES[1], "mask01", False, True)
    assert _launches() - before == 3
    q = torch.zeros(6, 64)
    with pytest.raises(LocovError, match="no CPU fallback"):
        th.attention_core(q, q, q, torch.zeros(2, 3), 2)


def test_scale_argument_and_default():
    from locov_amd import ops
    shape = SHAPES[1]
    nseq, H, S, d = shape
    qkv, _, bias, _ = _inputs(shape, "mask01")
    E = H * d
    dev = torch.device("cuda")
    q, k, v = (qkv[:, i * E:(i + 1) * E].contiguous().to(dev) for i in range(3))
    a = ops.mha(q, k, v, bias.to(dev), H)
    b = ops.mha(q, k, v, bias.to(dev), H, scale=1.0 / math.sqrt(d))
    assert torch.equal(a, b)
    c = ops.mha(q, k, v, bias.to(dev), H, scale=0.5)
    want = tr.attention(*(t.double().cpu() for t in (q, k, v)), bias.double(), H, scale=0.5)
    # |ctx| <= max |v| < 5 and S = 17 terms: fp32 rounding stays below 17 x 2^-24 x 5 x a few = 2e-5; a scale that was ignored
    # (0.5 against the default 0.177) moves ctx by O(1)
    np.testing.assert_allclose(c.cpu().double().numpy(), want.numpy(), rtol=0, atol=2e-5)
