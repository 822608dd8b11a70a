"""CPU proof that the error gate of the bf16 GEMM / convolution tests (bf16_ref.assert_gate, used by tests/test_gpu_bf16.py)
bites: a float64 reference of bf16 operands passes it when accumulated in fp32, and each plausible kernel bug -- a dropped
8-element K chunk (at the ragged tail or in the middle), a convolution tap dropped at an image edge, the shift left out,
operands truncated instead of rounded to nearest even -- exceeds it by at least 10x."""
import torch

from bf16_ref import bf16_rne, bf16_trunc, conv_ref, gate_ratio, gemm_ref

MARGIN = 10.0


def _gemm_case(K, seed=0, M=96, N=40):
    g = torch.Generator().manual_seed(seed)
    x32 = torch.randn(M, K, generator=g)
    w32 = torch.randn(N, K, generator=g) * 0.05
    sc = torch.rand(N, generator=g) + 0.5
    sh = torch.randn(N, generator=g)
    return x32, w32, sc, sh


def test_fp32_accumulation_of_the_same_operands_passes():
    for K in (8, 200, 1096):
        x32, w32, sc, sh = _gemm_case(K, seed=K)
        x, w = bf16_rne(x32), bf16_rne(w32)
        ref, S = gemm_ref(x, w, sc, sh, relu=True)
        got = torch.relu((x.float() @ w.float().t()) * sc + sh)
        assert gate_ratio(got, ref, S, K) <= 1.0, K


def test_a_dropped_k_chunk_is_rejected():
    K = 200                                            # K % 64 == 8: the last 8-element chunk is the masked tail
    x32, w32, sc, sh = _gemm_case(K, seed=1)
    x, w = bf16_rne(x32), bf16_rne(w32)
    ref, S = gemm_ref(x, w, sc, sh)
    for k0 in (K - 8, 64):                              # the ragged tail, a chunk in the middle
        xm = x.clone()
        xm[:, k0:k0 + 8] = 0
        bad, _ = gemm_ref(xm, w, sc, sh)
        assert gate_ratio(bad, ref, S, K) >= MARGIN, k0


def test_a_dropped_shift_is_rejected():
    K = 512
    x32, w32, sc, sh = _gemm_case(K, seed=2)
    x, w = bf16_rne(x32), bf16_rne(w32)
    ref, S = gemm_ref(x, w, sc, sh)
    bad, _ = gemm_ref(x, w, sc)
    assert gate_ratio(bad, ref, S, K) >= MARGIN


def test_truncated_operands_are_rejected():
    for K in (64, 200, 1096):
        x32, w32, sc, sh = _gemm_case(K, seed=3 + K)
        ref, S = gemm_ref(bf16_rne(x32), bf16_rne(w32), sc, sh)
        bad, _ = gemm_ref(bf16_trunc(x32), bf16_trunc(w32), sc, sh)
        assert gate_ratio(bad, ref, S, K) >= MARGIN, K


def test_a_conv_tap_dropped_at_an_image_edge_is_rejected():
    g = torch.Generator().manual_seed(4)
    R, Cin, H, W, N = 3, 64, 7, 7, 40
    x = bf16_rne(torch.randn(R, Cin, H, W, generator=g))
    w = bf16_rne(torch.randn(N, Cin, 3, 3, generator=g) * 0.05)
    sc, sh = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    res = torch.randn(R, N, H, W, generator=g)
    ref, S = conv_ref(x, w, sc, sh, res)
    K = 9 * Cin
    # fp32 accumulation of the same operands passes
    got, _ = conv_ref(x.float(), w.float(), sc, sh, res)
    assert gate_ratio(got.float(), ref, S, K) <= 1.0
    # right-edge pixels (x = W-1) lose their valid left-neighbour tap (ky, kx) = (1, 0); top-row pixels their (2, 1) tap
    for (ky, kx), edge in (((1, 0), (slice(None), W - 1)), ((2, 1), (0, slice(None)))):
        only = torch.zeros_like(w)
        only[:, :, ky, kx] = w[:, :, ky, kx]
        lost, _ = conv_ref(x, only, sc)
        bad = ref.clone()
        bad[:, :, edge[0], edge[1]] -= lost[:, :, edge[0], edge[1]]
        assert gate_ratio(bad, ref, S, K) >= MARGIN, (ky, kx)
