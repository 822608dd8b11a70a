"""CPU-side checks of GroundingHead's hardmax alignment and triplet tail on the kernels (locov_grounding_align_fwd / _bwd,
locov_grounding_triplet_fwd / _bwd): declared, bound and exported, argument errors reported before any HIP call, and the float64
re-statement the GPU tests measure against (tests/grounding_variants_ref.py) pinned to the reference's own outputs
(tests/golden/g8_grounding_variants.npz)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import grounding_variants_ref as gvr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["locov_grounding_align_fwd", "locov_grounding_align_bwd", "locov_grounding_triplet_fwd", "locov_grounding_triplet_bwd"]
P = ctypes.c_void_p
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    from locov_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locov_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for macro, value in (("LOCOV_GROUNDING_ALIGN_SOFTMAX", _lib.GROUNDING_ALIGN_SOFTMAX),
                         ("LOCOV_GROUNDING_ALIGN_HARDMAX", _lib.GROUNDING_ALIGN_HARDMAX),
                         ("LOCOV_TRIPLET_HARDEST", _lib.TRIPLET_HARDEST), ("LOCOV_TRIPLET_EASIEST", _lib.TRIPLET_EASIEST),
                         ("LOCOV_TRIPLET_GIVEN", _lib.TRIPLET_GIVEN), ("LOCOV_GROUNDING_CE_MAX_B", ops.GROUNDING_CE_MAX_B)):
        assert re.search(rf"#define {macro} {value}\b", src), macro
    assert ops.GROUNDING_ALIGNMENTS == {"softmax": 0, "hardmax": 1}
    assert ops.TRIPLET_MINING == {"hardest": 0, "easiest": 1, "given": 2}
    assert lib.locov_abi_version() == 8 and re.search(r"#define LOCOV_ABI_VERSION 8\b", src)


def _err(lib):
    return lib.locov_last_error()


def test_grounding_align_rejects_bad_arguments(lib):
    S, cm, rm, a, b, dS = (P(256 * k) for k in range(1, 7))
    fwd = lambda B=2, T=5, NR=7, temp=10.0, align=1, w=a, r=b, s=S: lib.locov_grounding_align_fwd(s, B, T, NR, cm, rm, temp, align, w, r,
                                                                                                   None)
    bwd = lambda B=2, T=5, NR=7, temp=10.0, align=1, w=a, r=b, d=dS: lib.locov_grounding_align_bwd(S, B, T, NR, cm, rm, temp, align, w,
                                                                                                    r, d, None)
    for f in (fwd, bwd):
        for align in (2, -1, 7):
            assert f(align=align) == INVALID and b"unknown alignment" in _err(lib)
        assert f(w=None, r=None) == INVALID and b"both alignment directions are off" in _err(lib)
        for temp in (0.0, -1.0, float("nan")):
            assert f(temp=temp) == INVALID and b"temperature" in _err(lib)
        assert f(T=200, NR=200) == UNSUPPORTED and b"does not fit the LDS tile" in _err(lib)     # the limit of locov_grounding_fwd
        assert f(T=200, NR=200, align=0) == UNSUPPORTED
        for B in (0, -3):
            assert f(B=B) == INVALID and b"bad shape" in _err(lib)
    assert fwd(s=None) == INVALID and b"null pointer" in _err(lib)
    assert bwd(d=None) == INVALID and b"null pointer" in _err(lib)
    # the softmax entry points that were there before answer the same limit the same way
    assert lib.locov_grounding_fwd(S, 2, 200, 200, cm, rm, 10.0, a, b, None) == UNSUPPORTED


def test_grounding_triplet_rejects_bad_arguments(lib):
    c0, c1, cm, rm, out, pw0, pw1, idx = (P(256 * k) for k in range(1, 9))
    fwd = lambda B=4, mining=0, a=c0, b=c1, o=out, n=None: lib.locov_grounding_triplet_fwd(a, b, cm, rm, B, 9, 23, mining, 1.0, n, o,
                                                                                           pw0, pw1, None)
    bwd = lambda B=4, mining=0, d0=P(4096), d1=P(8192), n=None: lib.locov_grounding_triplet_bwd(c0, c1, cm, rm, B, 9, 23, mining, 1.0, n,
                                                                                                None, None, None, None, None, None, d0,
                                                                                                d1, None)
    for f in (fwd, bwd):
        for B in (0, 65, -1):
            assert f(B=B) == INVALID and b"1 <= B <= 64" in _err(lib)
        for mining in (3, -1, 11):
            assert f(mining=mining) == INVALID and b"unknown mining" in _err(lib)
        assert f(mining=2) == INVALID and b"need their indices" in _err(lib)           # GIVEN without indices
        assert f(mining=2, B=1) == INVALID
    assert fwd(a=None, b=None) == INVALID and b"null pointer" in _err(lib)
    assert fwd(o=None) == INVALID and b"null output" in _err(lib)
    assert fwd(o=None, mining=2, n=idx) == INVALID and b"null output" in _err(lib)
    assert bwd(d1=None) == INVALID and b"null gradient output" in _err(lib)


def test_ops_wrappers_check_their_arguments():
    from locov_amd import ops
    from locov_amd._lib import LocovError
    S, cm, rm = torch.zeros(6, 8), torch.zeros(2, 3), torch.zeros(2, 4)
    with pytest.raises(ValueError, match="unknown alignment"):
        ops.grounding_costs(S, cm, rm, 10.0, alignment="random_top3")
    with pytest.raises(ValueError, match="both alignment directions are off"):
        ops.grounding_costs(S, cm, rm, 10.0, alignment="hardmax", words=False, regions=False)
    with pytest.raises(ValueError, match="S must be"):
        ops.grounding_costs(torch.zeros(6, 9), cm, rm, 10.0, alignment="hardmax")
    with pytest.raises(LocovError, match="no CPU fallback"):                           # a missing device is an error, not eager torch
        ops.grounding_costs(S, cm, rm, 10.0, alignment="hardmax")
    c = torch.zeros(4, 4)
    cm, rm = torch.zeros(4, 3), torch.zeros(4, 5)
    with pytest.raises(ValueError, match="B <= 64"):
        ops.grounding_triplet(torch.zeros(65, 65), None, torch.zeros(65, 3), torch.zeros(65, 5), "hardest", 1.0)
    with pytest.raises(ValueError, match="unknown mining"):
        ops.grounding_triplet(c, c, cm, rm, "random", 1.0)
    for bad in (None, torch.zeros(2, 2, 4, dtype=torch.int32), torch.zeros(2, 2, 3, dtype=torch.int64),
                torch.zeros(4, 4, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"int64 \[2, 2, 4\]"):
            ops.grounding_triplet(c, c, cm, rm, "given", 1.0, neg_idx=bad)
    with pytest.raises(LocovError, match="no CPU fallback"):
        ops.grounding_triplet(c, None, cm, rm, "easiest", 1.0)


G8 = np.load(os.path.join(ROOT, "tests", "golden", "g8_grounding_variants.npz"))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["hardmax", "triplet_hardest", "triplet_easiest", "words_only", "regions_only_hardmax"])
def test_float64_restatement_matches_reference_vectors(name, B):
    """The yardstick of the GPU tests against the reference's own GroundingHead outputs, with the tolerances of
    tests/test_gpu_grounding.py::test_other_variants_match_reference_vectors."""
    cfg = json.loads(str(G8[name + "_cfg"]))
    p, q = f"{name}_b{B}_", f"b{B}_"
    region, cap = (torch.from_numpy(G8[q + k]).double() for k in ("region_features", "input_embeddings"))
    w = torch.from_numpy(G8["v2l_w"]).double().requires_grad_(True)
    b = torch.from_numpy(G8["v2l_b"]).double()
    losses, info, pw = gvr.head_forward(region, torch.from_numpy(G8[q + "region_mask"]), cap, torch.from_numpy(G8[q + "attention_mask"]),
                                        torch.from_numpy(G8[q + "special_tokens_mask"]), w, b, cfg)
    assert list(losses) == [str(n) for n in G8[p + "loss_names"]]
    assert list(info) == [str(n) for n in G8[p + "info_names"]]
    np.testing.assert_allclose([float(v.detach()) for v in losses.values()], G8[p + "losses"], rtol=2e-5, atol=2e-5, err_msg=p)
    np.testing.assert_array_equal(np.array([float(v) for v in info.values()], np.float32), G8[p + "info"], err_msg=p)
    if (p + "w2r") in G8:
        np.testing.assert_allclose(pw["w2r"].detach().numpy(), G8[p + "w2r"], rtol=2e-5, atol=2e-5, err_msg=p)
        np.testing.assert_allclose(pw["r2w"].detach().numpy(), G8[p + "r2w"], rtol=2e-5, atol=2e-5, err_msg=p)
    sum(losses.values()).backward()
    want, got = G8[p + "grad_v2l_w"], w.grad.numpy()
    assert np.abs(got - want).max() <= 2e-5 * max(np.abs(want).max(), 1e-3), (p, np.abs(got - want).max(), np.abs(want).max())


def test_given_negatives_index_the_matrix_without_its_diagonal():
    """The mapping the kernel uses for given indices -- reduced index k names row k above the diagonal position and k + 1 from it
    on -- is what gather on the matrix without its diagonal picks."""
    B = 5
    g = torch.Generator().manual_seed(3)
    cost = torch.randn(B, B, generator=g, dtype=torch.float64)
    idx = torch.randint(B - 1, (2, B), generator=g)
    j = torch.arange(B)
    cap = gvr.without_diagonal(cost, 0).gather(0, idx[0].view(1, B))[0]
    img = gvr.without_diagonal(cost, 1).gather(1, idx[1].view(B, 1))[:, 0]
    assert torch.equal(cap, cost[torch.where(idx[0] < j, idx[0], idx[0] + 1), j])
    assert torch.equal(img, cost[j, torch.where(idx[1] < j, idx[1], idx[1] + 1)])
