"""CPU-side checks of the one-launch distillation losses and of the grounding cross-entropy tail with distributions
(locov_distill_loss_fwd / _bwd, locov_grounding_ce_dist_fwd / _bwd): declared, bound and exported, argument errors reported before
any HIP call, and tensors off the device still on the torch code (no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["locov_distill_loss_fwd", "locov_distill_loss_bwd", "locov_grounding_ce_dist_fwd", "locov_grounding_ce_dist_bwd"]
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    from locov_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locov_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for macro, value in (("LOCOV_DISTILL_KD", _lib.DISTILL_KD), ("LOCOV_DISTILL_JS", _lib.DISTILL_JS),
                         ("LOCOV_DISTILL_MSE", _lib.DISTILL_MSE), ("LOCOV_DISTILL_MAX_B", _lib.DISTILL_MAX_B)):
        assert re.search(rf"#define {macro} {value}\b", src), macro
    assert _lib.DISTILL_MAX_B == 64 and lib.locov_abi_version() == 8


def _err(lib):
    return lib.locov_last_error()


def test_distill_loss_rejects_bad_arguments(lib):
    from locov_amd import _lib
    a, b, c, out = P(256), P(512), P(768), P(1024)
    KD, JS, MSE = _lib.DISTILL_KD, _lib.DISTILL_JS, _lib.DISTILL_MSE
    fwd = lambda B=4, kind=KD, temp=10.0, loss=out, trans=a: lib.locov_distill_loss_fwd(trans, b, c, B, kind, 0, temp, 1.0, loss, None)
    for B in (0, 65, -1):
        assert fwd(B=B) == -1 and b"1 <= B <= 64" in _err(lib)
    for kind in (3, -1, 17):
        assert fwd(kind=kind) == -1 and b"unknown kind" in _err(lib)
    for temp in (0.0, -1.0, float("nan")):
        assert fwd(temp=temp) == -1 and b"temperature" in _err(lib)
    assert fwd(kind=MSE, temp=0.0) == -1                                      # (rejected for every kind)
    assert fwd(trans=None) == -1 and b"null pointer" in _err(lib)
    assert fwd(loss=None) == -1 and b"null output" in _err(lib)
    assert fwd(kind=JS, loss=None) == -1 and b"null output" in _err(lib)
    bwd = lambda B=4, kind=KD, temp=10.0, gl=P(2048): lib.locov_distill_loss_bwd(a, b, c, B, kind, 1, temp, 1.0, gl, P(4096), None,
                                                                                  None, None)
    assert bwd(B=0) == -1 and bwd(B=65) == -1
    assert bwd(kind=5) == -1 and b"unknown kind" in _err(lib)
    assert bwd(temp=0.0) == -1 and b"temperature" in _err(lib)
    assert bwd(gl=None) == -1 and b"null grad_loss" in _err(lib)
    # nothing asks for a gradient (every input detached): a no-op success, no launch
    assert lib.locov_distill_loss_bwd(a, b, c, 4, KD, 1, 10.0, 1.0, P(2048), None, None, None, None) == 0
    with pytest.raises(_lib.LocovError, match="unknown kind"):
        _lib.check(fwd(kind=3), "locov_distill_loss_fwd")


def test_grounding_ce_dist_rejects_bad_arguments(lib):
    c0, c1, cm, rm, out, pw0, pw1 = (P(256 * k) for k in range(1, 8))
    fwd = lambda B=4, o=out, p0=pw0, p1=pw1, a=c0, b=c1: lib.locov_grounding_ce_dist_fwd(a, b, cm, rm, B, 9, 23, o, p0, p1, None)
    for B in (0, 65):
        assert fwd(B=B) == -1 and b"1 <= B <= 64" in _err(lib)
    assert fwd(a=None, b=None) == -1 and b"null pointer" in _err(lib)
    assert fwd(o=None) == -1 and b"null output" in _err(lib)
    assert fwd(p0=None) == -1 and b"null output" in _err(lib)                 # a distribution asked for without its output
    assert fwd(p1=None) == -1 and b"null output" in _err(lib)
    bwd = lambda B=4, d0=P(4096), d1=P(8192): lib.locov_grounding_ce_dist_bwd(c0, c1, cm, rm, B, 9, 23, None, None, None, None, None,
                                                                              None, d0, d1, None)
    assert bwd(B=0) == -1 and bwd(B=65) == -1
    assert bwd(d1=None) == -1 and b"null gradient output" in _err(lib)


G5 = np.load(os.path.join(ROOT, "tests", "golden", "g5_distill_losses.npz"))


@pytest.mark.parametrize("name", ["MultiDistillLoss", "MultiDistillLossJS", "MultiDistillLossL2"])
def test_cpu_tensors_keep_the_torch_code(monkeypatch, name):
    """Off the device the modules never reach the HIP path: the same values as tests/test_distill_losses.py's, also in float64."""
    from locov_amd import distill_losses as dl, ops

    def refuse(*a, **k):
        raise AssertionError("the HIP path was taken for CPU tensors")
    monkeypatch.setattr(ops, "distill_loss", refuse)
    for tt in (True, False):
        for c in range(int(G5["num_cases"])):
            trans, w2r, r2w = (torch.from_numpy(G5[f"c{c}_{k}"]) for k in ("trans", "w2r", "r2w"))
            mod = getattr(dl, name)(float(G5[f"c{c}_temp"]), loss_weight=0.7, detach_teacher=True, transformer_teacher=tt)
            want = float(G5[f"c{c}_{name}_tt{int(tt)}"])
            for dt in (torch.float32, torch.float64):
                got = float(mod(trans.to(dt), w2r.to(dt), r2w.to(dt)))
                assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), (c, dt, got, want)


def test_ops_wrappers_check_their_arguments():
    from locov_amd import ops
    x = torch.zeros(4, 4)
    with pytest.raises(ValueError, match="unknown kind"):
        ops.distill_loss("ce", x, x, x, 10.0)
    with pytest.raises(ValueError, match="1 <= B <= 64"):
        ops.distill_loss("kd", torch.zeros(65, 65), torch.zeros(65, 65), torch.zeros(65, 65), 10.0)
    with pytest.raises(ValueError, match=r"\[B, B\]"):
        ops.distill_loss("kd", x, torch.zeros(4, 3), x, 10.0)
    with pytest.raises(ValueError, match="temperature"):
        ops.distill_loss("js", x, x, x, 0.0)
    with pytest.raises(ValueError, match="B <= 64"):
        ops.grounding_ce_dist(torch.zeros(65, 65), None, torch.zeros(65, 3), torch.zeros(65, 5))
    from locov_amd._lib import LocovError
    with pytest.raises(LocovError, match="no CPU fallback"):
        ops.distill_loss("kd", x, x, x, 10.0)
