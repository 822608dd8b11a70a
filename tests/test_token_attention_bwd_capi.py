"""CPU-side checks of the multi-token class predictor's way back (locov_token_attention_bwd): declared, bound and exported with
the ABI number unchanged, argument errors reported before any HIP call, and the float64 restatement the GPU tests lean on
(tests/token_ref.py) pinned to the vectors recorded from the reference: g6 (scores, attention) and g9 (gradients)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import token_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
P = ctypes.c_void_p
CONFIGS = [(m, a, t) for m in ("dot", "cosine") for a in ("softmax", "hardmax") for t in (1, 10)]


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_symbol_is_declared_bound_and_exported(lib):
    from locov_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locov_hip.h")).read(), flags=re.S)
    assert re.search(r"\blocov_token_attention_bwd\s*\(", src)
    assert "locov_token_attention_bwd" in _lib.SIGNATURES and hasattr(lib, "locov_token_attention_bwd")
    # one more pointer than the forward (grad_scores, grad_att, grad_sim in place of scores, att)
    assert len(_lib.SIGNATURES["locov_token_attention_bwd"][1]) == len(_lib.SIGNATURES["locov_token_attention_fwd"][1]) + 1
    assert lib.locov_abi_version() == 8 and _lib.ABI_VERSION == 8        # the change only adds an export


def test_rejects_bad_arguments_before_any_hip_call(lib):
    sim, off, cnt, gmin, gs, ga, out = (P(256 * k) for k in range(1, 8))

    def bwd(R=4, Ttot=20, K1=10, Tmax=5, temp=1.0, sim=sim, off=off, cnt=cnt, gmin=gmin, gs=gs, ga=ga, out=out):
        return lib.locov_token_attention_bwd(sim, R, Ttot, off, cnt, K1, Tmax, temp, 0, 0, gmin, gs, ga, out, None)

    err = lib.locov_last_error
    assert bwd(R=0) == 0                                                  # no rows: a no-op success, no launch
    assert bwd(R=0, sim=None, gs=None, out=None) == 0
    for tmax in (33, 0, -1):
        assert bwd(Tmax=tmax) == -1 and b"Tmax must be in [1, 32]" in err()
    for temp in (0.0, -2.0, float("nan")):
        assert bwd(temp=temp) == -1 and b"temperature must be > 0" in err()
    assert bwd(R=-1) == -1 and b"bad shape" in err()
    assert bwd(Ttot=0) == -1 and bwd(K1=0) == -1
    assert bwd(gs=None) == -1 and b"null pointer grad_scores" in err()
    assert bwd(out=None) == -1 and b"null pointer grad_sim" in err()
    assert bwd(sim=None) == -1 and b"null pointer sim" in err()
    assert bwd(off=None) == -1 and b"tok_off" in err()
    assert bwd(gmin=None) == -1 and b"null pointer gmin" in err()


def test_op_has_no_cpu_path():
    from locov_amd import _lib, ops
    off, cnt, _ = token_ref.layout([2, 1])
    sim = torch.randn(3, 4, requires_grad=True)
    with pytest.raises(_lib.LocovError, match="no CPU fallback"):
        ops.token_attention_autograd(sim, torch.from_numpy(off), torch.from_numpy(cnt), 2, 1.0, torch.zeros(1))


def _g6_inputs(g6):
    ntok = [int(n) for n in g6["ntok"]]
    return ntok, [g6[f"emb{k}"] for k in range(len(ntok))], torch.from_numpy(g6["image_emb"])


@pytest.mark.parametrize("metric,align,temp", CONFIGS)
def test_float64_restatement_reproduces_the_recorded_forward_and_gradients(metric, align, temp):
    g6 = np.load(os.path.join(GOLD, "g6_grounding_module.npz"))
    g9 = np.load(os.path.join(GOLD, "g9_grounding_module_grad.npz"))
    ntok, embs, img = _g6_inputs(g6)
    tag = f"{metric}_{align}_t{temp}"
    gy, gatt = torch.from_numpy(g9["gy"]).double(), torch.from_numpy(g9["gatt"]).double()
    assert tuple(gy.shape) == (37, 10) and tuple(gatt.shape) == (37, 10, 5)
    for sfx in (("", "_att") if align == "softmax" else ("",)):
        x0 = img.double().requires_grad_(True)
        x = token_ref.normalize(x0) if metric == "cosine" else x0
        scores, att, sim = token_ref.grounding_module(x, embs, metric, align, float(temp))
        # forward: g6's gates (the recorded run is fp32)
        np.testing.assert_allclose(scores.detach().numpy(), g6[tag + "_scores"], atol=2e-5, rtol=1e-5)
        np.testing.assert_allclose(att.detach().numpy(), g6[tag + "_att"], atol=2e-6)
        loss = (scores * gy).sum() + ((att * gatt).sum() if sfx else 0.0)
        got = torch.autograd.grad(loss, x0)[0].numpy()
        want = g9[f"{tag}_grad{sfx}"]
        diff = np.abs(got - want).max()
        assert diff <= 2e-5 * max(np.abs(want).max(), 1e-3), (tag, sfx, diff, np.abs(want).max())
        # the figure recorded with the fixture is this very difference
        assert abs(diff - float(g9[f"{tag}_f64_diff{sfx}"])) <= 1e-9
        assert not any(k.endswith("hardmax_t1_grad_att") or k.endswith("hardmax_t10_grad_att") for k in g9.files)


def test_recorded_inputs_are_safe_for_hardmax():
    """No argmax can flip between the recorded run and another fp32 evaluation: the two best tokens of every (region, class)
    are at least 1e-4 apart, against a rounding of the fp32 similarity GEMM around 1e-6."""
    g6 = np.load(os.path.join(GOLD, "g6_grounding_module.npz"))
    ntok, embs, img = _g6_inputs(g6)
    for metric in ("dot", "cosine"):
        x = token_ref.normalize(img.double()) if metric == "cosine" else img.double()
        _, _, sim = token_ref.grounding_module(x, embs, metric, "hardmax", 1.0)
        off, cnt, _ = token_ref.layout(ntok)
        assert token_ref.hardmax_gap(sim, off, cnt, metric == "cosine") >= 1e-4


def test_closed_form_of_the_kernel_matches_autograd():
    """The formulas the kernel implements (csrc/token_attention.hip), evaluated in float64 numpy, against autograd through the
    restatement: softmax with and without an attention gradient, hardmax, cosine with NaN similarities, token-less classes in
    the middle and at the end."""
    rng = np.random.default_rng(11)
    num_tok = np.array([3, 0, 1, 5, 2, 0, 4, 0], np.int32)
    off = np.concatenate([[0], np.cumsum(np.maximum(num_tok, 1))[:-1]]).astype(np.int32)
    ttot, tmax, R = int(np.maximum(num_tok, 1).sum()), 5, 6
    for cosine in (False, True):
        for hardmax in (False, True):
            for temp in (1.0, 10.0):
                sim_np = rng.standard_normal((R, ttot)) * (0.3 if cosine else 2.0)
                if cosine:
                    sim_np[1, 0] = sim_np[3, 5] = sim_np[4, ttot - 1] = np.nan
                sim = torch.from_numpy(sim_np).requires_grad_(True)
                gmin = token_ref.padded_min(sim, off, num_tok, tmax, temp, cosine)
                scores, att = token_ref.token_attention(sim, off, num_tok, tmax, temp, cosine, hardmax, gmin)
                g = rng.standard_normal(tuple(scores.shape))
                ga = rng.standard_normal(tuple(att.shape))
                want = torch.autograd.grad((scores * torch.from_numpy(g)).sum() + (att * torch.from_numpy(ga)).sum(), sim)[0].numpy()
                got = np.full_like(sim_np, np.nan)
                fill = float(gmin) - 100.0
                for r in range(R):
                    for k, (o, n) in enumerate(zip(off, num_tok)):
                        if n == 0:
                            got[r, o] = 0.0
                            continue
                        v = sim_np[r, o:o + n].copy()
                        dead = np.isnan(v) & cosine
                        v[dead] = 0.0
                        s = np.concatenate([v / temp, np.full(tmax - n, fill)])
                        d = ((1 - v) if cosine else -v) / temp
                        if hardmax:
                            ds = g[r, k] * (np.arange(n) == int(np.argmax(s)))
                        else:
                            a = np.exp(s - s.max())
                            a = (a / a.sum())[:n]
                            ds = g[r, k] * a * (1 - d + (a * d).sum()) + a * (ga[r, k, :n] - (ga[r, k, :n] * a).sum())
                        got[r, o:o + n] = np.where(dead, 0.0, ds / temp)
                assert not np.isnan(got).any()                            # every element has a writer
                np.testing.assert_allclose(got, want, atol=1e-12, rtol=1e-10)
