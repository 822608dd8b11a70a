"""Training through the multi-token class predictor on the device: locov_token_attention_bwd, its autograd node,
the differentiable GroundingModule / EmbeddingGroundingFastRCNNOutputLayers and an STT fine-tune step through them.

Yardsticks: the float64 restatement tests/token_ref.py (pinned to the reference's vectors on the CPU by
tests/test_token_attention_bwd_capi.py), the gradients recorded from the reference's own autograd
(tests/golden/g9_grounding_module_grad.npz) and the single-vector predictor, which a bank of one token per class at
temperature 1 must reproduce.  Gates are this suite's existing ones:
    gradients vs recorded / float64 values   max|got - want| <= 2e-5 * max(max|want|, 1e-3)        (test_gpu_grounding.py)
    step-level comparisons                   losses within 2e-4 * max(|loss|, 1e-3), relative L2 of a gradient < 5e-3 (test_gpu_stt.py)
    forward                                  g6's atol 2e-5 / rtol 1e-5 (scores), atol 2e-6 (attention)
The reference's own fp32 gradients sit within 1.1e-6 (largest entry 4.4) of float64 -- the figures are stored in g9."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
G6 = np.load(os.path.join(GOLD, "g6_grounding_module.npz"))
G9 = np.load(os.path.join(GOLD, "g9_grounding_module_grad.npz"))
CONFIGS = [(m, a, t) for m in ("dot", "cosine") for a in ("softmax", "hardmax") for t in (1, 10)]
BASE = 48                                              # coco_instances.py: 48 seen classes (configs/coco_stt.yaml:20)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def assert_grad(got, want, what):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = want.detach().double().cpu().numpy() if torch.is_tensor(want) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{what}: max|got - want| {diff:.3g}  max|want| {top:.3g}  bound {2e-5 * max(top, 1e-3):.3g}")
    assert diff <= 2e-5 * max(top, 1e-3), (what, diff, top)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the float64 closed form on the SAME fp32 similarities
# ----------------------------------------------------------------------------------------------------------------------
def _bank_layout(rng, K1, tmax):
    """Token counts in [0, tmax] with token-less classes in the middle and at the end, and one class that fills tmax."""
    cnt = rng.integers(0, tmax + 1, size=K1)
    cnt[0] = tmax
    cnt[K1 // 2] = 0
    cnt[K1 // 3] = 0
    cnt[-1] = 0
    off = np.concatenate([[0], np.cumsum(np.maximum(cnt, 1))[:-1]])
    return off.astype(np.int32), cnt.astype(np.int32), int(np.maximum(cnt, 1).sum())


def _similarities(rng, R, off, cnt, ttot, cosine):
    """fp32 similarities on a grid: q / 64 + (token index) / 4096 with integer q -- two tokens of a class differ by at least
    1 / 4096 = 2.4e-4, so hardmax has no near-tie; exactly representable, |sim| < 1 (cosine) or < 4 (dot).  Under cosine some
    FIRST tokens (and a token-less class's column) are NaN: the forward zeroes them, 0 is first-token's own grid point."""
    tpos = np.zeros(ttot, np.int64)
    for o, n in zip(off, cnt):
        tpos[o:o + max(n, 1)] = np.arange(max(n, 1))
    q = rng.integers(-64, 64, size=(R, ttot)) if cosine else rng.integers(-256, 256, size=(R, ttot))
    sim = (q / 64.0 + tpos[None, :] / 4096.0).astype(np.float32)
    if cosine:
        first = off[cnt > 0]
        for c in rng.choice(first, size=min(len(first), 6), replace=False):
            sim[rng.integers(0, R), c] = np.nan
        sim[0, off[-1]] = np.nan                                # the token-less last class's column
        sim[R - 1, off[0]] = np.nan
    return sim


SHAPES = [(1, 10, 5), (1, 1204, 32), (37, 10, 1), (37, 10, 32), (37, 1204, 5), (1536, 10, 32), (1536, 1204, 1), (1536, 1204, 5)]


@pytest.mark.parametrize("metric,align,temp", CONFIGS)
def test_kernel_matches_float64_closed_form_on_the_same_similarities(pkg, metric, align, temp):
    from locov_amd import _lib, ops
    lib = _lib.load()
    cosine, hardmax = metric == "cosine", align == "hardmax"
    for case, (R, K1, tmax) in enumerate(SHAPES):
        rng = np.random.default_rng(100 * case + temp + 7 * cosine + 3 * hardmax)
        off, cnt, ttot = _bank_layout(rng, K1, tmax)
        sim_np = _similarities(rng, R, off, cnt, ttot, cosine)
        assert token_ref.hardmax_gap(torch.from_numpy(sim_np), off, cnt, cosine) >= 1e-4
        gy = torch.from_numpy(rng.standard_normal((R, K1)).astype(np.float32))
        ga = torch.from_numpy(rng.standard_normal((R, K1, tmax)).astype(np.float32))
        off_d, cnt_d = torch.from_numpy(off).cuda(), torch.from_numpy(cnt).cuda()
        gmin = token_ref.padded_min(torch.from_numpy(sim_np).cuda(), off, cnt, tmax, float(temp), cosine)
        for with_att in (False, True):
            what = f"{metric}_{align}_t{temp} R={R} K1={K1} Tmax={tmax} grad_att={with_att}"
            sim = torch.from_numpy(sim_np).cuda().requires_grad_(True)
            scores, att = ops.token_attention_autograd(sim, off_d, cnt_d, tmax, float(temp), gmin, cosine=cosine, hardmax=hardmax)
            assert scores.requires_grad and att.requires_grad
            outs, gouts = ([scores, att], [gy.cuda(), ga.cuda()]) if with_att else ([scores], [gy.cuda()])
            torch.cuda.synchronize()
            before = lib.locov_launch_count()
            (got,) = torch.autograd.grad(outs, [sim], gouts, retain_graph=True)
            assert lib.locov_launch_count() - before == 1, what         # the op's backward is ONE library launch
            (again,) = torch.autograd.grad(outs, [sim], gouts)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), what      # same bits on every run
            assert not torch.isnan(got).any(), what
            # float64 on the same fp32 values
            s64 = torch.from_numpy(sim_np).double().requires_grad_(True)
            r_scores, r_att = token_ref.token_attention(s64, off, cnt, tmax, float(temp), cosine, hardmax, gmin=float(gmin))
            loss = (r_scores * gy.double()).sum()
            if with_att and not hardmax:
                loss = loss + (r_att * ga.double()).sum()
            (want,) = torch.autograd.grad(loss, s64)
            np.testing.assert_allclose(scores.detach().cpu().numpy(), r_scores.detach().numpy(), atol=2e-5, rtol=1e-5, err_msg=what)
            np.testing.assert_allclose(att.detach().cpu().numpy(), r_att.detach().numpy(), atol=2e-6, err_msg=what)
            assert_grad(got, want, what)
            tokenless = torch.from_numpy(off[cnt == 0].astype(np.int64)).cuda()
            assert bool((got[:, tokenless] == 0).all()), what              # a token-less class's column
            if cosine:
                assert bool((got[torch.isnan(sim.detach())] == 0).all()), what


def test_only_the_attention_is_used(pkg):
    """scores unused: the node still sends one launch, with a zero gradient in its place."""
    from locov_amd import ops
    rng = np.random.default_rng(5)
    off, cnt, ttot = _bank_layout(rng, 10, 5)
    sim_np = _similarities(rng, 37, off, cnt, ttot, False)
    ga = torch.from_numpy(rng.standard_normal((37, 10, 5)).astype(np.float32))
    gmin = token_ref.padded_min(torch.from_numpy(sim_np).cuda(), off, cnt, 5, 1.0, False)
    sim = torch.from_numpy(sim_np).cuda().requires_grad_(True)
    _, att = ops.token_attention_autograd(sim, torch.from_numpy(off).cuda(), torch.from_numpy(cnt).cuda(), 5, 1.0, gmin)
    (got,) = torch.autograd.grad((att * ga.cuda()).sum(), sim)
    s64 = torch.from_numpy(sim_np).double().requires_grad_(True)
    _, r_att = token_ref.token_attention(s64, off, cnt, 5, 1.0, gmin=float(gmin))
    (want,) = torch.autograd.grad((r_att * ga.double()).sum(), s64)
    assert_grad(got, want, "attention only")


# ----------------------------------------------------------------------------------------------------------------------
# 2. the module against the gradients recorded from the reference;  6. evaluation unchanged
# ----------------------------------------------------------------------------------------------------------------------
def _g6_module(metric, align, temp):
    from locov_amd.roi_heads import GroundingModule
    ntok = G6["ntok"]
    gm = GroundingModule(48, len(ntok), 5, local_metric=metric, alignment=align, temperature=float(temp),
                         normalize_emb=metric == "cosine")
    gm.set_class_embeddings({k: torch.from_numpy(G6[f"emb{k}"]) for k in range(len(ntok))}, "cuda")
    return gm


@pytest.mark.parametrize("metric,align,temp", CONFIGS)
def test_module_matches_the_references_recorded_gradients(pkg, metric, align, temp):
    from locov_amd import ops
    gm = _g6_module(metric, align, temp)
    tag = f"{metric}_{align}_t{temp}"
    gy, gatt = torch.from_numpy(G9["gy"]).cuda(), torch.from_numpy(G9["gatt"]).cuda()
    for sfx in (("", "_att") if align == "softmax" else ("",)):
        for _ in range(2):                                    # the second call changes nothing
            x0 = torch.from_numpy(G6["image_emb"]).cuda().requires_grad_(True)
            x = ops.rownorm_autograd(x0, ops.NORM_L2) if metric == "cosine" else x0      # the predictor normalises first
            scores, att = gm(x)
            assert scores.requires_grad and att.requires_grad
            np.testing.assert_allclose(scores.detach().cpu().numpy(), G6[tag + "_scores"], atol=2e-5, rtol=1e-5)
            np.testing.assert_allclose(att.detach().cpu().numpy(), G6[tag + "_att"], atol=2e-6)
            loss = (scores * gy).sum()
            if sfx:
                loss = loss + (att * gatt).sum()
            (got,) = torch.autograd.grad(loss, x0)
            assert_grad(got, G9[f"{tag}_grad{sfx}"], tag + sfx)


@pytest.mark.parametrize("metric,align,temp", CONFIGS)
def test_evaluation_is_unchanged_bit_for_bit(pkg, metric, align, temp):
    """One module, one input: torch.no_grad() (the code path without autograd nodes) and the autograd node give the same bits."""
    from locov_amd import ops
    gm = _g6_module(metric, align, temp)
    x = torch.from_numpy(G6["image_emb"]).cuda()
    if metric == "cosine":
        x = ops.rownorm(x, ops.NORM_L2)
    with torch.no_grad():
        s0, a0 = gm(x)
    s1, a1 = gm(x)                                            # gradients enabled, nothing to carry one: the same path
    s2, a2 = gm(x.clone().requires_grad_(True))
    assert not s0.requires_grad and not s1.requires_grad and s2.requires_grad
    for s, a in ((s1, a1), (s2, a2)):
        assert torch.equal(s0.view(torch.int32), s.detach().view(torch.int32))
        assert torch.equal(a0.view(torch.int32), a.detach().view(torch.int32))
    gm.return_similarity = True
    s3, a3, (loc_sim, loc_dis) = gm(x.clone().requires_grad_(True))
    assert torch.equal(s0.view(torch.int32), s3.detach().view(torch.int32)) and len(loc_sim) == len(loc_dis) == 10
    assert all(t.requires_grad for t in loc_sim) and [t.shape[1] for t in loc_sim] == [max(int(n), 1) for n in G6["ntok"]] + [1]


# ----------------------------------------------------------------------------------------------------------------------
# 3. the predictor, built from a config, against the float64 restatement
# ----------------------------------------------------------------------------------------------------------------------
def _predictor(pkg, D, metric="dot", detach=False, classes=1203, c5=256):
    cfg = pkg.config.get_cfg()
    cfg.MODEL.ROI_BOX_HEAD.NAME = "EmbeddingGroundingFastRCNNOutputLayers"
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = D
    cfg.MODEL.ROI_BOX_HEAD.NORMALIZE_EMB_PRED = metric == "cosine"
    cfg.MODEL.MMSS_HEAD.GROUNDING.LOCAL_METRIC = metric
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = classes
    cfg.MODEL.ROI_HEADS.DETACH_CLASS_PREDICTOR = detach
    torch.manual_seed(11)
    pred = pkg.build_box_predictor(cfg, c5).cuda().train()
    rng = np.random.default_rng(4)
    ntok = rng.integers(1, 5, size=classes)
    embs = {k: (rng.standard_normal((n, D)) * 0.2).astype(np.float32) for k, n in enumerate(ntok)}
    pred.set_class_embeddings({k: torch.from_numpy(v) for k, v in embs.items()})
    with torch.no_grad():
        pred.bbox_pred.bias.normal_(std=0.01)
        pred.emb_pred.bias.normal_(std=0.01)
    temp = float(cfg.MODEL.MMSS_HEAD.GROUNDING.ALIGNMENT_TEMPERATURE)
    return pred, [embs[k] for k in range(classes)], temp, rng


@pytest.mark.parametrize("D", [64, 768])
@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_predictor_gradients_match_float64(pkg, D, metric):
    pred, embs, temp, rng = _predictor(pkg, D, metric)
    R = 96
    x_np = np.maximum(rng.standard_normal((R, 256)), 0).astype(np.float32)
    labels = torch.from_numpy(rng.integers(0, 1204, size=R))
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    scores, deltas = pred(x)
    assert scores.requires_grad and deltas.requires_grad and tuple(scores.shape) == (R, 1204)
    (F.cross_entropy(scores, labels.cuda()) + deltas.sum()).backward()
    # float64
    p64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in pred.named_parameters() if k.startswith(("emb_pred", "bbox_pred"))}
    x64 = torch.from_numpy(x_np).double().requires_grad_(True)
    emb = x64 @ p64["emb_pred.weight"].t() + p64["emb_pred.bias"]
    if metric == "cosine":
        emb = token_ref.normalize(emb)
    r_scores, _, _ = token_ref.grounding_module(emb, embs, metric, "softmax", temp)
    r_deltas = x64 @ p64["bbox_pred.weight"].t() + p64["bbox_pred.bias"]
    (F.cross_entropy(r_scores, labels) + r_deltas.sum()).backward()
    np.testing.assert_allclose(scores.detach().cpu().numpy(), r_scores.detach().numpy(), atol=1e-4)   # (test_gpu_grounding_predictor.py's gate)
    assert_grad(x.grad, x64.grad, f"D={D} {metric} x")
    for k, v in p64.items():
        got = dict(pred.named_parameters())[k].grad
        assert got is not None, k
        assert_grad(got, v.grad, f"D={D} {metric} {k}")
    assert all(p.grad is None for p in pred.cls_score.parameters())           # the token bank is frozen (:255-256)


def test_detached_class_predictor_keeps_the_bbox_pred_gradient(pkg):
    pred, _, _, rng = _predictor(pkg, 64, detach=True)
    assert pred.loss_weight["loss_cls"] == 0.0
    x_np = np.maximum(rng.standard_normal((50, 256)), 0).astype(np.float32)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    scores, deltas = pred(x)
    assert not scores.requires_grad and deltas.requires_grad
    deltas.sum().backward()
    assert pred.emb_pred.weight.grad is None and pred.emb_pred.bias.grad is None
    w64 = pred.bbox_pred.weight.detach().double().cpu()
    assert_grad(pred.bbox_pred.weight.grad, torch.from_numpy(x_np).double().sum(0, keepdim=True).expand(4, -1), "bbox_pred.weight")
    assert_grad(pred.bbox_pred.bias.grad, torch.full((4,), 50.0, dtype=torch.float64), "bbox_pred.bias")
    assert_grad(x.grad, w64.sum(0, keepdim=True).expand(50, -1), "x")


# ----------------------------------------------------------------------------------------------------------------------
# 4. / 5. an STT fine-tune step (configs/coco_stt.yaml) through the predictor
# ----------------------------------------------------------------------------------------------------------------------
# sizes of tests/test_gpu_stt.py: "small" keeps the suite fast; "coco_stt" = the config itself
SIZES = {"small": dict(res2=32, width=8, dim=96, batch=32, mid=64),
         "coco_stt": dict(res2=256, width=64, dim=768, batch=512, mid=512)}


def _stt_heads(pkg, oracle, predictor, backend, dtype, size, bank, temperature=None):
    """EmbeddingRes5ROIHeads of the STT stage with `predictor`; bank: [K+1, D] matrix (single-vector) or {class: [n, D]}."""
    from locov_amd.structures import ShapeSpec
    sz = SIZES[size]
    cfg = pkg.config.get_cfg()
    cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = sz["res2"]
    cfg.MODEL.RESNETS.WIDTH_PER_GROUP = sz["width"]
    cfg.MODEL.ROI_HEADS.NAME = "EmbeddingRes5ROIHeads"                      # coco_stt.yaml:18
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = BASE                                 # :20
    cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION = 1.0                            # :25
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = sz["batch"]
    cfg.MODEL.ROI_BOX_HEAD.NAME = predictor
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True                    # :29
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = sz["dim"]
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True                          # :33
    cfg.MODEL.ROI_BOX_HEAD.FREEZE_EMB_PRED = True                          # :36
    cfg.MODEL.ROI_BOX_HEAD.RES5_BACKEND = backend
    cfg.MODEL.ROI_BOX_HEAD.RES5_DTYPE = dtype
    if temperature is not None:
        cfg.MODEL.MMSS_HEAD.GROUNDING.ALIGNMENT_TEMPERATURE = temperature
    c_in = cfg.MODEL.RESNETS.RES2_OUT_CHANNELS * 4
    torch.manual_seed(3)
    heads = pkg.build_roi_heads(cfg, {"res4": ShapeSpec(channels=c_in, stride=16)})
    heads.res5.load_state_dict(oracle.make_res5_params(9, in_ch=c_in, mid=sz["mid"], out_ch=heads.output_shape))
    head = oracle.synth_head(np.random.default_rng(9), heads.output_shape, sz["dim"], BASE)
    with torch.no_grad():
        heads.box_predictor.emb_pred.weight.copy_(torch.from_numpy(head["emb_w"]))
        heads.box_predictor.emb_pred.bias.zero_()
        heads.box_predictor.bbox_pred.weight.copy_(torch.from_numpy(head["bbox_w"]))
        heads.box_predictor.bbox_pred.bias.zero_()
    # FREEZE_EMB_PRED is read by the single-vector predictor only (the reference's grounding predictor accepts the argument and
    # never reads it, box_emb_grounding_head.py:283); the STT stage freezes emb_pred, so the test does it for both
    for p in heads.box_predictor.emb_pred.parameters():
        p.requires_grad_(False)
    heads = heads.cuda().train(True)
    heads.box_predictor.set_class_embeddings(bank(head) if callable(bank) else bank)
    heads.num_classes = heads.box_predictor.num_classes
    assert heads.num_classes == BASE
    return heads, c_in


def _batch(oracle, n_img, r, n_gt, seed):
    from locov_amd.structures import Boxes, Instances
    rng = np.random.default_rng(seed)
    props, targets = [], []
    for _ in range(n_img):
        gt = oracle.synth_boxes(rng, n_gt)
        gt[:, 2:] = np.maximum(gt[:, 2:], gt[:, :2] + 24.0)
        b = oracle.synth_boxes(rng, r)
        b[:n_gt] = gt + rng.uniform(-4, 4, gt.shape).astype(np.float32)
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1.0)
        p = Instances((800, 1333))
        p.proposal_boxes = Boxes(torch.from_numpy(b).cuda())
        p.objectness_logits = torch.zeros(r, device="cuda")
        t = Instances((800, 1333))
        t.gt_boxes = Boxes(torch.from_numpy(gt).cuda())
        t.gt_classes = torch.from_numpy(rng.integers(0, BASE, n_gt)).cuda()
        props.append(p)
        targets.append(t)
    return props, targets


def _step(heads, c_in, oracle, n_props, which):
    feat = torch.randn(3, c_in, 50, 84, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    props, targets = _batch(oracle, 3, n_props, 6, seed=17)
    torch.manual_seed(77)
    out, losses = heads(None, {"res4": feat}, props, targets)
    assert out == [] and set(losses) == {"loss_cls", "loss_box_reg"}
    which(losses).backward()
    grads = {k: p.grad.clone() for k, p in heads.named_parameters() if p.grad is not None}
    return float(losses["loss_cls"].detach()), float(losses["loss_box_reg"].detach()), feat.grad.clone(), grads


def _assert_steps_agree(a, b):
    (ca, ba, fa, pa), (cb, bb, fb, pb) = a, b
    print(f"loss_cls {ca:.7g} / {cb:.7g}   loss_box_reg {ba:.7g} / {bb:.7g}")
    assert abs(ca - cb) <= 2e-4 * max(abs(cb), 1e-3) and abs(ba - bb) <= 2e-4 * max(abs(bb), 1e-3)
    rel_l2 = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30))
    assert float(fb.abs().max()) > 0 and rel_l2(fa, fb) < 5e-3, rel_l2(fa, fb)
    assert set(pa) == set(pb), set(pa) ^ set(pb)
    worst = max((rel_l2(pa[k], pb[k]), k) for k in pa)
    print("worst relative L2 of a parameter gradient:", worst, " res4:", rel_l2(fa, fb))
    assert worst[0] < 5e-3, worst


@pytest.mark.parametrize("dtype,size,n_props", [("fp32", "small", 80), ("f16x2", "small", 80), ("f16x2", "coco_stt", 1000)])
def test_one_token_per_class_at_temperature_one_is_the_single_vector_predictor(pkg, oracle, dtype, size, n_props):
    """Tmax = 1 (no padded slot): the softmax over one slot is 1, the module's scores are emb . bank^T and the background column is 0
    -- the single-vector bank's zero row.  The STT step with either predictor on the same weights: same losses, same gradients."""
    both = (lambda l: l["loss_cls"] + l["loss_box_reg"])
    single, c_in = _stt_heads(pkg, oracle, "EmbeddingFastRCNNOutputLayers", "hip", dtype, size, lambda head: torch.from_numpy(head["cls_w"]))
    bank = single.box_predictor.cls_score.weight.detach().cpu()
    assert bool((bank[-1] == 0).all())
    want = _step(single, c_in, oracle, n_props, both)
    multi, _ = _stt_heads(pkg, oracle, "EmbeddingGroundingFastRCNNOutputLayers", "hip", dtype, size,
                          {k: bank[k:k + 1].clone() for k in range(BASE)}, temperature=1.0)
    gm = multi.box_predictor.cls_score
    assert tuple(gm.mask_emb.shape) == (BASE + 1, 1) and not gm._padded
    # the module itself: scores = emb . bank^T, background column 0
    emb = torch.randn(64, bank.shape[1], generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        scores, _ = gm(emb)
    from locov_amd import ops
    assert torch.equal(scores[:, :BASE], ops.linear(emb, bank.cuda())[:, :BASE]) and bool((scores[:, BASE] == 0).all())
    got = _step(multi, c_in, oracle, n_props, both)
    assert "box_predictor.bbox_pred.weight" in got[3] and any(k.startswith("res5.") for k in got[3])
    assert not any(k.startswith("box_predictor.emb_pred") for k in got[3])
    _assert_steps_agree(got, want)


@pytest.mark.parametrize("dtype", ["fp32", "f16x2"])
def test_stt_step_with_multi_token_names_trains_res5_through_loss_cls(pkg, oracle, dtype):
    """48 classes of 1-4 tokens.  loss_cls.backward() ALONE reaches every Res5 weight and res4 through the multi-token class
    predictor; emb_pred (frozen, coco_stt.yaml:36) gets nothing; the hand-written Res5 and the stock library path agree."""
    D = SIZES["small"]["dim"]
    rng = np.random.default_rng(31)
    embs = {k: torch.from_numpy((rng.standard_normal((n, D)) * 0.5).astype(np.float32)) for k, n in enumerate(rng.integers(1, 5, size=BASE))}
    assert max(e.shape[0] for e in embs.values()) == 4 and min(e.shape[0] for e in embs.values()) == 1
    outs = {}
    for backend in ("miopen", "hip"):
        heads, c_in = _stt_heads(pkg, oracle, "EmbeddingGroundingFastRCNNOutputLayers", backend, dtype, "small", embs)
        assert tuple(heads.box_predictor.cls_score.mask_emb.shape) == (BASE + 1, 4)
        outs[backend] = c, b, fgrad, grads = _step(heads, c_in, oracle, 80, lambda l: l["loss_cls"])
        assert np.isfinite(c) and float(fgrad.abs().max()) > 0, backend                      # res4
        trainable = [k for k, p in heads.named_parameters() if k.startswith("res5.") and p.requires_grad]
        assert trainable
        for k in trainable:
            assert k in grads and float(grads[k].abs().max()) > 0, (backend, k)             # every Res5 weight
        assert not any(k.startswith("box_predictor.emb_pred") for k in grads)                # frozen
        assert not any(k.startswith("box_predictor.cls_score") for k in grads)               # the token bank
        g = grads.get("box_predictor.bbox_pred.weight")
        assert g is None or float(g.abs().max()) == 0                                        # loss_cls does not see bbox_pred
    _assert_steps_agree(outs["hip"], outs["miopen"])
