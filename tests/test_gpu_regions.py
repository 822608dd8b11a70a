"""GPU tests of the grounding branches' region assembly (locov_amd.mmss_regions -> ops -> locov_regions_* -> csrc/regions.hip)
against tests/regions_ref.py, the restatement of distill_prop_mmss_gcnn.py:273-328 / :348-399 fed the permutation the keys stand
for.  The forward only copies values and forms one IEEE quotient per coordinate, the backward only copies gradient rows into
zeros, so every comparison is bit for bit."""
import types

import numpy as np
import pytest
import torch

import regions_ref

pytestmark = pytest.mark.gpu

GH, GW, PADDED = 25, 42, (800, 1344)          # the LSM grid of a 1333 x 800 batch (stride 32)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _same(got, want, what=""):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, got.shape, want.shape)
    assert _bits(got) == _bits(want), what


def _sizes(B, rng, small=False):
    """Ragged image sizes: the first fills the padded batch, one sits a pixel over a cell boundary."""
    if small:
        return [(int(rng.integers(20, 64)), int(rng.integers(20, 96))) for _ in range(B)]          # <= 2 x 3 valid cells
    out = [PADDED, (33, 65)] + [(int(rng.integers(300, 801)), int(rng.integers(400, 1345))) for _ in range(B)]
    return out[:B]


def _grid_feat(B, C, layout, rng, requires_grad=False):
    """(leaf, logical [B, C, GH, GW] tensor on the device in the given memory layout, CPU copy of the values in NCHW)."""
    vals = torch.from_numpy(rng.standard_normal((B, C, GH, GW)).astype(np.float32))
    if layout == "nchw":
        leaf = vals.cuda().requires_grad_(requires_grad)
        return leaf, leaf, vals
    leaf = vals.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(requires_grad)
    return leaf, leaf.permute(0, 3, 1, 2), vals


def _check_dict(got, want, n_feat=None):
    assert set(got) == {"region_features", "region_mask", "region_loc", "mvm_mask", "target_region_features"}
    assert got["target_region_features"] is got["region_features"]
    assert got["region_mask"].dtype == torch.uint8 and got["region_loc"].dtype == torch.float32 and got["mvm_mask"].dtype == torch.float32
    for k in ("region_features", "region_mask", "region_loc", "mvm_mask"):
        assert got[k].is_cuda
        _same(got[k], want[k], k)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("B", [1, 2, 4, 32])
@pytest.mark.parametrize("spatial_dropout", [0, 7, 100])
def test_grid_regions_equal_the_reference(pkg, layout, B, spatial_dropout):
    rng = np.random.default_rng(100 * B + spatial_dropout)
    C = 2048 if B == 4 else 72
    sizes = _sizes(B, rng)
    _, feat, vals = _grid_feat(B, C, layout, rng)
    keys = rng.random((B, GH * GW))
    ext = regions_ref.grid_extents(sizes, PADDED, GH, GW)
    want = regions_ref.grid_regions(vals, sizes, PADDED, spatial_dropout, True, regions_ref.grid_perms(keys, ext, GW))
    got = pkg.grid_regions(feat, sizes, PADDED, spatial_dropout, True, keys=torch.from_numpy(keys).cuda())
    _check_dict(got, want)
    if spatial_dropout == 0:
        assert got["region_features"].data_ptr() == feat.data_ptr()               # a view, no kernel
    else:
        assert tuple(got["region_mask"].shape) == (B, spatial_dropout) and tuple(got["mvm_mask"].shape) == (B, GH * GW)
    # outside training :302 is not taken whatever SPATIAL_DROPOUT says
    _check_dict(pkg.grid_regions(feat, sizes, PADDED, spatial_dropout, False), regions_ref.grid_regions(vals, sizes, PADDED, spatial_dropout, False))


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("spatial_dropout", [7, 100])
def test_grid_with_fewer_valid_cells_than_spatial_dropout(pkg, layout, spatial_dropout):
    """Every image has at most 6 valid cells: the features have the padded length, the mask the configured width (:305)."""
    rng = np.random.default_rng(5)
    B, C = 3, 40
    sizes = _sizes(B, rng, small=True)
    _, feat, vals = _grid_feat(B, C, layout, rng)
    keys = rng.random((B, GH * GW))
    ext = regions_ref.grid_extents(sizes, PADDED, GH, GW)
    n = max(int(h) * int(w) for h, w in ext)
    assert n < spatial_dropout
    want = regions_ref.grid_regions(vals, sizes, PADDED, spatial_dropout, True, regions_ref.grid_perms(keys, ext, GW))
    got = pkg.grid_regions(feat, sizes, PADDED, spatial_dropout, True, keys=torch.from_numpy(keys).cuda())
    _check_dict(got, want)
    assert tuple(got["region_features"].shape) == (B, n, C) and tuple(got["region_mask"].shape) == (B, spatial_dropout)
    # mixed: one image with plenty of cells next to the small ones
    sizes[1] = (640, 1000)
    ext = regions_ref.grid_extents(sizes, PADDED, GH, GW)
    want = regions_ref.grid_regions(vals, sizes, PADDED, spatial_dropout, True, regions_ref.grid_perms(keys, ext, GW))
    _check_dict(pkg.grid_regions(feat, sizes, PADDED, spatial_dropout, True, keys=torch.from_numpy(keys).cuda()), want)


def _proposals(pkg, lengths, rng, sizes=None):
    from locov_amd.structures import Boxes, Instances
    props = []
    for i, r in enumerate(lengths):
        h, w = sizes[i] if sizes else (int(rng.integers(300, 801)), int(rng.integers(400, 1334)))
        b = np.zeros((r, 4), np.float32)
        b[:, 0], b[:, 1] = rng.uniform(0, w - 2, r), rng.uniform(0, h - 2, r)
        b[:, 2], b[:, 3] = b[:, 0] + rng.uniform(1, w / 2, r), b[:, 1] + rng.uniform(1, h / 2, r)
        p = Instances((h, w))
        p.proposal_boxes = Boxes(torch.from_numpy(b).cuda())
        props.append(p)
    return props


@pytest.mark.parametrize("as_list", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("lengths", [[200, 200, 200, 200], [200, 37, 150], [5, 1, 9], [300], [130, 180]])
def test_box_regions_equal_the_reference(pkg, as_list, training, lengths):
    rng = np.random.default_rng(sum(lengths))
    C, sd = 2048 if len(lengths) == 3 else 68, 100
    props = _proposals(pkg, lengths, rng)
    vals = torch.from_numpy(rng.standard_normal((sum(lengths), C)).astype(np.float32))
    keys = rng.random(sum(lengths))
    want, chosen = regions_ref.box_regions(list(vals.split(lengths)), [p.proposal_boxes.tensor.cpu() for p in props],
                                           [p.image_size for p in props], sd, training, regions_ref.box_perms(keys, lengths))
    feats = vals.cuda()
    arg = list(feats.split(lengths)) if as_list else feats
    got, idx = pkg.box_regions(arg, props, sd, training, keys=torch.from_numpy(keys).cuda())
    _check_dict(got, want)
    n = min(lengths) if not training else min(min(lengths), sd)
    assert tuple(got["region_features"].shape) == (len(lengths), n, C) and bool(got["region_mask"].all())
    assert idx.dtype == torch.int64 and idx.is_cuda and idx.cpu().tolist() == [c.tolist() for c in chosen]
    # separately allocated per-image tensors (no common storage): concatenated, the same result
    got2, idx2 = pkg.box_regions([t.clone() for t in feats.split(lengths)], props, sd, training, keys=torch.from_numpy(keys).cuda())
    _check_dict(got2, want)
    assert torch.equal(idx2, idx)


def test_duplicate_keys_fall_back_to_the_candidate_index(pkg):
    rng = np.random.default_rng(11)
    B, C = 2, 64
    sizes = _sizes(B, rng)
    _, feat, vals = _grid_feat(B, C, "channels_last", rng)
    keys = np.round(rng.random((B, GH * GW)) * 8) / 8                    # 9 distinct values over 1 050 cells
    keys[1] = 0.5                                                          # all equal: the first cells in index order
    ext = regions_ref.grid_extents(sizes, PADDED, GH, GW)
    perms = regions_ref.grid_perms(keys, ext, GW)
    assert perms[1].tolist() == sorted(perms[1].tolist())
    _check_dict(pkg.grid_regions(feat, sizes, PADDED, 100, True, keys=torch.from_numpy(keys).cuda()),
                regions_ref.grid_regions(vals, sizes, PADDED, 100, True, perms))
    lengths = [50, 30]
    props = _proposals(pkg, lengths, rng)
    bvals = torch.from_numpy(rng.standard_normal((80, C)).astype(np.float32))
    bkeys = np.round(rng.random(80) * 4) / 4
    want, chosen = regions_ref.box_regions(list(bvals.split(lengths)), [p.proposal_boxes.tensor.cpu() for p in props],
                                           [p.image_size for p in props], 20, True, regions_ref.box_perms(bkeys, lengths))
    got, idx = pkg.box_regions(bvals.cuda(), props, 20, True, keys=torch.from_numpy(bkeys).cuda())
    _check_dict(got, want)
    assert idx.cpu().tolist() == [c.tolist() for c in chosen]


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("case", ["full", "padded"])
def test_grid_backward_equals_autograd_through_the_index_chain(pkg, layout, case):
    rng = np.random.default_rng(21)
    B, C, sd = 4, 2048 if case == "full" else 36, 100
    sizes = _sizes(B, rng)
    if case == "padded":
        sizes[2] = (40, 70)                                                # 2 x 3 valid cells: 94 padding slots
    keys = rng.random((B, GH * GW))
    perms = regions_ref.grid_perms(keys, regions_ref.grid_extents(sizes, PADDED, GH, GW), GW)
    leaf, feat, vals = _grid_feat(B, C, layout, rng, requires_grad=True)
    up = torch.from_numpy(rng.standard_normal((B, sd, C)).astype(np.float32)).cuda()
    strides = []
    if feat is not leaf:
        feat.register_hook(lambda g: strides.append(g.stride()))
    grads = []
    for _ in range(2):
        leaf.grad = None
        pkg.grid_regions(feat, sizes, PADDED, sd, True, keys=torch.from_numpy(keys).cuda())["region_features"].backward(up)
        grads.append(leaf.grad.clone())
    assert _bits(grads[0]) == _bits(grads[1])                              # reproducible bits
    if layout == "channels_last":
        assert strides and all(s == feat.stride() for s in strides)       # autograd's permute-backward stays a view
    # torch autograd through reshape / permute / index / pad_sequence on the same indices, on the device
    ref_leaf = vals.cuda().requires_grad_(True)
    regions_ref.grid_regions(ref_leaf, sizes, PADDED, sd, True, perms)["region_features"].backward(up)
    want = ref_leaf.grad if layout == "nchw" else ref_leaf.grad.permute(0, 2, 3, 1)
    _same(leaf.grad, want.contiguous())
    # a row that was not selected has gradient exactly zero
    g = leaf.grad if layout == "nchw" else leaf.grad.permute(0, 3, 1, 2)
    chosen = torch.zeros(B, GH * GW, dtype=torch.bool)
    for i, p in enumerate(perms):
        chosen[i, torch.from_numpy(p[:sd].copy())] = True
    per_cell = g.reshape(B, C, GH * GW).abs().amax(dim=1).cpu()
    assert float(per_cell[~chosen].max()) == 0.0 and bool((per_cell[chosen] > 0).all())


@pytest.mark.parametrize("as_list", [True, False])
def test_box_backward_equals_autograd_through_the_index_chain(pkg, as_list):
    rng = np.random.default_rng(22)
    lengths, C, sd = [200, 37, 150], 2048, 100
    props = _proposals(pkg, lengths, rng)
    vals = torch.from_numpy(rng.standard_normal((sum(lengths), C)).astype(np.float32))
    keys = rng.random(sum(lengths))
    up = torch.from_numpy(rng.standard_normal((3, 37, C)).astype(np.float32)).cuda()
    grads = []
    for _ in range(2):
        leaf = vals.cuda().requires_grad_(True)
        src = leaf * 1.0                                                   # (a non-leaf, as the heads' box features are)
        arg = list(src.split(lengths)) if as_list else src
        out, idx = pkg.box_regions(arg, props, sd, True, keys=torch.from_numpy(keys).cuda())
        out["region_features"].backward(up)
        grads.append(leaf.grad.clone())
    assert _bits(grads[0]) == _bits(grads[1])
    ref = vals.cuda().requires_grad_(True)
    want, chosen = regions_ref.box_regions(list(ref.split(lengths)), [p.proposal_boxes.tensor for p in props], [p.image_size for p in props], sd,
                                           True, regions_ref.box_perms(keys, lengths))
    want["region_features"].backward(up)
    _same(grads[0], ref.grad)
    rows = torch.zeros(sum(lengths), dtype=torch.bool)
    for off, c in zip(np.cumsum([0] + lengths[:-1]), chosen):
        rows[torch.from_numpy(off + c)] = True
    assert float(grads[0].cpu()[~rows].abs().max()) == 0.0


def test_default_keys_select_every_valid_cell_equally_often(pkg):
    """A guard against a broken ranking, not a measurement: 2 000 seeded draws on a 3 x 4 grid, SPATIAL_DROPOUT 5; a valid cell is
    selected with probability p = 5 / valid per draw, so its count is Binomial(n, p) with sigma = sqrt(n p (1 - p)); every count
    must lie within 5 sigma of n p, and no invalid cell may ever be selected."""
    draws, sd, gh, gw = 2000, 5, 3, 4
    padded, sizes = (96, 128), [(96, 128), (64, 90)]                       # extents 3 x 4 (12 valid) and 2 x 3 (6 valid)
    ext = regions_ref.grid_extents(sizes, padded, gh, gw)
    assert ext.tolist() == [[3, 4], [2, 3]]
    cell_id = torch.arange(1, gh * gw + 1, dtype=torch.float32).reshape(1, 1, gh, gw).expand(2, 4, gh, gw).contiguous().cuda()
    torch.manual_seed(20240229)
    outs = []
    for _ in range(draws):
        d = pkg.grid_regions(cell_id, sizes, padded, sd, True)
        assert tuple(d["region_features"].shape) == (2, sd, 4)
        outs.append(d["region_features"][:, :, 0])
    picked = torch.stack(outs).cpu().numpy().astype(np.int64) - 1          # [draws, 2, sd] cell indices
    assert len({tuple(r) for r in picked[:, 0]}) > draws // 2              # the draws differ
    for i in range(2):
        counts = np.bincount(picked[:, i].reshape(-1), minlength=gh * gw)
        valid = np.array([(c // gw < ext[i, 0]) and (c % gw < ext[i, 1]) for c in range(gh * gw)])
        assert counts[~valid].sum() == 0, counts
        assert all(len(set(r)) == sd for r in picked[:, i])                # no cell twice in one draw
        p = sd / valid.sum()
        sigma = np.sqrt(draws * p * (1 - p))
        assert np.abs(counts[valid] - draws * p).max() <= 5 * sigma, (counts, draws * p, sigma)


def test_no_host_wait(pkg):
    rng = np.random.default_rng(31)
    B, C, lengths = 4, 256, [200, 180, 200, 64]
    sizes = _sizes(B, rng)
    props = _proposals(pkg, lengths, rng)
    box = torch.from_numpy(rng.standard_normal((sum(lengths), C)).astype(np.float32)).cuda().requires_grad_(True)
    gkeys, bkeys = torch.from_numpy(rng.random((B, GH * GW))).cuda(), torch.from_numpy(rng.random(sum(lengths))).cuda()
    for layout in ("nchw", "channels_last"):
        leaf, feat, _ = _grid_feat(B, C, layout, rng, requires_grad=True)

        def step():
            g = pkg.grid_regions(feat, sizes, PADDED, 100, True, keys=gkeys)
            b, idx = pkg.box_regions(list((box * 1.0).split(lengths)), props, 100, True, keys=bkeys)
            (g["region_features"].sum() + b["region_features"].sum()).backward()
            pkg.grid_regions(feat, sizes, PADDED, 0, True)
            return g, b, idx
        step()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
def _grounding_cfg():
    ns = types.SimpleNamespace
    g = ns(LOCAL_METRIC="dot", GLOBAL_METRIC="aligned_local", ALIGNMENT="softmax", ALIGNMENT_TEMPERATURE=10.0,
           LOSS="cross_entropy", NEGATIVE_MINING="random", TRIPLET_MARGIN=1.0, ALIGN_WORDS_TO_REGIONS=True,
           ALIGN_REGIONS_TO_WORDS=True, TEXT_INPUT="input_embeddings")
    return ns(MODEL=ns(MMSS_HEAD=ns(GROUNDING=g, DISTILLATION_LOSS=True)))


def _heads(pkg, oracle, layout):
    """The small Res5 of smoke() (128 -> (64) -> 256) under EmbeddingProposalsRes5ROIHeads in training mode."""
    from locov_amd.structures import ShapeSpec
    cfg = pkg.config.get_cfg()
    cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = 32
    cfg.MODEL.RESNETS.WIDTH_PER_GROUP = 8
    cfg.MODEL.ROI_BOX_HEAD.EMB_DIM = 96
    cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG = True
    cfg.MODEL.ROI_BOX_HEAD.EMBEDDING_BASED = True
    cfg.MODEL.ROI_BOX_HEAD.FREEZE_EMB_PRED = False
    cfg.MODEL.ROI_HEADS.NAME = "EmbeddingProposalsRes5ROIHeads"
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 24
    cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION = 1.0
    cfg.MODEL.ROI_HEADS.DETACH_CLASS_PREDICTOR = True
    if layout is not None:
        cfg.MODEL.ROI_BOX_HEAD.GRID_FEATURES_LAYOUT = layout
    torch.manual_seed(3)
    heads = pkg.build_roi_heads(cfg, {"res4": ShapeSpec(channels=128, stride=16)})
    heads.res5.load_state_dict(oracle.make_res5_params(9, in_ch=128, mid=64, out_ch=heads.output_shape))
    h = oracle.synth_head(np.random.default_rng(9), heads.output_shape, 96, 80)
    heads = heads.cuda().train()
    heads.box_predictor.set_class_embeddings(h["cls_w"])
    heads.num_classes = heads.box_predictor.num_classes
    return heads


def _batch(oracle, n_img, r, n_gt, seed):
    from locov_amd.structures import Boxes, Instances
    rng = np.random.default_rng(seed)
    props, targets = [], []
    for _ in range(n_img):
        gt = oracle.synth_boxes(rng, n_gt)
        b = oracle.synth_boxes(rng, r)
        b[:n_gt] = gt + rng.uniform(-4, 4, gt.shape).astype(np.float32)
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1.0)
        p, t = Instances((800, 1333)), Instances((800, 1333))
        p.proposal_boxes, p.objectness_logits = Boxes(torch.from_numpy(b).cuda()), torch.zeros(r, device="cuda")
        t.gt_boxes, t.gt_classes = Boxes(torch.from_numpy(gt).cuda()), torch.from_numpy(rng.integers(0, 80, n_gt)).cuda()
        props.append(p)
        targets.append(t)
    return props, targets


def _lsm_step(pkg, oracle, layout, middle):
    """ROI heads (training) -> region dictionaries -> GroundingHead with distributions (grid and boxes) -> backward.
    middle "fused": grid_regions / box_regions; "chain": the torch statement chain of regions_ref on the device tensors."""
    from locov_amd.grounding_head import GroundingHead
    heads = _heads(pkg, oracle, layout)
    ghead = GroundingHead(_grounding_cfg(), heads.output_shape, 96).cuda()
    ghead.v2l_projection = heads.box_predictor.emb_pred                      # tied, as LOAD_EMB_PRED_FROM_MMSS_HEAD ties them
    feat = torch.randn(2, 128, 50, 84, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    props, targets = _batch(oracle, 2, 60, 5, seed=31)
    sizes, sd = [(800, 1333), (704, 1100)], 100
    rng = np.random.default_rng(41)
    T = 12
    attn, special = np.ones((2, T), np.int64), np.zeros((2, T), np.int64)
    special[:, 0], special[0, 9:], attn[0, 10:] = 1, 1, 0
    special[1, -1] = 1
    cap = {"input_embeddings": torch.from_numpy(rng.standard_normal((2, T, 96)).astype(np.float32) * 0.1).cuda(),
           "attention_mask": torch.from_numpy(attn).cuda(), "special_tokens_mask": torch.from_numpy(special).cuda()}
    gkeys = rng.random((2, GH * GW))
    torch.manual_seed(77)                                                     # the proposal sampler draws from the global RNG
    grid, box_feats, sampled, losses = heads(None, {"res4": feat}, props, targets)
    assert tuple(grid.shape) == (2, heads.output_shape, GH, GW)
    lengths = [len(p) for p in sampled]
    bkeys = rng.random(sum(lengths))
    if middle == "fused":
        img = pkg.grid_regions(grid, sizes, PADDED, sd, True, keys=torch.from_numpy(gkeys).cuda())
        box, _ = pkg.box_regions(box_feats, sampled, sd, True, keys=torch.from_numpy(bkeys).cuda())
    else:
        img = regions_ref.grid_regions(grid, sizes, PADDED, sd, True, regions_ref.grid_perms(gkeys, regions_ref.grid_extents(sizes, PADDED, GH, GW), GW))
        box, _ = regions_ref.box_regions(box_feats, [p.proposal_boxes.tensor for p in sampled], [p.image_size for p in sampled], sd, True,
                                         regions_ref.box_perms(bkeys, lengths))
    out = dict(losses)
    for tag, d in (("", img), ("Box ", box)):
        _, l, dist = ghead(d, cap)
        out.update({tag + k: v for k, v in l.items()})
        out.update({tag + k: v for k, v in dist.items()})
    total = sum(v for k, v in out.items() if v.dim() == 0)
    return heads, feat, grid, out, total


def _run(pkg, oracle, layout, middle):
    heads, feat, grid, out, total = _lsm_step(pkg, oracle, layout, middle)
    total.backward()
    grads = {k: p.grad.clone() for k, p in heads.named_parameters() if p.grad is not None}
    return grid.detach(), {k: v.detach() for k, v in out.items()}, feat.grad.clone(), grads


def test_end_to_end_equals_the_torch_statement_chain(pkg, oracle):
    """Both sides run the same kernels around an assembly that only copies values: bit-identity.  (Were it ever to fail, the
    ceiling for any tolerance is tests/test_gpu_grounding.py's whole-head comparison, rtol 1e-3 / atol 2e-6, two fp32 evaluations
    of the same head -- after finding out which launch differs.)"""
    _, out_f, fg_f, pg_f = _run(pkg, oracle, "nchw", "fused")
    _, out_c, fg_c, pg_c = _run(pkg, oracle, "nchw", "chain")
    assert set(out_f) == set(out_c) and any(k.startswith("Box CE_loss") for k in out_f) and "loss_cls" in out_f
    for k in out_f:
        _same(out_f[k], out_c[k], k)
    assert "box_predictor.emb_pred.weight" in pg_f and float(pg_f["box_predictor.emb_pred.weight"].abs().max()) > 0
    _same(pg_f["box_predictor.emb_pred.weight"], pg_c["box_predictor.emb_pred.weight"], "emb_pred.weight")
    _same(fg_f, fg_c, "res4 gradient")
    assert set(pg_f) == set(pg_c)
    for k in pg_f:
        _same(pg_f[k], pg_c[k], k)


def test_channels_last_grid_features_are_the_same_values_without_the_transposes(pkg, oracle):
    from torch.profiler import ProfilerActivity, profile
    res, kernels = {}, {}
    for layout in ("nchw", "channels_last"):
        _run(pkg, oracle, layout, "fused")                                   # warm-up (operand caches, allocator)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            res[layout] = _run(pkg, oracle, layout, "fused")
            torch.cuda.synchronize()
        kernels[layout] = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    (g_n, out_n, fg_n, pg_n), (g_c, out_c, fg_c, pg_c) = res["nchw"], res["channels_last"]
    assert g_n.is_contiguous() and tuple(g_c.shape) == tuple(g_n.shape) and g_c.stride(1) == 1 and not g_c.is_contiguous()
    _same(g_c.contiguous(), g_n, "visual_grid_features")
    for k in out_n:
        _same(out_c[k], out_n[k], k)
    _same(fg_c, fg_n, "res4 gradient")
    assert set(pg_c) == set(pg_n)
    for k in pg_n:
        _same(pg_c[k], pg_n[k], k)
    # one transpose kernel serves both directions (nchw_to_nhwc_kernel): the res4 map's own pair stays, the grid output's pair goes
    count = {k: sum("nchw_to_nhwc" in n or "nhwc_to_nchw" in n for n in v) for k, v in kernels.items()}
    print("transpose launches per step:", count)
    assert count["nchw"] - count["channels_last"] == 2 and count["channels_last"] == 2, count
    assert any("regions_gather_nchw" in n for n in kernels["nchw"]) and not any("regions_gather_nchw" in n for n in kernels["channels_last"])
    assert any("regions_gather_rows" in n for n in kernels["channels_last"]) and any("regions_select" in n for n in kernels["channels_last"])
