"""The inputs of the ROIAlign-forward tests (tests/test_gpu_roi_align_fwd.py runs the kernels on them, tests/test_roi_align_ref.py
measures the fp32 oracle's distance from the float64 reference on the same inputs and checks the conditions without a GPU).
numpy only.

A case is a dict: `entry` ("nhwc": the even-grid pooler ops.roi_align_nhwc; "contract": ops.roi_align, modes exact and fast), the
shapes (N, H, W, C), the pooler (P -- an int for the even-grid pooler, (PH, PW) for the contract --, bin_stride, scale, sr,
aligned), rois [R,5] float32, the options of the even-grid pooler (in_bf16, and affine = None or (scale?, shift?, relu?)) and
`branch`, a list of (roi row, expectation) pairs that says which kernel branch the row is meant to reach -- checked from the
reference's grids and taps by check_conditions, never from a kernel's output.  Every case interleaves the image indices and has
two of them out of range (rows 3 and 6).
"""
import numpy as np

import roi_align_ref as ref
from roi_align_bwd_cases import K_MAX_AXIS, K_SEP_GRID, error_ratio, random_boxes, separable_build, special_boxes, with_indices  # noqa: F401

# the plan of locov_amd/csrc/roi_align_tiles.hip
K_TL_BINS = 16           # kTlBins: bins per axis a plan covers
K_TL_TAPS = 6            # kTlTaps: pixels per bin and axis
K_TL_WINDOW = 192        # kTlWinPix: pixels of the LDS window

GATE = 1e-5
BAD_ROWS = (3, 6)        # with_indices: an index past the last image, a negative one


def fwd_slices(C):
    """(channel slices per roi, channel quads per slice) of the even-grid pooler: nhwc_slices of roi_align_nhwc.hip -- a power of
    two up to 8 that leaves a slice at least 64 quads wide -- and the frame's ceil division (the last slice may be ragged)."""
    c4, n = C // 4, 1
    while n < 8 and c4 // (2 * n) >= 64:
        n *= 2
    return n, -(-c4 // n)


def pooled(case):
    return ref._pooled(case["P"])


def out_shape(case):
    PH, PW = pooled(case)
    s = case["bin_stride"]
    return len(case["rois"]), len(range(0, PH, s)), len(range(0, PW, s)), case["C"]


def pooler(case):
    return case["P"], case["scale"], case["sr"], case["aligned"]


def make_case(name, entry, N, H, W, C, P, bin_stride, scale, sr, aligned, n_random=42, seed=0, extra=None, branch=(), lo=0.6, hi=0.7,
              specials=True):
    rng = np.random.default_rng(3000 + seed)
    parts = [random_boxes(rng, n_random, H, W, scale, lo, hi)]
    if specials:
        parts.append(special_boxes(H, W, scale, aligned))
    first_extra = sum(len(p) for p in parts)
    if extra is not None:
        parts.append(np.asarray(extra, np.float32).reshape(-1, 4))
    rois = with_indices(np.concatenate(parts, 0), N, bad=True)
    assert len(rois) >= 8, "every case keeps the two out-of-range image indices"
    return dict(name=name, entry=entry, N=N, H=H, W=W, C=C, P=P, bin_stride=bin_stride, scale=scale, sr=sr, aligned=aligned, rois=rois,
                seed=seed, in_bf16=False, affine=None, branch=[(first_extra + i, what) for i, what in branch], first_special=n_random)


def variant(case, tag, **changes):
    c = dict(case)
    c.update(changes)
    c["name"] = f"{case['name']}-{tag}"
    return c


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even), returned as float32.  Finite inputs."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return u.view(np.float32)


def feature_map(case):
    """The map the kernel reads, [N,H,W,C] float32: seeded standard normal, rounded to bf16 where the case feeds a bf16 map."""
    rng = np.random.default_rng(7000 + case["seed"])
    f = rng.standard_normal((case["N"], case["H"], case["W"], case["C"])).astype(np.float32)
    return bf16_round(f) if case["in_bf16"] else f


def affine(case):
    """(ch_scale, ch_shift, relu): float32 [C] each or None.  Every channel has a scale and a shift of its own (signs mixed), so a
    slice that reads another slice's channels or another channel's affine shows."""
    if case["affine"] is None:
        return None, None, False
    has_scale, has_shift, relu = case["affine"]
    rng = np.random.default_rng(9000 + case["seed"])
    C = case["C"]
    sc = (rng.uniform(0.5, 2.0, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    sh = rng.uniform(-1.0, 1.0, C).astype(np.float32)
    assert len(np.unique(sc)) == C and len(np.unique(sh)) == C
    return (sc if has_scale else None), (sh if has_shift else None), bool(relu)


def pooled_reference(case):
    """float64 [R, OH, OW, C]: ROIAlign alone, on the map the kernel reads."""
    return ref.roi_align_fwd_f64(feature_map(case), case["rois"], *pooler(case), case["bin_stride"])


def reference(case, pooled_rows=None):
    """float64 [R, OH, OW, C]: roi_align_fwd_f64 on the map the kernel reads, then the per-channel scale, shift and ReLU in float64.
    A proposal with an out-of-range image index pools to zero and then gets the affine and the ReLU like any other row."""
    out = pooled_reference(case) if pooled_rows is None else np.array(pooled_rows, np.float64)
    sc, sh, relu = affine(case)
    if sc is not None:
        out = out * sc.astype(np.float64)
    if sh is not None:
        out = out + sh.astype(np.float64)
    if relu:
        out = np.maximum(out, 0.0)
    return out


def _axes(case, row):
    """Per axis (y, x) of roi `row`: (raw grid, valid, low, high) over the bins the entry evaluates."""
    roi = case["rois"][row]
    PH, PW = pooled(case)
    gh, gw = ref.grid_sizes(roi[None], *pooler(case))
    out = []
    for lo, hi, P, extent, grid in ((roi[2], roi[4], PH, case["H"], int(gh[0])), (roi[1], roi[3], PW, case["W"], int(gw[0]))):
        valid, low, high, _ = ref.axis_taps(lo, hi, P, np.arange(0, P, case["bin_stride"]), case["sr"], case["aligned"], case["scale"], extent)
        out.append((grid, valid, low, high))
    return out


def plan(case, row):
    """roi_plan_kernel of roi_align_tiles.hip for roi `row`, mirrored from the reference's taps.  Returns a dict:
      fast     the proposal takes the staged form
      why      None, or why it does not: "bins" (PH or PW > 16), "negative-grid", "grid" (a sampling grid >= 6), "tap" (a valid sample's
               high tap 6 or more pixels past its bin's base), "image-index" (the plan itself may be fine; the execute kernel writes zeros)
      y, x     per bin (first pixel, pixel count): base = the lowest low tap among the bin's valid samples, count = the highest tap
               offset + 1 (the last pixel's weight may be zero); (0, 0) for a bin without a valid sample.  None when refused
      rpr, cpr, nrg, ncg   bin rows / columns per region and the number of row / column groups, from the kernel's search: while
               ys1 * span(cpr) > 192 halve cpr (ys1 = the tallest single bin row); then all PH rows if they fit beside it, else grow
               rpr from 1 while rpr + 1 rows still fit.
    The kernel has one more refusal, `ys1 * span(cpr) > 192` after the halving ("a single bin wider than the window").  It is
    unreachable: the halving ends at cpr = 1 at the latest, where the span is one bin's count, and a count is at most 6 on either
    axis (a larger one was refused as "tap"), so the product is at most 36.  plan() asserts that instead of returning it, and no
    case is invented for it."""
    PH, PW = pooled(case)
    assert case["bin_stride"] == 1
    (gh, *ytaps), (gw, *xtaps) = _axes(case, row)
    b = int(case["rois"][row, 0])
    res = dict(fast=False, why=None, y=None, x=None, rpr=1, cpr=PW, nrg=PH, ncg=1)
    if PH > K_TL_BINS or PW > K_TL_BINS:
        res["why"] = "bins"
    elif gh < 0 or gw < 0:
        res["why"] = "negative-grid"
    elif gh >= K_TL_TAPS or gw >= K_TL_TAPS:
        res["why"] = "grid"
    if res["why"]:
        return res
    axes = []
    for valid, low, high in (ytaps, xtaps):
        bins = []
        for o in range(valid.shape[0]):
            if valid[o].any():
                base = int(low[o][valid[o]].min())
                khi = int((high[o][valid[o]] - base).max())
                if khi >= K_TL_TAPS:
                    res["why"] = "tap"
                    return res
                bins.append((base, khi + 1))
            else:
                bins.append((0, 0))
        axes.append(bins)
    res["y"], res["x"] = axes

    def max_span(bins, per):
        m = 0
        for b0 in range(0, len(bins), per):
            live = [(f, c) for f, c in bins[b0:b0 + per] if c > 0]
            if live:
                m = max(m, max(f + c for f, c in live) - min(f for f, _ in live))
        return m

    ys1 = max_span(axes[0], 1)
    cpr = PW
    while cpr > 1 and ys1 * max_span(axes[1], cpr) > K_TL_WINDOW:
        cpr = (cpr + 1) // 2
    cs = max_span(axes[1], cpr)
    assert ys1 * cs <= K_TL_WINDOW, "a single bin wider than the window: shown unreachable above"
    rpr = 1
    if max_span(axes[0], PH) * cs <= K_TL_WINDOW:
        rpr = PH
    else:
        while rpr < PH and max_span(axes[0], rpr + 1) * cs <= K_TL_WINDOW:
            rpr += 1
    res.update(rpr=rpr, cpr=cpr, nrg=-(-PH // rpr), ncg=-(-PW // cpr))
    if 0 <= b < case["N"]:
        res["fast"] = True
    else:
        res["why"] = "image-index"
    return res


def check_conditions(case, pooled_rows=None):
    """What keeps a case from passing for the wrong reason; returns the reference [R, OH, OW, C]."""
    raw = pooled_reference(case) if pooled_rows is None else pooled_rows
    want = reference(case, raw)
    name, rois, N = case["name"], case["rois"], case["N"]
    idx = rois[:, 0].astype(np.int64)
    bad = (idx < 0) | (idx >= N)
    assert set(np.flatnonzero(bad)) == set(BAD_ROWS) and (idx[list(BAD_ROWS)] >= N).any() and (idx[list(BAD_ROWS)] < 0).any(), name
    assert not raw[bad].any(), f"{name}: an out-of-range proposal pooled something"
    assert np.abs(raw[~bad]).max() > 0
    sc, sh, relu = affine(case)
    if relu:      # both sides of the clip, among the proposals that pool something
        live = reference(dict(case, affine=(case["affine"][0], case["affine"][1], False)), raw)[~bad]
        assert (live < 0).any() and (live > 0).any() and (want[~bad] == 0).any() and (want[~bad] > 0).any(), name
    if case["entry"] == "nhwc":
        n, per = fwd_slices(case["C"])
        assert n == case.get("slices", n), (name, n)
        if "slice_quads" in case:
            c4 = case["C"] // 4
            assert [min(per, c4 - s * per) for s in range(n)] == case["slice_quads"], name
    gh, gw = ref.grid_sizes(rois, *pooler(case))
    _, OH, OW, _ = out_shape(case)
    for row, what in case["branch"]:
        assert 0 <= idx[row] < N or what == "refused-image-index", (name, row)
        h, w = int(gh[row]), int(gw[row])
        tag = (name, row, what, h, w)
        if case["entry"] == "contract":
            pl = plan(case, row)
            if what == "one-region":
                assert pl["fast"] and pl["nrg"] == 1 and pl["ncg"] == 1 and np.abs(raw[row]).max() > 0, (tag, pl)
            elif what == "halved-columns":
                assert pl["fast"] and pl["cpr"] < pooled(case)[1] and pl["ncg"] > 1, (tag, pl)
            elif what == "some-rows":
                assert pl["fast"] and 1 < pl["rpr"] < pooled(case)[0], (tag, pl)
            elif what == "one-row":
                assert pl["fast"] and pl["rpr"] == 1 and pooled(case)[0] > 1, (tag, pl)
            elif what == "refused-grid":
                assert pl["why"] == "grid" and np.abs(raw[row]).max() > 0, (tag, pl)
            elif what == "refused-tap":
                assert pl["why"] == "tap" and np.abs(raw[row]).max() > 0, (tag, pl)
            elif what == "refused-negative-grid":
                assert pl["why"] == "negative-grid" and case["sr"] == 0 and case["aligned"] and not raw[row].any(), (tag, pl)
            elif what == "refused-image-index":
                assert pl["why"] == "image-index" and row in BAD_ROWS, (tag, pl)
            elif what == "refused-bins":
                assert pl["why"] == "bins", (tag, pl)
            else:
                raise AssertionError(what)
            continue
        lds = OH * max(h, 0) <= K_MAX_AXIS and OW * max(w, 0) <= K_MAX_AXIS
        sep_try = lds and 1 <= h <= K_SEP_GRID and 1 <= w <= K_SEP_GRID
        if what == "separable":          # per-pixel weights, and the bins do read pixels
            assert sep_try and not separable_build(case, row)[0] and np.abs(raw[row]).max() > 0, tag
        elif what == "nonsep-y":         # four taps from the LDS tables: the y grid is past the separable form's 16
            assert K_SEP_GRID < h and lds and 1 <= w <= K_SEP_GRID and OH == 7 and np.abs(raw[row]).max() > 0, tag
        elif what == "nonsep-x":
            assert K_SEP_GRID < w and lds and 1 <= h <= K_SEP_GRID and OW == 7 and np.abs(raw[row]).max() > 0, tag
        elif what == "onthefly-y":       # past the 192-entry tables
            assert OH * h > K_MAX_AXIS and w >= 1 and np.abs(raw[row]).max() > 0, tag
        elif what == "onthefly-x":
            assert OW * w > K_MAX_AXIS and h >= 1 and np.abs(raw[row]).max() > 0, tag
        elif what == "sep-bails":        # the separable build is tried and bails out: four taps from the LDS tables
            assert sep_try and separable_build(case, row)[0] and np.abs(raw[row]).max() > 0, tag
        elif what.startswith("all-miss"):    # samples on both axes, none of them inside [-1, extent] on at least one; and the form it takes
            (_, vy, _, _), (_, vx, _, _) = _axes(case, row)
            assert h >= 1 and w >= 1 and not (vy.any() and vx.any()) and not raw[row].any(), tag
            form = "onthefly" if not lds else "separable" if sep_try else "tables"
            assert what == "all-miss-" + form, (tag, form)
        elif what == "inverted-fixed":   # negative bin size under aligned and a fixed ratio: the samples run from the start BACK
            roi = rois[row]
            by = ref._axis_geometry(roi[2], roi[4], pooled(case)[0], case["sr"], True, case["scale"])[1]
            bx = ref._axis_geometry(roi[1], roi[3], pooled(case)[1], case["sr"], True, case["scale"])[1]
            assert case["aligned"] and case["sr"] > 0 and min(by, bx) < 0 and np.abs(raw[row]).max() > 0, tag
        else:
            raise AssertionError(what)
    return want


def oracle_forward(oracle, case, channels=16):
    """The fp32 oracle on the case's inputs (the first `channels` channels; rois with an image index out of range dropped, which
    the oracle refuses) -> ([R', OH, OW, c], the rows kept)."""
    c = min(channels, case["C"])
    idx = case["rois"][:, 0].astype(np.int64)
    keep = (idx >= 0) & (idx < case["N"])
    feat = np.ascontiguousarray(feature_map(case)[..., :c].transpose(0, 3, 1, 2))
    got = oracle.roi_align(feat, case["rois"][keep], pooled(case), case["scale"], case["sr"], case["aligned"])     # [R', c, PH, PW]
    s = case["bin_stride"]
    return got[:, :, ::s, ::s].transpose(0, 2, 3, 1), keep


# ------------------------------------------------------------------------------------------------------------------ the cases
def _m(v, scale, aligned):
    return (v + (0.5 if aligned else 0.0)) / scale


def _map_boxes(boxes, scale, aligned):
    """boxes in MAP coordinates -> image coordinates"""
    return np.array([[_m(v, scale, aligned) for v in row] for row in boxes], np.float32)


def pooler_cases():
    """Even-grid pooler, C = 64: (P, bin_stride) x aligned x sampling_ratio x scale paired over three map sizes.  Every case marks a
    small and a map-sized box whose separable build is asserted; under aligned and a fixed ratio the inverted special box as well."""
    grid = [((14, 2), True, 0, 16, (20, 30)), ((14, 2), False, 2, 8, (9, 17)), ((14, 2), False, 3, 32, (30, 44)), ((14, 2), True, 1, 16, (30, 44)),
            ((14, 1), True, 0, 8, (9, 17)), ((14, 1), False, 1, 32, (20, 30)), ((14, 1), True, 2, 16, (30, 44)), ((14, 1), False, 3, 16, (9, 17)),
            ((7, 1), True, 0, 32, (30, 44)), ((7, 1), False, 2, 16, (20, 30)), ((7, 1), True, 3, 8, (9, 17)), ((7, 1), False, 1, 8, (30, 44)),
            ((7, 2), False, 0, 16, (9, 17)), ((7, 2), True, 1, 32, (20, 30)), ((7, 2), True, 2, 8, (30, 44)), ((7, 2), False, 3, 32, (9, 17)),
            ((13, 2), True, 3, 32, (9, 17)), ((13, 2), False, 0, 8, (20, 30)), ((13, 2), True, 2, 16, (30, 44)), ((13, 2), False, 1, 16, (9, 17)),
            ((8, 2), True, 0, 16, (30, 44)), ((8, 2), False, 3, 8, (20, 30)), ((8, 2), True, 1, 8, (9, 17)), ((8, 2), False, 2, 32, (30, 44))]
    c = []
    for k, ((P, s), aligned, sr, inv_scale, (H, W)) in enumerate(grid):
        scale = 1.0 / inv_scale
        name = f"pooler-P{P}s{s}-{'aligned' if aligned else 'unaligned'}-sr{sr}-scale{inv_scale}-map{H}x{W}"
        # a box of about 6 x 5 map pixels (bins under one pixel: any fixed ratio keeps a bin's samples inside grid + 1 pixels), and,
        # with the adaptive grid (samples at most a pixel apart), one over most of the map
        extra = [[2.3, 1.7, 8.1, 6.9]] + ([[0.6, 0.4, W - 1.2, H - 0.7]] if sr == 0 else [])
        branch = [(i, "separable") for i in range(len(extra))]
        case = make_case(name, "nhwc", 2, H, W, 64, P, s, scale, sr, aligned, seed=k, extra=_map_boxes(extra, scale, aligned), branch=branch)
        if aligned and sr > 0:
            case["branch"].append((case["first_special"] + 3, "inverted-fixed"))      # special_boxes' x2 < x1
        c.append(case)
    return c


def branch_cases():
    """Even-grid pooler, the three arithmetic forms on a 40 x 40 map at scale 1/2, C = 8 (boxes in image coordinates)."""
    c = []
    tall = [[20.0, -30.0, 60.0, 570.0], [10.0, 4.0, 50.0, 640.0]]
    wide = [[-30.0, 20.0, 570.0, 60.0], [4.0, 10.0, 640.0, 50.0]]
    kw = dict(n_random=20, hi=0.4)
    # four taps from the LDS tables: 16 < grid <= 27 at 7 output rows (a box ~600 px high at scale 1/2: bins of ~21 pixels)
    c.append(make_case("tables-y-P14s2", "nhwc", 2, 40, 40, 8, 14, 2, 1 / 2, 0, True, seed=51, extra=tall, branch=[(0, "nonsep-y"), (1, "nonsep-y")], **kw))
    c.append(make_case("tables-x-P14s2", "nhwc", 2, 40, 40, 8, 14, 2, 1 / 2, 0, True, seed=52, extra=wide, branch=[(0, "nonsep-x"), (1, "nonsep-x")], **kw))
    c.append(make_case("tables-y+x-P7s1-unaligned", "nhwc", 2, 40, 40, 8, 7, 1, 1 / 2, 0, False, seed=56,
                       extra=[[20.0, -30.0, 60.0, 270.0], [-30.0, 20.0, 270.0, 60.0]], branch=[(0, "nonsep-y"), (1, "nonsep-x")], **kw))
    # the same boxes under a fixed ratio: the grid is 2 whatever the box, so the separable build is tried.  The boxes that hang over
    # the map on both sides keep ONE valid sample per bin: separable.  The boxes that start inside keep both samples of their first
    # bins, 11 pixels apart -- more than the grid + 1 entries of a bin's weights: the build bails out, four taps from the tables.
    c.append(make_case("tables-sep-bails-sr2-unaligned", "nhwc", 2, 40, 40, 8, 14, 2, 1 / 2, 2, False, seed=53, extra=tall + wide,
                       branch=[(0, "separable"), (1, "sep-bails"), (2, "separable"), (3, "sep-bails")], **kw))
    c.append(make_case("tables-sep-bails-sr3-aligned-P7s1", "nhwc", 2, 40, 40, 8, 7, 1, 1 / 2, 3, True, seed=57,
                       extra=[[10.0, 4.0, 50.0, 340.0], [4.0, 10.0, 340.0, 50.0]], branch=[(0, "sep-bails"), (1, "sep-bails")], **kw))
    # on the fly: OH * grid > 192 -- 14 rows x 18 samples, and 7 rows x 29
    c.append(make_case("onthefly-P14s1", "nhwc", 2, 40, 40, 8, 14, 1, 1 / 2, 0, True, seed=54,
                       extra=[[20.0, -100.0, 60.0, 400.0], [-100.0, 20.0, 400.0, 60.0]], branch=[(0, "onthefly-y"), (1, "onthefly-x")], **kw))
    c.append(make_case("onthefly-P14s2-grid29", "nhwc", 2, 40, 40, 8, 14, 2, 1 / 2, 0, True, seed=55,
                       extra=[[20.0, -300.0, 60.0, 500.0], [-300.0, 20.0, 500.0, 60.0]], branch=[(0, "onthefly-y"), (1, "onthefly-x")], **kw))
    # proposals whose samples all miss the map -- left of it, below it, past it on both axes -- in the separable form (grid 4), the
    # table form (grid 22 on y) and on the fly; and boxes inverted on x, on y and on both under aligned and a fixed ratio
    miss = [[-500.0, 10.0, -300.0, 60.0], [10.0, 90.0, 60.0, 300.0], [200.0, 300.0, 400.0, 420.0], [-400.0, -700.0, -300.0, -90.0],
            [-500.0, -1000.0, -300.0, -100.0]]
    c.append(make_case("all-miss-P14s2", "nhwc", 2, 40, 40, 8, 14, 2, 1 / 2, 0, True, seed=58, extra=miss, branch=[(0, "all-miss-separable"), (1, "all-miss-separable"), (2, "all-miss-separable"), (3, "all-miss-tables"), (4, "all-miss-onthefly")], **kw))
    inverted = [[60.0, 10.0, 20.0, 50.0], [10.0, 70.0, 50.0, 30.0], [66.0, 58.0, 8.0, 12.0]]
    for k, (P, s, sr) in enumerate(((14, 2, 2), (7, 1, 3), (13, 2, 1))):
        c.append(make_case(f"inverted-P{P}s{s}-sr{sr}-aligned", "nhwc", 2, 40, 40, 8, P, s, 1 / 2, sr, True, seed=59 + k, extra=inverted,
                           branch=[(i, "inverted-fixed") for i in range(3)], **kw))
    return c


def slice_cases():
    """Even-grid pooler, channel slices: 9 x 17 map, 20 proposals, every channel with its own scale and shift."""
    c = []
    spec = [(8, 1, [2], (14, 2, 0, True)), (36, 1, [9], (7, 1, 2, False)), (512, 2, [64, 64], (14, 2, 0, True)), (516, 2, [65, 64], (14, 2, 0, True)),
            (516, 2, [65, 64], (7, 1, 2, False)), (1028, 4, [65, 65, 65, 62], (13, 2, 3, True)), (1028, 4, [65, 65, 65, 62], (14, 2, 0, True)),
            (2048, 8, [64] * 8, (14, 2, 0, True))]
    for k, (C, n, quads, (P, s, sr, aligned)) in enumerate(spec):
        name = f"slices-C{C}-P{P}s{s}-sr{sr}-{'aligned' if aligned else 'unaligned'}"
        case = make_case(name, "nhwc", 2, 9, 17, C, P, s, 1 / 16, sr, aligned, n_random=14, seed=70 + k)
        case.update(slices=n, slice_quads=quads)
        c.append(case)
    return c


AFFINE_FORMS = (("scale", (True, False, False)), ("shift", (False, True, False)), ("scale+shift", (True, True, False)),
                ("scale+shift+relu", (True, True, True)), ("relu", (False, False, True)))


def option_cases():
    """The two maps the option tests share: a non-default pooler on C = 64, and a ragged two-slice C = 516."""
    a = make_case("options-C64-P13s2-sr2-unaligned", "nhwc", 2, 20, 30, 64, 13, 2, 1 / 8, 2, False, seed=80)
    b = make_case("options-C516-P7s2-sr0-aligned", "nhwc", 2, 9, 17, 516, 7, 2, 1 / 16, 0, True, n_random=14, seed=81)
    b.update(slices=2, slice_quads=[65, 64])
    return [a, b]


def affine_cases():
    return [variant(c, name, affine=form) for c in option_cases() for name, form in AFFINE_FORMS]


def sliced_affine_cases():
    """slice_cases with scale + shift + ReLU on: what the GPU test of the slices runs."""
    return [variant(c, "affine", affine=(True, True, True)) for c in slice_cases()]


def dtype_cases():
    """(case, out_bf16) for the four (input, output) dtype pairs, on both option maps."""
    return [(variant(c, f"{'bf16' if i else 'f32'}-to-{'bf16' if o else 'f32'}", in_bf16=i), o)
            for c in option_cases() for i in (False, True) for o in (False, True)]


def region_boxes(scale, aligned):
    """Boxes for the plan's region search on a ~70 x 70 map, map coordinates: 11 pixels (the whole footprint fits the window), 24
    (all columns beside some rows), 60 (the columns split, one row at a time), 100 (grid 8 at 14 bins), and an inverted one."""
    return _map_boxes([[5.3, 7.1, 16.4, 18.2], [40.2, 3.3, 51.0, 14.9], [10.4, 30.2, 34.1, 54.9], [6.2, 5.1, 66.3, 64.8], [3.1, 4.2, 58.6, 66.0],
                       [-20.3, -15.2, 79.9, 85.1], [50.0, 12.0, 14.0, 48.0]], scale, aligned)


def contract_cases():
    """The pooler contract (both modes run on every case)."""
    c = []
    rb = [(0, "one-region"), (1, "one-region"), (2, "some-rows"), (3, "halved-columns"), (3, "one-row"), (4, "halved-columns"), (5, "refused-grid"),
          (6, "refused-negative-grid")]
    c.append(make_case("contract-regions-P14-sr0-aligned-map70x70-C8", "contract", 2, 70, 70, 8, (14, 14), 1, 1 / 4, 0, True, n_random=24, seed=100,
                       hi=0.5, extra=region_boxes(1 / 4, True), branch=rb))
    c[-1]["branch"] += [(3, "refused-image-index"), (6, "refused-image-index")]
    c.append(make_case("contract-regions-P14-sr0-unaligned-map70x71-C8", "contract", 2, 70, 71, 8, (14, 14), 1, 1 / 8, 0, False, n_random=24, seed=101,
                       hi=0.5, extra=region_boxes(1 / 8, False)[:6], branch=rb[:7]))
    # a fixed ratio on boxes of 150+ map pixels: the two samples of a bin are 5+ pixels apart, the high tap 6+ pixels past the base
    big = _map_boxes([[-10.2, -8.1, 150.3, 161.0], [2.3, 1.1, 168.7, 40.2], [1.4, 3.3, 38.6, 175.2]], 1 / 4, True)
    c.append(make_case("contract-regions-P14-sr2-aligned-map70x70-C8", "contract", 2, 70, 70, 8, (14, 14), 1, 1 / 4, 2, True, n_random=24, seed=102,
                       hi=0.5, extra=np.concatenate([region_boxes(1 / 4, True)[:5], big]),
                       branch=[(0, "one-region"), (2, "some-rows"), (3, "halved-columns"), (5, "refused-tap"), (6, "refused-tap"), (7, "refused-tap")]))
    # pooled sizes: 7 x 7 (49 bins: the scalar write-out), 14 x 14 at a ragged last 32-channel workgroup, the 16-bin limit, 17 bins
    small = lambda scale, aligned: _map_boxes([[2.3, 1.7, 8.1, 6.9], [5.5, 3.2, 17.6, 12.1]], scale, aligned)
    c.append(make_case("contract-P7-sr0-aligned-map30x44-C36", "contract", 2, 30, 44, 36, (7, 7), 1, 1 / 16, 0, True, seed=103, extra=small(1 / 16, True),
                       branch=[(0, "one-region"), (1, "one-region")]))
    c.append(make_case("contract-P7-sr3-unaligned-map9x17-C64", "contract", 2, 9, 17, 64, (7, 7), 1, 1 / 32, 3, False, seed=104,
                       extra=small(1 / 32, False)[:1], branch=[(0, "one-region")]))
    c.append(make_case("contract-P14-sr0-unaligned-map30x44-C64", "contract", 2, 30, 44, 64, (14, 14), 1, 1 / 16, 0, False, seed=105,
                       extra=small(1 / 16, False), branch=[(0, "one-region"), (1, "one-region")]))
    c.append(make_case("contract-P14-sr2-aligned-map20x30-C36", "contract", 2, 20, 30, 36, (14, 14), 1, 1 / 8, 2, True, seed=106, extra=small(1 / 8, True),
                       branch=[(0, "one-region"), (1, "one-region")]))
    rg = region_boxes(1 / 4, True)
    # at 5 or 16 bins a grid under 6 needs a side under 30 / 96 pixels: 60 x 24 and 14 x 60 pixels, the long side on the 16-bin axis
    flat = _map_boxes([[4.2, 20.3, 64.5, 44.1], [20.3, 4.2, 34.6, 64.5]], 1 / 4, True)
    c.append(make_case("contract-P5x16-sr0-aligned-map70x70-C36", "contract", 2, 70, 70, 36, (5, 16), 1, 1 / 4, 0, True, n_random=24, seed=107, hi=0.5,
                       extra=np.concatenate([rg[:3], flat[:1]]), branch=[(0, "one-region"), (3, "halved-columns"), (3, "one-row")]))
    c.append(make_case("contract-P16x5-sr0-aligned-map70x70-C8", "contract", 2, 70, 70, 8, (16, 5), 1, 1 / 4, 0, True, n_random=24, seed=108, hi=0.5,
                       extra=np.concatenate([rg[:3], flat[1:]]), branch=[(0, "one-region"), (3, "some-rows")]))
    c.append(make_case("contract-P16x5-sr2-unaligned-map30x44-C64", "contract", 2, 30, 44, 64, (16, 5), 1, 1 / 16, 2, False, seed=109,
                       extra=small(1 / 16, False), branch=[(0, "one-region")]))
    case = make_case("contract-P17x4-sr0-aligned-map9x17-C8", "contract", 2, 9, 17, 8, (17, 4), 1, 1 / 16, 0, True, n_random=14, seed=110)
    case["branch"] = [(r, "refused-bins") for r in range(len(case["rois"])) if r not in BAD_ROWS]
    c.append(case)
    return c


def misc_cases():
    """Strided map / strided output / position-major / one proposal share the option maps; the strided map runs bf16 as well."""
    return [variant(c, "bf16-map", in_bf16=True) for c in option_cases()]


def nhwc_cases():
    return pooler_cases() + branch_cases() + slice_cases() + option_cases()


def all_cases():
    """Every case of the GPU file, variants included."""
    return nhwc_cases() + sliced_affine_cases() + affine_cases() + [c for c, _ in dtype_cases()] + misc_cases() + contract_cases()


def plain_cases():
    """The cases the fp32 oracle can run: no bf16 map, no affine."""
    return nhwc_cases() + contract_cases()
