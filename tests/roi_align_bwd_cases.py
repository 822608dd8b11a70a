"""The inputs of the ROIAlign-backward tests (tests/test_gpu_roi_align_bwd.py runs the kernels on them, tests/test_roi_align_ref.py
measures the fp32 oracle's distance from the float64 reference on the same inputs).  numpy only.

A case is a dict: the shapes (N, H, W, C), the pooler (P, bin_stride, scale, sr, aligned), pos_major, rois [R,5] float32 and
`branch`, a list of (roi row, expectation) pairs that says which kernel branch the row is meant to reach -- checked from the
reference's grid sizes by check_conditions, never from the kernel's output.
"""
import numpy as np

import roi_align_ref as ref

# thresholds of locov_amd/csrc/roi_align_nhwc_common.h and roi_align_nhwc_bwd.hip
K_SEP_GRID = 16          # kSepGrid: a larger grid on either axis leaves the separable form
K_MAX_AXIS = 192         # kMaxAxisN: OH * gh or OW * gw beyond it -> weights computed on the fly
K_NCHW_AXIS = 1024       # kMaxAxisEntries of roi_align.hip: the NCHW kernel's per-axis tables
K_TILE = 8               # kBT: the ownership kernel's tile edge
K_WINDOW_FLOATS = 5120   # the default 20 KB gradient window


def out_bins(P, bin_stride):
    return len(range(0, P, bin_stride))


def special_boxes(H, W, scale, aligned):
    """One of each awkward box, image coordinates: partly outside, larger than the map, zero-area, x2 < x1, narrower than one map
    pixel, flush against the right / bottom edge.  m(): map coordinate -> image coordinate."""
    off = 0.5 if aligned else 0.0
    m = lambda v: (v + off) / scale
    return np.array([
        [m(-2.5), m(-1.9), m(0.35 * W), m(0.4 * H)],           # partly outside
        [m(-1.0), m(-1.5), m(W + 3.0), m(H + 2.0)],            # larger than the map
        [m(0.55 * W), m(0.45 * H), m(0.55 * W), m(0.45 * H)],  # zero area
        [m(0.8 * W), m(0.2 * H), m(0.3 * W), m(0.7 * H)],      # x2 < x1
        [m(0.4 * W), m(0.1 * H), m(0.4 * W + 0.3), m(0.9 * H)],  # narrower than one map pixel
        [m(0.3 * W), m(0.35 * H), W / scale, H / scale],       # flush against the right / bottom edge
    ], np.float32)


def random_boxes(rng, n, H, W, scale, lo=0.6, hi=0.7):
    """n boxes with a corner anywhere on the map and sides between `lo` map pixels and `hi` of the map's sides."""
    x1 = rng.uniform(-0.1 * W, 0.9 * W, n)
    y1 = rng.uniform(-0.1 * H, 0.9 * H, n)
    w = rng.uniform(lo, max(hi * W, lo + 0.1), n)
    h = rng.uniform(lo, max(hi * H, lo + 0.1), n)
    return (np.stack([x1, y1, x1 + w, y1 + h], 1) / scale).astype(np.float32)


def with_indices(boxes, N, bad=True):
    """[R,5] rois: image indices INTERLEAVED (row r -> image r % N, not grouped by image); with `bad`, one random-box row gets an
    index past the last image and one a negative index."""
    R = len(boxes)
    idx = (np.arange(R) % N).astype(np.float32)
    if bad and R >= 8:
        idx[3] = N + 2
        idx[6] = -1
    return np.concatenate([idx[:, None], boxes], 1).astype(np.float32)


def make_case(name, N, H, W, C, P, bin_stride, scale, sr, aligned, pos_major=False, n_random=42, seed=0, extra=None, branch=(),
              lo=0.6, hi=0.7, specials=True, bad=True):
    rng = np.random.default_rng(1000 + seed)
    parts = [random_boxes(rng, n_random, H, W, scale, lo, hi)]
    if specials:
        parts.append(special_boxes(H, W, scale, aligned))
    first_extra = sum(len(p) for p in parts)
    if extra is not None:
        parts.append(np.asarray(extra, np.float32).reshape(-1, 4))
    rois = with_indices(np.concatenate(parts, 0), N, bad)
    return dict(name=name, N=N, H=H, W=W, C=C, P=P, bin_stride=bin_stride, scale=scale, sr=sr, aligned=aligned, pos_major=pos_major,
                rois=rois, seed=seed, branch=[(first_extra + i, what) for i, what in branch])


def gradient(case):
    """Seeded standard-normal gradient rows [R, OH, OW, C] float32 (ROI-major; the tests permute for pos_major)."""
    O = out_bins(case["P"], case["bin_stride"])
    rng = np.random.default_rng(5000 + case["seed"])
    return rng.standard_normal((len(case["rois"]), O, O, case["C"])).astype(np.float32)


def pooler(case):
    return case["P"], case["scale"], case["sr"], case["aligned"]


def reference(case, grad=None):
    g = gradient(case) if grad is None else grad
    return ref.roi_align_bwd_f64(g, (case["N"], case["H"], case["W"], case["C"]), case["rois"], *pooler(case), case["bin_stride"])


def silent_rows(case):
    """Rows that must contribute nothing: an image index out of range, or no samples on an axis (raw grid <= 0: under
    aligned=True and sampling_ratio 0 that is every empty and every inverted box)."""
    gh, gw = ref.grid_sizes(case["rois"], *pooler(case))
    idx = case["rois"][:, 0].astype(np.int64)
    return (idx < 0) | (idx >= case["N"]) | (gh <= 0) | (gw <= 0)


def footprint(case, row):
    """(pixel rows, pixel columns) with a non-zero weight for roi `row`, from the reference's axis matrices."""
    roi = case["rois"][row]
    bins = np.arange(0, case["P"], case["bin_stride"])
    wy = ref.axis_weights(roi[2], roi[4], case["P"], bins, case["sr"], case["aligned"], case["scale"], case["H"])
    wx = ref.axis_weights(roi[1], roi[3], case["P"], bins, case["sr"], case["aligned"], case["scale"], case["W"])
    return np.flatnonzero(wy.any(0)), np.flatnonzero(wx.any(0))


def separable_build(case, row):
    """The scatter kernel's separable build for roi `row`, mirrored from the reference's taps (roi_align_nhwc_common.h, the `sep_try` block of nhwc_roi_frame):
    per axis and bin, base = the lowest low tap among the bin's valid samples, and the build BAILS OUT when some valid sample's high
    tap lies more than `grid` pixels past base (the bin's per-pixel weights then do not fit grid + 1 entries).  Returns
    (bails, rows, columns): the size of the pixel rectangle the kernel derives from the build -- base .. base + highest tap offset
    per bin, which may end on a pixel whose weight is zero -- over the bins that have a valid sample."""
    roi = case["rois"][row]
    bins = np.arange(0, case["P"], case["bin_stride"])
    bails, spans = False, []
    for lo, hi, extent in ((roi[2], roi[4], case["H"]), (roi[1], roi[3], case["W"])):
        valid, low, high, _ = ref.axis_taps(lo, hi, case["P"], bins, case["sr"], case["aligned"], case["scale"], extent)
        first, last = [], []
        for o in range(len(bins)):
            if valid[o].any():
                base = low[o][valid[o]].min()
                khi = (high[o][valid[o]] - base).max()
                bails |= bool(khi > valid.shape[1])
                first.append(base)
                last.append(base + khi)
        spans.append(max(last) - min(first) + 1 if first else 0)
    return bails, spans[0], spans[1]


def dispatches_to_tiles(case):
    O = out_bins(case["P"], case["bin_stride"])
    return O == 7 and not case["pos_major"] and case["C"] % 128 == 0


def check_conditions(case, want=None, grad=None):
    """What keeps a case from passing for the wrong reason; returns the reference gradient."""
    grad = gradient(case) if grad is None else grad
    want = reference(case, grad) if want is None else want
    rois, N = case["rois"], case["N"]
    silent = silent_rows(case)
    idx = rois[:, 0].astype(np.int64)
    # the reference shows contributions on every image that has an in-range roi with samples
    for b in range(N):
        if np.any((idx == b) & ~silent):
            assert np.abs(want[b]).max() > 0, f"{case['name']}: image {b} got no gradient"
    # and the silent rows contributed exactly nothing: the same result with their gradient rows zeroed
    if silent.any():
        g0 = grad.copy()
        g0[silent] = 0
        assert np.array_equal(reference(case, g0), want), f"{case['name']}: a row without samples contributed"
    # the branch every marked roi is meant to reach, from the contract's grid sizes
    gh, gw = ref.grid_sizes(rois, *pooler(case))
    O = out_bins(case["P"], case["bin_stride"])
    for row, what in case["branch"]:
        assert 0 <= idx[row] < N, (case["name"], row)
        h, w = int(gh[row]), int(gw[row])
        lds = O * h <= K_MAX_AXIS and O * w <= K_MAX_AXIS
        if what == "nonsep-y":        # LDS tables, four taps per sample: the y grid is past the separable form's 16
            assert K_SEP_GRID < h and lds and 1 <= w <= K_SEP_GRID, (case["name"], row, h, w)
        elif what == "nonsep-x":
            assert K_SEP_GRID < w and lds and 1 <= h <= K_SEP_GRID, (case["name"], row, h, w)
        elif what == "onthefly-y":    # past the 192-entry tables
            assert O * h > K_MAX_AXIS, (case["name"], row, h, w)
        elif what == "onthefly-x":
            assert O * w > K_MAX_AXIS, (case["name"], row, h, w)
        elif what == "nchw-onthefly-y":   # past the NCHW kernel's 1024-entry tables (all P bins: bin_stride is 1 there)
            assert O * h > K_NCHW_AXIS, (case["name"], row, h, w)
        elif what == "nchw-onthefly-x":
            assert O * w > K_NCHW_AXIS, (case["name"], row, h, w)
        elif what == "sep-bails":     # grid small enough for the separable build to be tried, and the build bails out: four taps from LDS tables
            assert 1 <= h <= K_SEP_GRID and 1 <= w <= K_SEP_GRID and lds, (case["name"], row, h, w)
            assert separable_build(case, row)[0], (case["name"], row)
        elif what in ("window", "direct"):   # separable; the kernel's pixel rectangle fits / does not fit the gradient window
            assert 1 <= h <= K_SEP_GRID and 1 <= w <= K_SEP_GRID and lds, (case["name"], row, h, w)
            bails, rows, cols = separable_build(case, row)
            assert not bails and rows > 0 and cols > 0, (case["name"], row, rows, cols)
            nsl, c4 = scatter_slices(case["C"])
            floats = rows * cols * 4 * -(-c4 // nsl)
            assert (floats <= K_WINDOW_FLOATS) == (what == "window"), (case["name"], row, floats)
        elif what == "tiles-all":     # the roi has a weight on every 8 x 8 tile of the map
            py, px = footprint(case, row)
            assert set(py // K_TILE) == set(range(-(-case["H"] // K_TILE))), (case["name"], row)
            assert set(px // K_TILE) == set(range(-(-case["W"] // K_TILE))), (case["name"], row)
        else:
            raise AssertionError(what)
    return want


def scatter_slices(C):
    """(channel slices per roi, channel quads) of the scatter kernel's launcher (nhwc_slices + the backward's refinement)."""
    c4, n = C // 4, 1
    while n < 8 and c4 // (2 * n) >= 64:
        n *= 2
    while n < 8 and C // (2 * n) >= 128 and c4 % (2 * n) == 0:
        n *= 2
    return n, c4


def oracle_backward(oracle, case, channels=16):
    """The fp32 oracle's torchvision-style backward on the case's inputs (the first `channels` channels; rois with an image index
    out of range dropped, which the oracle refuses), fed a [R,C,P,P] gradient that is zero off the strided bins -> [N,H,W,c]."""
    c = min(channels, case["C"])
    idx = case["rois"][:, 0].astype(np.int64)
    keep = (idx >= 0) & (idx < case["N"])
    g = gradient(case)[keep][..., :c]
    P, s = case["P"], case["bin_stride"]
    full = np.zeros((int(keep.sum()), c, P, P), np.float32)
    full[:, :, ::s, ::s] = g.transpose(0, 3, 1, 2)
    got = oracle.roi_align_backward(full, (case["N"], c, case["H"], case["W"]), case["rois"][keep], case["scale"], case["sr"], case["aligned"])
    return got.transpose(0, 2, 3, 1)


def error_ratio(got, want):
    """max abs error over the gate's denominator max(|reference|.max(), 1); the gate is ratio <= 1e-5."""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1.0))


# ------------------------------------------------------------------------------------------------------------------ the cases
def _m(v, scale, aligned):
    return (v + (0.5 if aligned else 0.0)) / scale


def margin_boxes(H, W, scale, aligned, n=40, seed=77):
    """n boxes with one edge per axis within 2.5 map pixels of an 8-pixel tile boundary, on either side of it: the low or the high
    edge of the box (drawn per axis), the other edge 0.4-6 pixels away."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4), np.float64)
    for k, extent in ((0, W), (1, H)):
        bounds = np.arange(K_TILE, extent, K_TILE)
        edge = rng.choice(bounds, n) + rng.uniform(-2.5, 2.5, n)
        length = rng.uniform(0.4, 6.0, n)
        is_high = rng.random(n) < 0.5
        out[:, k] = np.where(is_high, edge - length, edge)
        out[:, k + 2] = np.where(is_high, edge, edge + length)
    return np.array([[_m(v, scale, aligned) for v in row] for row in out], np.float32)


def tiles_cases():
    """The ownership form: 7 x 7 strided bins, ROI-major, C % 128 == 0.  A pairwise cover of (P, bin_stride) x aligned x
    sampling_ratio x scale over the four map sizes; aligned=False meets every sampling_ratio."""
    c = []
    grid = [((14, 2), True, 0, 1 / 16, (20, 30), 128), ((14, 2), False, 2, 1 / 8, (9, 17), 128), ((14, 2), False, 3, 1 / 32, (5, 3), 128),
            ((13, 2), False, 0, 1 / 8, (8, 8), 128), ((13, 2), True, 2, 1 / 32, (20, 30), 128), ((13, 2), True, 3, 1 / 16, (9, 17), 128),
            ((7, 1), True, 0, 1 / 32, (9, 17), 128), ((7, 1), False, 2, 1 / 16, (5, 3), 128), ((7, 1), True, 3, 1 / 8, (8, 8), 128),
            ((13, 2), False, 3, 1 / 16, (20, 30), 256)]
    for k, ((P, s), aligned, sr, scale, (H, W), C) in enumerate(grid):
        name = f"tiles-P{P}s{s}-{'aligned' if aligned else 'unaligned'}-sr{sr}-scale{round(1 / scale)}-map{H}x{W}" + (f"-C{C}" if C != 128 else "")
        c.append(make_case(name, 2, H, W, C, P, s, scale, sr, aligned, seed=k))
    return c


def tiles_list_cases():
    """List edges of the ownership form on the 9 x 17 map (2 x 3 tiles): more proposals than one 2048-entry list pass holds, every
    one of them reaching every tile; one past a 256-thread listing step; a single proposal."""
    H, W, scale = 9, 17, 1 / 16
    rng = np.random.default_rng(91)
    n = 2100
    # only the even bins are evaluated, so the boxes are drawn from the LAST even bin (12): its first sample lands inside the last
    # tile of each axis (pixel 16 of 17 on x, pixel 8 of 9 on y), bins of 1.2-1.3 (two samples) and 0.6-0.8 pixels (one sample)
    bw, bh = rng.uniform(1.2, 1.3, n), rng.uniform(0.6, 0.8, n)
    x1, y1 = rng.uniform(15.2, 16.8, n) - 12.25 * bw, rng.uniform(7.2, 8.8, n) - 12.5 * bh
    x2, y2 = x1 + 14 * bw, y1 + 14 * bh
    big = np.array([[_m(v, scale, True) for v in row] for row in np.stack([x1, y1, x2, y2], 1)], np.float32)
    full = make_case("tiles-list-R2100-second-pass", 1, H, W, 128, 14, 2, scale, 0, True, n_random=0, seed=20, specials=False, bad=False,
                     extra=big, branch=[(i, "tiles-all") for i in range(n) if i != 2060])
    full["rois"][2060, 0] = 5                       # an index out of range in the SECOND pass: the first one fills all 2048 entries
    r257 = make_case("tiles-list-R257", 2, H, W, 128, 14, 2, scale, 0, True, n_random=251, seed=21)
    one = make_case("tiles-list-R1", 1, H, W, 128, 14, 2, scale, 0, True, n_random=0, seed=22, specials=False, bad=False,
                    extra=big[:1], branch=[(0, "tiles-all")])
    assert len(full["rois"]) == 2100 and len(r257["rois"]) == 257 and len(one["rois"]) == 1
    return [full, r257, one]


def tiles_margin_cases():
    c = []
    for k, (aligned, P, s) in enumerate(((True, 14, 2), (False, 7, 1), (True, 7, 1), (False, 14, 2))):
        H, W, scale = 20, 30, 1 / 16
        name = f"tiles-margin-{'aligned' if aligned else 'unaligned'}-P{P}s{s}"
        c.append(make_case(name, 2, H, W, 128, P, s, scale, 0, aligned, n_random=0, seed=30 + k, specials=False, bad=False,
                           extra=margin_boxes(H, W, scale, aligned, 40, 77 + k)))
    return c


def scatter_cases():
    """The scatter form: every reason the dispatcher has to leave the ownership form, and every branch of the kernel."""
    c = []
    # dispatcher reasons: C not a multiple of 128, position-major rows, grids other than 7 x 7
    c.append(make_case("scatter-C4", 2, 9, 17, 4, 14, 2, 1 / 16, 0, True, seed=40))
    c.append(make_case("scatter-C36-unaligned-sr3", 2, 9, 17, 36, 14, 2, 1 / 16, 3, False, seed=41))
    c.append(make_case("scatter-C132", 2, 9, 17, 132, 13, 2, 1 / 8, 0, True, seed=42))
    c.append(make_case("scatter-posmajor-C128", 2, 9, 17, 128, 14, 2, 1 / 16, 0, True, pos_major=True, seed=43))
    c.append(make_case("scatter-posmajor-C128-unaligned-sr2", 2, 20, 30, 128, 14, 2, 1 / 32, 2, False, pos_major=True, seed=44))
    c.append(make_case("scatter-grid14-P14s1", 2, 20, 30, 128, 14, 1, 1 / 16, 0, True, seed=45))
    c.append(make_case("scatter-grid4-P7s2", 2, 9, 17, 128, 7, 2, 1 / 16, 0, False, seed=46))
    c.append(make_case("scatter-grid2-P3s2", 2, 9, 17, 128, 3, 2, 1 / 16, 2, True, seed=47))
    c.append(make_case("scatter-grid1-P1s1", 2, 9, 17, 128, 1, 1, 1 / 16, 0, True, seed=48))
    # ragged channel slices: 257 quads -> four slices of 65, 65, 65 and 62
    c.append(make_case("scatter-ragged-C1028-map6x6", 2, 6, 6, 1028, 14, 2, 1 / 16, 0, True, n_random=20, seed=49))
    assert scatter_slices(1028) == (4, 257)
    # the window branch and the direct branch in one launch: tiny boxes (8-60 px) among boxes of 300+ px
    H, W, scale = 24, 28, 1 / 16
    rng = np.random.default_rng(50)
    tiny = np.concatenate([rng.uniform(0, 300, (12, 2)), np.zeros((12, 2))], 1)
    tiny[:, 2:] = tiny[:, :2] + rng.uniform(8, 60, (12, 2))
    large = np.concatenate([rng.uniform(0, 60, (6, 2)), np.zeros((6, 2))], 1)
    large[:, 2:] = large[:, :2] + rng.uniform(300, 380, (6, 2))
    c.append(make_case("scatter-window+direct-C132", 2, H, W, 132, 14, 2, scale, 0, True, n_random=20, seed=50, hi=0.3,
                       extra=np.concatenate([tiny, large]), branch=[(i, "window") for i in range(12)] + [(12 + i, "direct") for i in range(6)]))
    # the four-tap branch from LDS tables: 16 < grid <= 27 on a 7-row grid (a box ~600 px high at scale 1/2 overhangs the 40 x 40 map)
    tall = [[20.0, -30.0, 60.0, 570.0], [10.0, 4.0, 50.0, 640.0]]
    wide = [[-30.0, 20.0, 570.0, 60.0], [4.0, 10.0, 640.0, 50.0]]
    c.append(make_case("scatter-nonseparable-y-P14s2", 2, 40, 40, 8, 14, 2, 1 / 2, 0, True, n_random=20, seed=51, hi=0.4,
                       extra=tall, branch=[(0, "nonsep-y"), (1, "nonsep-y")]))
    c.append(make_case("scatter-nonseparable-x-P14s2", 2, 40, 40, 8, 14, 2, 1 / 2, 0, True, n_random=20, seed=52, hi=0.4,
                       extra=wide, branch=[(0, "nonsep-x"), (1, "nonsep-x")]))
    # the same boxes under a fixed sampling ratio: the grid is 2 whatever the box, so the tables and the separable build are tried
    # again.  The boxes that hang over the map on both sides keep ONE valid sample per bin (the other lies outside [-1, 40]): they
    # take the separable direct scatter.  The boxes that start inside keep both samples of their first bins, 11 pixels apart -- more
    # than the grid + 1 entries of a bin's weights: for them the build bails out and the four taps come from the LDS tables.
    c.append(make_case("scatter-fixed-sr2-unaligned-large-boxes", 2, 40, 40, 8, 14, 2, 1 / 2, 2, False, n_random=20, seed=53, hi=0.4,
                       extra=tall + wide, branch=[(0, "direct"), (1, "sep-bails"), (2, "direct"), (3, "sep-bails")]))
    # on the fly: OH * gh > 192 -- 14 rows x 18 samples, and the 7-row grid with gh >= 28
    c.append(make_case("scatter-onthefly-P14s1", 2, 40, 40, 8, 14, 1, 1 / 2, 0, True, n_random=20, seed=54, hi=0.4,
                       extra=[[20.0, -100.0, 60.0, 400.0], [-100.0, 20.0, 400.0, 60.0]], branch=[(0, "onthefly-y"), (1, "onthefly-x")]))
    c.append(make_case("scatter-onthefly-P14s2-grid29", 2, 40, 40, 8, 14, 2, 1 / 2, 0, True, n_random=20, seed=55, hi=0.4,
                       extra=[[20.0, -300.0, 60.0, 500.0], [-300.0, 20.0, 500.0, 60.0]], branch=[(0, "onthefly-y"), (1, "onthefly-x")]))
    return c


def accumulate_cases():
    return [make_case("tiles-accumulate-P13s2-unaligned-sr2", 2, 9, 17, 128, 13, 2, 1 / 8, 2, False, seed=60),
            make_case("scatter-accumulate-P7s2-unaligned-sr3-C36", 2, 9, 17, 36, 7, 2, 1 / 8, 3, False, seed=61)]


def strided_case():
    return make_case("tiles-strided-rows-ld160", 2, 9, 17, 128, 14, 2, 1 / 16, 0, True, seed=62)


def nchw_cases():
    """The NCHW backward (bin_stride 1, gradient [R,C,P,P]): P x sampling_ratio x aligned x C pairwise, a grid past the kernel's
    1024-entry tables, no rois at all."""
    c = []
    grid = [(7, 0, True, 3), (7, 2, False, 4), (14, 0, False, 6), (14, 2, True, 3), (7, 0, False, 6), (14, 2, False, 3), (14, 0, True, 4),
            (7, 2, True, 6)]
    for k, (P, sr, aligned, C) in enumerate(grid):
        name = f"nchw-P{P}-sr{sr}-{'aligned' if aligned else 'unaligned'}-C{C}"
        c.append(make_case(name, 2, 20, 30, C, P, 1, 1 / 16, sr, aligned, n_random=24, seed=70 + k))
    huge = [[-30000.0, -200.0, 31000.0, 900.0], [10.0, 10.0, 500.0, 30000.0]]          # grids 545 and 268: 7 x 545 > 1024
    for C in (3, 4):
        c.append(make_case(f"nchw-huge-grid-C{C}", 1, 40, 40, C, 7, 1, 1 / 16, 0, True, n_random=6, seed=80 + C, extra=huge,
                           branch=[(0, "nchw-onthefly-x"), (1, "nchw-onthefly-y")]))
    return c


def all_nhwc_cases():
    return tiles_cases() + tiles_list_cases() + tiles_margin_cases() + scatter_cases() + accumulate_cases() + [strided_case()]
