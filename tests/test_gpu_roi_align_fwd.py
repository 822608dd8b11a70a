"""The channels-last ROIAlign FORWARD kernels against a float64 reference of the operation (tests/roi_align_ref.py) on the whole
output, all channels.  The inputs live in tests/roi_align_fwd_cases.py:

  even-grid pooler (ops.roi_align_nhwc: roi_align_nhwc_kernel with its frame nhwc_roi_frame)
    pooler settings   (P, bin_stride) in (14,2) (14,1) (7,1) (7,2) (13,2) (8,2) x aligned x sampling_ratio 0 / 1 / 2 / 3 x scale 1/8,
                      1/16, 1/32 paired over maps of 9 x 17, 20 x 30 and 30 x 44, C = 64
    branches          separable per-pixel weights; four taps from the LDS tables (grid 17..27 at 7 output rows, on y and on x; the
                      separable build bailing out under a fixed ratio on a large box); weights on the fly (OH * grid > 192); proposals
                      whose samples all miss the map, in each of the three forms; boxes inverted on x / y / both under aligned and
                      a fixed ratio (negative bin size)
    channel slices    C = 8, 36, 512 (2 slices), 516 (65 + 64 quads), 1028 (65, 65, 65, 62) and 2048 (8), every channel with a scale
                      and a shift of its own + ReLU
    options           the map as a column block of a wider channels-last tensor (pixel stride C + 32, offsets 0 and 16, fp32 and
                      bf16, the neighbour columns 1e4), out= rows inside a wider matrix, scale / shift / ReLU in every combination,
                      the four (input, output) dtype pairs, position-major rows, R = 1 and R = 0
  pooler contract (ops.roi_align, modes "exact" and "fast": roi_align_contract.hip, roi_align_tiles.hip), both modes on every case
    the plan's region search (one region; halved columns; some rows per region; one row per region) and each reason it refuses a
    proposal (grid >= 6, a tap 6+ pixels past its bin's base, a negative raw grid, more than 16 bins) or the execute kernel writes
    zeros (image index out of range); pooled sizes 14 x 14, 7 x 7, (5, 16), (16, 5), (17, 4); C = 8, 36, 64.  The exact mode must
    also equal the fp32 oracle bit for bit.

Every case appends one of each awkward box (partly outside, larger than the map, zero area, x2 < x1, narrower than a map pixel,
flush against the far edges), interleaves the image indices and has two of them out of range.  check_conditions asserts, from the
reference's grids and taps alone, that each marked proposal reaches the branch it is marked for (cases.plan mirrors roi_plan_kernel
for the contract); tests/test_roi_align_ref.py runs the same assertions without a GPU.

Gate: fp32 output  max abs error <= 1e-5 x max(|reference|.max(), 1)  (the header's FAST-mode contract, the backward
tests); bf16 output one rounding on top, |got - want| <= 1e-5 x max(|want|.max(), 1) + 2^-8 |want|.  The fp32 oracle is within
1.7e-7 of the reference on every case (tests/test_roi_align_ref.py), a factor 60 inside the gate.

Worst measured ratio max abs error / max(|reference|.max(), 1) per group, MI355X (the fp32 oracle's worst beside it):
  group        kernel    oracle
  separable    1.6e-7    1.6e-7   (pooler settings, all-miss, inverted boxes, strided map, position-major, fp32 dtypes)
  tables       1.6e-7    1.3e-7
  on the fly   1.4e-7    1.0e-7
  sliced       1.7e-7    1.3e-7
  affine       1.6e-7    9.7e-8   (the oracle has no affine: its figure is the same maps pooled without one)
  bf16         1.6e-7    9.7e-8   (bf16 map, fp32 rows; the oracle's figure is the fp32 map's).  bf16 rows reach 0.99 of their bound:
                                  the rounding itself comes to 2^-8 |want| just above a power of two
  fast         1.5e-7    1.5e-7   (exact mode: 1.5e-7)
No case failed on the kernels as they were: these tests found no bug.  What they were checked against: six value-only changes
to scratch copies of the library, each turning red the tests of the branch it touches -- the affine read from the slice's
first quads (the sliced cases from C = 512 up and the C = 516 affine cases), the separable build dropping a bin's last pixel (every even-grid group), the plan's
pixel count one short (every contract case with a staged proposal), the last sample row dropped in the table form (tables-y
cases only), the last sample column dropped on the fly (onthefly cases only), the plan's later column groups one pixel to the
right (the four cases with a halved-columns mark only).
"""
import numpy as np
import pytest
import torch

import roi_align_fwd_cases as cases

pytestmark = pytest.mark.gpu

GATE = cases.GATE


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from locov_amd import ops as _ops, _lib
    _lib.load()
    return _ops


_REF = {}


def expected(case):
    """check_conditions + the float64 reference of a case, computed once per module and left unchanged."""
    if case["name"] not in _REF:
        want = cases.check_conditions(case)
        want.setflags(write=False)
        _REF[case["name"]] = want
    return _REF[case["name"]]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_map(case):
    f = dev(cases.feature_map(case))
    return f.to(torch.bfloat16) if case["in_bf16"] else f      # (exact: the values are bf16 already)


def run_nhwc(ops, case, feat=None, rois=None, **kw):
    sc, sh, relu = cases.affine(case)
    got = ops.roi_align_nhwc(dev_map(case) if feat is None else feat, dev(case["rois"]) if rois is None else rois, case["P"], case["scale"],
                             case["sr"], case["aligned"], bin_stride=case["bin_stride"], ch_scale=None if sc is None else dev(sc),
                             ch_shift=None if sh is None else dev(sh), relu=relu, **kw)
    torch.cuda.synchronize()
    return got


def gate(case, form, got, want):
    got = got.float().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (case["name"], got.shape, want.shape)
    ratio = cases.error_ratio(got, want)
    print(f"error ratio {case['name']} [{form}]: {ratio:.2e}")
    assert ratio <= GATE, f"{case['name']} [{form}]: {ratio:.3e} of the largest entry"


def gate_bf16(case, form, got, want):
    assert got.dtype == torch.bfloat16
    got = got.float().cpu().numpy()
    assert got.shape == want.shape
    bound = GATE * max(np.abs(want).max(), 1.0) + 2.0 ** -8 * np.abs(want)
    excess = float((np.abs(got - want) / bound).max())
    print(f"error / bound {case['name']} [{form}]: {excess:.2e}")
    assert excess <= 1.0, f"{case['name']} [{form}]: {excess:.3f} of the bf16 bound"


ids = lambda cs: [c["name"] for c in cs]
_POOLER, _BRANCH, _SLICED, _AFFINE = cases.pooler_cases(), cases.branch_cases(), cases.sliced_affine_cases(), cases.affine_cases()
_DTYPES, _OPTIONS, _CONTRACT = cases.dtype_cases(), cases.option_cases(), cases.contract_cases()


# ------------------------------------------------------------------------------------------------------------ even-grid pooler
@pytest.mark.parametrize("case", _POOLER, ids=ids(_POOLER))
def test_pooler_settings(ops, case):
    """separable: a small and (adaptive grid) a map-sized box asserted separable; under aligned and a fixed ratio the inverted box."""
    gate(case, "separable", run_nhwc(ops, case), expected(case))


@pytest.mark.parametrize("case", _BRANCH, ids=ids(_BRANCH))
def test_arithmetic_forms(ops, case):
    form = "on the fly" if case["name"].startswith("onthefly") else "tables" if case["name"].startswith("tables") else "separable"
    gate(case, form, run_nhwc(ops, case), expected(case))


@pytest.mark.parametrize("case", _SLICED, ids=ids(_SLICED))
def test_channel_slices(ops, case):
    """The slice count and the quads per slice are asserted by check_conditions from the restated nhwc_slices rule; scale + shift +
    ReLU with values of their own per channel, and the plain pooling of the same map."""
    gate(case, "sliced", run_nhwc(ops, case), expected(case))
    plain = next(c for c in cases.slice_cases() if case["name"] == c["name"] + "-affine")
    gate(plain, "sliced", run_nhwc(ops, plain), expected(plain))


@pytest.mark.parametrize("case", _AFFINE, ids=ids(_AFFINE))
def test_affine_and_relu(ops, case):
    gate(case, "affine", run_nhwc(ops, case), expected(case))


@pytest.mark.parametrize("case,out_bf16", _DTYPES, ids=[c["name"] for c, _ in _DTYPES])
def test_dtypes(ops, case, out_bf16):
    want = expected(case)
    if out_bf16:
        gate_bf16(case, "bf16", run_nhwc(ops, case, out_dtype=torch.bfloat16), want)
    else:
        got = run_nhwc(ops, case)
        assert got.dtype == torch.float32
        gate(case, "bf16" if case["in_bf16"] else "separable", got, want)


@pytest.mark.parametrize("in_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("base", _OPTIONS, ids=ids(_OPTIONS))
def test_map_as_a_column_block_of_a_wider_tensor(ops, base, offset, in_bf16):
    """Pixel stride C + 32, the block at column 0 or 16, every other column 1e4: the kernel must take the no-copy path (the
    conditions of ops.roi_align_nhwc for a channel slice hold for the tensor passed) and read nothing of its neighbours."""
    case = cases.variant(base, "bf16-map", in_bf16=True) if in_bf16 else base
    want = expected(case)
    N, H, W, C = case["N"], case["H"], case["W"], case["C"]
    f = dev_map(case)
    wide = torch.full((N, H, W, C + 32), 1e4, dtype=f.dtype, device="cuda")
    wide[..., offset:offset + C] = f
    block = wide[..., offset:offset + C]
    assert (block.is_cuda and block.stride(3) == 1 and block.stride(2) == C + 32 > C and block.stride(2) % 4 == 0
            and block.stride(1) == W * block.stride(2) and block.stride(0) == H * W * block.stride(2) and block.data_ptr() % 16 == 0
            and not block.is_contiguous())
    got = run_nhwc(ops, case, feat=block)
    gate(case, f"{'bf16' if in_bf16 else 'separable'}, map stride {C + 32}, column {offset}", got, want)
    assert torch.equal(got, run_nhwc(ops, case)), "the strided map must give the contiguous map's bits"


@pytest.mark.parametrize("pos_major", [False, True], ids=["roi-major", "position-major"])
@pytest.mark.parametrize("base", _OPTIONS, ids=ids(_OPTIONS))
def test_output_rows_inside_a_wider_matrix(ops, base, pos_major):
    """out= rows with row stride C + 32: the block holds the contiguous call's bits and the other columns keep theirs."""
    case = cases.variant(base, "scale+shift+relu", affine=(True, True, True))
    want = expected(case)
    R, OH, OW, C = want.shape
    plain = run_nhwc(ops, case, pos_major=pos_major)
    assert plain.shape == ((OH, OW, R, C) if pos_major else (R, OH, OW, C))
    gate(case, "affine, " + ("position-major" if pos_major else "roi-major"), plain.permute(2, 0, 1, 3) if pos_major else plain, want)
    sentinel = torch.randn(R * OH * OW, C + 32, generator=torch.Generator().manual_seed(5)).cuda()
    wide = sentinel.clone()
    block = wide[:, 16:16 + C]
    assert block.stride(0) == C + 32 and not block.is_contiguous() and block.data_ptr() % 16 == 0
    assert run_nhwc(ops, case, pos_major=pos_major, out=block) is block
    assert torch.equal(block, plain.reshape(-1, C))
    assert torch.equal(wide[:, :16], sentinel[:, :16]) and torch.equal(wide[:, 16 + C:], sentinel[:, 16 + C:])


@pytest.mark.parametrize("case", _POOLER[::5] + _BRANCH[::4] + _SLICED[3::3], ids=ids(_POOLER[::5] + _BRANCH[::4] + _SLICED[3::3]))
def test_position_major_rows_are_the_permuted_bits(ops, case):
    got = run_nhwc(ops, case)
    assert torch.equal(run_nhwc(ops, case, pos_major=True).permute(2, 0, 1, 3), got)
    assert torch.equal(run_nhwc(ops, case), got), "the pooler must be reproducible bit for bit"


@pytest.mark.parametrize("base", _OPTIONS + _BRANCH[:1], ids=ids(_OPTIONS + _BRANCH[:1]))
def test_one_proposal_and_none(ops, base):
    """R = 1: each of a few proposals on its own gives the row it has among the others; R = 0: the empty shape."""
    case = cases.variant(base, "scale+shift+relu", affine=(True, True, True))
    want = expected(case)
    _, OH, OW, C = want.shape
    rows = [0, cases.BAD_ROWS[0], len(case["rois"]) - 1] + [r for r, _ in case["branch"]]
    for r in rows:
        got = run_nhwc(ops, case, rois=dev(case["rois"][r:r + 1]))
        gate(case, f"affine, R = 1 (row {r})", got, want[r:r + 1])
    for pos_major, shape in ((False, (0, OH, OW, C)), (True, (OH, OW, 0, C))):
        got = run_nhwc(ops, case, rois=torch.zeros(0, 5, device="cuda"), pos_major=pos_major)
        assert got.shape == shape and got.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------- pooler contract
def run_contract(ops, case, mode):
    feat = dev(cases.feature_map(case)).permute(0, 3, 1, 2).contiguous()
    got = ops.roi_align(feat, dev(case["rois"]), cases.pooled(case), case["scale"], case["sr"], case["aligned"], mode=mode)
    torch.cuda.synchronize()
    return got                                              # [R, C, PH, PW]


@pytest.mark.parametrize("case", _CONTRACT, ids=ids(_CONTRACT))
def test_pooler_contract_both_modes(ops, oracle, case):
    """Both modes against float64; the exact mode also against the fp32 oracle bit for bit (out-of-range rows, which the oracle
    refuses: zeros); fast-mode proposals the plan refuses take the exact arithmetic, so their rows are the exact mode's bits."""
    want = expected(case)
    plans = [cases.plan(case, r) for r in range(len(case["rois"]))]
    exact = run_contract(ops, case, "exact")
    gate(case, "exact", exact.permute(0, 2, 3, 1), want)
    fast = run_contract(ops, case, "fast")
    gate(case, "fast", fast.permute(0, 2, 3, 1), want)
    got, keep = cases.oracle_forward(oracle, case, channels=case["C"])            # [R', PH, PW, C]
    exact = exact.cpu().numpy()
    assert np.array_equal(exact[keep], got.transpose(0, 3, 1, 2)) and not exact[~keep].any()
    refused = np.array([not p["fast"] for p in plans])
    assert np.array_equal(fast.cpu().numpy()[refused], exact[refused])
    if max(cases.pooled(case)) <= cases.K_TL_BINS:
        assert not refused.all() and not np.array_equal(fast.cpu().numpy(), exact), "the staged form IS another arithmetic"
    else:
        assert refused.all()
