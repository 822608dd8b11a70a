"""CPU-side checks of the grounding branches' region assembly (locov_amd/mmss_regions.py, csrc/regions.hip): the host arithmetic
(valid extents, output lengths), the reference restatement tests/regions_ref.py on grids small enough to check by hand, and the
C ABI entries -- declared, bound, exported, argument errors reported before any HIP call (no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import regions_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["locov_regions_select", "locov_regions_gather_fwd", "locov_regions_gather_bwd"]
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_valid_extents_equal_the_numpy_float32_statement():
    from locov_amd import mmss_regions
    padded, gh, gw = (800, 1344), 25, 42
    sizes = [(800, 1344),            # fills the padded batch
             (800, 1333), (704, 1056), (480, 640), (1, 1),
             (33, 1344),             # one pixel over a cell boundary (800 / 25 = 32 pixels per cell row): 2 rows
             (32, 1344),             # exactly on it: 1 row
             (800, 33), (800, 32)]
    got = mmss_regions.grid_extents(sizes, padded, gh, gw)
    f = np.asarray(sizes, dtype=np.float32)
    want = np.zeros(f.shape, dtype=np.int32)
    want[:, 0] = np.ceil(f[:, 0] * gh / padded[0])
    want[:, 1] = np.ceil(f[:, 1] * gw / padded[1])
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(got, regions_ref.grid_extents(sizes, padded, gh, gw))
    assert got[0].tolist() == [25, 42] and got[5].tolist() == [2, 42] and got[6].tolist() == [1, 42]
    assert got[7].tolist() == [25, 2] and got[8].tolist() == [25, 1] and got[4].tolist() == [1, 1]


def test_output_lengths():
    from locov_amd import mmss_regions as mr
    ext = np.array([[2, 3], [1, 2]], dtype=np.int32)
    assert mr.grid_output_length(ext, 100) == 6            # grids smaller than spatial_dropout: what pad_sequence yields
    assert mr.grid_output_length(ext, 5) == 5 and mr.grid_output_length(ext, 1) == 1
    assert mr.grid_output_length(np.array([[25, 42], [3, 3]], dtype=np.int32), 100) == 100
    assert mr.box_output_length([200, 180, 7], 100, True) == 7 and mr.box_output_length([200, 180], 100, True) == 100
    assert mr.box_output_length([200, 180], 100, False) == 180 and mr.box_output_length([200, 180], 0, True) == 180
    assert mr.box_output_length([1, 5], 100, True) == 1


def test_fp32_cell_centres_equal_numpy_for_every_grid_size():
    """(k + 0.5) / g as ONE IEEE float32 division (what the kernel forms) against numpy's statement of :293-294 with g a numpy
    int32 scalar (numpy 2 promotes that quotient to float64 and rounds on assignment to the float32 loc array)."""
    bad = total = 0
    for g in range(1, 513):
        gi = np.int32(g)
        want = np.zeros(g, dtype=np.float32)
        want[:] = (np.arange(gi, dtype=np.float32) + 0.5) / gi
        got = (np.arange(g, dtype=np.float32) + np.float32(0.5)) / np.float32(g)
        assert got.dtype == np.float32
        bad += int((got != want).sum())
        total += g
    assert total == 131328 and bad == 0


def test_reference_on_hand_checkable_grids():
    """2 x 3 grids, padded batch 20 x 30 pixels (10 pixels per cell)."""
    B, C, gh, gw = 2, 4, 2, 3
    feat = torch.arange(B * C * gh * gw, dtype=torch.float32).reshape(B, C, gh, gw)
    sizes, padded = [(20, 30), (10, 11)], (20, 30)          # image 1: 1 row, 2 columns (one pixel into the second cell)
    ext = regions_ref.grid_extents(sizes, padded, gh, gw)
    assert ext.tolist() == [[2, 3], [1, 2]]
    full = regions_ref.grid_regions(feat, sizes, padded, 0, True)
    assert full["region_mask"].dtype == torch.uint8 and full["region_mask"].tolist() == [[1, 1, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0]]
    assert tuple(full["region_features"].shape) == (2, 6, 4) and full["region_features"][1, 4].tolist() == [28.0, 34.0, 40.0, 46.0]
    loc = full["region_loc"]
    assert loc[0, 4].tolist() == [np.float32(0.5), np.float32(0.75)]                 # cell (y 1, x 1) of a 2 x 3 extent
    assert loc[1, 1].tolist() == [np.float32(0.75), np.float32(0.5)] and loc[1, 2:].abs().sum() == 0
    assert tuple(full["mvm_mask"].shape) == (2, 6) and full["target_region_features"] is full["region_features"]
    # keys -> permutation: ties fall back to the cell index, invalid cells never appear
    keys = np.array([[0.5, 0.1, 0.9, 0.1, 0.7, 0.3], [0.2, 0.2, 0.0, 0.0, 0.0, 0.0]])
    perms = regions_ref.grid_perms(keys, ext, gw)
    assert perms[0].tolist() == [1, 3, 5, 0, 4, 2] and perms[1].tolist() == [0, 1]
    sub = regions_ref.grid_regions(feat, sizes, padded, 4, True, perms)
    assert sub["region_mask"].tolist() == [[1, 1, 1, 1], [1, 1, 0, 0]] and tuple(sub["region_features"].shape) == (2, 4, 4)
    assert sub["region_features"][0, :, 0].tolist() == [1.0, 3.0, 5.0, 0.0] and sub["region_features"][1, 2:].abs().sum() == 0
    assert sub["region_loc"][1].tolist() == [[0.25, 0.5], [0.75, 0.5], [0.0, 0.0], [0.0, 0.0]]
    # smaller than spatial_dropout everywhere: the mask keeps the configured width, the features the padded length
    wide = regions_ref.grid_regions(feat, sizes, padded, 9, True, perms)
    assert tuple(wide["region_mask"].shape) == (2, 9) and tuple(wide["region_features"].shape) == (2, 6, 4)
    assert tuple(regions_ref.grid_regions(feat, sizes, padded, 4, False)["region_mask"].shape) == (2, 6)      # :302: not training
    # boxes
    bf = [torch.arange(12, dtype=torch.float32).reshape(3, 4), 100 + torch.arange(8, dtype=torch.float32).reshape(2, 4)]
    bx = [torch.tensor([[0., 0., 10., 20.], [10., 10., 30., 20.], [2., 4., 4., 8.]]), torch.tensor([[0., 0., 8., 8.], [4., 0., 8., 4.]])]
    d, chosen = regions_ref.box_regions(bf, bx, [(20, 40), (8, 16)], 100, True, regions_ref.box_perms([0.3, 0.1, 0.2, 0.5, 0.5], [3, 2]))
    assert [c.tolist() for c in chosen] == [[1, 2], [0, 1]] and d["region_mask"].tolist() == [[1, 1], [1, 1]]
    assert d["region_features"][0].tolist() == [[4., 5., 6., 7.], [8., 9., 10., 11.]]
    assert d["region_loc"][0].tolist() == [[0.5, 0.75], [np.float32(3 / 40), np.float32(6 / 20)]] and tuple(d["mvm_mask"].shape) == (2, 2)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_bound_and_exported(lib):
    from locov_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locov_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for macro, value in (("LOCOV_REGIONS_MAX_B", _lib.REGIONS_MAX_B), ("LOCOV_REGIONS_MAX_CANDIDATES", _lib.REGIONS_MAX_CANDIDATES),
                         ("LOCOV_REGIONS_GRID", _lib.REGIONS_GRID), ("LOCOV_REGIONS_GRID_ALL", _lib.REGIONS_GRID_ALL),
                         ("LOCOV_REGIONS_BOXES", _lib.REGIONS_BOXES), ("LOCOV_REGIONS_ROWS", _lib.REGIONS_ROWS),
                         ("LOCOV_REGIONS_NCHW", _lib.REGIONS_NCHW)):
        assert re.search(rf"#define {macro} {value}\b", src), macro
    assert lib.locov_abi_version() == 8                       # additive exports do not bump it


def test_regions_select_rejects_bad_arguments(lib):
    from locov_amd import _lib
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    outs = [P(256 * k) for k in range(1, 7)]                  # indices, src_row, inv, mask, loc, mvm

    def call(mode=_lib.REGIONS_GRID, B=2, counts=(6, 6), a=(2, 1), b=(3, 2), gw=3, boxes=None, n=4, limit=4, mask_w=4, mvm_w=6, keys=P(4096), o=outs):
        return lib.locov_regions_select(keys, mode, B, ints(*counts), ints(*a), ints(*b), gw, boxes, n, limit, mask_w, mvm_w, *o, None)
    err = lambda: lib.locov_last_error()
    assert call(mode=7) == -1 and b"unknown mode" in err()
    for B in (0, -1, _lib.REGIONS_MAX_B + 1):
        assert lib.locov_regions_select(P(4096), 0, B, ints(6), ints(2), ints(3), 3, None, 4, 4, 4, 6, *outs, None) == -1 and b"1 <= B <= 64" in err()
    assert lib.locov_regions_select(P(4096), 0, 2, None, None, None, 3, None, 4, 4, 4, 6, *outs, None) == -1 and b"null pointer" in err()
    assert call(counts=(6, -6)) == -1 and b"negative count" in err()
    assert call(n=-1) == -1 and b"negative count" in err()
    assert call(a=(2, -1)) == -1 and b"negative count" in err()
    assert call(a=(3, 1)) == -1 and b"exceeds the grid" in err()
    assert call(gw=0) == -1 and b"grid_w" in err()
    big = _lib.REGIONS_MAX_CANDIDATES + 3 - (_lib.REGIONS_MAX_CANDIDATES % 3)
    assert call(counts=(6, big)) == -3 and b"LDS budget" in err()
    assert call(keys=None) == -1 and b"null pointer" in err()
    assert call(o=[None] + outs[1:]) == -1 and b"null pointer" in err()
    assert call(o=outs[:5] + [None]) == -1 and b"mvm_mask" in err()
    # boxes
    ptrs = (ctypes.c_void_p * 2)(1 << 12, 1 << 13)
    box = lambda **k: call(mode=_lib.REGIONS_BOXES, a=(800, 600), b=(1333, 900), gw=1, mask_w=k.get("n", 4), mvm_w=k.get("n", 4), **k)
    assert box(counts=(9, 5)) == -1 and b"null pointer (boxes)" in err()
    assert box(counts=(9, 3), boxes=ptrs) == -1 and b"exceeds the 3 boxes" in err()
    assert box(counts=(9, _lib.REGIONS_MAX_CANDIDATES + 1), boxes=ptrs) == -3 and b"LDS budget" in err()
    assert box(counts=(9, 5), boxes=(ctypes.c_void_p * 2)(1 << 12, (1 << 13) + 4)) == -1 and b"misaligned" in err()
    assert box(counts=(9, 5), boxes=(ctypes.c_void_p * 2)(1 << 12, 0)) == -1 and b"null pointer" in err()
    with pytest.raises(_lib.LocovError, match="LDS budget"):
        _lib.check(call(counts=(6, big)), "locov_regions_select")


def test_regions_gather_rejects_bad_arguments(lib):
    from locov_amd import _lib
    src, row, out = P(256), P(512), P(1024)
    err = lambda: lib.locov_last_error()
    fwd = lambda layout=_lib.REGIONS_ROWS, ld=2048, B=4, n=100, C=2048, hw=0, s=src, r=row, o=out: \
        lib.locov_regions_gather_fwd(s, layout, ld, B, n, C, hw, r, o, None)
    assert fwd(layout=5) == -1 and b"unknown layout" in err()
    assert fwd(B=-1) == -1 and b"negative count" in err()
    assert fwd(C=-4) == -1 and b"negative count" in err()
    assert fwd(ld=1024) == -1 and b"ld 1024 < C" in err()
    assert fwd(layout=_lib.REGIONS_NCHW, hw=0) == -1 and b"hw" in err()
    assert fwd(s=None) == -1 and b"null pointer" in err()
    assert fwd(r=None) == -1 and fwd(o=None) == -1
    assert fwd(n=0, s=None, r=None, o=None) == 0              # nothing to gather: a no-op success, no launch
    bwd = lambda layout=_lib.REGIONS_ROWS, ld=2048, rows=800, C=2048, hw=0, g=src, i=row, o=out: \
        lib.locov_regions_gather_bwd(g, layout, ld, rows, C, hw, i, o, None)
    assert bwd(layout=-1) == -1 and b"unknown layout" in err()
    assert bwd(rows=-1) == -1 and b"negative count" in err()
    assert bwd(ld=8) == -1 and b"< C" in err()
    assert bwd(i=None) == -1 and b"null pointer" in err()
    assert bwd(layout=_lib.REGIONS_NCHW, hw=1050, rows=1051) == -1 and b"multiple of hw" in err()
    assert bwd(rows=0, g=None, i=None, o=None) == 0


def test_cpu_tensors_and_bad_shapes_are_rejected():
    import locov_amd
    from locov_amd import ops
    from locov_amd._lib import LocovError
    from locov_amd.structures import Boxes, Instances
    assert locov_amd.grid_regions is locov_amd.mmss_regions.grid_regions and locov_amd.box_regions is locov_amd.mmss_regions.box_regions
    x = torch.zeros(2, 8, 2, 3)
    with pytest.raises(LocovError, match="no CPU fallback"):
        locov_amd.grid_regions(x, [(20, 30), (10, 11)], (20, 30), 4)
    with pytest.raises(LocovError, match="no CPU fallback"):
        locov_amd.grid_regions(x, [(20, 30), (10, 11)], (20, 30), 0)
    with pytest.raises(ValueError, match="image sizes"):
        locov_amd.grid_regions(x, [(20, 30)], (20, 30), 4)
    with pytest.raises(ValueError, match=r"\[B, C, gh, gw\]"):
        locov_amd.grid_regions(x[0], [(20, 30)], (20, 30), 4)
    props = []
    for r in (3, 2):
        p = Instances((20, 40))
        p.proposal_boxes = Boxes(torch.zeros(r, 4))
        props.append(p)
    with pytest.raises(LocovError, match="no CPU fallback"):
        locov_amd.box_regions([torch.zeros(3, 8), torch.zeros(2, 8)], props, 100)
    with pytest.raises(ValueError, match="box_features"):
        locov_amd.box_regions(torch.zeros(6, 8), props, 100)
    with pytest.raises(ValueError, match="unknown mode"):
        ops.regions_select("cells", None, [6], [2], [3], 4, 4, 4, 6)
    with pytest.raises(ValueError, match="1 <= B <= 64"):
        ops.regions_select("grid_all", None, [6] * 65, [2] * 65, [3] * 65, 6, 6, 6, 6, device="cpu")


def test_the_list_of_split_views_is_recognised_without_a_copy():
    from locov_amd.mmss_regions import _one_matrix
    base = torch.arange(40, dtype=torch.float32).reshape(10, 4).requires_grad_(True) * 1.0
    parts = list(base.split([3, 5, 2], dim=0))
    assert _one_matrix(parts, [3, 5, 2]) is base
    assert _one_matrix(base, [3, 5, 2]) is base
    other = _one_matrix([parts[0], parts[2], parts[1]], [3, 2, 5])                  # not consecutive: concatenated
    assert other is not base and other[3:5].equal(base[8:10])
    assert _one_matrix([p.clone() for p in parts], [3, 5, 2]).equal(base)
    cols = _one_matrix(list(base[:, :2].split([3, 5, 2], dim=0)), [3, 5, 2])        # views of a view: their own base is `base`
    assert tuple(cols.shape) == (10, 2) and cols.equal(base[:, :2])


def test_layout_key_defaults_and_validation():
    from locov_amd.config import get_cfg
    assert get_cfg().MODEL.ROI_BOX_HEAD.GRID_FEATURES_LAYOUT == "nchw"
    from locov_amd import res5_train
    rows = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).reshape(24, 8)
    v = res5_train.to_nchw(rows, 2, 3, 4, channels_last=True)
    assert tuple(v.shape) == (2, 8, 3, 4) and v.stride(1) == 1 and v.data_ptr() == rows.data_ptr()
    assert v[1, 5, 2, 3] == rows[12 + 2 * 4 + 3, 5]
