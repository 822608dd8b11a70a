"""The two detection post-processing pipelines (csrc/detect.hip: candidates sorted in LDS; csrc/detect_wide.hip: any candidate count,
radix select) against the float64 reference of the operation itself (tests/detect_ref.py), on inputs where fp32 arithmetic makes no
rounding error (tests/detect_cases.py: integer boxes, dyadic thresholds, probabilities fed as they are).  No tolerance: counts, rows
and classes equal the reference's, scores and boxes equal it as int32 bit patterns, slots past counts[i] are not looked at, a second
call gives the same bits, and the flag word is 0 wherever a result is expected.  tests/test_detect_ref.py checks, without a GPU, that
every case reaches what it is meant to and that the reference equals the CPU torch chain on both of batched_nms's branches.

Every case runs through
  lds             ops._detect_postprocess_flags(per_class_above=None): the reference's result when every image has at most 8 192
                  candidates, else the flag word DETECT_FLAG_OVERFLOW and nothing else;
  wide_per_class  the wide pipeline with per_class_above = 1 (every image: one sweep per class on the unshifted boxes);
  wide_shifted    ... with 2^31 - 1 (every image: the class-shifted boxes);
  wide_mid        batches: a switch between two images' candidate counts (the fullest image per class, the others shifted);
the class-specific entry points where the deltas are [R, 4K].  The shifted and the per-class branch must agree on these inputs, since
both must equal the reference.  Where the device torch chain is cheap (fewer than 500 non-empty classes on the per-class branch) it
is held against the reference too; elsewhere the reference alone decides.

Case groups (detect_cases.py has the details and the marks):
  semantics       threshold_edge (scores at, one ulp above and below the threshold), iou_edge_{2,1,3}_4 (IoU exactly at, and the
                  nearest grid ratios around, the thresholds 1/2, 1/4, 3/4), zero_area (0/0 pairs, degenerate boxes inside a large
                  one), chain (survivors alternate across candidate positions 63/64/65 and 127/128), ties-topk* (one score: order
                  (row, class); top-k 1, inside the tie group, survivors, survivors + 1, 8 192), ragged / ragged_front_empty
                  ([65, 0, 1, 64, 63, 0] rows, clip limits per image), ragged_64_images
  limits          limit_classes (K = 32 767: classes 0 and 32 766), limit_rows (R = 16 383, 8 192 candidates in one class, row
                  16 382 leads the output), limit_K{255,256,257,1023,1024,1025} (rows [65, 63, 64])
  capacity        capacity_{8191,8192,8193}: the second image of two at, and one past, the LDS pipeline's capacity
  select          pairwise disjoint boxes, every candidate survives; the radix select ends after pass
                    1  select_distinct_pass1            2  select_distinct_pass2            3  select_low_score_bits_pass3
                    4  select_300x80, select_5x4000 (16 000 winners), select_129x128, select_250x121_distinct_then_ties,
                       select_one_image_of_two (image 1; image 0 has 8 000 survivors and no select)
                    5  select_8x5000, select_4x4097 (top-k 8 192, 8 193 winners)
                    -  select_128x128_full_sort: 16 384 survivors, no select, the last launch sorts them all
                  (a sixth pass cannot be reached: a fifth-pass bin holds at most 64 keys)
  sweep           sweep_8200 (K = 2, two rows per 16 x 16 cell and one single row at 4 096, so the kept set does not repeat 4 096
                  positions on; third copies more than 4 096 positions behind their suppressor; top-k 8 192, every survivor is
                  output: the NQ = 4 instances of dw_sweep_kernel, both branches), sweep_8200_second_image (the same behind a small
                  image), and their R = 520 siblings
  class_specific  cs_small (rows that overlap in class 0, are disjoint in class 1, clipped in class 2), cs_sweep (400 candidates of
                  one class, more than 128 survivors: suppression by an earlier 64-candidate step's survivor and inside a step)

That the tests bite: value-only changes, one at a time, to a scratch copy of the library (results only, no address or loop bound
past a buffer; none committed), and the tests of this file each turned red on the MI355X (219 tests in all):
  - `thresh = np << lo` without the `+ 1` in dw_select_kernel: 21 -- wide_per_class and wide_shifted of all nine select cases whose
    select runs (passes 1 to 5; not the full sort), and all three wide calls of select_one_image_of_two;
  - the kept-set word test of dw_sweep_kernel ignoring `64 * q`: 6 -- wide_per_class and wide_shifted of sweep_8200, all three wide
    calls of sweep_8200_second_image, wide_per_class of limit_rows.  (With a top-k of 300 and a kept set of every second position
    the shifted branch stayed green under this change: the extra survivors lay below the top-k, and kept words folded 4 096
    positions down looked like the right ones.  Hence the single row at 4 096 and the top-k of 8 192.);
  - `v > thr` to `v >= thr` in the count and emit kernels of both files: 36 -- every call that expects a result of threshold_edge,
    ragged, ragged_front_empty, ragged_64_images, capacity_*, cs_small and sweep_520_sibling_second_image, and the three wide calls
    of sweep_8200_second_image (each has scores equal to its threshold);
  - the survivor loop of dw_sweep_cs_kernel stopping after the first 64: 1 -- cs_sweep / wide_per_class;
  - the row bits dropped from the LDS sort key (det_emit_kernel): 27 -- the lds call of every case that expects a result from it,
    but ties-topk1 (row 0 leads it).
  Not run: dw_lo_bit of one pass off by 11.  No key then matches the prefix, the histogram is empty, and the last workgroup picks
  its bin from LDS words nobody wrote -- what that mutant does is not defined, so it proves nothing and is not worth a GPU run.  The
  select's arithmetic is covered by the first change, on the cases that end after each of the passes 1 to 5.
"""
import importlib.util
import os

import pytest
import torch

import detect_cases as dc
import detect_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_detect_ref_tests", os.path.join(HERE, "test_detect_ref.py"))
cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cpu)                     # (its helpers: torch_chain, assert_equals_reference)

CHAIN_CLASS_LIMIT = 500                           # per-class branch of the device torch chain: one NMS call (and host read) per class


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


def _switch(case, call):
    return {"lds": None, "wide_per_class": 1, "wide_shifted": dc.PCA_MAX, "wide_mid": case["mid"]}[call]


CALLS = [(n, c) for n in dc.names() for c in ("lds", "wide_per_class", "wide_shifted", "wide_mid") if _switch(dc.get(n), c) is not None
         or c == "lds"]


def _run(pkg, case, per_class_above):
    """One call: (per image (rows, classes, scores, boxes) up to counts[i], flag word)."""
    probs, deltas, props = (torch.from_numpy(case[k]).cuda() for k in ("probs", "deltas", "props"))
    out, flags = pkg.ops._detect_postprocess_flags(probs, deltas, props, case["sizes"], case["image_shapes"], case["weights"],
                                                   ref.SCALE_CLAMP, case["score_thresh"], case["nms_thresh"], case["topk"],
                                                   per_class_above=per_class_above)
    boxes, scores, classes, rows, counts = out
    torch.cuda.synchronize()
    assert len(counts) == len(case["sizes"]) and all(0 <= n <= case["topk"] for n in counts)
    boxes, scores, classes, rows = (t.cpu().numpy() for t in (boxes, scores, classes, rows))
    return [(rows[i, :n], classes[i, :n], scores[i, :n], boxes[i, :n]) for i, n in enumerate(counts)], flags


@pytest.mark.parametrize("name,call", CALLS)
def test_pipeline_equals_the_reference(pkg, name, call):
    case = dc.get(name)
    want = dc.reference(name)
    per_class_above = _switch(case, call)
    if call == "wide_mid":
        cand = dc.candidate_counts(name)
        assert min(cand) < per_class_above <= max(cand)
    got, flags = _run(pkg, case, per_class_above)
    if call == "lds" and max(dc.candidate_counts(name)) > dc.LDS_CAP:
        assert flags == pkg.ops._lib.DETECT_FLAG_OVERFLOW
        return
    assert flags == 0
    cpu.assert_equals_reference(got, want, f"{name} / {call}")
    again, flags = _run(pkg, case, per_class_above)
    assert flags == 0
    cpu.assert_equals_reference(again, want, f"{name} / {call}, second call")


def _chain_is_cheap(case, branch):
    return branch == "shifted" or dc.nonempty_classes(case) < CHAIN_CLASS_LIMIT


@pytest.mark.parametrize("name,branch", [(n, b) for n in dc.names() for b in cpu.BRANCHES if _chain_is_cheap(dc.get(n), b)])
def test_device_torch_chain_equals_the_reference(pkg, monkeypatch, name, branch):
    beh = pkg.roi_heads.box_emb_head
    got = cpu.torch_chain(beh, dc.get(name), "cuda", cpu.BRANCHES[branch], monkeypatch)
    cpu.assert_equals_reference(got, dc.reference(name), f"{name} / device chain, {branch}")
