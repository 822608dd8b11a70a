"""What the stream-contract tests (tests/stream_contract.py, tests/test_gpu_stream_contract.py) know about each case of
poison_cases.CASES, keyed by case name.  Importable without a GPU; tests/test_stream_contract_host.py checks the tables against the
case table and against the sources they cite.

The contract (include/locov_hip.h, "Conventions"): a call only enqueues work on the stream it is given, neither allocates nor
synchronises, and keeps no hidden state, so it can be captured in a hipGraph.  A case leaves the capture test only for a reason
written here, with the place in the source that gives it.

HOST_READS      case -> (file:line of the read, the sentence of the docstring or comment that documents it).  The op returns host
                values (counts, a flag word, a boolean index), so it waits for its own launches: every C call it makes comes before
                the read, but nothing that synchronises can be captured.
NOT_CAPTURABLE  case -> (file:line, who, reason) for anything else that cannot be captured.  who = ENTRY_POINT: the C entry point itself is
                an exception to the contract, and the header names it (HEADER_EXCEPTIONS, next to the locov_gemm_timing_* aid);
                WRAPPER: the entry point keeps the contract, the Python object around it does not; RUNTIME: the call keeps the
                contract and the HIP runtime replays what it enqueued wrongly.
LATE_CALLS      (case, symbol): C calls a case makes AFTER its documented host read -- the only calls that may be made once the delay
                in front of them is over.  The first C call of a case is never excused.
OWN_DECOY       case -> builder of the decoy inputs (CPU tensors of build()'s structure, shapes and dtypes) where all-zero inputs are
                not a valid call.
INSENSITIVE     case -> why no output depends on the content of any device input (the decoy cannot be told from the real inputs).
"""
from __future__ import annotations

_READ_COUNTS = ("locov_amd/ops.py:916", "The ONE host read of a post-processing call: its B + 1 ints to pinned memory behind an event")

ENTRY_POINT, WRAPPER, RUNTIME = "entry point", "wrapper", "runtime"

HOST_READS = {
    "rpn_proposals_chain129": _READ_COUNTS,
    "rpn_proposals_hwa65": _READ_COUNTS,
    "nms_321": ("locov_amd/ops.py:811", "nothing is copied to the host except the final count"),
    "detect_postprocess": _READ_COUNTS,
    "detect_postprocess_cs": _READ_COUNTS,
    "detect_postprocess_wide_shifted": _READ_COUNTS,
    "detect_postprocess_wide_per_class": _READ_COUNTS,
    "detect_postprocess_wide_cs_shifted": _READ_COUNTS,
    "detect_postprocess_wide_cs_per_class": _READ_COUNTS,
    "detect_postprocess_no_proposals": _READ_COUNTS,
    "detect_postprocess_cs_no_proposals": _READ_COUNTS,
    "detect_postprocess_wide_no_proposals": _READ_COUNTS,
    "detect_postprocess_wide_cs_no_proposals": _READ_COUNTS,
    "map_proposals_f32": ("locov_amd/ops.py:2959", "the call's ONE host read"),
    "map_proposals_f64": ("locov_amd/ops.py:2959", "the call's ONE host read"),
    "detector_rescale": ("locov_amd/ops.py:2758", "ONE host read (the N counts)"),
}
# what a cited line must contain to be a host read: a download, a wait, or an index by a device mask (a nonzero() behind it)
HOST_READ_TOKENS = (".tolist()", ".synchronize()", ".bool()]", ".item()")

NOT_CAPTURABLE = {
    "augment_images": ("locov_amd/csrc/image_augment.hip:392", ENTRY_POINT,
                       "locov_augment_images uploads its descriptor table with hipMemcpyAsync from a pageable std::vector: the runtime may "
                       "wait for the stream before it stages the bytes, and a captured copy node would keep the pointer to host memory "
                       "that is freed when the call returns"),
}
_SGD_TABLE = ("locov_amd/ops.py:3115", WRAPPER,
              "ops.SgdTable (the wrapper, not locov_sgd_step) queries the event of the upload issued two fills ago and allocates its "
              "pinned buffers at its first fill: on a capturing stream the runtime refuses both (hipErrorCapturedEvent for the query of an "
              "event last recorded on that stream, pin_memory likewise) and the capture is invalidated")
NOT_CAPTURABLE.update({name: _SGD_TABLE for name in ("sgd_step_norm_clip_aligned", "sgd_step_norm_clip_scalar", "sgd_step_value_clip")})
_MEMSET_NODE = ("the call zeroes words it then accumulates into (an operand-scale slot, counters, a flag) with hipMemsetAsync on its stream, as "
                "the contract allows, and the first replay of the captured call is right; from the second replay on, the HIP runtime this "
                "was measured on replays a captured memset node with a wrong third 32-bit word (shown without any project code: "
                "docs/experiments.md, 'Stream contract (tests)'), and whatever is derived from that word is wrong")
NOT_CAPTURABLE.update({
    "split_scale_from_amax_with_memset": ("locov_amd/csrc/gemm_split.hip:864", RUNTIME, _MEMSET_NODE),
    "winograd_conv3x3_split_ex_device_scale": ("locov_amd/csrc/winograd.hip:512", RUNTIME, _MEMSET_NODE),
    "winograd_wgrad_split": ("locov_amd/csrc/winograd.hip:630", RUNTIME, _MEMSET_NODE),
    "winograd_wgrad_split_v": ("locov_amd/csrc/winograd.hip:630", RUNTIME, _MEMSET_NODE),
    "rpn_label_sample_loss": ("locov_amd/csrc/rpn_train.hip:358", RUNTIME, _MEMSET_NODE),
})
# the C entry points among NOT_CAPTURABLE: include/locov_hip.h's "Conventions" names exactly these, next to locov_gemm_timing_*
HEADER_EXCEPTIONS = ("locov_augment_images",)

LATE_CALLS = set()

OWN_DECOY = {}

_NO_ROWS = ("a call without a single proposal launches no kernel that reads an input: the entry point fills the empty slots "
            "(det_run of csrc/detect.hip, dw_run of csrc/detect_wide.hip)")
INSENSITIVE = {
    "detect_postprocess_no_proposals": _NO_ROWS,
    "detect_postprocess_cs_no_proposals": _NO_ROWS,
    "detect_postprocess_wide_no_proposals": _NO_ROWS,
    "detect_postprocess_wide_cs_no_proposals": _NO_ROWS,
}

MAX_NOT_CAPTURED, MAX_INSENSITIVE = 30, 8


def capture_set(cases):
    """The cases of `cases` that the capture test runs: all but HOST_READS and NOT_CAPTURABLE."""
    return [c for c in cases if c.name not in HOST_READS and c.name not in NOT_CAPTURABLE]
