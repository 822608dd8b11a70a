"""CPU-side checks of the classification-loss entry points (csrc/cls_loss.hip: locov_cls_loss, locov_cls_loss_workspace_bytes): the
exports, argument errors before anything touches a device, and the torch path of the predictor's classification statistics
([D2-upstream, unverified] _log_classification_stats).  No compute on a device: there is no GPU here."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("locov_cls_loss_workspace_bytes", "locov_cls_loss")


@pytest.fixture(scope="module")
def lib():
    from locov_amd import build, _lib
    build.build_extension()
    return _lib.load()


def test_exports(lib):
    from locov_amd import _lib
    with open(os.path.join(ROOT, "include", "locov_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.locov_abi_version() == _lib.ABI_VERSION == 8
    assert "#define LOCOV_ABI_VERSION 8" in header


def test_workspace_bytes(lib):
    f = lib.locov_cls_loss_workspace_bytes
    assert f(0) == 0 and f(-3) == 0
    assert 0 < f(1) <= f(5) <= f(1536) <= f(10 ** 7)
    assert f(10 ** 7) == f(10 ** 9)                                   # (a bounded number of blocks: grid-stride over the rows)
    assert f(1536) % 8 == 0


def _call(lib, R=1536, C=1204, ld=None, scores=256, labels=512, ws=1024, ws_bytes=None, loss=2048, dscores=4096, stats=8192):
    p = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = lib.locov_cls_loss_workspace_bytes(R)
    return lib.locov_cls_loss(p(scores), C if ld is None else ld, p(labels), R, C, -100, p(ws), ws_bytes, p(loss), p(dscores), p(stats),
                              None)


@pytest.mark.parametrize("kw,msg", [
    ({"C": 0, "ld": 4}, b"C >= 1"),
    ({"ld": 1203}, b"row stride"),
    ({"loss": 0}, b"null pointer"),
    ({"scores": 0}, b"null pointer"),
    ({"labels": 0}, b"null pointer"),
    ({"ws_bytes": 8}, b"workspace too small"),
    ({"ws": 0}, b"workspace too small"),
    ({"R": -1}, b"R >= 0"),
])
def test_argument_errors_are_reported_before_any_launch(lib, kw, msg):
    """(the pointers are small fake addresses: a call that got as far as a launch would not return an argument error)"""
    rc = _call(lib, **kw)
    assert rc < 0
    err = lib.locov_last_error()
    assert err.startswith(b"locov_cls_loss") and msg in err, err


# ------------------------------------------------------------------ the predictor's statistics, torch path

def _predictor(num_classes):
    from locov_amd.roi_heads import box_emb_head as beh
    return beh.FastRCNNOutputLayers(8, box2box_transform=beh.Box2BoxTransform((10.0, 10.0, 5.0, 5.0)), num_classes=num_classes,
                                    cls_agnostic_bbox_reg=True)


def _proposals(gt_classes):
    from locov_amd.structures import Boxes, Instances
    p = Instances((100, 100))
    n = len(gt_classes)
    p.proposal_boxes = Boxes(torch.tensor([[10., 10., 50., 50.]] * n).reshape(n, 4))
    p.gt_boxes = Boxes(torch.tensor([[12., 8., 48., 55.]] * n).reshape(n, 4))
    p.gt_classes = torch.tensor(gt_classes, dtype=torch.int64)
    return p


class _Storage:
    def __init__(self):
        self.scalars = {}

    def put_scalar(self, name, value):
        self.scalars[name] = float(value)


def test_cpu_statistics_follow_the_upstream_definition():
    bp = _predictor(3)                                                # classes 0..2, background 3
    assert bp.classification_stats() == {}                            # (nothing before the first losses() call)
    scores = torch.tensor([[5., 0., 0., 0.],      # gt 0, pred 0: accurate foreground
                           [0., 0., 1., 3.],      # gt 2, pred bg: false negative
                           [0., 4., 0., 0.],      # gt 0, pred 1: wrong foreground
                           [0., 0., 0., 2.],      # gt bg, pred bg: accurate background
                           [2., 2., 0., 0.],      # gt 1, pred 0 (the lowest index among equal maxima)
                           [1., 0., 0., 0.]],     # gt bg, pred 0
                          requires_grad=True)
    deltas = torch.zeros(6, 4, requires_grad=True)
    losses = bp.losses((scores, deltas), [_proposals([0, 2, 0, 3, 1, 3])])
    want = torch.nn.functional.cross_entropy(scores, torch.tensor([0, 2, 0, 3, 1, 3]))
    assert torch.equal(losses["loss_cls"], want)                      # the CPU path is the torch line, unchanged
    stats = bp.classification_stats()
    assert stats == {"cls_accuracy": 2 / 6, "fg_cls_accuracy": 1 / 4, "false_negative": 1 / 4}
    from locov_amd.roi_heads.labelling import _EVENTS, get_event_storage
    assert get_event_storage() is _EVENTS                             # (Detectron2 is not installed here: the stand-in)
    for k in list(_EVENTS.scalars):
        if k.startswith("fast_rcnn/"):
            del _EVENTS.scalars[k]
    assert bp.log_classification_stats() == stats
    assert {k: v for k, v in _EVENTS.scalars.items() if k.startswith("fast_rcnn/")} == \
        {"fast_rcnn/cls_accuracy": 2 / 6, "fast_rcnn/fg_cls_accuracy": 1 / 4, "fast_rcnn/false_negative": 1 / 4}
    mine = _Storage()
    bp.log_classification_stats(prefix="stt", storage=mine)
    assert sorted(mine.scalars) == ["stt/cls_accuracy", "stt/false_negative", "stt/fg_cls_accuracy"]


def test_cpu_statistics_without_foreground_rows_put_only_the_accuracy():
    bp = _predictor(3)
    scores = torch.tensor([[0., 0., 0., 2.], [1., 0., 0., 0.], [0., 0., 0., 0.5]])
    bp.losses((scores, torch.zeros(3, 4)), [_proposals([3, 3, 3])])
    mine = _Storage()
    assert bp.log_classification_stats(storage=mine) == {"cls_accuracy": 2 / 3}
    assert mine.scalars == {"fast_rcnn/cls_accuracy": 2 / 3}
    # a call without proposals clears them (upstream returns early for num_instances == 0)
    bp.losses((scores[:0], torch.zeros(0, 4)), [])
    mine = _Storage()
    assert bp.log_classification_stats(storage=mine) == {} and mine.scalars == {}


def test_cpu_statistics_skip_ignored_rows_like_upstream():
    bp = _predictor(3)
    scores = torch.tensor([[3., 0., 0., 0.], [0., 3., 0., 0.], [0., 0., 0., 1.]])
    bp.losses((scores, torch.zeros(3, 4)), [_proposals([0, -100, 3])])
    # (num_instances counts every row, the ignored one included, as gt_classes.numel() upstream)
    assert bp.classification_stats() == {"cls_accuracy": 2 / 3, "fg_cls_accuracy": 1.0, "false_negative": 0.0}


def test_ops_cls_loss_rejects_host_tensors():
    from locov_amd import ops
    from locov_amd._lib import LocovError
    with pytest.raises(LocovError):
        ops.cls_loss(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.cls_loss([[0.0]], torch.zeros(1, dtype=torch.int64))
