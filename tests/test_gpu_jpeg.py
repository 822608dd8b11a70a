"""The JPEG decoder on the device (csrc/jpeg.hip through ops.decode_jpeg_images / ops.jpeg_decode_records) against its definition
locov_amd.jpeg -- which tests/test_jpeg_host.py holds to Pillow's bytes -- on the fixture's streams; its outputs under poisoned
allocations; its stream contract; and DatasetMapper on a cuda device against the "cpu" mapper, from files."""
import numpy as np
import pytest
import torch

import jpeg_cases as jc
import poison
import poison_cases
import stream_contract as sc
from locov_amd import jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import locov_amd
    from locov_amd import _lib
    _lib.load()
    return locov_amd


_WANT = {}


def _want(s, fmt):
    """The definition's bytes of a stream, computed once per session and shared."""
    if (s.name, fmt) not in _WANT:
        _WANT[s.name, fmt] = jpeg.decode_jpeg_host(s.data, fmt)
    return _WANT[s.name, fmt]


def _differing(got, streams, fmt):
    bad = {}
    for g, s in zip(got, streams):
        want = _want(s, fmt)
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == want.shape, (s.name, tuple(g.shape), want.shape)
        n = int((g.cpu().numpy() != want).sum())
        if n:
            bad[s.name] = n
    return bad


def test_each_stream_alone_gives_the_definitions_bytes(pkg):
    streams = jc.supported()
    got = [pkg.ops.decode_jpeg_images([s.data], "RGB", "cuda")[0] for s in streams]
    assert not _differing(got, streams, "RGB")
    grey = [s for s in streams if s.grey]
    assert not _differing([pkg.ops.decode_jpeg_images([s.data], "L", "cuda")[0] for s in grey], grey, "L")


@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_all_streams_in_one_call_give_the_definitions_bytes(pkg, fmt):
    """Every size, layout and encoder option of the fixture in one batch; the fixture's order, then reversed (other neighbours in the
    workspace and in the launch grids)."""
    streams = jc.supported()
    assert len(streams) > pkg.ops.IMAGE_BATCH_MAX_IMAGES - 8 and {"444", "422", "420", "grey"} <= {s.name.split("_")[2] for s in streams}
    for order in (streams, streams[::-1]):
        for lo in range(0, len(order), pkg.ops.IMAGE_BATCH_MAX_IMAGES):
            part = order[lo:lo + pkg.ops.IMAGE_BATCH_MAX_IMAGES]
            launches = pkg._lib.load().locov_launch_count()
            got = pkg.ops.decode_jpeg_images([s.data for s in part], fmt, "cuda")
            assert pkg._lib.load().locov_launch_count() - launches == 2
            assert not _differing(got, part, fmt)


def test_streams_with_scaled_quantisers_are_refused_or_give_pillows_bytes(pkg):
    """The fixture's quality-100 streams with multiplied quantisers: what the host stage accepts the kernels decode to Pillow's bytes
    (the fixture's, not the definition's), the rest is refused by the op."""
    scaled = jc.scaled()
    status = pkg.ops.jpeg_entropy_decode([s.data for s in scaled]).status
    accepted = [s for s, st in zip(scaled, status) if st == 0]
    assert 10 <= len(accepted) <= len(scaled) - 10 and len(accepted) <= pkg.ops.IMAGE_BATCH_MAX_IMAGES
    got = pkg.ops.decode_jpeg_images([s.data for s in accepted], "RGB", "cuda")
    bad = {s.name: n for g, s in zip(got, accepted) if (n := int((g.cpu().numpy() != jc.expected(s, "RGB")).sum()))}
    assert not bad, bad
    refused = next(s for s, st in zip(scaled, status) if st != 0)
    with pytest.raises(ValueError, match="range where"):
        pkg.ops.decode_jpeg_images([refused.data], "RGB", "cuda")


def test_grey_streams_in_one_call_as_l(pkg):
    grey = [s for s in jc.supported() if s.grey]
    assert not _differing(pkg.ops.decode_jpeg_images([s.data for s in grey], "L", "cuda"), grey, "L")


def test_the_op_refuses_what_it_does_not_take(pkg):
    one = jc.supported()[0].data
    with pytest.raises(ValueError, match="at most 64"):
        pkg.ops.decode_jpeg_images([one] * 65, "RGB", "cuda")
    for s in jc.fallbacks():
        with pytest.raises(ValueError, match="stream 1"):
            pkg.ops.decode_jpeg_images([one, s.data], "RGB", "cuda")
    with pytest.raises(ValueError, match="above 1096"):
        pkg.ops.decode_jpeg_images([jc.guard_case()], "RGB", "cuda")
    assert pkg.ops.decode_jpeg_images([], "RGB", "cuda") == []
    # the C entry point's own checks, before any launch
    batch = pkg.ops.jpeg_entropy_decode([one])
    records = batch.records.cuda()
    w, h, ncomp, hs, vs, off, size, qt = batch.descs[0]
    for bad, what in (((w, h, ncomp, hs, vs, off + 8, size, qt), "misaligned"), ((w, h, ncomp, hs, vs, off, size + 4096, qt), "does not fit"),
                      ((w, h, ncomp, 1, 2, off, size, qt), "layouts"), ((0, h, ncomp, hs, vs, off, size, qt), None),
                      ((w, h, ncomp, hs, vs, off, 4, qt), "block starts"), ((w, h, ncomp, hs, vs, off, size, records.numel()), "quantisation")):
        with pytest.raises((pkg.ops.LocovError, ValueError), match=what):
            pkg.ops.jpeg_decode_records(records, [bad], "RGB")


def _batch(pkg, names):
    streams = [jc.by_name(n) for n in names]
    return streams, pkg.ops.jpeg_entropy_decode([s.data for s in streams], pin_memory=True)


MIXED = ["mixed_70x150_420_q90", "smooth_1x1_420_q75", "noise_40x24_422_q75_rstrow", "bw_16x33_grey_q50", "smooth_33x9_444_q75",
         "noise_3x3_420_q90", "noise_17x23_420_q100", "smooth_2x35_422_q75"]


@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_poisoned_outputs_and_workspace_give_the_same_bytes(pkg, fmt):
    """Outputs and workspace come from torch.empty: under 0x00, 0x7B and 0xFF the bytes are the definition's and the guard bands on
    both sides of every allocation hold -- every byte that is read was written by the call, nothing is written outside."""
    streams, batch = _batch(pkg, MIXED)
    records = batch.records.cuda()
    for pattern in poison.PATTERNS:
        with poison.poisoned(pattern) as arenas:
            got = pkg.ops.jpeg_decode_records(records, batch.descs, fmt)
            torch.cuda.synchronize()
            assert len(arenas.arenas) == len(streams) + 1 and arenas.passed_through == 0        # the outputs and the workspace
            assert arenas.guards_intact(), arenas.broken_guards()
            assert not _differing(got, streams, fmt), pattern
    grey, gbatch = _batch(pkg, ["bw_16x33_grey_q50", "smooth_7x5_grey_q75", "noise_40x24_grey_q75_rst2"])
    for pattern in poison.PATTERNS:
        with poison.poisoned(pattern) as arenas:
            got = pkg.ops.jpeg_decode_records(gbatch.records.cuda(), gbatch.descs, "L")
            torch.cuda.synchronize()
            assert arenas.guards_intact(), arenas.broken_guards()
            assert not _differing(got, grey, "L"), pattern


# ---- the stream contract: the case of tests/poison_cases.py's shape, run by tests/stream_contract.py ---------------------------
_CASE_DESCS = []


def _case_inputs():
    from locov_amd import ops
    batch = ops.jpeg_entropy_decode([jc.by_name(n).data for n in MIXED])
    _CASE_DESCS[:] = batch.descs
    return {"records": batch.records.clone()}            # the upload is the caller's: outside the call, outside the captured part


def _case_run(d):
    from locov_amd import ops
    return ops.jpeg_decode_records(d["records"], _CASE_DESCS, "BGR")


CASE = poison_cases.Case("jpeg_decode_mixed", ("locov_jpeg_decode",), _case_inputs, _case_run)
_EAGER = {}


def _eager(monkeypatch):
    if not _EAGER:
        _EAGER["run"] = sc.run_eager(CASE, monkeypatch)
    return _EAGER["run"]


def test_the_eager_case_is_the_definition(pkg, monkeypatch):
    got = _eager(monkeypatch)[0]
    for g, n in zip(got, MIXED):
        assert np.array_equal(g.numpy(), _want(jc.by_name(n), "BGR")), n


def test_results_behind_a_delay_on_a_side_stream_equal_eager(pkg, monkeypatch):
    monkeypatch.setattr(sc, "LAUNCHING", sc.LAUNCHING | set(CASE.covers))
    want, host_ms, scales = _eager(monkeypatch)
    ms = sc.delay_ms_for(host_ms)
    got, calls = sc.run_delayed(CASE, monkeypatch, pkg._lib.load(), ms, scales)
    print(f"{CASE.name}: eager enqueue {host_ms:.2f} ms, delay {ms:.0f} ms, calls {calls}")
    assert [sym for sym, _ in calls] == ["locov_jpeg_decode"]
    assert all(pending for _, pending in calls), f"the call returned after the {ms:.0f} ms delay in front of it was over: it waited for its stream"
    poison.compare(CASE, got, want, "behind a delay on a side stream against eager")


def test_the_decoy_would_have_been_noticed(pkg, monkeypatch):
    want = _eager(monkeypatch)[0]
    got = sc.run_on_decoy(CASE, monkeypatch)                       # records of zeros: no coefficient anywhere, mid-grey images
    assert len(got) == len(want) and any(not poison.same_bits(a, b) for a, b in zip(got, want))
    assert all(int(g.min()) == int(g.max()) == 128 for g in got)


def test_capture_and_two_replays_equal_eager(pkg, monkeypatch):
    want, _, scales = _eager(monkeypatch)
    first, second = sc.run_captured(CASE, monkeypatch, scales)
    poison.compare(CASE, first, want, "first replay of the captured case against eager")
    poison.compare(CASE, second, want, "second replay of the captured case against eager")


# ---- the mapper ------------------------------------------------------------------------------------------------------------------
def _cfg(device, fmt="BGR", **inp):
    from locov_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.DEVICE = device
    for k, v in dict(MIN_SIZE_TRAIN=(40, 48, 64), MAX_SIZE_TRAIN=90, FORMAT=fmt, **inp).items():
        cfg.INPUT[k] = v
    return cfg


FILES = ["mixed_70x150_420_q90", "smooth_17x23_420_q75_progressive", "noise_40x24_420_q75_cut_scan", "smooth_9x7_png",
         "noise_40x24_422_q75_rstrow", "bw_16x33_grey_q50", "smooth_33x9_444_q75", "noise_40x24_420_q75_cut", "smooth_17x23_420_q75_segments",
         "noise_40x24_420_q75_noeoi"]
ALL_ON = dict(COLOR_JITTER=0.4, RANDOM_GRAY_SCALE=True, GAUSSIAN_BLUR=True, RANDOM_ERASE=True)


def _files(tmp_path, names):
    dicts = []
    for i, n in enumerate(names):
        path = tmp_path / f"{i:03d}_{n}.{'png' if n.endswith('png') else 'jpg'}"
        path.write_bytes(jc.by_name(n).data)
        w, h = (int(v) for v in n.split("_")[1].split("x"))        # (as a dataset's json holds them: the black image's size)
        dicts.append({"file_name": str(path), "image_id": i, "height": h, "width": w, "caption": ["one", "two"],
                      "annotations": [{"bbox": [1.0, 2.0, 6.0, 4.0], "bbox_mode": 1, "category_id": 3}]})
    return dicts


def _same(got, want, device_images=True):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["image"].is_cuda == device_images and torch.equal(g["image"].cpu(), w["image"].cpu()), g["file_name"]
        assert (g["height"], g["width"], g["caption"]) == (w["height"], w["width"], w["caption"]), g["file_name"]
        assert torch.equal(g["instances"].gt_boxes.tensor.cpu(), w["instances"].gt_boxes.tensor.cpu())


@pytest.mark.parametrize("fmt", ["BGR", "RGB"])
def test_map_batch_from_files_equals_the_cpu_mapper(pkg, tmp_path, monkeypatch, fmt):
    """One batch of supported streams, a progressive one, truncated ones (the black image, "A black image."), a stream without EOI
    and a PNG: the cuda mapper's dicts are the "cpu" mapper's, which reads every file with Pillow."""
    import PIL.Image  # noqa: F401  (the cpu mapper reads with Pillow: no skip, a machine without it fails here)
    from locov_amd import data
    dicts = _files(tmp_path, FILES)
    on_device, on_host = data.DatasetMapper(_cfg("cuda", fmt), True, device="cuda", seed=5), data.DatasetMapper(_cfg("cpu", fmt), True, device="cpu", seed=5)
    sample = on_device.draw_sample(dicts)
    reads, plain_read = [], data._read_file
    monkeypatch.setattr(data, "_read_file", lambda path, f: (reads.append(path), plain_read(path, f))[1])
    decoded = []
    monkeypatch.setattr(pkg.ops, "jpeg_decode_records", lambda r, descs, f, _op=pkg.ops.jpeg_decode_records: (decoded.append(len(descs)), _op(r, descs, f))[1])
    got = on_device.map_batch(dicts, sample)
    device_path = [n for n in FILES if jc.by_name(n).kind == "ok"]
    assert decoded == [len(device_path)] and on_device._decoded == {}
    assert reads == [d["file_name"] for d, n in zip(dicts, FILES) if n not in device_path]         # Pillow answers for the rest, once each
    want = on_host.map_batch(dicts, sample)
    _same(got, want)
    black = [i for i, n in enumerate(FILES) if "_cut" in n or "_noeoi" in n]                       # (Pillow refuses a file without EOI too)
    assert all(got[i]["caption"] == "A black image." and not got[i]["image"].any() for i in black)
    assert sum(g["caption"] == "A black image." for g in got) == len(black) == 3
    # the switch: everything through Pillow, the same dicts
    monkeypatch.setenv("LOCOV_FUSED_JPEG", "0")
    del reads[:], decoded[:]
    off = on_device.map_batch(dicts, sample)
    assert decoded == [] and reads == [d["file_name"] for d in dicts]
    _same(off, want)


def test_map_batch_from_files_with_train_aug_equals_the_cpu_mapper(pkg, tmp_path, monkeypatch):
    import PIL.Image  # noqa: F401  (the cpu mapper reads with Pillow: no skip, a machine without it fails here)
    from locov_amd import data
    from locov_amd import strong_augment as sa
    dicts = _files(tmp_path, FILES)
    cfg = _cfg("cuda", **ALL_ON)
    aug = sa.build_complete_augmentation(cfg, True)
    on_device = data.DatasetMapper(cfg, True, device="cuda", seed=7, train_aug=aug)
    on_host = data.DatasetMapper(_cfg("cpu", **ALL_ON), True, device="cpu", seed=7, train_aug=aug)
    reads, plain_read = [], data._read_file
    monkeypatch.setattr(data, "_read_file", lambda path, f: (reads.append(path), plain_read(path, f))[1])
    sample = on_device.draw_sample(dicts)                          # the erasers' sizes come from the entropy stage's verdict
    host_sample = on_host.draw_sample(dicts)
    assert [tuple(s["erase"]) for s in sample["strong"]] == [tuple(s["erase"]) for s in host_sample["strong"]]
    del reads[:]
    on_device.draw_sample(dicts)
    device_path = [n for n in FILES if jc.by_name(n).kind == "ok"]
    assert reads == [d["file_name"] for d, n in zip(dicts, FILES) if n not in device_path]
    got = on_device.map_batch(dicts)                               # draws again with the mapper's own generator: the whole path in one call
    assert all(g["image"].is_cuda for g in got) and on_device._decoded == {}
    sample = on_device.draw_sample(dicts)
    sample["erase_noise"] = on_device.erase_noise(sample).cpu()
    _same(on_device.map_batch(dicts, sample), on_host.map_batch(dicts, sample))
    monkeypatch.setenv("LOCOV_FUSED_JPEG", "0")
    _same(on_device.map_batch(dicts, sample), on_host.map_batch(dicts, sample))


def test_a_batch_of_65_files_is_split_by_the_mapper(pkg, tmp_path, monkeypatch):
    import PIL.Image  # noqa: F401  (the cpu mapper reads with Pillow: no skip, a machine without it fails here)
    from locov_amd import data
    names = [s.name for s in jc.supported()]
    names = (names + names)[:pkg.ops.IMAGE_BATCH_MAX_IMAGES + 1]
    dicts = _files(tmp_path, names)
    on_device, on_host = data.DatasetMapper(_cfg("cuda"), True, device="cuda", seed=2), data.DatasetMapper(_cfg("cpu"), True, device="cpu", seed=2)
    decoded = []
    monkeypatch.setattr(pkg.ops, "jpeg_decode_records", lambda r, descs, f, _op=pkg.ops.jpeg_decode_records: (decoded.append(len(descs)), _op(r, descs, f))[1])
    sample = on_device.draw_sample(dicts)
    got = on_device.map_batch(dicts, sample)
    assert decoded == [64, 1]
    _same(got, on_host.map_batch(dicts, sample))
