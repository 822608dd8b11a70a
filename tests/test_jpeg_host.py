"""The JPEG decoder without a GPU: locov_amd.jpeg (the definition) against Pillow's bytes, and the library's host stage
(csrc/jpeg_entropy.h through ops.jpeg_parse / ops.jpeg_entropy_decode) against the definition.  The streams are the fixture's
(tests/golden/g14_jpeg.npz: every size, layout and encoder option of make_golden_g14.py)."""
import io

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from locov_amd import data, jpeg, ops
from locov_amd.config import get_cfg


def _diff(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (got.shape, want.shape)
    return int((got != want).sum())


@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_the_definition_gives_pillows_bytes_of_the_fixture(fmt):
    assert len(jc.supported()) >= 60
    bad = {s.name: n for s in jc.supported() if (n := _diff(jpeg.decode_jpeg_host(s.data, fmt), jc.expected(s, fmt)))}
    assert not bad, f"streams with differing bytes ({fmt}): {bad}"


def test_a_grey_stream_as_l_is_one_channel_and_a_colour_stream_as_l_is_refused():
    grey = [s for s in jc.supported() if s.grey]
    assert len(grey) >= 8
    for s in grey:
        assert _diff(jpeg.decode_jpeg_host(s.data, "L"), jc.expected(s, "L")) == 0, s.name
    with pytest.raises(ValueError, match="host path"):
        jpeg.decode_jpeg_host(jc.by_name("smooth_17x23_420_q75").data, "L")


def test_the_definition_gives_a_live_pillows_bytes():
    Image = pytest.importorskip("PIL.Image")
    for s in jc.supported():
        live = np.asarray(Image.open(io.BytesIO(s.data)).convert("RGB"))
        assert _diff(jpeg.decode_jpeg_host(s.data, "RGB"), live) == 0, s.name
    # sizes around every rule of the upsampling, each layout, fresh noise
    rng = np.random.default_rng(14)
    for w, h in [(1, 1), (2, 2), (3, 5), (4, 4), (5, 4), (6, 3), (15, 17), (16, 16), (17, 15), (31, 33), (48, 8)]:
        for sub in ("4:4:4", "4:2:2", "4:2:0"):
            buf = io.BytesIO()
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, "JPEG", quality=int(rng.choice([20, 60, 92])), subsampling=sub)
            live = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
            assert _diff(jpeg.decode_jpeg_host(buf.getvalue(), "RGB"), live) == 0, (w, h, sub)


def test_the_library_parses_a_header_as_the_definition_does():
    for s in jc.streams() + [jc.Stream("guard", "ok", jc.guard_case(), None)]:
        want, got = jpeg.parse_jpeg(s.data), ops.jpeg_parse(s.data)
        assert (bool(got.supported), got.reason) == (want.supported, want.reason), s.name
        assert want.supported == (s.kind in ("ok", "scaled", "no_eoi") or s.name.endswith("cut_scan")), (s.name, want.why)
        if not want.supported:
            continue
        for field in ("width", "height", "ncomp", "restart_interval", "scan_start"):
            assert getattr(got, field) == getattr(want, field), (s.name, field)
        for field in ("comp_id", "comp_h", "comp_v", "comp_tq", "comp_td", "comp_ta"):
            assert list(getattr(got, field)) == getattr(want, field), (s.name, field)
        for field in ("qt_present", "qt", "dc_present", "ac_present", "dc_counts", "ac_counts", "dc_symbols", "ac_symbols"):
            assert np.array_equal(np.ctypeslib.as_array(getattr(got, field)), getattr(want, field)), (s.name, field)
        assert want.components == [(want.comp_id[c], want.comp_h[c], want.comp_v[c], want.comp_tq[c]) for c in range(want.ncomp)]


def test_the_library_decodes_the_scans_into_the_definitions_records():
    every = jc.streams()
    batch = ops.jpeg_entropy_decode([s.data for s in every])                   # one batched call: the threads
    assert [i for i in batch.index if every[i].kind != "scaled"] == [i for i, s in enumerate(every) if s.kind == "ok"]
    for i, s in enumerate(every):
        status, record = jpeg.entropy_decode_host(s.data)
        assert batch.status[i] == status, (s.name, batch.status[i], status)
        if status != jpeg.STATUS_OK:
            assert batch.record(i) is None
            continue
        got = batch.record(i)
        assert got.size % 4 == 0 and got.size - record.size < 4 and not got[record.size:].any(), s.name
        assert np.array_equal(got[:record.size], record), s.name
        nb = jpeg.parse_jpeg(s.data).nblocks
        assert record[0] == 0 and record[nb] == record.size - nb - 1 and (np.diff(record[:nb + 1].astype(np.int64)) >= 0).all()
    # alone, each stream gives what it gave in the batch
    for i in (0, 5, len(every) - 3):
        alone = ops.jpeg_entropy_decode([every[i].data])
        assert alone.status == [batch.status[i]]
        if batch.status[i] == 0:
            assert np.array_equal(alone.record(0), batch.record(i))


@pytest.mark.parametrize("s", jc.fallbacks(), ids=[s.name for s in jc.fallbacks()])
def test_every_fallback_case_is_refused_with_its_reason(s):
    reasons = jc.REFUSALS[s.kind]
    reasons = (reasons,) if isinstance(reasons, str) else reasons
    ok, why = jpeg.stream_supported(s.data)
    assert not ok and any(r in why for r in reasons), why
    with pytest.raises(ValueError) as e:
        jpeg.decode_jpeg_host(s.data, "RGB")
    assert why in str(e.value)
    with pytest.raises(ValueError) as e:                                       # the op refuses before it asks for a GPU
        ops.decode_jpeg_images([jc.supported()[0].data, s.data], "RGB", "cpu")
    assert "stream 1" in str(e.value) and why in str(e.value)


def test_a_stream_past_the_magnitude_guard_is_not_supported():
    base = jc.by_name("noise_17x23_420_q100")
    assert jpeg.stream_supported(base.data) == (True, "decoded")
    guard = jc.guard_case()
    assert jpeg.parse_jpeg(guard).supported                                    # the header alone cannot know
    assert jpeg.stream_supported(guard) == (False, jpeg.STATUSES[jpeg.STATUS_MAGNITUDE])
    assert ops.jpeg_entropy_decode([guard]).status == [jpeg.STATUS_MAGNITUDE]
    with pytest.raises(ValueError, match=f"above {jpeg.MAX_DEQUANTISED}"):
        ops.decode_jpeg_images([guard], "RGB", "cpu")
    # the limit itself: the largest magnitude at which pass 1's results stay inside 16 bits, below the 32-bit limit of both passes
    l1 = 61214
    assert (l1 * jpeg.MAX_DEQUANTISED + 1024) >> 11 <= 32767 < (l1 * (jpeg.MAX_DEQUANTISED + 1) + 1024) >> 11
    assert l1 * ((l1 * 1173 + 1024) >> 11) + (1 << 17) < 2 ** 31 <= l1 * ((l1 * 1174 + 1024) >> 11) + (1 << 17)
    # ... and 61214 is the largest absolute row sum of the pass (the final outputs'; the definition's own arithmetic on unit inputs)
    basis = jpeg._idct_1d(np.eye(8, dtype=np.int64) << 20, 20)                 # [input, output] weights, scaled by 2^13
    assert int(np.abs(basis).sum(axis=0).max()) == l1


def test_streams_with_scaled_quantisers_are_refused_or_give_pillows_bytes():
    """Quality-100 noise with its quantisers multiplied by 3, 4 and 6 reconstructs far outside [0, 255]: past |x| = 512 libjpeg's
    range-limit table wraps where libjpeg-turbo's SIMD code saturates.  The per-block guard refuses exactly the blocks that get
    there, so every such stream is either refused (by the definition and by the library alike) or decoded to Pillow's bytes."""
    scaled = jc.scaled()
    batch = ops.jpeg_entropy_decode([s.data for s in scaled])
    accepted = refused = 0
    for i, s in enumerate(scaled):
        ok, why = jpeg.stream_supported(s.data)
        assert (batch.status[i] == jpeg.STATUS_OK) == ok, s.name
        if not ok:
            assert batch.status[i] == jpeg.STATUS_MAGNITUDE and why == jpeg.STATUSES[jpeg.STATUS_MAGNITUDE], (s.name, why)
            refused += 1
            continue
        accepted += 1
        assert _diff(jpeg.decode_jpeg_host(s.data, "RGB"), jc.expected(s, "RGB")) == 0, s.name
        # every block of an accepted stream is inside the range where the table is the clamp
        h = jpeg.parse_jpeg(s.data)
        record = batch.record(i)
        nb = h.nblocks
        coef = np.zeros((nb, 64), np.int64)
        owner = np.repeat(np.arange(nb), np.diff(record[:nb + 1].astype(np.int64)))
        entries = record[nb + 1:nb + 1 + int(record[nb])]
        coef[owner, (entries >> 16) & 63] = (entries & 0xFFFF).astype(np.uint16).view(np.int16)
        at = 0
        for c in range(h.ncomp):
            bw, bh = h.plane_blocks(c)
            deq = coef[at:at + bw * bh] * h.qt[h.comp_tq[c]].astype(np.int64)
            assert all(jpeg.block_in_range(b) for b in deq), s.name
            at += bw * bh
    assert accepted >= 10 and refused >= 10, (accepted, refused)
    # the bound behind the cheap half of the guard, on its worst case: all weight on the inputs with the largest weights
    W = np.array(jpeg.IDCT_WEIGHTS, np.int64)
    basis = np.abs(jpeg._idct_1d(np.eye(8, dtype=np.int64) << 20, 20))         # [input, output]
    assert [int(v) for v in basis.max(axis=1)] == list(jpeg.IDCT_WEIGHTS) and int(W.sum()) == 83241
    assert jpeg.RANGE_SUM_LIMIT / 2 ** 29 + W.sum() / 2 ** 18 + 0.5 <= 511 and jpeg.RANGE_SUM_LIMIT // 8192 // 2048 + 1 <= jpeg.MAX_PASS1
    rng = np.random.default_rng(3)
    for _ in range(200):                                                       # blocks at the limit: the exact condition holds
        d = np.zeros(64, np.int64)
        idx = rng.choice(64, int(rng.integers(1, 9)), replace=False)
        w = W[idx >> 3] * W[idx & 7]
        share = rng.dirichlet(np.ones(len(idx))) * jpeg.RANGE_SUM_LIMIT
        d[idx] = np.minimum(share // w, jpeg.MAX_DEQUANTISED) * rng.choice([-1, 1], len(idx))
        assert int((W[np.arange(64) >> 3] * W[np.arange(64) & 7] * np.abs(d)).sum()) <= jpeg.RANGE_SUM_LIMIT
        assert jpeg.block_in_range(d)
    # a quantiser of 0 cannot hide a runaway DC: the quantised value is bounded on its own
    assert jpeg.MAX_QUANTISED_DC == 32767


def test_the_op_refuses_more_than_one_batch_and_unknown_formats():
    one = jc.supported()[0].data
    with pytest.raises(ValueError, match="at most 64"):
        ops.decode_jpeg_images([one] * 65, "RGB", "cpu")
    with pytest.raises(ValueError, match="format"):
        ops.decode_jpeg_images([one], "YUV", "cpu")
    with pytest.raises(ValueError, match="Pillow's conversion"):
        ops.decode_jpeg_images([jc.by_name("smooth_17x23_420_q75").data], "L", "cpu")
    with pytest.raises(ops.LocovError, match="ROCm GPU"):
        ops.decode_jpeg_images([one], "RGB", "cpu")


def test_a_cpu_mapper_reads_files_exactly_as_before(tmp_path, monkeypatch):
    """device="cpu": every file goes through _read_file, once, and no entry point of the JPEG decoder is touched."""
    import PIL.Image  # noqa: F401  (the cpu mapper reads with Pillow: no skip, a machine without it fails here)
    names = ["smooth_40x24_420_q75", "smooth_17x23_420_q75_progressive", "noise_40x24_420_q75_cut_scan", "smooth_9x7_png", "bw_16x33_grey_q50"]
    dicts = []
    for n in names:
        path = tmp_path / (n + (".png" if n.endswith("png") else ".jpg"))
        path.write_bytes(jc.by_name(n).data)
        dicts.append({"file_name": str(path), "caption": ["one", "two"]})
    dicts[2].update(height=24, width=40)                                       # (the black image's size)
    cfg = get_cfg()
    cfg.MODEL.DEVICE = "cpu"
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.FORMAT = (0,), "BGR"
    reads, plain_read = [], data._read_file
    monkeypatch.setattr(data, "_read_file", lambda path, fmt: (reads.append(path), plain_read(path, fmt))[1])
    for name in ("jpeg_parse", "jpeg_entropy_stage", "jpeg_pack", "jpeg_decode_records", "decode_jpeg_images"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a CPU mapper called the JPEG decoder"))
    mapper = data.DatasetMapper(cfg, True, device="cpu", seed=3)
    out = mapper.map_batch(dicts)
    assert reads == [d["file_name"] for d in dicts] and mapper._decoded == {}
    assert [o["caption"] == "A black image." for o in out] == [False, False, True, False, False]
    assert not out[2]["image"].any() and tuple(out[2]["image"].shape) == (3, 24, 40)
    sample ={"short_edge": [0] * 5, "flip": [False] * 5, "caption": [0] * 5}
    out = mapper.map_batch(dicts, sample)
    want = np.ascontiguousarray(jc.expected(jc.by_name(names[0]), "BGR").transpose(2, 0, 1))
    assert np.array_equal(out[0]["image"].numpy(), want) and (out[0]["height"], out[0]["width"]) == (24, 40)
    assert np.array_equal(out[4]["image"].numpy(), jc.expected(jc.by_name(names[4]), "BGR").transpose(2, 0, 1))
    assert torch.equal(out[1]["image"], torch.from_numpy(np.ascontiguousarray(plain_read(dicts[1]["file_name"], "BGR").transpose(2, 0, 1))))
