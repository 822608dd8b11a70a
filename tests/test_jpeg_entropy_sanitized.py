"""The host stage of the JPEG decoder (csrc/jpeg_entropy.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program: tools/jpeg_entropy_check.cpp is compiled with g++ and run as a subprocess over the fixture's streams, every truncation of
two of them and a few hundred seeded single-byte corruptions of one.  Nothing here is loaded into python and nothing is preloaded."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the sanitized build of tools/jpeg_entropy_check.cpp needs it")
    exe = str(tmp_path_factory.mktemp("jpeg_check") / "jpeg_entropy_check")
    # (the sanitizer runtimes are linked into the program itself: it runs the same whatever else the process is started with)
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
           "-static-libasan", "-static-libubsan",
           "-Wall", "-Wextra", os.path.join(ROOT, "tools", "jpeg_entropy_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    return exe


def _run(exe, directory):
    """{file name: (supported, reason, status, record bytes)} of a clean run: exit status 0 and no sanitizer report."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(directory)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        name, *fields = line.split()
        kv = dict(f.split("=") for f in fields)
        out[name] = (int(kv["supported"]), int(kv["reason"]), int(kv["status"]), int(kv["record_bytes"]))
    return out


def test_the_fixtures_streams_decode_clean(checker, tmp_path):
    from locov_amd import jpeg
    for s in jc.streams():
        (tmp_path / s.name).write_bytes(s.data)
    (tmp_path / "guard").write_bytes(jc.guard_case())
    (tmp_path / "empty").write_bytes(b"")
    got = _run(checker, tmp_path)
    assert len(got) == len(jc.streams()) + 2
    for s in jc.streams():
        supported, reason, status, record_bytes = got[s.name]
        want = jpeg.parse_jpeg(s.data)
        assert (bool(supported), reason) == (want.supported, want.reason), s.name
        assert (record_bytes > 0) == (status == 0) and record_bytes % 16 == 0, (s.name, status)
        assert status == jpeg.entropy_decode_host(s.data)[0] if want.supported else status == jpeg.STATUS_UNSUPPORTED, (s.name, status)
        assert s.kind == "scaled" or (status == 0) == (s.kind == "ok"), (s.name, status)
    assert got["guard"][2] == jpeg.STATUS_MAGNITUDE and got["empty"][:2] == (0, jpeg.REASON_NOT_JPEG)


@pytest.mark.parametrize("name", ["noise_40x24_420_q75_rst2", "smooth_33x9_422_q5_optimize"])
def test_every_truncation_ends_in_a_status(checker, tmp_path, name):
    data = jc.by_name(name).data
    for n in range(len(data)):
        (tmp_path / f"{n:05d}").write_bytes(data[:n])
    got = _run(checker, tmp_path)
    assert len(got) == len(data)
    assert all(status < 0 and record_bytes == 0 for _, _, status, record_bytes in got.values()), \
        [k for k, v in got.items() if v[2] >= 0]                       # a stream without its last byte has no EOI


def test_corrupted_streams_end_in_a_status(checker, tmp_path):
    data = jc.by_name("mixed_70x150_420_q90").data
    rng = np.random.default_rng(1407)
    header_end = data.index(b"\xff\xda")
    places = np.concatenate([rng.integers(2, header_end + 14, 150), rng.integers(header_end + 14, len(data), 250)])
    for k, at in enumerate(places):
        bad = bytearray(data)
        bad[at] ^= int(rng.integers(1, 256))
        (tmp_path / f"{k:03d}_{at}").write_bytes(bytes(bad))
    got = _run(checker, tmp_path)
    assert len(got) == len(places)
    decoded = sum(v[2] == 0 for v in got.values())
    assert 0 < decoded < len(places)                                   # a flipped coefficient bit still decodes; a broken table or marker does not
    assert all((v[3] > 0) == (v[2] == 0) and -8 <= v[2] <= 0 for v in got.values())
