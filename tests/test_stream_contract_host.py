"""The tables of tests/stream_cases.py against the case table and the sources they cite (no GPU): every case is captured or has a
written reason, the caps on the exceptions hold, and the header names the exceptions the tables name."""
import os
import re

import stream_cases
import stream_contract
from poison_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {c.name for c in CASES}
BY_NAME = {c.name: c for c in CASES}


def _source(cite):
    """(the cited line, the whole file with runs of whitespace and comment leaders folded) of a 'path:line' citation."""
    path, line = cite.rsplit(":", 1)
    with open(os.path.join(ROOT, path)) as f:
        text = f.read()
    lines = text.split("\n")
    assert 1 <= int(line) <= len(lines), cite
    return lines[int(line) - 1], " ".join(re.sub(r"^\s*(#|//)", " ", ln) for ln in lines).split()


def test_every_case_is_captured_or_has_a_reason_and_none_is_both():
    captured = {c.name for c in stream_cases.capture_set(CASES)}
    left_out = set(stream_cases.HOST_READS) | set(stream_cases.NOT_CAPTURABLE)
    assert captured | left_out == NAMES
    assert not captured & left_out
    assert not set(stream_cases.HOST_READS) & set(stream_cases.NOT_CAPTURABLE)


def test_every_name_in_every_table_is_a_case():
    late = {case for case, _ in stream_cases.LATE_CALLS}
    for table in (stream_cases.HOST_READS, stream_cases.NOT_CAPTURABLE, stream_cases.OWN_DECOY, stream_cases.INSENSITIVE, late):
        assert set(table) <= NAMES, sorted(set(table) - NAMES)
    # a late call needs a documented host read to come after, and is a symbol the case covers
    for case, symbol in stream_cases.LATE_CALLS:
        assert case in stream_cases.HOST_READS and symbol in BY_NAME[case].covers, (case, symbol)


def test_the_caps_hold():
    assert len(set(stream_cases.HOST_READS) | set(stream_cases.NOT_CAPTURABLE)) <= stream_cases.MAX_NOT_CAPTURED == 30
    assert len(stream_cases.INSENSITIVE) <= stream_cases.MAX_INSENSITIVE == 8


def test_every_host_read_cites_a_line_that_reads_and_a_sentence_that_is_there():
    for name, (cite, sentence) in stream_cases.HOST_READS.items():
        assert cite and sentence.strip(), name
        line, words = _source(cite)
        assert any(tok in line for tok in stream_cases.HOST_READ_TOKENS), f"{name}: {cite} is no host read: {line.strip()!r}"
        assert " ".join(sentence.split()) in " ".join(words), f"{name}: {cite.rsplit(':', 1)[0]} does not say {sentence!r}"


def test_every_other_reason_is_written_and_cites_its_source():
    for name, (cite, who, reason) in stream_cases.NOT_CAPTURABLE.items():
        assert len(reason.split()) >= 8, name
        assert who in (stream_cases.ENTRY_POINT, stream_cases.WRAPPER, stream_cases.RUNTIME), name
        line, _ = _source(cite)
        # an entry point's or the runtime's reason cites the HIP call in the kernel source, a wrapper's the Python line
        assert ("hipMem" in line) if who != stream_cases.WRAPPER else cite.split(":")[0].endswith(".py") and line.strip(), f"{name}: {cite}"
    for name, reason in stream_cases.INSENSITIVE.items():
        assert len(reason.split()) >= 8, name


def test_the_header_names_the_exceptions_the_tables_name():
    covered = {sym for name, (_, who, _) in stream_cases.NOT_CAPTURABLE.items() if who == stream_cases.ENTRY_POINT
               for sym in BY_NAME[name].covers}
    assert set(stream_cases.HEADER_EXCEPTIONS) == covered
    with open(os.path.join(ROOT, "include", "locov_hip.h")) as f:
        header = f.read()
    start = header.index("Conventions")
    conventions = header[start:header.index("*/", start)]
    exceptions = conventions.split("Exception", 1)[1].split("\n *   - ", 1)[0]                 # up to the next bullet
    named = set(re.findall(r"locov_[a-z0-9_]+", exceptions))
    timing = {n for n in named if n.startswith("locov_gemm_timing")}
    assert timing, "the timing aid is the first exception"
    assert named - timing == covered, (sorted(named - timing), sorted(covered))


def test_every_own_decoy_has_the_structure_of_build():
    for name, builder in stream_cases.OWN_DECOY.items():
        want, got = BY_NAME[name].build(), builder()
        assert type(got) is type(want) and set(got) == set(want), name
        for key in want:
            w, g = stream_contract.tensors_of(want[key]), stream_contract.tensors_of(got[key])
            if not w:
                assert got[key] == want[key], (name, key)
                continue
            assert len(w) == len(g), (name, key)
            for a, b in zip(w, g):
                assert not b.is_cuda and a.shape == b.shape and a.dtype == b.dtype, (name, key)


def test_the_zero_decoy_keeps_structure_shapes_and_dtypes_and_every_host_value():
    for case in CASES:
        if case.name in stream_cases.OWN_DECOY:
            continue
        want, got = case.build(), stream_contract.decoy_inputs(case)
        assert set(got) == set(want)
        for key in want:
            w, g = stream_contract.tensors_of(want[key]), stream_contract.tensors_of(got[key])
            assert [(t.shape, t.dtype) for t in w] == [(t.shape, t.dtype) for t in g]
            assert all(not bool(t.any()) for t in g)
            if not w:
                assert got[key] == want[key]


def test_delay_is_sized_with_a_margin_and_a_floor():
    assert stream_contract.delay_ms_for(0.0) == stream_contract.FLOOR_MS >= 20.0
    assert stream_contract.delay_ms_for(100.0) == stream_contract.FACTOR * 100.0 and stream_contract.FACTOR >= 2.0
