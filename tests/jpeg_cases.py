"""The JPEG fixture (tests/golden/g14_jpeg.npz, written by tests/golden/make_golden_g14.py) as Python objects, shared by the host,
sanitizer and GPU tests of the JPEG decoder.  Plain helper module: no fixture is registered and nothing is patched on import."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_jpeg.npz")

# kind -> what the refusal must say: the header's reason, or the entropy stage's status
REFUSALS = {
    "progressive": "SOF2 or above",
    "cut": ("the header ends before the scan", "the data runs out inside the scan", "a marker inside the scan"),
    "no_eoi": "no EOI behind the scan",
    "sampling": "sampling layout outside",
    "png": "not a JPEG stream",
}


class Stream(NamedTuple):
    name: str
    kind: str                      # "ok", "scaled" (quantisers scaled up: refused, or decoded to Pillow's bytes), or a key of REFUSALS
    data: bytes
    rgb: Optional[np.ndarray]      # Pillow's decode, [height, width, 3]; None unless kind is "ok" or "scaled"

    @property
    def grey(self) -> bool:
        return "_grey_" in self.name


_CACHE = {}


def streams():
    """Every stream of the fixture, read once."""
    if "all" not in _CACHE:
        with np.load(GOLDEN) as z:
            f = {k: z[k] for k in z.files}
        out = []
        for i, name in enumerate(f["names"]):
            data = f["data"][f["data_off"][i]:f["data_off"][i + 1]].tobytes()
            kind = str(f["kind"][i])
            rgb = None
            if kind in ("ok", "scaled"):
                rgb = f["rgb"][f["rgb_off"][i]:f["rgb_off"][i + 1]].reshape(int(f["height"][i]), int(f["width"][i]), 3)
            out.append(Stream(str(name), kind, data, rgb))
        _CACHE["all"] = out
        _CACHE["versions"] = (str(f["pillow_version"]), str(f["libjpeg_turbo_version"]))
    return _CACHE["all"]


def supported():
    return [s for s in streams() if s.kind == "ok"]


def fallbacks():
    return [s for s in streams() if s.kind not in ("ok", "scaled")]


def scaled():
    return [s for s in streams() if s.kind == "scaled"]


def by_name(name: str) -> Stream:
    return next(s for s in streams() if s.name == name)


def guard_case() -> bytes:
    """The 17x23 quality-100 noise stream with every quantiser patched to 255: its dequantised coefficients leave the magnitude
    guard (jpeg.MAX_DEQUANTISED), where libjpeg-turbo's 16-bit SIMD and the C code part ways."""
    data = bytearray(by_name("noise_17x23_420_q100").data)
    at, found = 2, 0
    while data[at + 1] != 0xDA:
        seg = (data[at + 2] << 8) | data[at + 3]
        if data[at + 1] == 0xDB:
            p = at + 4
            while p < at + 2 + seg:
                assert data[p] >> 4 == 0
                data[p + 1:p + 65] = b"\xff" * 64
                p += 65
                found += 1
        at += 2 + seg
    assert found == 2
    return bytes(data)


def expected(s: Stream, fmt: str) -> np.ndarray:
    """Pillow's bytes of a supported stream in `fmt` order ("L": grey streams only, one channel)."""
    if fmt == "L":
        assert s.grey
        return np.ascontiguousarray(s.rgb[:, :, :1])
    return np.ascontiguousarray(s.rgb[:, :, ::-1]) if fmt == "BGR" else s.rgb
