"""Baseline JPEG decoding, restated: the DEFINITION of the device decoder (ops.decode_jpeg_images: csrc/jpeg_entropy.h, csrc/jpeg.hip).

As in data.py the numpy path of this module is the definition, and its bytes are Pillow's (libjpeg-turbo's defaults: the "islow"
inverse DCT, fancy upsampling, the 16-bit fixed-point colour tables):

  parse_jpeg(data)          the header: size, components, tables, restart interval, where the scan starts, and `supported`
  entropy_decode_host(data) the scan as the sparse coefficient record the device takes (below)
  decode_jpeg_host(data, fmt)  HWC uint8 in INPUT.FORMAT order ("RGB", "BGR", or "L" for a grey stream)

Supported: SOF0 / SOF1 (8-bit, Huffman), one component or three with chroma 1x1 and luma (h, v) in {(1, 1), (2, 1), (2, 2)}, one
interleaved scan, DRI / RSTn, any DHT, 0xFF00 stuffing, fill bytes in front of a marker, APPn / COM.  Everything else is
`supported = False` with a reason, and any anomaly inside the scan is a negative status: for those Pillow answers, with its own
error semantics -- this decoder never guesses what libjpeg's recovery would do.

The record of one image (uint32 words): block_start[nblocks + 1], then one word per non-zero quantised coefficient,
(natural-order index << 16) | (value & 0xFFFF), the DC prediction already undone.  Blocks are in component-plane raster order over
the MCU-padded grid (component 0's plane, then 1's, then 2's); block b's words are [block_start[b], block_start[b + 1]), counted
from the first entry, in the order the scan holds them (zigzag).

The pixel pipeline (restated from libjpeg's public jidctint.c, jdsample.c, jdcolor.c, jdmaster.c):
  * dequantise, then the "islow" IDCT: CONST_BITS 13, PASS1_BITS 2, a column pass descaled by 11, a row pass descaled by 18, the
    result looked up in the range-limit table at (x & 1023) -- the table already holds the +128 level shift;
  * a component with half the luma's width is upsampled by the "fancy" triangle filters when its real width exceeds 2 samples
    (jdsample.c: `do_fancy && downsampled_width > 2`), else by replication; neighbours are clamped at the component's real
    downsampled size ceil(W * h / hmax) x ceil(H * v / vmax), not at the MCU-padded plane;
  * YCbCr -> RGB through the fixed-point tables, then a clamp; grey is replicated.

The magnitude guards: which streams are decoded at all.  libjpeg's C code and libjpeg-turbo's SIMD code are the same function only
inside a range, and this decoder takes no stream outside it (STATUS_MAGNITUDE; Pillow decodes it):
  * per coefficient, |dequantised| <= MAX_DEQUANTISED = 1096 (and |quantised DC| <= 32767 whatever the quantiser).  Both IDCT passes
    are the same linear map of 8 inputs; every intermediate of jidctint's flow graph is a linear functional of them, and the largest
    sum of absolute weights over all of them is 61214 = 7.4724 * 2^13 (the final outputs' own).  With |d| <= M, pass 1 ends at
    |ws| <= (61214 * M + 2^10) >> 11 and every pass-2 value below 61214 * |ws|max + 2^17: below 2^31 up to M = 1173, and with pass 1
    inside 16 bits up to M = 1096.  No 32-bit value of either pass can overflow for an accepted stream.
  * per block, the range limit.  The C code looks the descaled pass-2 result x up in a table at (x & 1023), which WRAPS; the SIMD code
    saturates (pack with signed saturation, then + 128).  The two agree exactly for x in [-512, 511].  With W_k the largest absolute
    weight of input k in the one-dimensional pass (IDCT_WEIGHTS: 8192 for k = 0 and 4, up to 11363 for the others, scaled by 2^13),
        |ws| <= sum_k W_k |d_kl| / 2^11 + 1      and      |x| <= sum_l W_l |ws_l| / 2^18 + 1/2 <= S / 2^29 + 0.82,
        S = sum_kl W_k W_l |d_kl|                (sum_l W_l = 83241 < 0.32 * 2^18),
    so S <= RANGE_SUM_LIMIT = 510 * 2^29 keeps every x inside [-511, 511] -- and every pass-1 value below 510 * 2^16 / 2^11 + 1 =
    16321, so that sums of two of them stay inside 16 bits as well.  A block above the limit (white noise at quality 100 is) is not
    refused on the bound: the host runs the two passes on it (block_in_range) and takes it if every pass-1 value is within 16383 and
    every pass-2 result within [-512, 511] -- the exact condition.
Coefficients of 8-bit pixels stay near 1024 and their reconstruction near [-128, 127], so real photographs pass; a stream with a
damaged or crafted quantisation table is where the guards act.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

MAX_DEQUANTISED = 1096
MAX_QUANTISED_DC = 32767
IDCT_WEIGHTS = (8192, 11363, 10703, 11362, 8192, 11362, 10704, 11363)     # largest |weight| of input k over the pass's 8 outputs, x 2^13
RANGE_SUM_LIMIT = 510 << 29
MAX_PASS1 = 16383

# natural-order index of zigzag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63], dtype=np.int32)

# why a header is not supported (locov_jpeg_header.reason; include/locov_jpeg.h lists the same codes)
(REASON_OK, REASON_NOT_JPEG, REASON_TRUNCATED_HEADER, REASON_SOF, REASON_ARITHMETIC, REASON_PRECISION, REASON_COMPONENTS, REASON_RGB,
 REASON_SAMPLING, REASON_SCANS, REASON_DNL, REASON_QT16, REASON_MISSING_TABLE, REASON_BAD_TABLE, REASON_SIZE, REASON_SEGMENT) = range(16)
REASONS = {
    REASON_OK: "supported",
    REASON_NOT_JPEG: "not a JPEG stream (no SOI)",
    REASON_TRUNCATED_HEADER: "the header ends before the scan",
    REASON_SOF: "SOF2 or above (progressive, lossless or differential)",
    REASON_ARITHMETIC: "arithmetic coding",
    REASON_PRECISION: "sample precision is not 8 bits",
    REASON_COMPONENTS: "neither 1 nor 3 components",
    REASON_RGB: "RGB-coded components (Adobe transform 0)",
    REASON_SAMPLING: "sampling layout outside 4:4:4, 4:2:2, 4:2:0 and grey",
    REASON_SCANS: "not one interleaved scan over the whole spectrum",
    REASON_DNL: "the height comes from a DNL segment",
    REASON_QT16: "16-bit quantisation table",
    REASON_MISSING_TABLE: "a table the scan names is missing",
    REASON_BAD_TABLE: "malformed Huffman or quantisation table",
    REASON_SIZE: "empty image",
    REASON_SEGMENT: "malformed segment",
}

# what the entropy stage answers (locov_jpeg_entropy_decode's per-image status)
(STATUS_OK, STATUS_BAD_CODE, STATUS_MARKER, STATUS_DATA_END, STATUS_NO_EOI, STATUS_MAGNITUDE, STATUS_SPACE, STATUS_INDEX,
 STATUS_UNSUPPORTED) = 0, -1, -2, -3, -4, -5, -6, -7, -8
STATUSES = {
    STATUS_OK: "decoded",
    STATUS_BAD_CODE: "a bit pattern that is no Huffman code",
    STATUS_MARKER: "a marker inside the scan that is not the expected RSTn",
    STATUS_DATA_END: "the data runs out inside the scan",
    STATUS_NO_EOI: "no EOI behind the scan",
    STATUS_MAGNITUDE: f"a dequantised coefficient above {MAX_DEQUANTISED}, or a block that leaves the range where libjpeg's table and its SIMD clamp agree",
    STATUS_SPACE: "the record does not fit its buffer",
    STATUS_INDEX: "a run past coefficient 63",
    STATUS_UNSUPPORTED: "the header is not supported",
}


@dataclass
class JpegHeader:
    """locov_jpeg_header of include/locov_jpeg.h, field by field.  Tables a stream does not define stay zero with present = 0."""
    supported: bool = False
    reason: int = REASON_NOT_JPEG
    width: int = 0
    height: int = 0
    ncomp: int = 0
    comp_id: List[int] = field(default_factory=lambda: [0, 0, 0])
    comp_h: List[int] = field(default_factory=lambda: [0, 0, 0])
    comp_v: List[int] = field(default_factory=lambda: [0, 0, 0])
    comp_tq: List[int] = field(default_factory=lambda: [0, 0, 0])
    comp_td: List[int] = field(default_factory=lambda: [0, 0, 0])
    comp_ta: List[int] = field(default_factory=lambda: [0, 0, 0])
    restart_interval: int = 0
    scan_start: int = 0
    qt_present: np.ndarray = field(default_factory=lambda: np.zeros(4, np.uint8))
    qt: np.ndarray = field(default_factory=lambda: np.zeros((4, 64), np.uint16))           # natural order
    dc_present: np.ndarray = field(default_factory=lambda: np.zeros(4, np.uint8))
    ac_present: np.ndarray = field(default_factory=lambda: np.zeros(4, np.uint8))
    dc_counts: np.ndarray = field(default_factory=lambda: np.zeros((4, 16), np.uint8))
    ac_counts: np.ndarray = field(default_factory=lambda: np.zeros((4, 16), np.uint8))
    dc_symbols: np.ndarray = field(default_factory=lambda: np.zeros((4, 256), np.uint8))
    ac_symbols: np.ndarray = field(default_factory=lambda: np.zeros((4, 256), np.uint8))

    @property
    def why(self) -> str:
        return REASONS[self.reason]

    @property
    def components(self) -> List[Tuple[int, int, int, int]]:
        """(id, h, v, quantisation table) per component"""
        return [(self.comp_id[c], self.comp_h[c], self.comp_v[c], self.comp_tq[c]) for c in range(self.ncomp)]

    # the geometry every stage shares
    @property
    def mcus(self) -> Tuple[int, int]:                               # (across, down)
        return -(-self.width // (8 * self.comp_h[0])), -(-self.height // (8 * self.comp_v[0]))

    def plane_blocks(self, c: int) -> Tuple[int, int]:               # (blocks across, blocks down) of component c's padded plane
        mx, my = self.mcus
        return mx * self.comp_h[c], my * self.comp_v[c]

    @property
    def nblocks(self) -> int:
        return sum(bw * bh for bw, bh in (self.plane_blocks(c) for c in range(self.ncomp)))

    def real_size(self, c: int) -> Tuple[int, int]:                  # (width, height) of component c in samples, unpadded
        return -(-self.width * self.comp_h[c] // self.comp_h[0]), -(-self.height * self.comp_v[c] // self.comp_v[0])


def _fail(h: JpegHeader, reason: int) -> JpegHeader:
    h.supported, h.reason = False, reason
    return h


def parse_jpeg(data) -> JpegHeader:
    """The header of a JPEG stream up to its first scan, and whether this decoder takes the stream (module docstring).  Never
    raises on malformed input: `supported` is False and `reason` says why."""
    d = bytes(data)
    n = len(d)
    h = JpegHeader()
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        return _fail(h, REASON_NOT_JPEG)
    pos, seen_sof, adobe_transform, jfif = 2, False, -1, False
    while True:
        # a marker: 0xFF, any number of fill 0xFF, the code
        if pos >= n or d[pos] != 0xFF:
            return _fail(h, REASON_TRUNCATED_HEADER if pos >= n else REASON_SEGMENT)
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return _fail(h, REASON_TRUNCATED_HEADER)
        m = d[pos]
        pos += 1
        if m == 0xD8 or m == 0xD9 or m == 0x00 or m == 0x01 or 0xD0 <= m <= 0xD7:      # SOI again, EOI before a scan, stray codes
            return _fail(h, REASON_SEGMENT)
        if pos + 2 > n:
            return _fail(h, REASON_TRUNCATED_HEADER)
        seg = (d[pos] << 8) | d[pos + 1]
        if seg < 2:
            return _fail(h, REASON_SEGMENT)
        if pos + seg > n:
            return _fail(h, REASON_TRUNCATED_HEADER)
        p, end = pos + 2, pos + seg
        pos = end
        if m == 0xC0 or m == 0xC1:
            if seen_sof:
                return _fail(h, REASON_SEGMENT)
            seen_sof = True
            if end - p < 6:
                return _fail(h, REASON_SEGMENT)
            precision, h.height, h.width, nc = d[p], (d[p + 1] << 8) | d[p + 2], (d[p + 3] << 8) | d[p + 4], d[p + 5]
            if precision != 8:
                return _fail(h, REASON_PRECISION)
            if nc != 1 and nc != 3:
                return _fail(h, REASON_COMPONENTS)
            if end - p != 6 + 3 * nc:
                return _fail(h, REASON_SEGMENT)
            h.ncomp = nc
            for c in range(nc):
                h.comp_id[c], hv, h.comp_tq[c] = d[p + 6 + 3 * c], d[p + 7 + 3 * c], d[p + 8 + 3 * c]
                h.comp_h[c], h.comp_v[c] = hv >> 4, hv & 15
                if h.comp_tq[c] > 3:
                    return _fail(h, REASON_SEGMENT)
            if h.height == 0:
                return _fail(h, REASON_DNL)
            if h.width == 0:
                return _fail(h, REASON_SIZE)
        elif 0xC2 <= m <= 0xCF and m != 0xC4 and m != 0xC8 and m != 0xCC:
            return _fail(h, REASON_ARITHMETIC if m >= 0xC9 else REASON_SOF)
        elif m == 0xCC:
            return _fail(h, REASON_ARITHMETIC)
        elif m == 0xC8:
            return _fail(h, REASON_SOF)
        elif m == 0xDC:
            return _fail(h, REASON_DNL)
        elif m == 0xC4:
            while p < end:
                if end - p < 17:
                    return _fail(h, REASON_BAD_TABLE)
                tc, th = d[p] >> 4, d[p] & 15
                if tc > 1 or th > 3:
                    return _fail(h, REASON_BAD_TABLE)
                counts = d[p + 1:p + 17]
                total = sum(counts)
                if total > 256 or end - p < 17 + total:
                    return _fail(h, REASON_BAD_TABLE)
                code = 0                                             # the canonical codes must fit their lengths
                for length in range(16):
                    code = (code + counts[length]) << 1
                    if code > (2 << (length + 1)):                    # (code / 2 > 2^(length + 1): more codes than the length holds)
                        return _fail(h, REASON_BAD_TABLE)
                present, cnt, sym = (h.dc_present, h.dc_counts, h.dc_symbols) if tc == 0 else (h.ac_present, h.ac_counts, h.ac_symbols)
                present[th] = 1
                cnt[th] = np.frombuffer(counts, np.uint8)
                sym[th] = 0
                sym[th, :total] = np.frombuffer(d[p + 17:p + 17 + total], np.uint8)
                if tc == 0 and any(s > 15 for s in d[p + 17:p + 17 + total]):
                    return _fail(h, REASON_BAD_TABLE)
                p += 17 + total
        elif m == 0xDB:
            while p < end:
                pq, tq = d[p] >> 4, d[p] & 15
                if tq > 3 or pq > 1:
                    return _fail(h, REASON_BAD_TABLE)
                if pq == 1:
                    return _fail(h, REASON_QT16)
                if end - p < 65:
                    return _fail(h, REASON_BAD_TABLE)
                h.qt_present[tq] = 1
                h.qt[tq, ZIGZAG] = np.frombuffer(d[p + 1:p + 65], np.uint8)
                p += 65
        elif m == 0xDD:
            if seg != 4:
                return _fail(h, REASON_SEGMENT)
            h.restart_interval = (d[p] << 8) | d[p + 1]
        elif m == 0xE0:
            if end - p >= 5 and d[p:p + 5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if end - p >= 12 and d[p:p + 5] == b"Adobe":
                adobe_transform = d[p + 11]
        elif m == 0xDA:
            if not seen_sof:
                return _fail(h, REASON_SEGMENT)
            if end - p < 1:
                return _fail(h, REASON_SEGMENT)
            ns = d[p]
            if end - p != 4 + 2 * ns:
                return _fail(h, REASON_SEGMENT)
            if ns != h.ncomp:
                return _fail(h, REASON_SCANS)
            for c in range(ns):
                if d[p + 1 + 2 * c] != h.comp_id[c]:
                    return _fail(h, REASON_SCANS)
                h.comp_td[c], h.comp_ta[c] = d[p + 2 + 2 * c] >> 4, d[p + 2 + 2 * c] & 15
                if h.comp_td[c] > 3 or h.comp_ta[c] > 3:
                    return _fail(h, REASON_SEGMENT)
            if d[p + 1 + 2 * ns] != 0 or d[p + 2 + 2 * ns] != 63 or d[p + 3 + 2 * ns] != 0:
                return _fail(h, REASON_SCANS)
            h.scan_start = end
            break
        # every other segment (APPn, COM, ...) is skipped
    # the rules on the finished header
    if h.ncomp == 3:
        if adobe_transform == 0 or (adobe_transform < 0 and not jfif and h.comp_id == [0x52, 0x47, 0x42]):
            return _fail(h, REASON_RGB)
        if (h.comp_h[1], h.comp_v[1], h.comp_h[2], h.comp_v[2]) != (1, 1, 1, 1) or (h.comp_h[0], h.comp_v[0]) not in ((1, 1), (2, 1), (2, 2)):
            return _fail(h, REASON_SAMPLING)
    elif h.comp_h[0] < 1 or h.comp_v[0] < 1 or h.comp_h[0] > 4 or h.comp_v[0] > 4:
        return _fail(h, REASON_SAMPLING)
    else:
        h.comp_h[0] = h.comp_v[0] = 1          # (a single-component scan is not interleaved: its sampling factors mean nothing)
    for c in range(h.ncomp):
        if not (h.qt_present[h.comp_tq[c]] and h.dc_present[h.comp_td[c]] and h.ac_present[h.comp_ta[c]]):
            return _fail(h, REASON_MISSING_TABLE)
    h.supported, h.reason = True, REASON_OK
    return h


# ---- the entropy stage ----------------------------------------------------------------------------------------------------------

class _Stop(Exception):
    def __init__(self, status: int):
        self.status = status


class _Bits:
    """The scan's bits, a byte at a time: 0xFF00 is the byte 0xFF; 0xFF and anything else is a marker, at which the bits end."""

    def __init__(self, d: bytes, pos: int):
        self.d, self.pos, self.acc, self.n = d, pos, 0, 0

    def _byte(self) -> None:
        d, p = self.d, self.pos
        if p >= len(d):
            raise _Stop(STATUS_DATA_END)
        b = d[p]
        if b == 0xFF:
            if p + 1 >= len(d):
                raise _Stop(STATUS_DATA_END)
            if d[p + 1] != 0:
                raise _Stop(STATUS_MARKER)
            p += 1
        self.pos = p + 1
        self.acc = ((self.acc << 8) | b) & 0xFFFFFFFF
        self.n += 8

    def bit(self) -> int:
        if self.n == 0:
            self._byte()
        self.n -= 1
        return (self.acc >> self.n) & 1

    def receive(self, s: int) -> int:
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def marker(self) -> int:
        """Drops the padding bits and reads a marker (fill bytes allowed); -1 at the end of the data, -2 when no marker follows."""
        self.n = 0
        d, p = self.d, self.pos
        if p >= len(d):
            return -1
        if d[p] != 0xFF:
            return -2
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            return -1
        self.pos = p + 1
        return d[p]


def _huffman(counts, symbols):
    """(mincode, maxcode, first symbol index) per length 1..16 of a canonical table"""
    tab, code, k = [], 0, 0
    for length in range(16):
        n = int(counts[length])
        tab.append((code, code + n - 1, k) if n else None)
        code, k = (code + n) << 1, k + n
    return tab, [int(s) for s in symbols]


def _decode(bits: _Bits, table) -> int:
    tab, symbols = table
    code = 0
    for length in range(16):
        code = (code << 1) | bits.bit()
        t = tab[length]
        if t is not None and t[0] <= code <= t[1]:
            return symbols[t[2] + code - t[0]]
    raise _Stop(STATUS_BAD_CODE)


def _extend(v: int, s: int) -> int:
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def block_in_range(coef) -> bool:
    """The exact per-block condition of the module docstring on dequantised coefficients [8, 8]: both passes run, every pass-1
    value within MAX_PASS1 and every descaled pass-2 result within [-512, 511]."""
    x = np.asarray(coef, dtype=np.int64).reshape(1, 8, 8)
    ws = _idct_1d(x.transpose(0, 2, 1), CONST_BITS - PASS1_BITS).transpose(0, 2, 1)
    if int(np.abs(ws).max()) > MAX_PASS1:
        return False
    out = _idct_1d(ws, CONST_BITS + PASS1_BITS + 3)
    return -512 <= int(out.min()) and int(out.max()) <= 511


def _block_ok(words, q) -> bool:
    """A block's entries against the range guard: the weighted sum first, the two passes only above its limit."""
    total, coef = 0, None
    for w in words:
        i, v = (w >> 16) & 63, w & 0xFFFF
        v = v - 65536 if v >= 32768 else v
        total += IDCT_WEIGHTS[i >> 3] * IDCT_WEIGHTS[i & 7] * abs(v * q[i])
    if total <= RANGE_SUM_LIMIT:
        return True
    coef = [0] * 64
    for w in words:
        i, v = (w >> 16) & 63, w & 0xFFFF
        coef[i] = (v - 65536 if v >= 32768 else v) * q[i]
    return block_in_range(coef)


def entropy_decode_host(data, header: Optional[JpegHeader] = None) -> Tuple[int, Optional[np.ndarray]]:
    """(status, record): the scan of a supported stream as the coefficient record of the module docstring, uint32 words.  A
    negative status (STATUS_*) comes with no record."""
    d = bytes(data)
    h = parse_jpeg(d) if header is None else header
    if not h.supported:
        return STATUS_UNSUPPORTED, None
    mx, my = h.mcus
    dc = [_huffman(h.dc_counts[h.comp_td[c]], h.dc_symbols[h.comp_td[c]]) for c in range(h.ncomp)]
    ac = [_huffman(h.ac_counts[h.comp_ta[c]], h.ac_symbols[h.comp_ta[c]]) for c in range(h.ncomp)]
    qt = [[int(q) for q in h.qt[h.comp_tq[c]]] for c in range(h.ncomp)]
    base, planes = [], []
    for c in range(h.ncomp):
        base.append(sum(bw * bh for bw, bh in planes))
        planes.append(h.plane_blocks(c))
    blocks: List[List[int]] = [[] for _ in range(h.nblocks)]
    bits = _Bits(d, h.scan_start)
    pred = [0] * h.ncomp
    zz = [int(z) for z in ZIGZAG]
    try:
        for mcu in range(mx * my):
            if h.restart_interval and mcu and mcu % h.restart_interval == 0:
                m = bits.marker()
                if m == -1:
                    raise _Stop(STATUS_DATA_END)
                if m != 0xD0 + ((mcu // h.restart_interval - 1) & 7):
                    raise _Stop(STATUS_MARKER)
                pred = [0] * h.ncomp
            my_, mx_ = divmod(mcu, mx)
            for c in range(h.ncomp):
                hs, vs = h.comp_h[c], h.comp_v[c]
                for k in range(hs * vs):
                    bx, by = mx_ * hs + k % hs, my_ * vs + k // hs
                    out = blocks[base[c] + by * planes[c][0] + bx]
                    s = _decode(bits, dc[c])
                    if s > 15:
                        raise _Stop(STATUS_BAD_CODE)
                    pred[c] += _extend(bits.receive(s), s)
                    if abs(pred[c]) > MAX_QUANTISED_DC or abs(pred[c] * qt[c][0]) > MAX_DEQUANTISED:
                        raise _Stop(STATUS_MAGNITUDE)
                    if pred[c]:
                        out.append(pred[c] & 0xFFFF)
                    i = 1
                    while i < 64:
                        rs = _decode(bits, ac[c])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            i += 16
                            continue
                        i += r
                        if i > 63:
                            raise _Stop(STATUS_INDEX)
                        v = _extend(bits.receive(s), s)
                        if abs(v * qt[c][zz[i]]) > MAX_DEQUANTISED:
                            raise _Stop(STATUS_MAGNITUDE)
                        out.append((zz[i] << 16) | (v & 0xFFFF))
                        i += 1
                    if not _block_ok(out, qt[c]):
                        raise _Stop(STATUS_MAGNITUDE)
        if bits.marker() != 0xD9:
            raise _Stop(STATUS_NO_EOI)
    except _Stop as stop:
        return stop.status, None
    counts = np.array([len(b) for b in blocks], dtype=np.int64)
    record = np.empty(h.nblocks + 1 + int(counts.sum()), dtype=np.uint32)
    record[0] = 0
    record[1:h.nblocks + 1] = np.cumsum(counts)
    record[h.nblocks + 1:] = [w for b in blocks for w in b]
    return STATUS_OK, record


def stream_supported(data) -> Tuple[bool, str]:
    """(supported, why): the whole verdict on a stream -- its header's, and for a header the decoder takes the entropy stage's,
    which alone knows of a truncated scan, a missing EOI or a coefficient past the magnitude guard."""
    h = parse_jpeg(data)
    if not h.supported:
        return False, h.why
    status = entropy_decode_host(data, h)[0]
    return status == STATUS_OK, STATUSES[status]


# ---- the pixel pipeline ---------------------------------------------------------------------------------------------------------

CONST_BITS, PASS1_BITS = 13, 2
FIX_0_298631336, FIX_0_390180644, FIX_0_541196100, FIX_0_765366865, FIX_0_899976223, FIX_1_175875602 = 2446, 3196, 4433, 6270, 7373, 9633
FIX_1_501321110, FIX_1_847759065, FIX_1_961570560, FIX_2_053119869, FIX_2_562915447, FIX_3_072711026 = 12299, 15137, 16069, 16819, 20995, 25172


def _idct_1d(x, shift: int):
    """jidctint's one-dimensional pass over x[..., 8] (int64 here; inside the guard every value fits 32 bits), descaled by `shift`."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (x[..., i] for i in range(8))
    z1 = (d2 + d6) * FIX_0_541196100
    tmp2 = z1 + d6 * -FIX_1_847759065
    tmp3 = z1 + d2 * FIX_0_765366865
    tmp0 = (d0 + d4) << CONST_BITS
    tmp1 = (d0 - d4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d7, d5, d3, d1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * FIX_1_175875602
    tmp0, tmp1, tmp2, tmp3 = tmp0 * FIX_0_298631336, tmp1 * FIX_2_053119869, tmp2 * FIX_3_072711026, tmp3 * FIX_1_501321110
    z1, z2, z3, z4 = z1 * -FIX_0_899976223, z2 * -FIX_2_562915447, z3 * -FIX_1_961570560 + z5, z4 * -FIX_0_390180644 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = 1 << (shift - 1)
    outs = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + half) >> shift for o in outs], axis=-1)


_RANGE_LIMIT = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, np.int64), np.arange(0, 128)]).astype(np.uint8)


def idct_blocks(coef: np.ndarray) -> np.ndarray:
    """Dequantised coefficients [n, 8, 8] (row, column) -> samples uint8 [n, 8, 8]: columns first, then rows, then the range limit."""
    x = coef.astype(np.int64)
    ws = _idct_1d(x.transpose(0, 2, 1), CONST_BITS - PASS1_BITS).transpose(0, 2, 1)          # along each column
    out = _idct_1d(ws, CONST_BITS + PASS1_BITS + 3)                                          # along each row
    return _RANGE_LIMIT[out & 1023]


def record_planes(h: JpegHeader, record: np.ndarray) -> List[np.ndarray]:
    """The MCU-padded sample plane of every component from a record."""
    nb = h.nblocks
    start, entries = record[:nb + 1].astype(np.int64), record[nb + 1:]
    coef = np.zeros((nb, 64), dtype=np.int64)
    owner = np.repeat(np.arange(nb), np.diff(start))
    coef[owner, (entries >> 16) & 63] = (entries & 0xFFFF).astype(np.uint16).view(np.int16)
    planes, at = [], 0
    for c in range(h.ncomp):
        bw, bh = h.plane_blocks(c)
        q = h.qt[h.comp_tq[c]].astype(np.int64)
        px = idct_blocks((coef[at:at + bw * bh] * q).reshape(-1, 8, 8))
        planes.append(px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
        at += bw * bh
    return planes


def _upsample_h2v1(s: np.ndarray) -> np.ndarray:
    """[h, w] -> [h, 2 w]: jdsample.c's h2v1_fancy_upsample, or replication up to 2 samples of width."""
    s = s.astype(np.int64)
    if s.shape[1] <= 2:
        return np.repeat(s, 2, axis=1)
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 1) >> 2, (3 * s + right + 2) >> 2
    return out


def _upsample_h2v2(s: np.ndarray) -> np.ndarray:
    """[h, w] -> [2 h, 2 w]: h2v2_fancy_upsample, or replication up to 2 samples of width."""
    s = s.astype(np.int64)
    if s.shape[1] <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    up, down = np.concatenate([s[:1], s[:-1]], axis=0), np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), dtype=np.int64)
    for v, far in ((0, up), (1, down)):
        c = 3 * s + far
        left, right = np.concatenate([c[:, :1], c[:, :-1]], axis=1), np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        out[v::2, 0::2], out[v::2, 1::2] = (3 * c + left + 8) >> 4, (3 * c + right + 7) >> 4
    return out


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    """jdcolor.c's build_ycc_rgb_table and ycc_rgb_convert: [h, w] x 3 -> uint8 [h, w, 3] (RGB)."""
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((_fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def planes_to_image(h: JpegHeader, planes: List[np.ndarray], fmt: str) -> np.ndarray:
    H, W = h.height, h.width
    if h.ncomp == 1:
        y = planes[0][:H, :W]
        return np.ascontiguousarray(y[:, :, None] if fmt == "L" else np.repeat(y[:, :, None], 3, axis=2))
    if fmt == "L":
        raise ValueError("a colour stream as 'L' is Pillow's conversion: the host path")
    hs, vs = h.comp_h[0], h.comp_v[0]
    chroma = []
    for c in (1, 2):
        cw, ch = h.real_size(c)
        s = planes[c][:ch, :cw]
        s = _upsample_h2v2(s) if (hs, vs) == (2, 2) else _upsample_h2v1(s) if (hs, vs) == (2, 1) else s
        chroma.append(s[:H, :W])
    rgb = ycc_to_rgb(planes[0][:H, :W], chroma[0], chroma[1])
    return np.ascontiguousarray(rgb[:, :, ::-1]) if fmt == "BGR" else rgb


def decode_jpeg_host(data, fmt: str = "RGB") -> np.ndarray:
    """HWC uint8 of a supported stream in `fmt` order: Pillow's bytes (np.asarray(Image.open(...).convert("RGB")), reversed for
    "BGR"; "L" for a grey stream).  ValueError with the reason for anything else -- the caller takes Pillow."""
    if fmt not in ("RGB", "BGR", "L"):
        raise ValueError(f"decode_jpeg_host: format {fmt!r} is none of 'RGB', 'BGR', 'L'")
    h = parse_jpeg(data)
    if not h.supported:
        raise ValueError(f"decode_jpeg_host: {h.why}")
    status, record = entropy_decode_host(data, h)
    if status != STATUS_OK:
        raise ValueError(f"decode_jpeg_host: {STATUSES[status]}")
    return planes_to_image(h, record_planes(h, record), fmt)
