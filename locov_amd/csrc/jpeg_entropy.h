// The host stage of the JPEG decoder (include/locov_jpeg.h): header parsing and Huffman decoding of baseline scans into sparse
// coefficient records.  Plain C++17, no HIP header: jpeg.hip includes it for the library, tools/jpeg_entropy_check.cpp compiles it
// with g++ under the sanitizers.  locov_amd/jpeg.py (parse_jpeg, entropy_decode_host) is the definition; this file restates it
// statement by statement, with a table-driven Huffman decoder in place of the bit-by-bit one (same symbols, same statuses).
// Every read of the input and every write of the output is bounds-checked, every failure is a status, nothing throws.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>

#include "../../include/locov_jpeg.h"

namespace locov {
namespace jpeg {

constexpr int kMaxThreads = 16;

// natural-order index of zigzag position k
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline void fail(locov_jpeg_header *h, int reason)
{
    h->supported = 0;
    h->reason = reason;
}

// parse_jpeg of jpeg.py
inline void parse(const uint8_t *d, int64_t n, locov_jpeg_header *h)
{
    std::memset(h, 0, sizeof(*h));
    h->reason = LOCOV_JPEG_REASON_NOT_JPEG;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return;
    int64_t pos = 2;
    bool seen_sof = false, jfif = false;
    int adobe_transform = -1;
    for (;;) {
        if (pos >= n) return fail(h, LOCOV_JPEG_REASON_TRUNCATED_HEADER);
        if (d[pos] != 0xFF) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
        while (pos < n && d[pos] == 0xFF) pos++;
        if (pos >= n) return fail(h, LOCOV_JPEG_REASON_TRUNCATED_HEADER);
        const int m = d[pos++];
        if (m == 0xD8 || m == 0xD9 || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
        if (pos + 2 > n) return fail(h, LOCOV_JPEG_REASON_TRUNCATED_HEADER);
        const int64_t seg = (d[pos] << 8) | d[pos + 1];
        if (seg < 2) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
        if (pos + seg > n) return fail(h, LOCOV_JPEG_REASON_TRUNCATED_HEADER);
        int64_t p = pos + 2;
        const int64_t end = pos + seg;
        pos = end;
        if (m == 0xC0 || m == 0xC1) {
            if (seen_sof) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            seen_sof = true;
            if (end - p < 6) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            const int precision = d[p], nc = d[p + 5];
            h->height = (d[p + 1] << 8) | d[p + 2];
            h->width = (d[p + 3] << 8) | d[p + 4];
            if (precision != 8) return fail(h, LOCOV_JPEG_REASON_PRECISION);
            if (nc != 1 && nc != 3) return fail(h, LOCOV_JPEG_REASON_COMPONENTS);
            if (end - p != 6 + 3 * nc) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            h->ncomp = nc;
            for (int c = 0; c < nc; c++) {
                h->comp_id[c] = d[p + 6 + 3 * c];
                h->comp_h[c] = d[p + 7 + 3 * c] >> 4;
                h->comp_v[c] = d[p + 7 + 3 * c] & 15;
                h->comp_tq[c] = d[p + 8 + 3 * c];
                if (h->comp_tq[c] > 3) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            }
            if (h->height == 0) return fail(h, LOCOV_JPEG_REASON_DNL);
            if (h->width == 0) return fail(h, LOCOV_JPEG_REASON_SIZE);
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return fail(h, m >= 0xC9 ? LOCOV_JPEG_REASON_ARITHMETIC : LOCOV_JPEG_REASON_SOF);
        } else if (m == 0xCC) {
            return fail(h, LOCOV_JPEG_REASON_ARITHMETIC);
        } else if (m == 0xC8) {
            return fail(h, LOCOV_JPEG_REASON_SOF);
        } else if (m == 0xDC) {
            return fail(h, LOCOV_JPEG_REASON_DNL);
        } else if (m == 0xC4) {
            while (p < end) {
                if (end - p < 17) return fail(h, LOCOV_JPEG_REASON_BAD_TABLE);
                const int tc = d[p] >> 4, th = d[p] & 15;
                if (tc > 1 || th > 3) return fail(h, LOCOV_JPEG_REASON_BAD_TABLE);
                int total = 0;
                for (int l = 0; l < 16; l++) total += d[p + 1 + l];
                if (total > 256 || end - p < 17 + total) return fail(h, LOCOV_JPEG_REASON_BAD_TABLE);
                int64_t code = 0;                                 // the canonical codes must fit their lengths
                for (int l = 0; l < 16; l++) {
                    code = (code + d[p + 1 + l]) << 1;
                    if (code > ((int64_t)2 << (l + 1))) return fail(h, LOCOV_JPEG_REASON_BAD_TABLE);
                }
                uint8_t *present = tc == 0 ? h->dc_present : h->ac_present;
                uint8_t *cnt = tc == 0 ? h->dc_counts[th] : h->ac_counts[th];
                uint8_t *sym = tc == 0 ? h->dc_symbols[th] : h->ac_symbols[th];
                present[th] = 1;
                std::memcpy(cnt, d + p + 1, 16);
                std::memset(sym, 0, 256);
                std::memcpy(sym, d + p + 17, (size_t)total);
                if (tc == 0)
                    for (int k = 0; k < total; k++)
                        if (sym[k] > 15) return fail(h, LOCOV_JPEG_REASON_BAD_TABLE);
                p += 17 + total;
            }
        } else if (m == 0xDB) {
            while (p < end) {
                const int pq = d[p] >> 4, tq = d[p] & 15;
                if (tq > 3 || pq > 1) return fail(h, LOCOV_JPEG_REASON_BAD_TABLE);
                if (pq == 1) return fail(h, LOCOV_JPEG_REASON_QT16);
                if (end - p < 65) return fail(h, LOCOV_JPEG_REASON_BAD_TABLE);
                h->qt_present[tq] = 1;
                for (int k = 0; k < 64; k++) h->qt[tq][kZigzag[k]] = d[p + 1 + k];
                p += 65;
            }
        } else if (m == 0xDD) {
            if (seg != 4) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            h->restart_interval = (d[p] << 8) | d[p + 1];
        } else if (m == 0xE0) {
            if (end - p >= 5 && std::memcmp(d + p, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (end - p >= 12 && std::memcmp(d + p, "Adobe", 5) == 0) adobe_transform = d[p + 11];
        } else if (m == 0xDA) {
            if (!seen_sof) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            if (end - p < 1) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            const int ns = d[p];
            if (end - p != 4 + 2 * ns) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            if (ns != h->ncomp) return fail(h, LOCOV_JPEG_REASON_SCANS);
            for (int c = 0; c < ns; c++) {
                if (d[p + 1 + 2 * c] != h->comp_id[c]) return fail(h, LOCOV_JPEG_REASON_SCANS);
                h->comp_td[c] = d[p + 2 + 2 * c] >> 4;
                h->comp_ta[c] = d[p + 2 + 2 * c] & 15;
                if (h->comp_td[c] > 3 || h->comp_ta[c] > 3) return fail(h, LOCOV_JPEG_REASON_SEGMENT);
            }
            if (d[p + 1 + 2 * ns] != 0 || d[p + 2 + 2 * ns] != 63 || d[p + 3 + 2 * ns] != 0) return fail(h, LOCOV_JPEG_REASON_SCANS);
            h->scan_start = end;
            break;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
    // the rules on the finished header
    if (h->ncomp == 3) {
        const bool rgb_ids = h->comp_id[0] == 0x52 && h->comp_id[1] == 0x47 && h->comp_id[2] == 0x42;
        if (adobe_transform == 0 || (adobe_transform < 0 && !jfif && rgb_ids)) return fail(h, LOCOV_JPEG_REASON_RGB);
        const int hs = h->comp_h[0], vs = h->comp_v[0];
        if (h->comp_h[1] != 1 || h->comp_v[1] != 1 || h->comp_h[2] != 1 || h->comp_v[2] != 1 ||
            !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)))
            return fail(h, LOCOV_JPEG_REASON_SAMPLING);
    } else if (h->comp_h[0] < 1 || h->comp_v[0] < 1 || h->comp_h[0] > 4 || h->comp_v[0] > 4) {
        return fail(h, LOCOV_JPEG_REASON_SAMPLING);
    } else {
        h->comp_h[0] = h->comp_v[0] = 1;                          // (a single-component scan is not interleaved)
    }
    for (int c = 0; c < h->ncomp; c++)
        if (!(h->qt_present[h->comp_tq[c]] && h->dc_present[h->comp_td[c]] && h->ac_present[h->comp_ta[c]]))
            return fail(h, LOCOV_JPEG_REASON_MISSING_TABLE);
    h->supported = 1;
    h->reason = LOCOV_JPEG_REASON_OK;
}

// ---- the geometry every stage shares --------------------------------------------------------------------------------------------
struct Geometry {
    int ncomp, hs[3], vs[3];
    int64_t mcux, mcuy, bw[3], bh[3], base[3], nblocks;           // plane c: bw x bh blocks, the first is block base[c]
    int per_mcu, mcu_base[3];                                     // blocks of one MCU, and where component c's begin in it
};

// Whether a header can be decoded at all: the ranges everything below indexes with.  (A header from parse() with supported = 1
// passes; one filled in by hand is checked like any other input.)
inline bool geometry(const locov_jpeg_header &h, Geometry &g)
{
    if (h.supported != 1 || (h.ncomp != 1 && h.ncomp != 3)) return false;
    if (h.width < 1 || h.width > 65535 || h.height < 1 || h.height > 65535 || h.restart_interval < 0 || h.scan_start < 0) return false;
    for (int c = 0; c < h.ncomp; c++) {
        if (h.comp_h[c] < 1 || h.comp_h[c] > 2 || h.comp_v[c] < 1 || h.comp_v[c] > 2) return false;
        if (c > 0 && (h.comp_h[c] != 1 || h.comp_v[c] != 1)) return false;
        if (h.comp_tq[c] < 0 || h.comp_tq[c] > 3 || h.comp_td[c] < 0 || h.comp_td[c] > 3 || h.comp_ta[c] < 0 || h.comp_ta[c] > 3) return false;
    }
    if (h.ncomp == 1 && (h.comp_h[0] != 1 || h.comp_v[0] != 1)) return false;
    g.ncomp = h.ncomp;
    g.mcux = (h.width + 8 * h.comp_h[0] - 1) / (8 * h.comp_h[0]);
    g.mcuy = (h.height + 8 * h.comp_v[0] - 1) / (8 * h.comp_v[0]);
    g.nblocks = 0;
    g.per_mcu = 0;
    for (int c = 0; c < h.ncomp; c++) {
        g.hs[c] = h.comp_h[c];
        g.vs[c] = h.comp_v[c];
        g.bw[c] = g.mcux * g.hs[c];
        g.bh[c] = g.mcuy * g.vs[c];
        g.base[c] = g.nblocks;
        g.nblocks += g.bw[c] * g.bh[c];
        g.mcu_base[c] = g.per_mcu;
        g.per_mcu += g.hs[c] * g.vs[c];
    }
    return true;
}

inline int64_t entropy_bytes(const locov_jpeg_header &h, int64_t len)
{
    Geometry g;
    if (!geometry(h, g) || len < h.scan_start) return 0;
    const int64_t by_blocks = 64 * g.nblocks, by_bytes = 4 * (len - h.scan_start);
    return 4 * (g.nblocks + 1) + 4 * (by_blocks < by_bytes ? by_blocks : by_bytes);
}

inline int64_t record_bytes_for(int64_t nblocks, int64_t entries) { return (4 * (nblocks + 1 + entries) + 15) / 16 * 16; }

// ---- Huffman ----------------------------------------------------------------------------------------------------------------------
constexpr int kLookBits = 9;

struct HuffTable {
    uint16_t look[1 << kLookBits];                                // (length << 8) | symbol for a code of <= kLookBits bits, else 0
    int32_t mincode[17], maxcode[17], first[17];                  // per length 1 .. 16; maxcode = -1: no code of that length
    uint8_t symbols[256];
};

inline void build_table(const uint8_t counts[16], const uint8_t symbols[256], HuffTable &t)
{
    std::memset(t.look, 0, sizeof(t.look));
    std::memcpy(t.symbols, symbols, 256);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        const int n = counts[l - 1];
        t.mincode[l] = code;
        t.maxcode[l] = n ? code + n - 1 : -1;
        t.first[l] = k;
        if (l <= kLookBits)
            for (int i = 0; i < n && k + i < 256; i++) {
                const int32_t c = code + i;
                if (c >= (1 << l)) break;                         // (never for a table parse() accepted)
                const int lo = c << (kLookBits - l), span = 1 << (kLookBits - l);
                for (int j = 0; j < span; j++) t.look[lo + j] = (uint16_t)((l << 8) | symbols[k + i]);
            }
        code = (code + n) << 1;
        k += n;
    }
}

// The scan's bits.  0xFF00 is the byte 0xFF; 0xFF and anything else is a marker, at which the bits end (stop = STATUS_MARKER), as
// they do at the end of the data (STATUS_DATA_END).  Bytes are buffered ahead; a status is only raised when more bits are needed
// than the stream holds in front of that point, which is when the bit-by-bit definition raises it.
struct BitReader {
    const uint8_t *d;
    int64_t pos, end;
    uint64_t acc;
    int n, stop;

    void fill()
    {
        while (n <= 56 && !stop) {
            if (pos >= end) {
                stop = LOCOV_JPEG_STATUS_DATA_END;
                break;
            }
            const uint8_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= end) {
                    stop = LOCOV_JPEG_STATUS_DATA_END;
                    break;
                }
                if (d[pos + 1] != 0) {
                    stop = LOCOV_JPEG_STATUS_MARKER;
                    break;
                }
                pos += 2;
            } else {
                pos += 1;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }

    uint32_t peek(int k) const                                    // the next k <= 16 bits, zero-padded past the last one
    {
        if (n >= k) return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1);
        const uint64_t have = n ? acc & (~(uint64_t)0 >> (64 - n)) : 0;
        return (uint32_t)(have << (k - n)) & ((1u << k) - 1);
    }

    // a symbol, or a negative status
    int decode(const HuffTable &t)
    {
        fill();
        const uint16_t e = t.look[peek(kLookBits)];
        int len = 0, sym = 0;
        if (e) {
            len = e >> 8;
            sym = e & 255;
        } else {
            const uint32_t bits = peek(16);
            for (int l = kLookBits + 1; l <= 16; l++) {
                const int32_t c = (int32_t)(bits >> (16 - l));
                if (t.maxcode[l] >= 0 && c >= t.mincode[l] && c <= t.maxcode[l]) {
                    const int at = t.first[l] + c - t.mincode[l];
                    if (at > 255) return LOCOV_JPEG_STATUS_BAD_CODE;
                    len = l;
                    sym = t.symbols[at];
                    break;
                }
            }
        }
        if (len == 0 || len > n) return n >= 16 ? LOCOV_JPEG_STATUS_BAD_CODE : (stop ? stop : LOCOV_JPEG_STATUS_DATA_END);
        n -= len;
        return sym;
    }

    // s <= 15 bits into v; 0 or a negative status
    int receive(int s, int32_t &v)
    {
        if (n < s) {
            fill();
            if (n < s) return stop ? stop : LOCOV_JPEG_STATUS_DATA_END;
        }
        v = s ? (int32_t)((acc >> (n - s)) & ((1u << s) - 1)) : 0;
        n -= s;
        return 0;
    }

    // Drops the padding bits and reads a marker (fill bytes allowed): its code, -1 at the end of the data, -2 when no marker follows.
    int marker()
    {
        for (int whole = n / 8; whole > 0; whole--)               // un-read the bytes that were buffered ahead
            pos -= (pos >= 2 && d[pos - 1] == 0x00 && d[pos - 2] == 0xFF) ? 2 : 1;
        n = 0;
        stop = 0;
        if (pos >= end) return -1;
        if (d[pos] != 0xFF) return -2;
        int64_t p = pos;
        while (p < end && d[p] == 0xFF) p++;
        if (p >= end) return -1;
        pos = p + 1;
        return d[p];
    }
};

inline int32_t extend(int32_t v, int s) { return (s == 0 || v >= (1 << (s - 1))) ? v : v - (1 << s) + 1; }

// ---- the range guard (include/locov_jpeg.h: LOCOV_JPEG_RANGE_SUM_LIMIT) ---------------------------------------------------------------
// largest |weight| of input k over the eight outputs of jidctint's one-dimensional pass, scaled by 2^13
constexpr int64_t kIdctWeight[8] = {8192, 11363, 10703, 11362, 8192, 11362, 10704, 11363};
constexpr int64_t kRangeSumLimit = (int64_t)510 << 29;
constexpr int32_t kMaxPass1 = 16383;

// jidctint.c's one-dimensional pass over d[0], d[stride], ..., in place, descaled by SHIFT (the kernel's idct8, on the host).  Inside
// the per-coefficient guard no value leaves 32 bits.
template <int SHIFT>
inline void idct8_host(int32_t *d, int stride)
{
    const int32_t d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride],
                  d6 = d[6 * stride], d7 = d[7 * stride];
    int32_t z1 = (d2 + d6) * 4433;
    int32_t tmp2 = z1 + d6 * -15137, tmp3 = z1 + d2 * 6270;
    int32_t tmp0 = (d0 + d4) * 8192, tmp1 = (d0 - d4) * 8192;
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d7;
    tmp1 = d5;
    tmp2 = d3;
    tmp3 = d1;
    z1 = tmp0 + tmp3;
    int32_t z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const int32_t z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr int32_t half = 1 << (SHIFT - 1);
    d[0] = (tmp10 + tmp3 + half) >> SHIFT;
    d[7 * stride] = (tmp10 - tmp3 + half) >> SHIFT;
    d[stride] = (tmp11 + tmp2 + half) >> SHIFT;
    d[6 * stride] = (tmp11 - tmp2 + half) >> SHIFT;
    d[2 * stride] = (tmp12 + tmp1 + half) >> SHIFT;
    d[5 * stride] = (tmp12 - tmp1 + half) >> SHIFT;
    d[3 * stride] = (tmp13 + tmp0 + half) >> SHIFT;
    d[4 * stride] = (tmp13 - tmp0 + half) >> SHIFT;
}

// block_in_range of jpeg.py: dequantised coefficients [8][8] (overwritten) -> whether every pass-1 value is within kMaxPass1 and every
// descaled pass-2 result within [-512, 511], where libjpeg's wrapping table and libjpeg-turbo's saturating SIMD code agree
inline bool block_in_range(int32_t *coef)
{
    for (int c = 0; c < 8; c++) idct8_host<11>(coef + c, 8);
    for (int i = 0; i < 64; i++)
        if (coef[i] > kMaxPass1 || coef[i] < -kMaxPass1) return false;
    for (int r = 0; r < 8; r++) idct8_host<18>(coef + 8 * r, 1);
    for (int i = 0; i < 64; i++)
        if (coef[i] > 511 || coef[i] < -512) return false;
    return true;
}

// _block_ok of jpeg.py: a block's entries against the range guard -- the weighted sum first, the two passes only above its limit
inline bool block_ok(const uint32_t *words, int64_t n, const uint16_t *q)
{
    int64_t total = 0;
    for (int64_t k = 0; k < n; k++) {
        const int i = (words[k] >> 16) & 63;
        const int32_t d = (int32_t)(int16_t)(words[k] & 0xFFFFu) * (int32_t)q[i];
        total += kIdctWeight[i >> 3] * kIdctWeight[i & 7] * (d < 0 ? -d : d);
    }
    if (total <= kRangeSumLimit) return true;
    int32_t coef[64] = {0};
    for (int64_t k = 0; k < n; k++) {
        const int i = (words[k] >> 16) & 63;
        coef[i] = (int32_t)(int16_t)(words[k] & 0xFFFFu) * (int32_t)q[i];
    }
    return block_in_range(coef);
}

// entropy_decode_host of jpeg.py, into the staging layout: uint32 start[nblocks + 1] in SCAN order, then the entries.
// Returns the status; *record_bytes is the size of the packed record.
inline int decode_scan(const uint8_t *d, int64_t len, const locov_jpeg_header &h, void *staging, int64_t staging_bytes, int64_t *record_bytes)
{
    *record_bytes = 0;
    Geometry g;
    if (!geometry(h, g) || h.scan_start > len) return LOCOV_JPEG_STATUS_UNSUPPORTED;
    if (!staging || ((uintptr_t)staging & 3) || staging_bytes < 4 * (g.nblocks + 1)) return LOCOV_JPEG_STATUS_SPACE;
    uint32_t *start = static_cast<uint32_t *>(staging);
    uint32_t *ent = start + g.nblocks + 1;
    const int64_t cap = staging_bytes / 4 - (g.nblocks + 1);
    int64_t count = 0;

    HuffTable dc[3], ac[3];
    const uint16_t *qt[3];
    for (int c = 0; c < g.ncomp; c++) {
        if (!(h.qt_present[h.comp_tq[c]] && h.dc_present[h.comp_td[c]] && h.ac_present[h.comp_ta[c]])) return LOCOV_JPEG_STATUS_UNSUPPORTED;
        build_table(h.dc_counts[h.comp_td[c]], h.dc_symbols[h.comp_td[c]], dc[c]);
        build_table(h.ac_counts[h.comp_ta[c]], h.ac_symbols[h.comp_ta[c]], ac[c]);
        qt[c] = h.qt[h.comp_tq[c]];
    }
    BitReader br{d, h.scan_start, len, 0, 0, 0};
    int32_t pred[3] = {0, 0, 0};
    const int64_t mcus = g.mcux * g.mcuy;
    int64_t blk = 0;
    for (int64_t mcu = 0; mcu < mcus; mcu++) {
        if (h.restart_interval && mcu && mcu % h.restart_interval == 0) {
            const int m = br.marker();
            if (m == -1) return LOCOV_JPEG_STATUS_DATA_END;
            if (m != 0xD0 + (int)((mcu / h.restart_interval - 1) & 7)) return LOCOV_JPEG_STATUS_MARKER;
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < g.ncomp; c++) {
            for (int k = 0; k < g.hs[c] * g.vs[c]; k++, blk++) {
                start[blk] = (uint32_t)count;
                int s = br.decode(dc[c]);
                if (s < 0) return s;
                if (s > 15) return LOCOV_JPEG_STATUS_BAD_CODE;    // (never for a table parse() accepted)
                int32_t v;
                int rc = br.receive(s, v);
                if (rc < 0) return rc;
                pred[c] += extend(v, s);
                if (pred[c] > 32767 || pred[c] < -32767) return LOCOV_JPEG_STATUS_MAGNITUDE;     // (whatever the quantiser, 0 included)
                const int32_t dq = pred[c] * (int32_t)qt[c][0];
                if (dq > LOCOV_JPEG_MAX_DEQUANTISED || dq < -LOCOV_JPEG_MAX_DEQUANTISED) return LOCOV_JPEG_STATUS_MAGNITUDE;
                if (pred[c]) {
                    if (count >= cap) return LOCOV_JPEG_STATUS_SPACE;
                    ent[count++] = (uint32_t)pred[c] & 0xFFFFu;
                }
                int i = 1;
                while (i < 64) {
                    const int rs = br.decode(ac[c]);
                    if (rs < 0) return rs;
                    const int r = rs >> 4;
                    s = rs & 15;
                    if (s == 0) {
                        if (r != 15) break;
                        i += 16;
                        continue;
                    }
                    i += r;
                    if (i > 63) return LOCOV_JPEG_STATUS_INDEX;
                    rc = br.receive(s, v);
                    if (rc < 0) return rc;
                    v = extend(v, s);
                    const int nat = kZigzag[i];
                    const int32_t da = v * (int32_t)qt[c][nat];
                    if (da > LOCOV_JPEG_MAX_DEQUANTISED || da < -LOCOV_JPEG_MAX_DEQUANTISED) return LOCOV_JPEG_STATUS_MAGNITUDE;
                    if (count >= cap) return LOCOV_JPEG_STATUS_SPACE;
                    ent[count++] = ((uint32_t)nat << 16) | ((uint32_t)v & 0xFFFFu);
                    i++;
                }
                if (!block_ok(ent + start[blk], count - start[blk], qt[c])) return LOCOV_JPEG_STATUS_MAGNITUDE;
            }
        }
    }
    if (br.marker() != 0xD9) return LOCOV_JPEG_STATUS_NO_EOI;
    if (count > 0xFFFFFFFFll) return LOCOV_JPEG_STATUS_SPACE;
    start[g.nblocks] = (uint32_t)count;
    *record_bytes = record_bytes_for(g.nblocks, count);
    return LOCOV_JPEG_STATUS_OK;
}

// staging (scan order) -> the record (component-plane raster order); false when the staging is not what decode_scan leaves
inline bool pack_record(const locov_jpeg_header &h, const void *staging, int64_t record_bytes, void *record)
{
    Geometry g;
    if (!geometry(h, g) || !staging || !record || ((uintptr_t)staging & 3) || ((uintptr_t)record & 3)) return false;
    const uint32_t *start = static_cast<const uint32_t *>(staging);
    const uint32_t *ent = start + g.nblocks + 1;
    const int64_t total = start[g.nblocks];
    if (record_bytes != record_bytes_for(g.nblocks, total)) return false;
    uint32_t *out_start = static_cast<uint32_t *>(record);
    uint32_t *out = out_start + g.nblocks + 1;
    int64_t at = 0, b = 0;
    for (int c = 0; c < g.ncomp; c++)
        for (int64_t by = 0; by < g.bh[c]; by++)
            for (int64_t bx = 0; bx < g.bw[c]; bx++, b++) {
                const int64_t mcu = (by / g.vs[c]) * g.mcux + bx / g.hs[c];
                const int64_t m = mcu * g.per_mcu + g.mcu_base[c] + (by % g.vs[c]) * g.hs[c] + bx % g.hs[c];
                const int64_t s = start[m], e = start[m + 1];
                if (s > e || e > total || at + (e - s) > total) return false;
                out_start[b] = (uint32_t)at;
                std::memcpy(out + at, ent + s, (size_t)(e - s) * 4);
                at += e - s;
            }
    out_start[g.nblocks] = (uint32_t)at;
    if (at != total) return false;
    const int64_t used = 4 * (g.nblocks + 1 + total);
    std::memset(static_cast<uint8_t *>(record) + used, 0, (size_t)(record_bytes - used));
    return true;
}

// fn(i) for i in [0, n) on up to min(kMaxThreads, n) threads (the caller's among them); a thread that cannot be started is done without
template <typename F>
inline void parallel_for(int n, F fn)
{
    if (n <= 0) return;
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
    };
    const int extra = (n < kMaxThreads ? n : kMaxThreads) - 1;
    std::thread threads[kMaxThreads];
    int started = 0;
    for (int t = 0; t < extra; t++) {
        try {
            threads[started] = std::thread(work);
            started++;
        } catch (...) {
            break;
        }
    }
    work();
    for (int t = 0; t < started; t++) threads[t].join();
}

}  // namespace jpeg
}  // namespace locov
