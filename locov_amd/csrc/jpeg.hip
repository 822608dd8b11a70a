// Baseline JPEG decoding for the dataset mapper (include/locov_jpeg.h; locov_amd/jpeg.py is the definition, its bytes are Pillow's):
//   locov_jpeg_parse / _entropy_bytes / _entropy_decode / _entropy_pack : the host stage, csrc/jpeg_entropy.h, bound here
//   locov_jpeg_decode : the pixel pipeline of up to LOCOV_LABEL_MAX_IMAGES images of different sizes and layouts, two launches
//     idct_kernel   eight lanes own an 8x8 block, a wave eight blocks, a workgroup 32.  The block lies in LDS as int32 [8][9] at a
//                   stride of 72 words: ds_read_b32 / ds_write_b32 bank on (word % 32) within a 32-lane half, and both the column
//                   access (word = slot * 72 + r * 9 + lane) and the row access (slot * 72 + lane * 9 + k) of the four blocks of a
//                   half then fall on 32 different banks (72 = 8 mod 32; 9 is odd).  Zero-fill, scatter entry * quantiser, jidctint's
//                   column pass (descale 11), row pass (descale 18), range limit, one 8-byte store per lane into the component plane.
//     color_kernel  a workgroup owns 16 x 64 output pixels, a thread four of a row: the luma as one dword, the chroma through
//                   jdsample.c's h2v1 / h2v2 triangle filters with neighbours clamped at the component's real size (replication up to
//                   2 samples of real width), jdcolor.c's fixed-point tables as multiplications, and the HWC bytes through LDS so
//                   that the global stores are whole dwords wherever the row's alignment allows.
// Integer arithmetic only, no atomics, no memset, nothing read by the host; the per-image table travels by value.
#include "common.h"
#include "jpeg_entropy.h"

namespace locov {
namespace {

constexpr int kBlocksPerGroup = 32, kRowStride = 9, kBlockStride = 72;
constexpr int kTH = 16, kTW = 64;
constexpr int kTileWords = kTW * 3 / 4 + 1;

struct JpegImage {
    uint32_t rec_word;                                            // the record: words from `records`
    uint32_t qt_half;                                             // the quantisation tables: uint16 elements from `records`
    uint32_t plane16;                                             // the planes: 16-byte units from the workspace
    uint32_t n_entries;                                           // words behind the block starts (padding included): the clamp
    uint16_t width, height, mcux, mcuy;
    uint8_t ncomp, hs, vs, pad;
};

struct JpegArgs {
    JpegImage img[LOCOV_LABEL_MAX_IMAGES];
    uint8_t *out[LOCOV_LABEL_MAX_IMAGES];
    int boff1[LOCOV_LABEL_MAX_IMAGES + 1];                        // idct workgroups of image i: [boff1[i], boff1[i + 1])
    int boff2[LOCOV_LABEL_MAX_IMAGES + 1];                        // colour tiles of image i
    int n_img, format;
};

// jidctint.c's one-dimensional pass (CONST_BITS 13): d[0 .. 8) -> the eight outputs, descaled by SHIFT
template <int SHIFT>
__device__ __forceinline__ void idct8(int32_t d[8])
{
    int32_t z1 = (d[2] + d[6]) * 4433;
    int32_t tmp2 = z1 + d[6] * -15137;
    int32_t tmp3 = z1 + d[2] * 6270;
    int32_t tmp0 = (d[0] + d[4]) * 8192;
    int32_t tmp1 = (d[0] - d[4]) * 8192;
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7];
    tmp1 = d[5];
    tmp2 = d[3];
    tmp3 = d[1];
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
    d[7] = (tmp10 - tmp3 + half) >> SHIFT;
    d[1] = (tmp11 + tmp2 + half) >> SHIFT;
    d[6] = (tmp11 - tmp2 + half) >> SHIFT;
    d[2] = (tmp12 + tmp1 + half) >> SHIFT;
    d[5] = (tmp12 - tmp1 + half) >> SHIFT;
    d[3] = (tmp13 + tmp0 + half) >> SHIFT;
    d[4] = (tmp13 - tmp0 + half) >> SHIFT;
}

// jdmaster.c's post-IDCT range-limit table at (x & 1023): the level shift and the clamp, wrapping as the table does
__device__ __forceinline__ uint32_t range_limit(int32_t x)
{
    const int i = x & 1023;
    return (uint32_t)(i < 128 ? 128 + i : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(JpegArgs a, const uint32_t *records, uint8_t *workspace)
{
    __shared__ int32_t tile[kBlocksPerGroup * kBlockStride];

    const int b = blockIdx.x, tid = threadIdx.x;
    int img = 0;
    while (img + 1 < a.n_img && b >= a.boff1[img + 1]) img++;
    const JpegImage im = a.img[img];
    const int slot = tid >> 3, j = tid & 7;
    const int64_t g = (int64_t)(b - a.boff1[img]) * kBlocksPerGroup + slot;
    const int64_t bw0 = (int64_t)im.mcux * im.hs, bh0 = (int64_t)im.mcuy * im.vs;
    const int64_t n0 = bw0 * bh0, nc = (int64_t)im.mcux * im.mcuy;
    const int64_t nblocks = n0 + (im.ncomp == 3 ? 2 * nc : 0);
    const bool active = g < nblocks;

    int32_t *blk = tile + slot * kBlockStride;
#pragma unroll
    for (int k = 0; k < kBlockStride / 8; k++) blk[j + 8 * k] = 0;
    __syncthreads();

    // the block's place: component, plane, position
    int comp = 0;
    int64_t local = g, bw = bw0, plane = 0;
    if (active && g >= n0) {
        comp = g >= n0 + nc ? 2 : 1;
        local = g - n0 - (comp == 2 ? nc : 0);
        bw = im.mcux;
        plane = n0 * 64 + (comp == 2 ? nc * 64 : 0);
    }
    if (active) {
        const uint32_t *start = records + im.rec_word;
        const uint32_t *entries = start + nblocks + 1;
        const uint16_t *q = reinterpret_cast<const uint16_t *>(records) + im.qt_half + comp * 64;
        uint32_t s = start[g], e = start[g + 1];
        if (e > im.n_entries) e = im.n_entries;                   // (never for a record of the host stage)
        for (uint32_t i = s + j; i < e; i += 8) {
            const uint32_t w = entries[i];
            const int idx = (w >> 16) & 63;
            blk[(idx >> 3) * kRowStride + (idx & 7)] = (int32_t)(int16_t)(w & 0xFFFFu) * (int32_t)q[idx];
        }
    }
    __syncthreads();

    int32_t d[8];
#pragma unroll
    for (int r = 0; r < 8; r++) d[r] = blk[r * kRowStride + j];   // column j
    idct8<11>(d);
#pragma unroll
    for (int r = 0; r < 8; r++) blk[r * kRowStride + j] = d[r];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = blk[j * kRowStride + k];   // row j
    idct8<18>(d);
    if (active) {
        const int64_t by = local / bw, bx = local - by * bw;
        uint8_t *dst = workspace + (int64_t)im.plane16 * 16 + plane + (by * 8 + j) * (bw * 8) + bx * 8;
        uint2 px;
        px.x = range_limit(d[0]) | (range_limit(d[1]) << 8) | (range_limit(d[2]) << 16) | (range_limit(d[3]) << 24);
        px.y = range_limit(d[4]) | (range_limit(d[5]) << 8) | (range_limit(d[6]) << 16) | (range_limit(d[7]) << 24);
        *reinterpret_cast<uint2 *>(dst) = px;                     // (8-byte aligned: the plane starts on 16, its width is a multiple of 8)
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// Four neighbouring output samples (x .. x + 3, x a multiple of 4) of a chroma plane of half the luma's width, in row y of the output
__device__ __forceinline__ void chroma_h2(const uint8_t *plane, int pw, int cw, int ch, int vs, int x, int y, int out[4])
{
    const int i0 = x >> 1;
    if (vs == 1) {
        const uint8_t *row = plane + (int64_t)y * pw;
        if (cw <= 2) {
            out[0] = out[1] = row[clampi(i0, 0, cw - 1)];
            out[2] = out[3] = row[clampi(i0 + 1, 0, cw - 1)];
            return;
        }
        int s[4];
#pragma unroll
        for (int k = 0; k < 4; k++) s[k] = row[clampi(i0 - 1 + k, 0, cw - 1)];
        out[0] = (3 * s[1] + s[0] + 1) >> 2;
        out[1] = (3 * s[1] + s[2] + 2) >> 2;
        out[2] = (3 * s[2] + s[1] + 1) >> 2;
        out[3] = (3 * s[2] + s[3] + 2) >> 2;
        return;
    }
    const int cy = clampi(y >> 1, 0, ch - 1);
    const uint8_t *near = plane + (int64_t)cy * pw;
    if (cw <= 2) {
        out[0] = out[1] = near[clampi(i0, 0, cw - 1)];
        out[2] = out[3] = near[clampi(i0 + 1, 0, cw - 1)];
        return;
    }
    const uint8_t *far = plane + (int64_t)clampi((y & 1) ? cy + 1 : cy - 1, 0, ch - 1) * pw;
    int c[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = clampi(i0 - 1 + k, 0, cw - 1);
        c[k] = 3 * near[i] + far[i];
    }
    out[0] = (3 * c[1] + c[0] + 8) >> 4;
    out[1] = (3 * c[1] + c[2] + 7) >> 4;
    out[2] = (3 * c[2] + c[1] + 8) >> 4;
    out[3] = (3 * c[2] + c[3] + 7) >> 4;
}

__device__ __forceinline__ uint32_t clip8(int v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void jpeg_color_kernel(JpegArgs a, const uint8_t *workspace)
{
    __shared__ uint32_t tile[kTH][kTileWords];                    // a row's HWC bytes, [y][x * channels + c]

    const int b = blockIdx.x, tid = threadIdx.x;
    int img = 0;
    while (img + 1 < a.n_img && b >= a.boff2[img + 1]) img++;
    const JpegImage im = a.img[img];
    const int W = im.width, H = im.height;
    const int oc = a.format == LOCOV_JPEG_L ? 1 : 3;
    const int tiles_x = (W + kTW - 1) / kTW;
    const int local = b - a.boff2[img];
    const int ty0 = local / tiles_x, tx0 = local - ty0 * tiles_x;
    const int x0 = tx0 * kTW, y0 = ty0 * kTH;

    {
        const int ty = tid >> 4, q = tid & 15;
        const int x = x0 + 4 * q, y = y0 + ty;
        if (x < W && y < H) {
            const uint8_t *planes = workspace + (int64_t)im.plane16 * 16;
            const int pw0 = im.mcux * im.hs * 8, ph0 = im.mcuy * im.vs * 8;
            const uint32_t yy = *reinterpret_cast<const uint32_t *>(planes + (int64_t)y * pw0 + x);
            uint32_t px[4][3];
            if (im.ncomp == 1) {
#pragma unroll
                for (int p = 0; p < 4; p++) px[p][0] = px[p][1] = px[p][2] = (yy >> (8 * p)) & 255u;
            } else {
                const int pwc = im.mcux * 8, phc = im.mcuy * 8;
                const uint8_t *cbp = planes + (int64_t)pw0 * ph0, *crp = cbp + (int64_t)pwc * phc;
                int cb[4], cr[4];
                if (im.hs == 1) {
                    const uint32_t u = *reinterpret_cast<const uint32_t *>(cbp + (int64_t)y * pwc + x);
                    const uint32_t v = *reinterpret_cast<const uint32_t *>(crp + (int64_t)y * pwc + x);
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        cb[p] = (int)((u >> (8 * p)) & 255u);
                        cr[p] = (int)((v >> (8 * p)) & 255u);
                    }
                } else {
                    const int cw = (W + 1) >> 1, ch = (H + im.vs - 1) / im.vs;
                    chroma_h2(cbp, pwc, cw, ch, im.vs, x, y, cb);
                    chroma_h2(crp, pwc, cw, ch, im.vs, x, y, cr);
                }
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int l = (int)((yy >> (8 * p)) & 255u), u = cb[p] - 128, v = cr[p] - 128;
                    const uint32_t r = clip8(l + ((91881 * v + 32768) >> 16));
                    const uint32_t g = clip8(l + ((-22554 * u + 32768 - 46802 * v) >> 16));
                    const uint32_t bl = clip8(l + ((116130 * u + 32768) >> 16));
                    px[p][0] = a.format == LOCOV_JPEG_BGR ? bl : r;
                    px[p][1] = g;
                    px[p][2] = a.format == LOCOV_JPEG_BGR ? r : bl;
                }
            }
            if (oc == 1) {
                tile[ty][q] = px[0][0] | (px[1][0] << 8) | (px[2][0] << 16) | (px[3][0] << 24);
            } else {
                tile[ty][3 * q] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
                tile[ty][3 * q + 1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
                tile[ty][3 * q + 2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
            }
        }
    }
    __syncthreads();

    // the stores: sixteen threads per row; whole dwords between the row's first and last aligned address, bytes at its two ends
    const int r = tid >> 4, k = tid & 15;
    if (y0 + r >= H) return;
    const int nb = (W - x0 < kTW ? W - x0 : kTW) * oc;
    uint8_t *dst = a.out[img] + ((int64_t)(y0 + r) * W + x0) * oc;
    int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > nb) head = nb;
    const int nd = (nb - head) >> 2, tail = nb - head - 4 * nd;
    const uint32_t *row = tile[r];
    for (int i = k; i < nd; i += 16) {
        const int o = head + 4 * i, sh = (o & 3) * 8;
        uint32_t w = row[o >> 2];
        if (sh) w = (w >> sh) | (row[(o >> 2) + 1] << (32 - sh));
        *reinterpret_cast<uint32_t *>(dst + o) = w;
    }
    if (k == 0)
        for (int o = 0; o < head; o++) dst[o] = (uint8_t)(row[o >> 2] >> ((o & 3) * 8));
    if (k == 1)
        for (int o = nb - tail; o < nb; o++) dst[o] = (uint8_t)(row[o >> 2] >> ((o & 3) * 8));
}

// One descriptor's geometry; false outside the limits of the header
struct Layout {
    int64_t mcux, mcuy, nblocks, plane_bytes;
};

bool layout_of(const locov_jpeg_desc &d, Layout &l)
{
    if (d.width < 1 || d.width > 65535 || d.height < 1 || d.height > 65535) return false;
    if (d.ncomp == 1) {
        if (d.hs != 1 || d.vs != 1) return false;
    } else if (d.ncomp == 3) {
        if (!((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return false;
    } else {
        return false;
    }
    l.mcux = ceil_div(d.width, 8 * d.hs);
    l.mcuy = ceil_div(d.height, 8 * d.vs);
    l.nblocks = l.mcux * l.mcuy * (d.hs * d.vs + (d.ncomp == 3 ? 2 : 0));
    l.plane_bytes = ceil_div(l.nblocks * 64, 16) * 16;
    return true;
}

}  // namespace
}  // namespace locov

using namespace locov;

extern "C" {

int locov_jpeg_parse(const void *data_host, int64_t len, locov_jpeg_header *header)
{
    LOCOV_REQUIRE(header && (data_host || len == 0) && len >= 0, "locov_jpeg_parse: null pointer or negative length");
    jpeg::parse(static_cast<const uint8_t *>(data_host), len, header);
    return LOCOV_OK;
}

int64_t locov_jpeg_entropy_bytes(const locov_jpeg_header *header, int64_t len)
{
    return header ? jpeg::entropy_bytes(*header, len) : 0;
}

int locov_jpeg_entropy_decode(const void *const *data_host, const int64_t *lens_host, const locov_jpeg_header *headers_host,
                              void *const *staging_host, const int64_t *staging_bytes_host, int n, int32_t *status_host,
                              int64_t *record_bytes_host)
{
    LOCOV_REQUIRE(n >= 0, "locov_jpeg_entropy_decode: negative count");
    if (n == 0) return LOCOV_OK;
    LOCOV_REQUIRE(data_host && lens_host && headers_host && staging_host && staging_bytes_host && status_host && record_bytes_host,
                  "locov_jpeg_entropy_decode: null pointer");
    jpeg::parallel_for(n, [&](int i) {
        record_bytes_host[i] = 0;
        if (!data_host[i] || lens_host[i] < 0) {
            status_host[i] = LOCOV_JPEG_STATUS_UNSUPPORTED;
            return;
        }
        status_host[i] = jpeg::decode_scan(static_cast<const uint8_t *>(data_host[i]), lens_host[i], headers_host[i], staging_host[i],
                                           staging_bytes_host[i], &record_bytes_host[i]);
    });
    return LOCOV_OK;
}

int locov_jpeg_entropy_pack(const locov_jpeg_header *headers_host, const void *const *staging_host, const int64_t *record_bytes_host,
                            void *const *records_host, int n)
{
    LOCOV_REQUIRE(n >= 0, "locov_jpeg_entropy_pack: negative count");
    if (n == 0) return LOCOV_OK;
    LOCOV_REQUIRE(headers_host && staging_host && record_bytes_host && records_host, "locov_jpeg_entropy_pack: null pointer");
    std::atomic<int> bad{-1};
    jpeg::parallel_for(n, [&](int i) {
        if (record_bytes_host[i] == 0) return;                    // (an image the decode refused)
        if (!jpeg::pack_record(headers_host[i], staging_host[i], record_bytes_host[i], records_host[i])) bad.store(i);
    });
    LOCOV_REQUIRE(bad.load() < 0, "locov_jpeg_entropy_pack: image %d: the staging is not what locov_jpeg_entropy_decode left for %lld bytes",
                  bad.load(), (long long)record_bytes_host[bad.load()]);
    return LOCOV_OK;
}

int64_t locov_jpeg_decode_workspace_bytes(const locov_jpeg_desc *descs_host, int n_images)
{
    if (n_images < 0 || n_images > LOCOV_LABEL_MAX_IMAGES || (n_images > 0 && !descs_host)) return -1;
    int64_t total = 0;
    for (int i = 0; i < n_images; i++) {
        Layout l;
        if (!layout_of(descs_host[i], l)) return -1;
        total += l.plane_bytes;
    }
    return total;
}

int locov_jpeg_decode(const void *records, int64_t record_bytes, const locov_jpeg_desc *descs_host, int n_images, int format,
                      void *const *outs_host, void *workspace, int64_t workspace_bytes, locov_stream_t stream)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= LOCOV_LABEL_MAX_IMAGES, "locov_jpeg_decode: 0..%d images per call", LOCOV_LABEL_MAX_IMAGES);
    if (n_images == 0) return LOCOV_OK;
    LOCOV_REQUIRE(format == LOCOV_JPEG_RGB || format == LOCOV_JPEG_BGR || format == LOCOV_JPEG_L, "locov_jpeg_decode: unknown format %d", format);
    LOCOV_REQUIRE(records && descs_host && outs_host && workspace, "locov_jpeg_decode: null pointer");
    LOCOV_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "locov_jpeg_decode: records and workspace must be 16-byte aligned");
    JpegArgs a{};
    int64_t planes = 0, groups = 0, tiles = 0;
    for (int i = 0; i < n_images; i++) {
        const locov_jpeg_desc &d = descs_host[i];
        Layout l;
        LOCOV_REQUIRE(layout_of(d, l), "locov_jpeg_decode: image %d: %d x %d, %d components, luma %d x %d is outside the decoder's layouts", i,
                      d.width, d.height, d.ncomp, d.hs, d.vs);
        LOCOV_REQUIRE(format != LOCOV_JPEG_L || d.ncomp == 1, "locov_jpeg_decode: image %d: format L takes grey streams only", i);
        LOCOV_REQUIRE(outs_host[i], "locov_jpeg_decode: null pointer (image %d)", i);
        LOCOV_REQUIRE(d.record_offset >= 0 && (d.record_offset & 15) == 0 && d.record_bytes >= 4 * (l.nblocks + 1) &&
                          d.record_offset <= record_bytes && d.record_bytes <= record_bytes - d.record_offset &&
                          d.record_offset / 4 <= (int64_t)UINT32_MAX,
                      "locov_jpeg_decode: image %d: a record of %lld bytes at %lld does not fit %lld bytes of records (or is misaligned, or "
                      "smaller than its %lld block starts)", i, (long long)d.record_bytes, (long long)d.record_offset, (long long)record_bytes,
                      (long long)l.nblocks + 1);
        LOCOV_REQUIRE(d.qt_offset >= 0 && (d.qt_offset & 3) == 0 && d.qt_offset <= record_bytes && 128 * d.ncomp <= record_bytes - d.qt_offset &&
                          d.qt_offset / 2 <= (int64_t)UINT32_MAX,
                      "locov_jpeg_decode: image %d: quantisation tables at %lld leave the %lld bytes of records (or are misaligned)", i,
                      (long long)d.qt_offset, (long long)record_bytes);
        const int64_t entries = d.record_bytes / 4 - (l.nblocks + 1);
        JpegImage &im = a.img[i];
        im.rec_word = (uint32_t)(d.record_offset / 4);
        im.qt_half = (uint32_t)(d.qt_offset / 2);
        im.plane16 = (uint32_t)(planes / 16);
        im.n_entries = (uint32_t)(entries > (int64_t)UINT32_MAX ? UINT32_MAX : entries);
        im.width = (uint16_t)d.width;
        im.height = (uint16_t)d.height;
        im.mcux = (uint16_t)l.mcux;
        im.mcuy = (uint16_t)l.mcuy;
        im.ncomp = (uint8_t)d.ncomp;
        im.hs = (uint8_t)d.hs;
        im.vs = (uint8_t)d.vs;
        a.out[i] = static_cast<uint8_t *>(outs_host[i]);
        a.boff1[i] = (int)groups;
        a.boff2[i] = (int)tiles;
        planes += l.plane_bytes;
        groups += ceil_div(l.nblocks, kBlocksPerGroup);
        tiles += ceil_div(d.height, kTH) * ceil_div(d.width, kTW);
        LOCOV_REQUIRE(groups <= INT32_MAX && tiles <= INT32_MAX && planes / 16 <= (int64_t)UINT32_MAX,
                      "locov_jpeg_decode: the batch leaves the launch grid at image %d", i);
    }
    LOCOV_REQUIRE(workspace_bytes >= planes, "locov_jpeg_decode: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)planes);
    a.boff1[n_images] = (int)groups;
    a.boff2[n_images] = (int)tiles;
    a.n_img = n_images;
    a.format = format;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)groups), dim3(256), 0, as_stream(stream), a, static_cast<const uint32_t *>(records),
                       static_cast<uint8_t *>(workspace));
    const int rc = check_launch("locov_jpeg_decode (idct)");
    if (rc != LOCOV_OK) return rc;
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), a, static_cast<const uint8_t *>(workspace));
    return check_launch("locov_jpeg_decode (colour)");
}

}  // extern "C"
