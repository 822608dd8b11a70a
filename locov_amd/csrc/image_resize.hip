// The input pipeline's image side in ONE launch for the whole batch (data.py: DatasetMapper.map_batch):
//   locov_resize_flip_images : Pillow's 8-bit bilinear resize (ImagingResample: a horizontal pass that writes rounded bytes, then a
//                              vertical pass over those bytes), Detectron2's HFlip / VFlip and the HWC -> CHW transposition of N
//                              images of different sizes.
// Compiled with -ffp-contract=off: the coefficients are formed here in fp64, every operation rounded on its own, exactly as
// Pillow's precompute_coeffs forms them on the host, so the integer taps -- and with them every output byte -- are Pillow's.
// A workgroup owns a kTH x kTW tile of one image's output.  It forms the taps of its 64 columns and 16 rows, runs the horizontal
// pass over the source rows its band needs into LDS (the "strip": rounded bytes, [row][channel][column]), and the vertical pass
// reads four columns per 32-bit LDS word.  The flip is an index reversal at the store.  No workspace, no atomics, nothing read by
// the host; the per-image tables travel in a by-value argument struct (the idiom of image_batch.hip).
#include "common.h"

#include <cmath>

namespace locov {
namespace {

constexpr int kTH = 16, kTW = 64, kQuads = kTW / 4;
constexpr int kTaps = LOCOV_RESIZE_MAX_TAPS;
// Source rows of one band: (kTH - 1) * scale + 2 * support + 1 <= 17 * 8 + 1 = 137 at the tap limit (scale = support = 8).  The host
// walks every band of every image with the device's own window arithmetic before the launch: the largest band it finds is the
// launch's dynamic LDS strip (more workgroups per CU for the common mild scales), and none may exceed kStripRows.
constexpr int kStripRows = 144;
constexpr int kPrecisionBits = 22;                                // Pillow's PRECISION_BITS for 8-bit channels: 32 - 8 - 2

struct ResizeArgs {
    const uint8_t *src[LOCOV_LABEL_MAX_IMAGES];                   // image i: [h[i], w[i], C], contiguous, any byte alignment
    uint8_t *dst[LOCOV_LABEL_MAX_IMAGES];                         // its output: [C, oh[i], ow[i]], contiguous, any byte alignment
    int h[LOCOV_LABEL_MAX_IMAGES], w[LOCOV_LABEL_MAX_IMAGES], oh[LOCOV_LABEL_MAX_IMAGES], ow[LOCOV_LABEL_MAX_IMAGES];
    int boff[LOCOV_LABEL_MAX_IMAGES + 1];                         // workgroups of image i: [boff[i], boff[i + 1])
    uint8_t flip[LOCOV_LABEL_MAX_IMAGES];
    int n_img, channels;
};

// precompute_coeffs' window of output index xx: the first source index and the number of taps.  Shared by the kernel and by the
// host's checks (both sides are IEEE fp64 with no contraction, so they agree bit for bit).
__host__ __device__ inline void axis_window(int in, int out, int xx, double &scale, double &fs, double &center, int &xmin, int &count)
{
    scale = (double)in / (double)out;
    fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    center = ((double)xx + 0.5) * scale;
    xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    count = xmax - xmin;
}

__host__ __device__ inline int axis_taps(int in, int out)        // precompute_coeffs' ksize
{
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(1.0 * fs) * 2 + 1;
}

__device__ __forceinline__ double bilinear_filter(double t)
{
    if (t < 0.0) t = -t;
    return t < 1.0 ? 1.0 - t : 0.0;
}

// The integer taps of output index xx into k[0 .. count).  The weights are formed twice (once for their sum, once to be divided by
// it) instead of being kept in an indexed array: the same operations on the same operands give the same doubles.
__device__ void axis_coeffs(int in, int out, int xx, int *k, int &xmin_out, int &count_out)
{
    double scale, fs, center;
    int xmin, count;
    axis_window(in, out, xx, scale, fs, center, xmin, count);
    if (count > kTaps) count = kTaps;                             // (never: the host refuses more taps)
    const double ss = 1.0 / fs;
    double ww = 0.0;
    for (int x = 0; x < count; x++) ww += bilinear_filter(((double)(x + xmin) - center + 0.5) * ss);
    for (int x = 0; x < count; x++) {
        double wx = bilinear_filter(((double)(x + xmin) - center + 0.5) * ss);
        if (ww != 0.0) wx /= ww;
        k[x] = wx < 0.0 ? (int)(-0.5 + wx * (double)(1 << kPrecisionBits)) : (int)(0.5 + wx * (double)(1 << kPrecisionBits));
    }
    xmin_out = xmin;
    count_out = count;
}

__device__ __forceinline__ unsigned clip8(int acc)
{
    const int v = acc >> kPrecisionBits;
    return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void resize_flip_kernel(ResizeArgs a, int strip_rows)
{
    extern __shared__ uint32_t strip[];                           // [strip_rows][channel][quad of columns]: what the batch needs, <= 36 KiB
    __shared__ int hk[kTW][kTaps], vk[kTH][kTaps];
    __shared__ int hmin[kTW], hcnt[kTW], vmin[kTH], vcnt[kTH];

    const int b = blockIdx.x, tid = threadIdx.x;
    int img = 0;
    while (img + 1 < a.n_img && b >= a.boff[img + 1]) img++;
    const int C = a.channels, h = a.h[img], w = a.w[img], oh = a.oh[img], ow = a.ow[img], flip = a.flip[img];
    const int tiles_x = (ow + kTW - 1) / kTW;
    const int local = b - a.boff[img];
    const int by = local / tiles_x, bx = local - by * tiles_x;
    const int x0 = bx * kTW, y0 = by * kTH;
    const int th = oh - y0 < kTH ? oh - y0 : kTH;                 // (>= 1: the grid holds no empty band)

    if (tid < kTW) {
        hmin[tid] = 0;
        hcnt[tid] = 0;                                            // a column past the image: no taps, never stored
        if (x0 + tid < ow) axis_coeffs(w, ow, x0 + tid, hk[tid], hmin[tid], hcnt[tid]);
    } else if (tid < kTW + kTH) {
        const int t = tid - kTW;
        vmin[t] = 0;
        vcnt[t] = 0;
        if (t < th) axis_coeffs(h, oh, y0 + t, vk[t], vmin[t], vcnt[t]);
    }
    __syncthreads();

    // the source rows of this band: the windows' ends do not decrease with the output row
    const int rlo = vmin[0];
    int nrows = vmin[th - 1] + vcnt[th - 1] - rlo;
    if (nrows > strip_rows) nrows = strip_rows;                   // (never: strip_rows is the host's maximum over every band)

    // horizontal pass: four columns of one channel of one source row per item, channels on neighbouring lanes
    const uint8_t *src = a.src[img];
    const int hitems = nrows * kQuads * C;
    for (int it = tid; it < hitems; it += 256) {
        const int rq = it / C, c = it - rq * C;
        const int q = rq & (kQuads - 1), r = rq / kQuads;
        const uint8_t *row = src + ((int64_t)(rlo + r) * w) * C + c;
        // every tap's byte is asked for before the first is used: the address of a tap past its window is the window's first
        // (always inside the row) and its coefficient 0, so a chunk's 16 loads are unconditional and in flight together
        int m[4], n[4], acc[4], nmax = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            m[j] = hmin[q * 4 + j];
            n[j] = hcnt[q * 4 + j];
            nmax = n[j] > nmax ? n[j] : nmax;
            acc[j] = 1 << (kPrecisionBits - 1);
        }
        for (int i0 = 0; i0 < nmax; i0 += 4) {
            int px[4][4], kk[4][4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int ii = 0; ii < 4; ii++) {
                    const bool on = i0 + ii < n[j];
                    const int i = on ? i0 + ii : 0;
                    px[j][ii] = (int)row[(int64_t)(m[j] + i) * C];
                    kk[j][ii] = on ? hk[q * 4 + j][i] : 0;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int ii = 0; ii < 4; ii++) acc[j] += kk[j][ii] * px[j][ii];
            }
        }
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) packed |= clip8(acc[j]) << (8 * j);
        strip[(r * C + c) * kQuads + q] = packed;
    }
    __syncthreads();

    // vertical pass over the strip's rounded bytes; the quad is the fastest index, so a wave writes whole runs of an output row
    uint8_t *dst = a.dst[img];
    const int vitems = th * kQuads * C;
    for (int it = tid; it < vitems; it += 256) {
        const int q = it & (kQuads - 1), rest = it / kQuads;
        const int c = rest / th, ty = rest - c * th;
        const int x = x0 + q * 4;
        const int nv = ow - x < 4 ? ow - x : 4;
        if (nv <= 0) continue;
        const int base = vmin[ty] - rlo, n = vcnt[ty];
        int acc[4];
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = 1 << (kPrecisionBits - 1);
        for (int i = 0; i < n; i++) {
            const int k = vk[ty][i];
            const uint32_t word = strip[((base + i) * C + c) * kQuads + q];
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] += k * (int)((word >> (8 * j)) & 255u);
        }
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = clip8(acc[j]);
        const int y = y0 + ty, yd = flip == LOCOV_FLIP_VERTICAL ? oh - 1 - y : y;
        uint8_t *drow = dst + ((int64_t)c * oh + yd) * ow;
        if (flip == LOCOV_FLIP_HORIZONTAL) {
            if (nv == 4) {
                uint8_t *p = drow + (ow - 4 - x);
                if (((uintptr_t)p & 3) == 0) {
                    *reinterpret_cast<uint32_t *>(p) = v[3] | (v[2] << 8) | (v[1] << 16) | (v[0] << 24);
                    continue;
                }
            }
            for (int j = 0; j < nv; j++) drow[ow - 1 - x - j] = (uint8_t)v[j];
        } else {
            uint8_t *p = drow + x;
            if (nv == 4 && ((uintptr_t)p & 3) == 0) {
                *reinterpret_cast<uint32_t *>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
                continue;
            }
            for (int j = 0; j < nv; j++) p[j] = (uint8_t)v[j];
        }
    }
}

// The most source rows a band of kTH output rows of this axis reads, with the kernel's own window arithmetic.
int max_band_rows(int in, int out)
{
    int most = 0;
    for (int y0 = 0; y0 < out; y0 += kTH) {
        const int y1 = (y0 + kTH < out ? y0 + kTH : out) - 1;
        double scale, fs, center;
        int lo, n0, last, n1;
        axis_window(in, out, y0, scale, fs, center, lo, n0);
        axis_window(in, out, y1, scale, fs, center, last, n1);
        if (last + n1 - lo > most) most = last + n1 - lo;
    }
    return most;
}

bool sizes_supported(int in_h, int in_w, int out_h, int out_w, int channels)
{
    if (in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || channels < 1 || channels > LOCOV_IMAGE_MAX_CHANNELS) return false;
    if ((int64_t)in_h * in_w * channels > INT32_MAX || (int64_t)out_h * out_w * channels > INT32_MAX) return false;
    return axis_taps(in_h, out_h) <= kTaps && axis_taps(in_w, out_w) <= kTaps;
}

}  // namespace
}  // namespace locov

using namespace locov;

extern "C" {

int locov_resize_supported(int in_h, int in_w, int out_h, int out_w, int channels)
{
    return sizes_supported(in_h, in_w, out_h, out_w, channels) ? 1 : 0;
}

int locov_resize_flip_images(const void *const *images_host, const int *heights_host, const int *widths_host, void *const *outs_host,
                             const int *out_heights_host, const int *out_widths_host, const int *flips_host, int n_images, int channels,
                             locov_stream_t stream)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= LOCOV_LABEL_MAX_IMAGES, "locov_resize_flip_images: 0..%d images per call", LOCOV_LABEL_MAX_IMAGES);
    if (n_images == 0) return LOCOV_OK;
    LOCOV_REQUIRE(channels >= 1 && channels <= LOCOV_IMAGE_MAX_CHANNELS, "locov_resize_flip_images: channels must be 1..%d, got %d",
                  LOCOV_IMAGE_MAX_CHANNELS, channels);
    LOCOV_REQUIRE(images_host && heights_host && widths_host && outs_host && out_heights_host && out_widths_host && flips_host,
                  "locov_resize_flip_images: null pointer");
    ResizeArgs a{};
    int64_t blocks = 0;
    int strip_rows = 1;
    for (int i = 0; i < n_images; i++) {
        const int h = heights_host[i], w = widths_host[i], oh = out_heights_host[i], ow = out_widths_host[i], flip = flips_host[i];
        LOCOV_REQUIRE(images_host[i] && outs_host[i], "locov_resize_flip_images: null pointer (image %d)", i);
        LOCOV_REQUIRE(h >= 1 && w >= 1 && oh >= 1 && ow >= 1, "locov_resize_flip_images: image %d: sizes must be positive, got %d x %d -> %d x %d",
                      i, h, w, oh, ow);
        LOCOV_REQUIRE(flip == LOCOV_FLIP_NONE || flip == LOCOV_FLIP_HORIZONTAL || flip == LOCOV_FLIP_VERTICAL,
                      "locov_resize_flip_images: image %d: unknown flip %d", i, flip);
        LOCOV_REQUIRE((int64_t)h * w * channels <= INT32_MAX && (int64_t)oh * ow * channels <= INT32_MAX,
                      "locov_resize_flip_images: image %d: %d x %d -> %d x %d x %d channels leaves the int32 offsets", i, h, w, oh, ow, channels);
        LOCOV_REQUIRE(axis_taps(h, oh) <= kTaps && axis_taps(w, ow) <= kTaps,
                      "locov_resize_flip_images: image %d: %d x %d -> %d x %d needs %d x %d taps, over the limit of %d", i, h, w, oh, ow,
                      axis_taps(h, oh), axis_taps(w, ow), kTaps);
        const int band_rows = max_band_rows(h, oh);
        LOCOV_REQUIRE(band_rows <= kStripRows, "locov_resize_flip_images: image %d: a band of %d source rows does not fit the strip", i, band_rows);
        if (band_rows > strip_rows) strip_rows = band_rows;
        a.src[i] = static_cast<const uint8_t *>(images_host[i]);
        a.dst[i] = static_cast<uint8_t *>(outs_host[i]);
        a.h[i] = h;
        a.w[i] = w;
        a.oh[i] = oh;
        a.ow[i] = ow;
        a.flip[i] = (uint8_t)flip;
        a.boff[i] = (int)blocks;
        blocks += ceil_div(oh, kTH) * ceil_div(ow, kTW);
        LOCOV_REQUIRE(blocks <= INT32_MAX, "locov_resize_flip_images: the batch leaves the launch grid at image %d", i);
    }
    a.boff[n_images] = (int)blocks;
    a.n_img = n_images;
    a.channels = channels;
    const size_t strip_bytes = (size_t)strip_rows * channels * kQuads * sizeof(uint32_t);     // <= 144 * 4 * 16 * 4 = 36 KiB
    hipLaunchKernelGGL(resize_flip_kernel, dim3((unsigned)blocks), dim3(256), strip_bytes, as_stream(stream), a, strip_rows);
    return check_launch("locov_resize_flip_images");
}

}  // extern "C"
