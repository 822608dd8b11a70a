// The two ends of the detector call, each as ONE launch for the whole batch (meta_arch.py: preprocess_image / _postprocess):
//   locov_preprocess_images : (x - pixel_mean) / pixel_std of N images of different sizes, padded into one [N, C, Hb, Wb] fp32 batch
//   locov_detector_rescale  : detector_postprocess' box part -- scale, clip, drop the empty boxes, kept rows compacted in order
// Compiled with -ffp-contract=off: the subtraction, the division and the products round one by one, as the torch ops they stand for.
// The per-image tables travel in a by-value argument struct (the idiom of detect_common.h's DetGeom): no H2D copy, no workspace.
#include "box_clip_common.h"
#include "select_common.h"

namespace locov {
namespace {

struct ImageBatchArgs {
    const void *src[LOCOV_LABEL_MAX_IMAGES];                     // image i: [C, h[i], w[i]], contiguous, any byte alignment
    int h[LOCOV_LABEL_MAX_IMAGES], w[LOCOV_LABEL_MAX_IMAGES];
    float mean[LOCOV_IMAGE_MAX_CHANNELS], std[LOCOV_IMAGE_MAX_CHANNELS];
    int n_img, channels;
};

template <typename T>
__device__ __forceinline__ float normalised(T x, float mean, float std)
{
    return __fdiv_rn(__fsub_rn((float)x, mean), std);             // two roundings, an IEEE division: torch's (x - mean) / std
}

// One thread per 16 bytes of the FLAT output (its base is 16-byte aligned; its rows are not when Wb % 4 != 0, so a quad may
// run over the end of a row, of a plane or of an image).  Consecutive lanes read consecutive source addresses.  Where a quad
// lies inside one source row and that address is aligned, the four pixels come in one load.
template <typename T>
__global__ __launch_bounds__(256) void preprocess_images_kernel(ImageBatchArgs a, float pad, float *__restrict__ out, int Hb, int Wb,
                                                                int64_t total)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t first = q * 4;
    if (first >= total) return;
    const unsigned plane = (unsigned)Hb * (unsigned)Wb;           // (< 2^31: checked by the host)
    const int pl = (int)(first / plane);                          // (at most 64 x 4 planes)
    const unsigned rem = (unsigned)(first - (int64_t)pl * plane);
    int y = (int)(rem / (unsigned)Wb), x = (int)(rem - (unsigned)y * (unsigned)Wb);
    int n = pl / a.channels, c = pl - n * a.channels;

    float v[4];
    const int h = a.h[n], w = a.w[n];
    bool done = false;
    if (first + 4 <= total && x + 4 <= Wb) {                      // the quad stays in one output row
        if (y >= h || x >= w) {
            v[0] = v[1] = v[2] = v[3] = pad;
            done = true;
        } else if (x + 4 <= w) {
            const T *p = static_cast<const T *>(a.src[n]) + ((int64_t)c * h + y) * w + x;
            const float m = a.mean[c], s = a.std[c];
            if constexpr (sizeof(T) == 1) {
                if (((uintptr_t)p & 3) == 0) {
                    const unsigned u = *reinterpret_cast<const unsigned *>(p);
                    v[0] = normalised<unsigned>(u & 255u, m, s);
                    v[1] = normalised<unsigned>((u >> 8) & 255u, m, s);
                    v[2] = normalised<unsigned>((u >> 16) & 255u, m, s);
                    v[3] = normalised<unsigned>(u >> 24, m, s);
                    done = true;
                }
            } else {
                if (((uintptr_t)p & 15) == 0) {
                    const float4 u = *reinterpret_cast<const float4 *>(p);
                    v[0] = normalised<float>(u.x, m, s);
                    v[1] = normalised<float>(u.y, m, s);
                    v[2] = normalised<float>(u.z, m, s);
                    v[3] = normalised<float>(u.w, m, s);
                    done = true;
                }
            }
            if (!done) {
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = normalised<T>(p[j], m, s);
                done = true;
            }
        }
    }
    if (!done) {                                                  // element by element, carrying x -> y -> channel -> image
        const int valid = total - first < 4 ? (int)(total - first) : 4;
        for (int j = 0; j < 4; j++) {
            v[j] = pad;
            if (j < valid) {
                const int hh = a.h[n], ww = a.w[n];
                if (y < hh && x < ww)
                    v[j] = normalised<T>(static_cast<const T *>(a.src[n])[((int64_t)c * hh + y) * ww + x], a.mean[c], a.std[c]);
                if (++x == Wb) {
                    x = 0;
                    if (++y == Hb) {
                        y = 0;
                        if (++c == a.channels) {
                            c = 0;
                            n++;                                  // (n == n_img only past the last valid element)
                        }
                    }
                }
            }
        }
        if (valid < 4) {
            for (int j = 0; j < valid; j++) out[first + j] = v[j];
            return;
        }
    }
    *reinterpret_cast<float4 *>(out + first) = make_float4(v[0], v[1], v[2], v[3]);
}

struct RescaleArgs {
    int roff[LOCOV_LABEL_MAX_IMAGES + 1];                         // rows of image i: [roff[i], roff[i + 1])
    float sx[LOCOV_LABEL_MAX_IMAGES], sy[LOCOV_LABEL_MAX_IMAGES];
    float w[LOCOV_LABEL_MAX_IMAGES], h[LOCOV_LABEL_MAX_IMAGES];   // the output sizes, as the fp32 limits torch's clamp compares with
};

// One workgroup per image: 256 rows at a time, block_ballot_rank gives each kept row its place.
__global__ __launch_bounds__(256) void detector_rescale_kernel(const float4 *__restrict__ boxes, RescaleArgs a, float4 *__restrict__ out_boxes,
                                                               int64_t *__restrict__ src, int *__restrict__ counts)
{
    __shared__ int wave_kept[4];
    const int img = blockIdx.x, lo = a.roff[img], n = a.roff[img + 1] - lo;
    const float sx = a.sx[img], sy = a.sy[img], W = a.w[img], H = a.h[img];
    const int tid = threadIdx.x;
    int kept = 0;
    for (int base = 0; base < n; base += 256) {
        const int r = base + tid;
        bool keep = false;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) {
            b = boxes[(int64_t)lo + r];
            b.x = clamp_like_torch(__fmul_rn(b.x, sx), W);
            b.y = clamp_like_torch(__fmul_rn(b.y, sy), H);
            b.z = clamp_like_torch(__fmul_rn(b.z, sx), W);
            b.w = clamp_like_torch(__fmul_rn(b.w, sy), H);
            keep = (__fsub_rn(b.z, b.x) > 0.f) && (__fsub_rn(b.w, b.y) > 0.f);
        }
        int all;
        const int at = kept + block_ballot_rank<256>(keep, wave_kept, all);
        if (keep) {
            out_boxes[(int64_t)lo + at] = b;
            src[(int64_t)lo + at] = r;
        }
        kept += all;
        __syncthreads();
    }
    for (int r = kept + tid; r < n; r += 256) {
        out_boxes[(int64_t)lo + r] = make_float4(0.f, 0.f, 0.f, 0.f);
        src[(int64_t)lo + r] = -1;
    }
    if (tid == 0) counts[img] = kept;
}

}  // namespace
}  // namespace locov

using namespace locov;

extern "C" {

int locov_preprocess_images(const void *const *images_host, const int *heights_host, const int *widths_host, int n_images, int dtype,
                            int channels, const float *mean_host, const float *std_host, float pad_value, float *out, int Hb, int Wb,
                            locov_stream_t stream)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= LOCOV_LABEL_MAX_IMAGES, "locov_preprocess_images: 0..%d images per call", LOCOV_LABEL_MAX_IMAGES);
    if (n_images == 0) return LOCOV_OK;
    LOCOV_REQUIRE(dtype == LOCOV_IMAGE_U8 || dtype == LOCOV_IMAGE_F32, "locov_preprocess_images: unknown dtype %d", dtype);
    LOCOV_REQUIRE(channels >= 1 && channels <= LOCOV_IMAGE_MAX_CHANNELS, "locov_preprocess_images: channels must be 1..%d, got %d",
                  LOCOV_IMAGE_MAX_CHANNELS, channels);
    LOCOV_REQUIRE(images_host && heights_host && widths_host && mean_host && std_host && out, "locov_preprocess_images: null pointer");
    LOCOV_REQUIRE(Hb >= 1 && Wb >= 1 && (int64_t)Hb * Wb <= INT32_MAX, "locov_preprocess_images: bad batch size %d x %d", Hb, Wb);
    LOCOV_REQUIRE((uintptr_t)out % 16 == 0, "locov_preprocess_images: out must be 16-byte aligned");
    ImageBatchArgs a{};
    const unsigned elem = dtype == LOCOV_IMAGE_U8 ? 1 : 4;
    for (int i = 0; i < n_images; i++) {
        const int h = heights_host[i], w = widths_host[i];
        LOCOV_REQUIRE(h >= 0 && w >= 0 && h <= Hb && w <= Wb, "locov_preprocess_images: image %d is %d x %d, larger than the batch's %d x %d",
                      i, h, w, Hb, Wb);
        LOCOV_REQUIRE(h == 0 || w == 0 || images_host[i], "locov_preprocess_images: null pointer (image %d)", i);
        LOCOV_REQUIRE((uintptr_t)images_host[i] % elem == 0, "locov_preprocess_images: image %d is not aligned to its element size", i);
        a.src[i] = images_host[i];
        a.h[i] = h;
        a.w[i] = w;
    }
    for (int c = 0; c < channels; c++) {
        a.mean[c] = mean_host[c];
        a.std[c] = std_host[c];
    }
    a.n_img = n_images;
    a.channels = channels;
    const int64_t total = (int64_t)n_images * channels * Hb * Wb;
    const int64_t blocks = ceil_div(ceil_div(total, 4), 256);
    LOCOV_REQUIRE(blocks <= INT32_MAX, "locov_preprocess_images: %lld output elements leave the launch grid", (long long)total);
    if (dtype == LOCOV_IMAGE_U8)
        hipLaunchKernelGGL(preprocess_images_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a, pad_value, out, Hb, Wb, total);
    else
        hipLaunchKernelGGL(preprocess_images_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a, pad_value, out, Hb, Wb, total);
    return check_launch("locov_preprocess_images");
}

int locov_detector_rescale(const float *boxes, const int *roff_host, const float *scale_x_host, const float *scale_y_host,
                           const int *out_h_host, const int *out_w_host, int n_images, float *out_boxes, int64_t *src, int *counts,
                           locov_stream_t stream)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= LOCOV_LABEL_MAX_IMAGES, "locov_detector_rescale: 0..%d images per call", LOCOV_LABEL_MAX_IMAGES);
    if (n_images == 0) return LOCOV_OK;
    LOCOV_REQUIRE(roff_host && scale_x_host && scale_y_host && out_h_host && out_w_host && counts, "locov_detector_rescale: null pointer");
    RescaleArgs a{};
    LOCOV_REQUIRE(roff_host[0] == 0, "locov_detector_rescale: roff[0] must be 0");
    for (int i = 0; i < n_images; i++) {
        LOCOV_REQUIRE(roff_host[i + 1] >= roff_host[i], "locov_detector_rescale: roff must not decrease (image %d)", i);
        a.roff[i] = roff_host[i];
        a.sx[i] = scale_x_host[i];
        a.sy[i] = scale_y_host[i];
        a.w[i] = (float)out_w_host[i];
        a.h[i] = (float)out_h_host[i];
    }
    a.roff[n_images] = roff_host[n_images];
    if (roff_host[n_images] > 0) {
        LOCOV_REQUIRE(boxes && out_boxes && src, "locov_detector_rescale: null pointer");
        LOCOV_REQUIRE((uintptr_t)boxes % 16 == 0 && (uintptr_t)out_boxes % 16 == 0 && (uintptr_t)src % 8 == 0,
                      "locov_detector_rescale: boxes / out_boxes must be 16-byte aligned, src 8-byte aligned");
        LOCOV_REQUIRE(boxes != out_boxes, "locov_detector_rescale: out_boxes must not be boxes");
    }
    hipLaunchKernelGGL(detector_rescale_kernel, dim3((unsigned)n_images), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float4 *>(boxes), a, reinterpret_cast<float4 *>(out_boxes), src, counts);
    return check_launch("locov_detector_rescale");
}

}  // extern "C"
