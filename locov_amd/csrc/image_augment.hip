// The strong augmentation of the dataset mapper for the whole batch (strong_augment.py: apply_host is the definition):
//   locov_augment_images : torchvision's ColorJitter (any order of brightness / contrast / saturation / hue), RandomGrayscale,
//                          Pillow's GaussianBlur and up to three RandomErasing on N planar uint8 [3, h, w] images of different
//                          sizes, with the bytes Pillow's C and the two torch expressions give.
// Compiled with -ffp-contract=off: Image.blend is d + f * (x - d) in fp32 with the product rounded before the sum, the HSV
// conversions mix fp32 and fp64 step by step, and every division is the correctly rounded one.
// Two launches, one when no image's chain has contrast:
//   1. contrast_sum_kernel: ImageEnhance.Contrast blends towards the mean of L over the WHOLE image as it stands when contrast
//      runs.  A workgroup redoes the operations before contrast on kChunk pixels and writes their integer sum of L to the workspace.
//   2. augment_kernel: a workgroup owns a kTH x kTW output tile.  It sums its image's partials (integers: any order gives the same
//      sum), loads the tile with a halo of three pass-reaches per side (clipped to the image), runs the jitter chain and the
//      grayscale per pixel in registers, the three horizontal and three vertical box passes between two LDS buffers (a pixel's
//      three bytes in one 32-bit word), and substitutes the erasers' bytes at the store.
// The per-image table is built on the host, copied to the head of the workspace and read from there: 64 images' draws do not fit a
// kernel's argument block.  No atomics, vector stores only, nothing read by the host.
#include "common.h"

#include <cmath>
#include <vector>

namespace locov {
namespace {

constexpr int kTH = 32, kTW = 64;
constexpr int kMaxReach = 2;                                      // one box pass reads (int)fr + 1 to each side: 2 up to sigma 2.44
constexpr int kMaxHalo = 3 * kMaxReach;
constexpr int kRegion = (kTH + 2 * kMaxHalo) * (kTW + 2 * kMaxHalo);   // 44 x 76 words: 13 KiB per buffer
constexpr int kThreads = 256;
constexpr int kChunk = 4096;                                      // pixels per partial sum: 4096 * 255 fits 32 bits
constexpr int kPasses = 3;

struct ImageDesc {                                                // what the kernels read per image; the host derives it from the draws
    const uint8_t *src;
    uint8_t *dst;
    int64_t noise_at[LOCOV_AUG_MAX_ERASERS];                      // first fp32 of eraser e's [3, eh, ew] block
    int h, w;
    int n_ops, ops[4];
    float factor[3];                                              // brightness, contrast, saturation
    int hue_shift, gray;
    int reach, radius;                                            // reach 0: no blur
    uint32_t ww, fw;
    int n_erase, erase[LOCOV_AUG_MAX_ERASERS][4];                 // (i, j, eh, ew)
    int boff, poff, n_part;                                       // first workgroup of launch 2; first partial and their number (0: no contrast)
};

static_assert(sizeof(ImageDesc) == 168, "the per-image table entry: 64 of them are 10.5 KiB, past a kernel's argument block");

// _gaussian_blur_radius(sigma, 3), Pillow's mix of fp32 and fp64 (host only).
float box_radius(float sigma)
{
    const float s2 = sigma * sigma / (float)kPasses;
    const float L = (float)sqrt(12.0 * (double)s2 + 1.0);
    const float l = (float)floor(((double)L - 1.0) / 2.0);
    float a = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * s2);
    a /= 6.0f * (s2 - (l + 1.0f) * (l + 1.0f));
    return l + a;
}

bool sigma_supported(float sigma)
{
    if (!(sigma > 0.0f) || !(sigma <= 16.0f)) return false;
    return (int)box_radius(sigma) + 1 <= kMaxReach;
}

__device__ __forceinline__ int luma(int r, int g, int b)
{
    return (int)(((uint32_t)r * 19595u + (uint32_t)g * 38470u + (uint32_t)b * 7471u + 0x8000u) >> 16);
}

// Image.blend(degenerate, image, f) of one byte
__device__ __forceinline__ int blend(int d, int x, float f)
{
    const float t = (float)d + f * (float)(x - d);
    if (f >= 0.0f && f <= 1.0f) return (int)t;
    return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t;
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// convert("HSV"), the shift of H, convert("RGB")
__device__ void hue(int &r, int &g, int &b, int shift)
{
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = (float)((double)bc - (double)gc);
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double x = (double)h / 6.0 + 1.0;                   // in [5/6, 11/6]: fmod(x, 1) = x - floor(x), exactly
        h = (float)(x - floor(x));
        uh = clip8((int)((double)h * 255.0));
        us = clip8((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = maxc;
        return;
    }
    const double v = (double)maxc, fs = (double)us / 255.0;
    const double hh = (double)uh * 6.0 / 255.0;
    const double i = floor(hh), f = hh - i;
    const int p = clip8((int)floor(v * (1.0 - fs) + 0.5));
    const int q = clip8((int)floor(v * (1.0 - fs * f) + 0.5));
    const int t = clip8((int)floor(v * (1.0 - fs * (1.0 - f)) + 0.5));
    switch ((int)i % 6) {
        case 0: r = maxc; g = t; b = p; break;
        case 1: r = q; g = maxc; b = p; break;
        case 2: r = p; g = maxc; b = t; break;
        case 3: r = p; g = q; b = maxc; break;
        case 4: r = t; g = p; b = maxc; break;
        default: r = maxc; g = p; b = q; break;
    }
}

// Operations [first, last) of the image's chain on one pixel; `mean` is contrast's grey level.
__device__ void jitter(const ImageDesc &d, int first, int last, int mean, int &r, int &g, int &b)
{
    for (int k = first; k < last; k++) {
        const int op = d.ops[k];
        if (op == LOCOV_AUG_OP_BRIGHTNESS) {
            const float f = d.factor[0];
            r = blend(0, r, f); g = blend(0, g, f); b = blend(0, b, f);
        } else if (op == LOCOV_AUG_OP_CONTRAST) {
            const float f = d.factor[1];
            r = blend(mean, r, f); g = blend(mean, g, f); b = blend(mean, b, f);
        } else if (op == LOCOV_AUG_OP_SATURATION) {
            const float f = d.factor[2];
            const int l = luma(r, g, b);
            r = blend(l, r, f); g = blend(l, g, f); b = blend(l, b, f);
        } else {
            hue(r, g, b, d.hue_shift);
        }
    }
}

__device__ __forceinline__ int contrast_at(const ImageDesc &d)
{
    for (int k = 0; k < d.n_ops; k++)
        if (d.ops[k] == LOCOV_AUG_OP_CONTRAST) return k;
    return -1;
}

// The sum of `v` over the workgroup, in every thread.  `red` holds kThreads words.
__device__ uint64_t block_sum(uint64_t v, uint64_t *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kThreads) void contrast_sum_kernel(const ImageDesc *__restrict__ table, int n_img, uint32_t *partials)
{
    __shared__ uint64_t red[kThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    int img = -1;
    for (int i = 0; i < n_img; i++)
        if (table[i].n_part > 0 && b >= table[i].poff && b < table[i].poff + table[i].n_part) img = i;
    if (img < 0) return;                                          // (never: the grid is the partials' count)
    const ImageDesc &d = table[img];                              // uniform reads from the workspace, not a per-lane copy
    const int64_t n = (int64_t)d.h * d.w;
    const int upto = contrast_at(d);
    const int64_t p0 = (int64_t)(b - d.poff) * kChunk;
    uint64_t sum = 0;
    for (int k = tid; k < kChunk; k += kThreads) {
        const int64_t p = p0 + k;
        if (p >= n) break;
        int r = d.src[p], g = d.src[n + p], bl = d.src[2 * n + p];
        jitter(d, 0, upto, 0, r, g, bl);
        sum += (uint64_t)luma(r, g, bl);
    }
    sum = block_sum(sum, red);
    if (tid == 0) partials[b] = (uint32_t)sum;
}

__device__ __forceinline__ uint32_t box_pass(const uint32_t *in, int base, int stride, int pos, int lo, int hi, int radius, uint32_t ww,
                                             uint32_t fw)
{
    // pos: the index along the line within the region, [lo, hi] the region's ends of that line; the region never ends inside the
    // image short of what a byte that is kept needs, so clamping to it is clamping to the image wherever it matters
    uint32_t acc[3] = {0, 0, 0};
    for (int k = -radius; k <= radius; k++) {
        const int q = min(max(pos + k, lo), hi);
        const uint32_t word = in[base + q * stride];
        acc[0] += word & 255u; acc[1] += (word >> 8) & 255u; acc[2] += (word >> 16) & 255u;
    }
    const uint32_t a = in[base + min(max(pos - radius - 1, lo), hi) * stride], z = in[base + min(max(pos + radius + 1, lo), hi) * stride];
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t far = ((a >> (8 * c)) & 255u) + ((z >> (8 * c)) & 255u);
        out |= ((acc[c] * ww + far * fw + (1u << 23)) >> 24) << (8 * c);
    }
    return out;
}

__global__ __launch_bounds__(kThreads) void augment_kernel(const ImageDesc *__restrict__ table, int n_img, const uint32_t *partials, const float *noise)
{
    __shared__ uint32_t buf[2][kRegion];
    __shared__ uint64_t red[kThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    int img = 0;
    while (img + 1 < n_img && b >= table[img + 1].boff) img++;
    const ImageDesc &d = table[img];                              // uniform reads from the workspace, not a per-lane copy
    const int h = d.h, w = d.w;
    const int64_t n = (int64_t)h * w;

    int mean = 0;
    if (d.n_part > 0) {                                           // int(sum / count + 0.5), ImageStat's double division
        uint64_t sum = 0;
        for (int k = tid; k < d.n_part; k += kThreads) sum += partials[d.poff + k];
        sum = block_sum(sum, red);
        mean = (int)((double)sum / (double)n + 0.5);
    }

    const int tiles_x = (w + kTW - 1) / kTW;
    const int local = b - d.boff;
    const int by = local / tiles_x, bx = local - by * tiles_x;
    const int x0 = bx * kTW, y0 = by * kTH;
    const int halo = kPasses * d.reach;
    const int rx0 = max(x0 - halo, 0), rx1 = min(x0 + kTW + halo, w);       // the region: the tile and its halo, inside the image
    const int ry0 = max(y0 - halo, 0), ry1 = min(y0 + kTH + halo, h);
    const int rw = rx1 - rx0, rh = ry1 - ry0;                               // <= kTW + 2 kMaxHalo, kTH + 2 kMaxHalo

    for (int it = tid; it < rw * rh; it += kThreads) {
        const int yy = it / rw, xx = it - yy * rw;
        const int64_t p = (int64_t)(ry0 + yy) * w + (rx0 + xx);
        int r = d.src[p], g = d.src[n + p], bl = d.src[2 * n + p];
        jitter(d, 0, d.n_ops, mean, r, g, bl);
        if (d.gray) r = g = bl = luma(r, g, bl);
        buf[0][it] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)bl << 16);
    }
    __syncthreads();

    int cur = 0;
    if (d.reach > 0) {
        for (int pass = 0; pass < 2 * kPasses; pass++) {
            const bool horizontal = pass < kPasses;
            for (int it = tid; it < rw * rh; it += kThreads) {
                const int yy = it / rw, xx = it - yy * rw;
                buf[cur ^ 1][it] = horizontal ? box_pass(buf[cur], yy * rw, 1, xx, 0, rw - 1, d.radius, d.ww, d.fw)
                                              : box_pass(buf[cur], xx, rw, yy, 0, rh - 1, d.radius, d.ww, d.fw);
            }
            __syncthreads();
            cur ^= 1;
        }
    }

    const int tw = min(kTW, w - x0), th = min(kTH, h - y0);
    for (int it = tid; it < kTW * th; it += kThreads) {
        const int ty = it / kTW, tx = it - ty * kTW;
        if (tx >= tw) continue;
        const int x = x0 + tx, y = y0 + ty;
        const uint32_t word = buf[cur][(y - ry0) * rw + (x - rx0)];
        int v[3] = {(int)(word & 255u), (int)((word >> 8) & 255u), (int)((word >> 16) & 255u)};
        for (int e = 0; e < d.n_erase; e++) {                     // a later eraser wins
            const int i = d.erase[e][0], j = d.erase[e][1], eh = d.erase[e][2], ew = d.erase[e][3];
            if (y >= i && y < i + eh && x >= j && x < j + ew) {
                const float *blk = noise + d.noise_at[e] + (int64_t)(y - i) * ew + (x - j);
#pragma unroll
                for (int c = 0; c < 3; c++) v[c] = (int)(blk[(int64_t)c * eh * ew] * 255.0f) & 255;
            }
        }
        const int64_t p = (int64_t)y * w + x;
        d.dst[p] = (uint8_t)v[0];
        d.dst[n + p] = (uint8_t)v[1];
        d.dst[2 * n + p] = (uint8_t)v[2];
    }
}

constexpr int64_t kTableAlign = 256;

int64_t table_bytes(int n_images) { return ceil_div((int64_t)n_images * (int64_t)sizeof(ImageDesc), kTableAlign) * kTableAlign; }

bool has_contrast(const locov_augment_desc &d)
{
    for (int k = 0; k < d.n_ops && k < 4; k++)
        if (d.ops[k] == LOCOV_AUG_OP_CONTRAST) return true;
    return false;
}

int64_t partials_of(const locov_augment_desc &d)
{
    return has_contrast(d) && d.height >= 1 && d.width >= 1 ? ceil_div((int64_t)d.height * d.width, kChunk) : 0;
}

}  // namespace
}  // namespace locov

using namespace locov;

extern "C" {

int locov_augment_supported(float sigma) { return sigma_supported(sigma) ? 1 : 0; }

int64_t locov_augment_images_workspace_bytes(const locov_augment_desc *descs_host, int n_images)
{
    if (!descs_host || n_images <= 0 || n_images > LOCOV_LABEL_MAX_IMAGES) return 0;
    int64_t parts = 0;
    for (int i = 0; i < n_images; i++) parts += partials_of(descs_host[i]);
    return table_bytes(n_images) + parts * (int64_t)sizeof(uint32_t);
}

int locov_augment_images(const void *const *images_host, void *const *outs_host, const locov_augment_desc *descs_host, int n_images,
                         const float *noise, int64_t n_noise, void *workspace, int64_t workspace_bytes, locov_stream_t stream)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= LOCOV_LABEL_MAX_IMAGES, "locov_augment_images: 0..%d images per call", LOCOV_LABEL_MAX_IMAGES);
    if (n_images == 0) return LOCOV_OK;
    LOCOV_REQUIRE(images_host && outs_host && descs_host && workspace, "locov_augment_images: null pointer");
    LOCOV_REQUIRE(n_noise >= 0, "locov_augment_images: n_noise must not be negative");
    LOCOV_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)noise & 3) == 0, "locov_augment_images: misaligned workspace (16) or noise (4)");
    std::vector<ImageDesc> table((size_t)n_images);
    int64_t blocks = 0, parts = 0;
    for (int i = 0; i < n_images; i++) {
        const locov_augment_desc &s = descs_host[i];
        ImageDesc &d = table[(size_t)i];
        d = ImageDesc{};
        LOCOV_REQUIRE(images_host[i] && outs_host[i], "locov_augment_images: null pointer (image %d)", i);
        LOCOV_REQUIRE(images_host[i] != outs_host[i], "locov_augment_images: image %d: the output must not be the input", i);
        LOCOV_REQUIRE(s.height >= 1 && s.width >= 1, "locov_augment_images: image %d: sizes must be positive, got %d x %d", i, s.height, s.width);
        LOCOV_REQUIRE((int64_t)s.height * s.width * 3 <= INT32_MAX, "locov_augment_images: image %d: %d x %d x 3 leaves int32", i, s.height, s.width);
        LOCOV_REQUIRE(s.n_ops >= 0 && s.n_ops <= 4, "locov_augment_images: image %d: 0..4 jitter operations, got %d", i, s.n_ops);
        unsigned seen = 0;
        for (int k = 0; k < s.n_ops; k++) {
            const int op = s.ops[k];
            LOCOV_REQUIRE(op >= LOCOV_AUG_OP_BRIGHTNESS && op <= LOCOV_AUG_OP_HUE, "locov_augment_images: image %d: unknown operation %d", i, op);
            LOCOV_REQUIRE(!(seen & (1u << op)), "locov_augment_images: image %d: repeated operation %d", i, op);
            seen |= 1u << op;
            d.ops[k] = op;
        }
        LOCOV_REQUIRE(std::isfinite(s.brightness) && std::isfinite(s.contrast) && std::isfinite(s.saturation),
                      "locov_augment_images: image %d: a factor is not finite", i);
        LOCOV_REQUIRE(s.hue_shift >= 0 && s.hue_shift <= 255, "locov_augment_images: image %d: hue_shift must be 0..255, got %d", i, s.hue_shift);
        LOCOV_REQUIRE(s.sigma == 0.0f || sigma_supported(s.sigma), "locov_augment_images: image %d: sigma %g is outside the supported range", i,
                      (double)s.sigma);
        LOCOV_REQUIRE(s.n_erase >= 0 && s.n_erase <= LOCOV_AUG_MAX_ERASERS, "locov_augment_images: image %d: 0..%d erasers, got %d", i,
                      LOCOV_AUG_MAX_ERASERS, s.n_erase);
        int64_t at = s.noise_offset;
        LOCOV_REQUIRE(at >= 0, "locov_augment_images: image %d: negative noise offset", i);
        for (int e = 0; e < s.n_erase; e++) {
            const int ei = s.erase[e][0], ej = s.erase[e][1], eh = s.erase[e][2], ew = s.erase[e][3];
            LOCOV_REQUIRE(ei >= 0 && ej >= 0 && eh >= 0 && ew >= 0 && (int64_t)ei + eh <= s.height && (int64_t)ej + ew <= s.width,
                          "locov_augment_images: image %d: eraser %d (%d, %d, %d, %d) leaves the image", i, e, ei, ej, eh, ew);
            const int64_t count = (int64_t)3 * eh * ew;
            LOCOV_REQUIRE(at + count <= n_noise, "locov_augment_images: image %d: eraser %d reads noise [%lld, %lld) past the tensor's %lld", i, e,
                          (long long)at, (long long)(at + count), (long long)n_noise);
            LOCOV_REQUIRE(count == 0 || noise, "locov_augment_images: null noise");
            d.noise_at[e] = at;
            for (int k = 0; k < 4; k++) d.erase[e][k] = s.erase[e][k];
            at += count;
        }
        d.src = static_cast<const uint8_t *>(images_host[i]);
        d.dst = static_cast<uint8_t *>(outs_host[i]);
        d.h = s.height;
        d.w = s.width;
        d.n_ops = s.n_ops;
        d.factor[0] = s.brightness;
        d.factor[1] = s.contrast;
        d.factor[2] = s.saturation;
        d.hue_shift = s.hue_shift;
        d.gray = s.gray ? 1 : 0;
        d.n_erase = s.n_erase;
        if (s.sigma != 0.0f) {                                    // one box pass, as ImagingLineBoxBlur forms its weights
            const float fr = box_radius(s.sigma);
            d.radius = (int)fr;
            d.reach = d.radius + 1;
            d.ww = (uint32_t)((float)(1u << 24) / (fr * 2.0f + 1.0f));
            d.fw = ((1u << 24) - (uint32_t)(2 * d.radius + 1) * d.ww) / 2;
        }
        d.boff = (int)blocks;
        d.poff = (int)parts;
        d.n_part = (int)partials_of(s);
        blocks += ceil_div(s.height, kTH) * ceil_div(s.width, kTW);
        parts += d.n_part;
        LOCOV_REQUIRE(blocks <= INT32_MAX && parts <= INT32_MAX, "locov_augment_images: the batch leaves the launch grid at image %d", i);
    }
    const int64_t need = table_bytes(n_images) + parts * (int64_t)sizeof(uint32_t);
    LOCOV_REQUIRE(workspace_bytes >= need, "locov_augment_images: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);

    ImageDesc *dev_table = static_cast<ImageDesc *>(workspace);
    uint32_t *partials = reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + table_bytes(n_images));
    // pageable memory: the copy is staged before the call returns, so `table` may go; the runtime may wait for the stream first
    if (hipMemcpyAsync(dev_table, table.data(), (size_t)n_images * sizeof(ImageDesc), hipMemcpyHostToDevice, as_stream(stream)) != hipSuccess)
        return set_error(LOCOV_ERR_LAUNCH, "locov_augment_images: the table's copy to the workspace failed");
    if (parts > 0) {
        hipLaunchKernelGGL(contrast_sum_kernel, dim3((unsigned)parts), dim3(kThreads), 0, as_stream(stream), dev_table, n_images, partials);
        const int rc = check_launch("locov_augment_images (contrast)");
        if (rc != LOCOV_OK) return rc;
    }
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, as_stream(stream), dev_table, n_images, partials, noise);
    return check_launch("locov_augment_images");
}

}  // extern "C"
