// The ResNet stem in one launch: conv 7x7 / stride 2 / pad 3 (3 -> 64), FrozenBN, ReLU, max-pool 3x3 / stride 2 / pad 1.
//
// [D2-upstream] detectron2.modeling.backbone.resnet.BasicStem (the reference tree has no source for it).  x is the NCHW image
// batch, y the pooled map in channels-last rows [N, PH, PW, 64] -- what Res5Stage.forward_rows takes.  The conv intermediate
// ([N, 64, CH, CW], 68 MB per 1333 x 800 image) is never written: it lives in registers.
//
// One wave owns a band of pooled outputs, 8 columns wide and `band` rows tall, i.e. 17 conv columns (one of overlap with the
// neighbour) by 2 band + 1 conv rows (one of overlap).  It walks the conv rows top to bottom, eight at a time: the 21 x 39 x 3
// input rows those eight need are staged in LDS with zeros outside the image (global reads coalesced along W).  A lane is an output
// channel: its 147 filter taps stay in VGPRs for the whole band (staged through LDS once per workgroup so that the global read
// of w is coalesced), the patch is read as wave-uniform 16-byte LDS broadcasts, and a conv row is 17 accumulators x 147 v_fmac_f32
// (exact fp32 products, fp32 accumulation, taps in (c, u, v) order).  A conv row is reduced to its 8 horizontal window maxima at
// once and the vertical maximum runs over the rows as they are produced, so a pooled row leaves after every second conv row:
// transposed through a 2 KB LDS slab so that the global store is one 16-byte vector of 4 channels per lane (1 KB contiguous per
// instruction).  237 VGPRs, no scratch, two workgroups per CU.
//
// The kernel is bound by the v_fmac_f32 issue rate, so the host chooses the band height that spreads the conv rows evenly over
// the wave slots (stem_band): 5 pooled rows for one 800 x 1333 image (1680 waves on 2048 slots), 34 for eight (2016 waves).
//
// Conv rows / columns outside [0, CH) x [0, CW) do not exist (they are NOT convolutions of zero padding): they enter the maximum
// as 0, which every existing post-ReLU value dominates, and each pooled window holds at least its centre (2p, 2q).
// Every output element is produced by one lane in one fixed order from its own image only, whatever the band height: the result
// of an image does not depend on N or on the other images of the launch.  No atomics, vector stores only.
#include "common.h"

#include <climits>
#include <cstdlib>

namespace locov {
namespace {

constexpr int kCout = 64, kTaps = 3 * 7 * 7;
constexpr int kTW = 8;                                 // pooled columns of one wave
constexpr int kCC = 2 * kTW + 1;                       // its conv columns: 17
constexpr int kGroup = 8;                              // conv rows per staged patch
constexpr int kPR = 2 * (kGroup - 1) + 7, kPC = 4 * kTW + 7;    // the patch: 21 x 39 per channel
constexpr int kPitch = 40;                             // patch row pitch (16-byte rows)
constexpr int kPlane = kPR * kPitch, kPatch = 3 * kPlane;
constexpr int kWaves = 4;
constexpr int kSlab = kTW * kCout;                     // one pooled row of a band
static_assert(kWaves * kPatch >= kCout * kTaps, "the weights are staged in the patch area");
static_assert(kPitch >= kPC && kPitch % 4 == 0 && 2 * (kCC - 1) + 6 < kPitch, "patch row");

__global__ __launch_bounds__(kWaves * kWave, 2) void resnet_stem_kernel(const float *__restrict__ x, int H, int W,
                                                                        const float *__restrict__ w, const float *__restrict__ scale,
                                                                        const float *__restrict__ shift, float *__restrict__ y, int CH,
                                                                        int CW, int PH, int PW, int band, int bands, int tilesQ,
                                                                        int64_t tiles)
{
    __shared__ __attribute__((aligned(16))) float lds[kWaves * kPatch + kWaves * kSlab];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;

    // the filter: global -> LDS in 16-byte chunks, then channel `lane`'s 147 taps into registers (stride 147 words: no bank conflict)
    for (int i = threadIdx.x; i < kCout * kTaps / 4; i += kWaves * kWave)
        reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(w)[i];
    __syncthreads();
    float wr[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) wr[t] = lds[lane * kTaps + t];
    const float sc = scale[lane], sh = shift[lane];

    // a wave past the last band repeats the last band without storing (every wave meets every barrier)
    int64_t tile = (int64_t)blockIdx.x * kWaves + wave;
    const bool live = tile < tiles;
    if (!live) tile = tiles - 1;
    const int tq = (int)(tile % tilesQ);
    const int64_t rest = tile / tilesQ;
    const int tb = (int)(rest % bands);
    const int64_t n = rest / bands;
    const int p0 = tb * band, q0 = tq * kTW;
    const int r0 = 4 * p0 - 5, c0 = 4 * q0 - 5;           // image position of conv row 2 p0 - 1's first tap: 2 (2 p0 - 1) - 3

    float *patch = lds + wave * kPatch;
    float *slab = lds + kWaves * kPatch + wave * kSlab;
    const float *xn = x + n * 3 * (int64_t)H * W;

    float cur[kTW];
#pragma unroll
    for (int q = 0; q < kTW; ++q) cur[q] = 0.0f;

    const int nrows = 2 * band + 1;                       // conv rows 2 p0 - 1 + i, i < nrows (the same for every wave: barriers)
#pragma unroll 1
    for (int g0 = 0; g0 < nrows; g0 += kGroup) {
        __syncthreads();                                  // (the filter / the previous patch has been read)
        for (int e = lane; e < kPatch; e += kWave) {
            const int c = e / kPlane, rem = e - c * kPlane;
            const int r = rem / kPitch, col = rem - r * kPitch;
            const int gr = r0 + 2 * g0 + r, gc = c0 + col;
            float v = 0.0f;
            if (col < kPC && gr >= 0 && gr < H && gc >= 0 && gc < W) v = xn[((int64_t)c * H + gr) * W + gc];
            patch[e] = v;
        }
        __syncthreads();
        const int gend = min(kGroup, nrows - g0);
#pragma unroll 1
        for (int ii = 0; ii < gend; ++ii) {
            const int i = g0 + ii;
            const int ci = 2 * p0 - 1 + i;                // conv row of this pass (wave-uniform)
            float h[kTW];
#pragma unroll
            for (int q = 0; q < kTW; ++q) h[q] = 0.0f;
            if (ci >= 0 && ci < CH) {
                float acc[kCC];
#pragma unroll
                for (int p = 0; p < kCC; ++p) acc[p] = 0.0f;
#pragma unroll
                for (int cu = 0; cu < 21; ++cu) {         // filter row (c, u) = (cu / 7, cu % 7)
                    const float4 *row = reinterpret_cast<const float4 *>(patch + (cu / 7) * kPlane + (2 * ii + cu % 7) * kPitch);
                    float xr[kPitch];
#pragma unroll
                    for (int j = 0; j < kPitch / 4; ++j) {
                        const float4 t = row[j];
                        xr[4 * j] = t.x; xr[4 * j + 1] = t.y; xr[4 * j + 2] = t.z; xr[4 * j + 3] = t.w;
                    }
#pragma unroll
                    for (int v = 0; v < 7; ++v) {
#pragma unroll
                        for (int p = 0; p < kCC; ++p) acc[p] = fmaf(xr[2 * p + v], wr[cu * 7 + v], acc[p]);
                    }
                }
                float a[kCC];
#pragma unroll
                for (int p = 0; p < kCC; ++p) {
                    const int cj = 2 * q0 - 1 + p;
                    a[p] = (cj >= 0 && cj < CW) ? fmaxf(fmaf(acc[p], sc, sh), 0.0f) : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < kTW; ++q) h[q] = fmaxf(fmaxf(a[2 * q], a[2 * q + 1]), a[2 * q + 2]);
            }
#pragma unroll
            for (int q = 0; q < kTW; ++q) cur[q] = fmaxf(cur[q], h[q]);
            if (i >= 2 && (i & 1) == 0) {                 // conv row 2 p + 1 closes pooled row p = p0 + i / 2 - 1 ...
                __syncthreads();                          // (the slab's previous readers are done)
#pragma unroll
                for (int q = 0; q < kTW; ++q) slab[q * kCout + lane] = cur[q];
                __syncthreads();
                const int p = p0 + i / 2 - 1;
#pragma unroll
                for (int it = 0; it < kTW / 4; ++it) {
                    const int pix = it * 4 + (lane >> 4), c4 = (lane & 15) * 4;
                    const float4 v = *reinterpret_cast<const float4 *>(slab + pix * kCout + c4);
                    const int q = q0 + pix;
                    if (live && p < PH && q < PW)
                        *reinterpret_cast<float4 *>(y + ((n * PH + p) * PW + q) * kCout + c4) = v;
                }
#pragma unroll
                for (int q = 0; q < kTW; ++q) cur[q] = h[q];  // ... and opens the next one
            }
        }
    }
}

// Wave slots of the current device at this kernel's occupancy (2 waves per SIMD, 8 per CU), asked once per device
int wave_slots()
{
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 2048;
    if (cached[dev] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cached[dev] = 8 * cus;
    }
    return cached[dev];
}

// The band height: `cols` band columns (images x 8-wide column strips) of PH pooled rows each on `slots` wave slots.  The kernel
// is FMA-bound once a SIMD holds two waves (one alone waits for its LDS reads: 7.4 us per conv row against 8.9 us for two
// together at 1333 x 800), so a launch takes rounds x (2 band + 1) conv rows with rounds = ceil(waves / slots).  Tried: the
// heights that fill 1 .. 8 x slots waves; the cheapest wins (ties: the fewer waves).  Measured at 800 x 1333: one image 125 us
// at the chosen 5 rows (174 at 4, 166 at 9, 217 at 13), eight images 614 us at the chosen 34 (773 at 4, 646 at 17, 1000 at 67).
int stem_band(int64_t cols, int PH, int slots)
{
    int best = PH;
    int64_t best_cost = INT64_MAX;
    for (int k = 1; k <= 8; ++k) {
        int64_t bands = (int64_t)k * slots / cols;
        if (bands < 1) bands = 1;
        if (bands > PH) bands = PH;
        const int band = (int)ceil_div(PH, bands);
        const int64_t waves = cols * ceil_div(PH, band);
        const int64_t cost = ceil_div(waves, slots) * (2 * band + 1);
        if (cost < best_cost) best_cost = cost, best = band;
    }
    return best;
}

}  // namespace
}  // namespace locov

extern "C" int locov_resnet_stem_fwd(const float *x, int N, int H, int W, const float *w, const float *scale, const float *shift, int Cout,
                                     float *y, locov_stream_t stream)
{
    using namespace locov;
    LOCOV_REQUIRE(Cout == kCout, "locov_resnet_stem_fwd: Cout = %d is not supported (the stem kernel is built for 64 channels)", Cout);
    LOCOV_REQUIRE(N >= 0 && H > 0 && W > 0, "locov_resnet_stem_fwd: bad shape N = %d, H = %d, W = %d", N, H, W);
    if (N == 0) return LOCOV_OK;
    LOCOV_REQUIRE(x && w && scale && shift && y, "locov_resnet_stem_fwd: null pointer");
    LOCOV_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)scale % 4 == 0 && (uintptr_t)shift % 4 == 0 && (uintptr_t)w % 16 == 0 &&
                      (uintptr_t)y % 16 == 0,
                  "locov_resnet_stem_fwd: misaligned pointer (w and y: 16 bytes)");
    const int CH = (H + 1) / 2, CW = (W + 1) / 2, PH = (CH + 1) / 2, PW = (CW + 1) / 2;
    const int tilesQ = (PW + kTW - 1) / kTW;
    // N H W < 2^57 keeps every element offset of x (3 N H W) and of y (64 PH PW <= 64 H W per image) inside int64
    LOCOV_REQUIRE((int64_t)N * H <= (INT64_MAX / 64) / W, "locov_resnet_stem_fwd: index overflow (N H W too large)");
    const int64_t cols = (int64_t)N * tilesQ;
    int band = stem_band(cols, PH, wave_slots());
    if (const char *forced = getenv("LOCOV_STEM_BAND")) {    // developer A/B and the tests: every band height gives the same bits
        const int b = atoi(forced);
        if (b > 0) band = b < PH ? b : PH;
    }
    const int bands = (int)ceil_div(PH, band);
    const int64_t tiles = cols * bands;
    const int64_t blocks = ceil_div(tiles, kWaves);
    LOCOV_REQUIRE(blocks <= INT_MAX, "locov_resnet_stem_fwd: index overflow (%lld workgroups)", (long long)blocks);
    hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)blocks), dim3(kWaves * kWave), 0, as_stream(stream), x, H, W, w, scale, shift, y, CH,
                       CW, PH, PW, band, bands, tilesQ, tiles);
    return check_launch("locov_resnet_stem_fwd");
}
