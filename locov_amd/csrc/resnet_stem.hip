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
//
// Training.  The stem's only trainable tensor is conv1.weight (FrozenBN is buffers, images carry no gradient).  The training
// forward (kSel) is the same kernel and additionally writes `sel`, one byte per pooled element: 3 di + dj of the conv position
// (2p - 1 + di, 2q - 1 + dj) that first attains the window maximum in row-major scan (torch's max-pool rule) when that maximum
// is > 0, 9 when the pooled value is 0 (nothing passes the ReLU).  The weight gradient (resnet_stem_wgrad_kernel) routes g through
// sel back to the conv positions and accumulates dw[o, c, u, v] = scale[o] sum gconv[n, i, j, o] x[n, c, 2i - 3 + u, 2j - 3 + v] in
// the forward's layout: a lane is an output channel, the 147 accumulators stay in registers (the taps are not needed: which is
// why the forward saves sel instead of the backward recomputing the maximum next to 147 taps), the patch is read as wave-uniform
// LDS broadcasts.  Per-wave partials are reduced in fixed order: in the workgroup through LDS, across workgroups through the
// workspace and a second small launch.  No atomics: two launches give the same bits.
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

// One wave's patch: image rows [gr0, gr0 + 21) x columns [gc0, gc0 + 39) of the three channels, zeros outside the image
__device__ __forceinline__ void stage_patch(float *patch, const float *__restrict__ xn, int H, int W, int gr0, int gc0, int lane)
{
    for (int e = lane; e < kPatch; e += kWave) {
        const int c = e / kPlane, rem = e - c * kPlane;
        const int r = rem / kPitch, col = rem - r * kPitch;
        const int gr = gr0 + r, gc = gc0 + col;
        float v = 0.0f;
        if (col < kPC && gr >= 0 && gr < H && gc >= 0 && gc < W) v = xn[((int64_t)c * H + gr) * W + gc];
        patch[e] = v;
    }
}

constexpr int kNoSel = 9;                              // sel of a pooled zero: no conv position receives its gradient

template <bool kSel>
__global__ __launch_bounds__(kWaves * kWave, 2) void resnet_stem_kernel(const float *__restrict__ x, int H, int W,
                                                                        const float *__restrict__ w, const float *__restrict__ scale,
                                                                        const float *__restrict__ shift, float *__restrict__ y,
                                                                        uint8_t *__restrict__ sel, int CH, int CW, int PH, int PW,
                                                                        int band, int bands, int tilesQ, int64_t tiles)
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
    [[maybe_unused]] int code[kTW], hj[kTW];              // kSel: where cur / h come from (3 di + dj of the open window / dj)
#pragma unroll
    for (int q = 0; q < kTW; ++q) code[q] = hj[q] = 0;

    const int nrows = 2 * band + 1;                       // conv rows 2 p0 - 1 + i, i < nrows (the same for every wave: barriers)
#pragma unroll 1
    for (int g0 = 0; g0 < nrows; g0 += kGroup) {
        __syncthreads();                                  // (the filter / the previous patch has been read)
        stage_patch(patch, xn, H, W, r0 + 2 * g0, c0, lane);
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
                if constexpr (kSel) {                     // the first column that holds the row's maximum (a missing column is 0: it matters only where h is 0)
#pragma unroll
                    for (int q = 0; q < kTW; ++q) hj[q] = a[2 * q] == h[q] ? 0 : (a[2 * q + 1] == h[q] ? 1 : 2);
                }
            }
            if constexpr (kSel) {                         // a later row takes the window over only when strictly larger
                const int di = i == 0 ? 0 : 2 - (i & 1);
#pragma unroll
                for (int q = 0; q < kTW; ++q)
                    if (h[q] > cur[q]) code[q] = 3 * di + hj[q];
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
                if constexpr (kSel) {
                    if (live && p < PH) {
#pragma unroll
                        for (int q = 0; q < kTW; ++q)
                            if (q0 + q < PW) sel[((n * PH + p) * PW + q0 + q) * kCout + lane] = (uint8_t)(cur[q] > 0.0f ? code[q] : kNoSel);
                    }
#pragma unroll
                    for (int q = 0; q < kTW; ++q) code[q] = hj[q];
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

// ---- the weight gradient ---------------------------------------------------------------------------------------------------
// One wave owns `band` conv rows of a strip of kGC = 16 conv columns (no overlap: a conv position belongs to one wave) and walks
// them top to bottom, eight at a time, over the forward's patch.  The gradient of a conv position is gathered from the pooled
// windows that can have selected it -- an even row / column lies in one window (di / dj = 1), an odd one in two (2 of the window
// before it, 0 of the one behind) -- so a conv row reads 9 pooled columns of one or two pooled rows, 64 channels wide (coalesced).
// The workgroups are persistent (at most kWgradBlocks, tiles dealt round-robin): the workspace holds one [147][64] partial per
// workgroup whatever N is.  256 VGPRs and 36 bytes of scratch per lane (two accumulator pairs and a few loop invariants: four
// scratch accesses per 2 352 FMAs), two workgroups per CU; measured at four 800 x 1333 images: 0.50 ms against the forward's 0.37.
constexpr int kGC = 16;                               // conv columns of one wave
constexpr int kGQ = kGC / 2 + 1;                       // the pooled columns they can belong to: 9
constexpr int kWgradBlocks = 512;
static_assert(2 * (kGC - 1) + 7 <= kPC, "the forward's patch covers the strip");
static_assert(kWaves * kPatch >= kTaps * kCout, "a wave's partial is reduced through the patch area");

__global__ __launch_bounds__(kWaves * kWave, 2) void resnet_stem_wgrad_kernel(const float *__restrict__ x, int H, int W,
                                                                              const float *__restrict__ g,
                                                                              const uint8_t *__restrict__ sel,
                                                                              float *__restrict__ part, int CH, int CW, int PH, int PW,
                                                                              int band, int bands, int tilesC, int64_t tiles, int rounds)
{
    __shared__ __attribute__((aligned(16))) float lds[kWaves * kPatch];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    float *patch = lds + wave * kPatch;

    float acc[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) acc[t] = 0.0f;

#pragma unroll 1
    for (int round = 0; round < rounds; ++round) {        // (the same count for every wave of the launch: barriers)
        int64_t tile = ((int64_t)round * gridDim.x + blockIdx.x) * kWaves + wave;
        const bool live = tile < tiles;
        if (!live) tile = tiles - 1;
        const int tc = (int)(tile % tilesC);
        const int64_t rest = tile / tilesC;
        const int tb = (int)(rest % bands);
        const int64_t n = rest / bands;
        const int i0 = tb * band, j0 = tc * kGC, qb = tc * (kGC / 2);
        const float *xn = x + n * 3 * (int64_t)H * W;
        const float *gn = g + n * (int64_t)PH * PW * kCout;
        const uint8_t *sn = sel + n * (int64_t)PH * PW * kCout;
#pragma unroll 1
        for (int g0 = 0; g0 < band; g0 += kGroup) {
            __syncthreads();                              // (the previous patch has been read)
            stage_patch(patch, xn, H, W, 2 * (i0 + g0) - 3, 2 * j0 - 3, lane);
            __syncthreads();
            const int gend = min(kGroup, band - g0);
#pragma unroll 1
            for (int ii = 0; ii < gend; ++ii) {
                const int ci = i0 + g0 + ii;              // conv row of this pass (wave-uniform)
                if (!live || ci >= CH) continue;
                float gc[kGC];
#pragma unroll
                for (int p = 0; p < kGC; ++p) gc[p] = 0.0f;
                // the pooled rows conv row ci belongs to: even -> (ci / 2, di 1); odd -> ((ci - 1) / 2, di 2) then ((ci + 1) / 2, di 0)
                const int nwin = (ci & 1) ? 2 : 1;
#pragma unroll 1
                for (int wi = 0; wi < nwin; ++wi) {
                    const int pw = (ci & 1) ? (ci - 1) / 2 + wi : ci / 2;
                    const int di = (ci & 1) ? 2 - 2 * wi : 1;
                    if (pw >= PH) continue;
                    const int64_t at = ((int64_t)pw * PW + qb) * kCout + lane;
                    const int nq = PW - qb;               // pooled columns that exist from qb on (wave-uniform)
#pragma unroll
                    for (int k = 0; k < kGQ; ++k) {
                        int dj = -1;                      // 0, 1, 2: the column 2q - 1 + dj of this conv row
                        float gv = 0.0f;
                        if (k < nq) dj = (int)sn[at + k * kCout] - 3 * di, gv = gn[at + k * kCout];
                        if (k > 0) gc[2 * k - 1] += dj == 0 ? gv : 0.0f;
                        if (k < kGQ - 1) {
                            gc[2 * k] += dj == 1 ? gv : 0.0f;
                            gc[2 * k + 1] += dj == 2 ? gv : 0.0f;
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);        // (patch reads hoisted over the gather would spill the accumulators)
#pragma unroll
                for (int cu = 0; cu < 21; ++cu) {         // filter row (c, u) = (cu / 7, cu % 7)
                    const float4 *prow = reinterpret_cast<const float4 *>(patch + (cu / 7) * kPlane + (2 * ii + cu % 7) * kPitch);
                    float xr[2 * (kGC - 1) + 7];          // 37 of the row's 40 words
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        const float4 t = prow[j];
                        xr[4 * j] = t.x; xr[4 * j + 1] = t.y; xr[4 * j + 2] = t.z; xr[4 * j + 3] = t.w;
                    }
                    xr[36] = reinterpret_cast<const float *>(prow)[36];
#pragma unroll
                    for (int v = 0; v < 7; ++v) {
#pragma unroll
                        for (int p = 0; p < kGC; ++p) acc[cu * 7 + v] = fmaf(gc[p], xr[2 * p + v], acc[cu * 7 + v]);
                    }
                    if (cu % 3 == 2) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }

    // the workgroup's partial: ((wave 0 + wave 1) + wave 2) + wave 3, through the patch area
#pragma unroll 1
    for (int src = 1; src < kWaves; ++src) {
        __syncthreads();
        if (wave == src) {
#pragma unroll
            for (int t = 0; t < kTaps; ++t) lds[t * kCout + lane] = acc[t];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int cu = 0; cu < 21; ++cu) {             // seven at a time: 147 loads in flight next to 147 accumulators would spill
#pragma unroll
                for (int v = 0; v < 7; ++v) acc[cu * 7 + v] += lds[(cu * 7 + v) * kCout + lane];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (wave == 0) {
        float *dst = part + (int64_t)blockIdx.x * kTaps * kCout;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) dst[t * kCout + lane] = acc[t];
    }
}

// dw[o, t] = scale[o] * (the workgroups' partials [b][t][o] summed in a fixed order)
__global__ __launch_bounds__(256) void resnet_stem_wgrad_reduce_kernel(const float *__restrict__ part, int blocks,
                                                                       const float *__restrict__ scale, float *__restrict__ dw)
{
    // 32 elements per workgroup, each summed by 8 threads (thread s: b = s, s + 8, ...) whose sums are added in the order s = 0 .. 7
    static_assert(kTaps * kCout % 32 == 0, "whole workgroups");
    __shared__ float slices[8][32];
    const int col = threadIdx.x & 31, slice = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + col;                   // t * 64 + o
    float s = 0.0f;
    for (int b = slice; b < blocks; b += 8) s += part[(int64_t)b * kTaps * kCout + e];
    slices[slice][col] = s;
    __syncthreads();
    if (slice != 0) return;
#pragma unroll
    for (int k = 1; k < 8; ++k) s += slices[k][col];
    const int t = e / kCout, o = e - t * kCout;
    dw[o * kTaps + t] = s * scale[o];
}

struct WgradPlan {
    int CH, CW, PH, PW, tilesC, band, bands, blocks, rounds;
    int64_t tiles;
};

// The split of the conv rows into bands: as stem_band, on the kWgradBlocks x kWaves wave slots of the persistent launch
bool wgrad_plan(int N, int H, int W, WgradPlan &p)
{
    p.CH = (H + 1) / 2, p.CW = (W + 1) / 2, p.PH = (p.CH + 1) / 2, p.PW = (p.CW + 1) / 2;
    p.tilesC = (p.CW + kGC - 1) / kGC;
    const int slots = kWgradBlocks * kWaves;
    const int64_t cols = (int64_t)N * p.tilesC;
    int best = p.CH;
    int64_t best_cost = INT64_MAX;
    for (int k = 1; k <= 8; ++k) {
        int64_t bands = (int64_t)k * slots / cols;
        if (bands < 1) bands = 1;
        if (bands > p.CH) bands = p.CH;
        const int band = (int)ceil_div(p.CH, bands);
        const int64_t waves = cols * ceil_div(p.CH, band);
        const int64_t cost = ceil_div(waves, slots) * band;
        if (cost < best_cost) best_cost = cost, best = band;
    }
    p.band = best;
    int max_blocks = kWgradBlocks;
    // developer A/B and the tests (a small input has bands of one row on one round of workgroups): a forced band height, fewer
    // workgroups.  Either changes the order of the sums, not what is summed.
    if (const char *forced = getenv("LOCOV_STEM_WGRAD_BAND")) {
        const int b = atoi(forced);
        if (b > 0) p.band = b < p.CH ? b : p.CH;
    }
    if (const char *forced = getenv("LOCOV_STEM_WGRAD_BLOCKS")) {
        const int b = atoi(forced);
        if (b > 0 && b < max_blocks) max_blocks = b;
    }
    p.bands = (int)ceil_div(p.CH, p.band);
    p.tiles = cols * p.bands;
    const int64_t wgs = ceil_div(p.tiles, kWaves);
    p.blocks = (int)(wgs < max_blocks ? wgs : max_blocks);
    const int64_t rounds = ceil_div(p.tiles, (int64_t)p.blocks * kWaves);
    p.rounds = (int)rounds;
    return rounds <= INT_MAX;
}

template <bool kSel>
int stem_fwd(const char *who, const float *x, int N, int H, int W, const float *w, const float *scale, const float *shift, int Cout,
             float *y, uint8_t *sel, locov_stream_t stream)
{
    LOCOV_REQUIRE(Cout == kCout, "%s: Cout = %d is not supported (the stem kernel is built for 64 channels)", who, Cout);
    LOCOV_REQUIRE(N >= 0 && H > 0 && W > 0, "%s: bad shape N = %d, H = %d, W = %d", who, N, H, W);
    if (N == 0) return LOCOV_OK;
    LOCOV_REQUIRE(x && w && scale && shift && y && (sel || !kSel), "%s: null pointer", who);
    LOCOV_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)scale % 4 == 0 && (uintptr_t)shift % 4 == 0 && (uintptr_t)w % 16 == 0 &&
                      (uintptr_t)y % 16 == 0,
                  "%s: misaligned pointer (w and y: 16 bytes)", who);
    const int CH = (H + 1) / 2, CW = (W + 1) / 2, PH = (CH + 1) / 2, PW = (CW + 1) / 2;
    const int tilesQ = (PW + kTW - 1) / kTW;
    // N H W < 2^57 keeps every element offset of x (3 N H W) and of y / sel (64 PH PW <= 64 H W per image) inside int64
    LOCOV_REQUIRE((int64_t)N * H <= (INT64_MAX / 64) / W, "%s: index overflow (N H W too large)", who);
    const int64_t cols = (int64_t)N * tilesQ;
    int band = stem_band(cols, PH, wave_slots());
    if (const char *forced = getenv("LOCOV_STEM_BAND")) {    // developer A/B and the tests: every band height gives the same bits
        const int b = atoi(forced);
        if (b > 0) band = b < PH ? b : PH;
    }
    const int bands = (int)ceil_div(PH, band);
    const int64_t tiles = cols * bands;
    const int64_t blocks = ceil_div(tiles, kWaves);
    LOCOV_REQUIRE(blocks <= INT_MAX, "%s: index overflow (%lld workgroups)", who, (long long)blocks);
    hipLaunchKernelGGL(resnet_stem_kernel<kSel>, dim3((unsigned)blocks), dim3(kWaves * kWave), 0, as_stream(stream), x, H, W, w, scale, shift,
                       y, sel, CH, CW, PH, PW, band, bands, tilesQ, tiles);
    return check_launch(who);
}

}  // namespace
}  // namespace locov

extern "C" int locov_resnet_stem_fwd(const float *x, int N, int H, int W, const float *w, const float *scale, const float *shift, int Cout,
                                     float *y, locov_stream_t stream)
{
    return locov::stem_fwd<false>("locov_resnet_stem_fwd", x, N, H, W, w, scale, shift, Cout, y, nullptr, stream);
}

extern "C" int locov_resnet_stem_fwd_sel(const float *x, int N, int H, int W, const float *w, const float *scale, const float *shift,
                                         int Cout, float *y, uint8_t *sel, locov_stream_t stream)
{
    return locov::stem_fwd<true>("locov_resnet_stem_fwd_sel", x, N, H, W, w, scale, shift, Cout, y, sel, stream);
}

extern "C" int64_t locov_resnet_stem_wgrad_workspace_bytes(int N, int H, int W)
{
    using namespace locov;
    WgradPlan p;
    if (N <= 0 || H <= 0 || W <= 0 || !wgrad_plan(N, H, W, p)) return 0;
    return (int64_t)p.blocks * kTaps * kCout * (int64_t)sizeof(float);
}

extern "C" int locov_resnet_stem_wgrad(const float *x, int N, int H, int W, const float *g, const uint8_t *sel, const float *scale, int Cout,
                                       float *dw, void *workspace, int64_t workspace_bytes, locov_stream_t stream)
{
    using namespace locov;
    LOCOV_REQUIRE(Cout == kCout, "locov_resnet_stem_wgrad: Cout = %d is not supported (the stem kernels are built for 64 channels)", Cout);
    LOCOV_REQUIRE(N >= 0 && H > 0 && W > 0, "locov_resnet_stem_wgrad: bad shape N = %d, H = %d, W = %d", N, H, W);
    if (N == 0) return LOCOV_OK;
    LOCOV_REQUIRE(x && g && sel && scale && dw && workspace, "locov_resnet_stem_wgrad: null pointer");
    LOCOV_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)g % 4 == 0 && (uintptr_t)scale % 4 == 0 && (uintptr_t)dw % 4 == 0 &&
                      (uintptr_t)workspace % 4 == 0,
                  "locov_resnet_stem_wgrad: misaligned pointer (4 bytes)");
    LOCOV_REQUIRE((int64_t)N * H <= (INT64_MAX / 64) / W, "locov_resnet_stem_wgrad: index overflow (N H W too large)");
    WgradPlan p;
    LOCOV_REQUIRE(wgrad_plan(N, H, W, p), "locov_resnet_stem_wgrad: index overflow (too many tiles per workgroup)");
    const int64_t need = (int64_t)p.blocks * kTaps * kCout * (int64_t)sizeof(float);
    LOCOV_REQUIRE(workspace_bytes >= need, "locov_resnet_stem_wgrad: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)need);
    float *part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(resnet_stem_wgrad_kernel, dim3((unsigned)p.blocks), dim3(kWaves * kWave), 0, as_stream(stream), x, H, W, g, sel, part,
                       p.CH, p.CW, p.PH, p.PW, p.band, p.bands, p.tilesC, p.tiles, p.rounds);
    if (int rc = check_launch("locov_resnet_stem_wgrad")) return rc;
    hipLaunchKernelGGL(resnet_stem_wgrad_reduce_kernel, dim3(kTaps * kCout / 32), dim3(256), 0, as_stream(stream), part, p.blocks,
                       scale, dw);
    return check_launch("locov_resnet_stem_wgrad");
}
