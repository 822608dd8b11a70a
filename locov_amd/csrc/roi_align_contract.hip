// The pooler contract ([R,C,ph,pw] out of an NCHW map; roi_emb_heads.py:182-187,243-245) at HBM speed: gather from a
// channels-last COPY of the map, transpose in LDS, write NCHW.
//
// Gathering from NCHW costs one scattered dword per lane and tap (5-10 cache lines per wave
// instruction: the texture-address path, not HBM, bounds the kernel at ~0.6 TB/s).  From a
// channels-last copy a tap is one contiguous C-vector: 16 lanes x 16 B cover 64 channels, a wave
// covers several bins per instruction.  One workgroup = one ROI x kT2Ch channels: results go to an
// LDS tile [ch][ph*pw] (odd row stride) and leave as one contiguous, fully coalesced run of
// kT2Ch*ph*pw floats -- exactly the layout of out[r, c0:c0+kT2Ch, :, :].
// Arithmetic and summation order per output element are those of roi_align_nchw_kernel (and of
// the oracle): the result is bit-identical.
#include "roi_align_nhwc_common.h"

#include <type_traits>

namespace locov {

#ifndef LOCOV_T2_STORE_AUX
#define LOCOV_T2_STORE_AUX 2                               // the pooler-contract kernel's NCHW stores: nt 2.88 ms, plain 2.94, sc1 2.98 (tools/ab_t2.py)
#endif

constexpr int kT2Threads = 256;
constexpr int kT2Ch = 32;          // channels per workgroup (one 128-byte line per tap; ~25 KiB LDS tile)
constexpr int kT2Axis = 256;       // per-axis LDS table entries (larger sampling grids: computed on the fly)

// ---- small proposals: the whole footprint in LDS (roi_align_win_kernel) --------------------------------------------------
// A proposal of up to ~11 x 11 map pixels (side <= ~180 image pixels: 6 of 10 bench proposals) touches at most 14 x 14 pixels, and
// the [32 ch][bins] transpose tile is 25 KB = 197 pixels x 128 B.  For those ROIs the workgroup fetches the pixel rectangle ONCE
// (<= 7 loads per thread, all in flight: one memory latency instead of one per pass of 32 bins), takes every tap from LDS -- the
// same values in the same per-sample order: bit-identical -- keeps its 7 results per thread in registers and only then re-uses
// the same LDS bytes as the transpose tile.  LDS per workgroup and waves per CU are those of the direct form (what sank round 3's
// LDS-staged kernel and round 4's pipelined one was occupancy).  roi_window_rect decides per workgroup, from the proposal's coordinates
// alone, which path it takes.
constexpr int kWinPitch = 4 * kT2Ch;                      // bytes per pixel of the window (32 channels)
constexpr int kWinMaxPasses = 7;                          // results per thread kept in registers: bins <= 7 * 32
#ifndef LOCOV_ROIALIGN_WINDOW
#define LOCOV_ROIALIGN_WINDOW 1                           // developer A/B: 0 = every proposal takes the direct form
#endif

// conservative pixel rectangle of every tap of the ROI: one pixel of margin on each side absorbs the difference between this
// estimate's rounding and axis_sample_n's.  Returns false when it does not fit `cap` pixels (or the ROI cannot use the window).
__device__ __forceinline__ bool roi_window_rect(float start_h, float start_w, float bin_h, float bin_w, int gh, int gw, int PH, int PW, int H,
                                                int W, int cap, bool valid_b, int &y0, int &x0, int &wh, int &ww)
{
    if (!LOCOV_ROIALIGN_WINDOW || !valid_b || gh <= 0 || gw <= 0 || PH * PW > kWinMaxPasses * (kT2Threads / (kT2Ch / 4)) || PH * gh > kT2Axis ||
        PW * gw > kT2Axis)
        return false;
    // every sample lies between the ROI's two edges (an inverted ROI under a forced sampling ratio runs from the far edge back)
    const float ya_ = start_h, yb_ = start_h + (float)PH * bin_h, xa_ = start_w, xb_ = start_w + (float)PW * bin_w;
    const float yf = fminf(ya_, yb_), yl = fmaxf(ya_, yb_), xf = fminf(xa_, xb_), xl = fmaxf(xa_, xb_);
    if (!(yl - yf < 64.f) || !(xl - xf < 64.f) || !(yf > -1.0e6f) || !(xf > -1.0e6f) || !(yl < 1.0e6f) || !(xl < 1.0e6f)) return false;   // (also rejects NaN)
    const int ya = max((int)floorf(fmaxf(yf, 0.f)) - 1, 0), yb = min((int)floorf(fmaxf(yl, 0.f)) + 2, H - 1);
    const int xa = max((int)floorf(fmaxf(xf, 0.f)) - 1, 0), xb = min((int)floorf(fmaxf(xl, 0.f)) + 2, W - 1);
    y0 = min(ya, H - 1);
    x0 = min(xa, W - 1);
    wh = max(yb - y0 + 1, 1);
    ww = max(xb - x0 + 1, 1);
    // (the window path stages at most kWinMaxPasses pixels per thread group: a tile of more than 224 floats per channel row could hold more)
    return wh * ww <= min(cap, kWinMaxPasses * (kT2Threads / (kT2Ch / 4)));
}

// the finished LDS tile [kT2Ch][ts] -> out[r, c0 : c0 + kT2Ch, :, :]: one contiguous run (every thread of the workgroup, behind a barrier)
__device__ __forceinline__ void t2_store_tile(const float *tile, int ts, int bins, int C, int c0, int64_t r, float *__restrict__ out)
{
    const int cn = min(kT2Ch, C - c0);
    float *dst = out + (r * C + c0) * (int64_t)bins;
    if ((bins & 3) == 0) {
        // 16 bytes per lane: four consecutive bins of one channel (a channel's run is a multiple of 4 floats, so a quad never
        // straddles two channels); (channel, bin quad) advance incrementally -- no division per element
        const int qpc = bins >> 2;                                     // quads per channel
        int c = 0, b4 = threadIdx.x;
        while (b4 >= qpc) {
            b4 -= qpc;
            c++;
        }
        const int step_c = kT2Threads / qpc, step_b = kT2Threads - step_c * qpc;
        while (c < cn) {
            const float *t = tile + c * ts + 4 * b4;
            const float4 v = {t[0], t[1], t[2], t[3]};
            store4_policy<LOCOV_T2_STORE_AUX>(dst + (c * bins + 4 * b4), v);
            c += step_c;
            b4 += step_b;
            if (b4 >= qpc) {
                b4 -= qpc;
                c++;
            }
        }
        return;
    }
    const float inv_bins = 1.0f / (float)bins;
    for (int idx = threadIdx.x; idx < cn * bins; idx += kT2Threads) {
        const int c = (int)(((float)idx + 0.5f) * inv_bins);       // idx / bins, exact for these sizes (no integer divide)
        dst[idx] = tile[c * ts + (idx - c * bins)];
    }
}

// (a device function of roi_align_nhwc2nchw_kernel, not a launch of its own: as two launches the direct form's texture-bound large
//  proposals and the window form's store-bound small ones ran one after the other instead of beside each other -- 3.05 ms against
//  2.84; the two paths share the kernel's register allocation, the larger of the two)
__device__ __forceinline__ void roi_align_window_path(const float *__restrict__ feat, int b, int H, int W, int C, const RoiGeom &g, int PH, int PW,
                                                      float *__restrict__ out, float *smem, int y0, int x0, int wh, int ww)
{
    const int bins = PH * PW;
    const int ts = bins | 1;                                  // odd row stride of the transpose tile
    float *tile = smem;                                       // [kT2Ch][ts] -- first the pixel window, then the tile
    char *win = reinterpret_cast<char *>(smem);
    AxisSampleN *ytab = reinterpret_cast<AxisSampleN *>(smem + kT2Ch * ts + (4 - (kT2Ch * ts) % 4) % 4);
    AxisSampleN *xtab = ytab + kT2Axis;

    const int64_t r = blockIdx.x;
    const int c0 = blockIdx.y * kT2Ch;
    const float start_h = g.start_h, start_w = g.start_w, bin_h = g.bin_h, bin_w = g.bin_w, count = g.count;
    const int gh = g.grid_h, gw = g.grid_w, prod = gh * gw;      // (the window is only taken with both grids > 0)

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int QN = kT2Ch / 4;                             // lanes (channel quads) per bin / per pixel
    constexpr int BPW = 64 / QN;                              // bins per wave instruction
    constexpr int PPP = kT2Threads / QN;                      // pixels (and bins) per pass of the workgroup
    const int q = lane % QN, sub = lane / QN;
    const int cq = c0 + 4 * q;
    const bool c_ok = cq < C;                                 // C % 4 == 0: a quad is all-in or all-out
    const unsigned ystride = (unsigned)W * C * (unsigned)sizeof(float), xstride = (unsigned)C * (unsigned)sizeof(float);
    const float *img = feat + (int64_t)b * H * W * C;
    const __amdgpu_buffer_rsrc_t img_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(img), 0, (unsigned)H * ystride, 0x00020000);

    // 1. the window's pixels, every load of this thread in flight: pixel p = (row p / ww, column p % ww), its 128 bytes by 8 lanes
    const int npx = wh * ww;
    const float inv_ww = 1.0f / (float)ww;
    const int p0 = threadIdx.x / QN, qq = threadIdx.x % QN;
    const unsigned qoff = (unsigned)(c0 + 4 * qq < C ? c0 + 4 * qq : 0) * (unsigned)sizeof(float);
    float4 stage[kWinMaxPasses];
#pragma unroll
    for (int i = 0; i < kWinMaxPasses; i++) {
        const int p = p0 + i * PPP;
        stage[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (p < npx) {
            const int wr = (int)(((float)p + 0.5f) * inv_ww), wc = p - wr * ww;         // exact for these small integers
            stage[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                      img_rsrc, (unsigned)(y0 + wr) * ystride + (unsigned)(x0 + wc) * xstride + qoff, 0, 0));
        }
    }
    // 2. (under those loads) the sampling tables, with WINDOW byte offsets: row offset for y, pixel offset for x.  A sample outside
    // [-1, size] has weights 0 and points at the window's first row / column (0 * finite = 0, as in the direct form)
    const int ny = PH * gh, nx = PW * gw;
    for (int t = threadIdx.x; t < ny; t += kT2Threads) {
        AxisSampleN a = axis_sample_n(start_h, bin_h, t / gh, t % gh, gh, H);
        a.lo = min(max(a.lo - y0, 0), wh - 1) * (ww * kWinPitch);
        a.hi = min(max(a.hi - y0, 0), wh - 1) * (ww * kWinPitch);
        ytab[t] = a;
    }
    for (int t = threadIdx.x; t < nx; t += kT2Threads) {
        AxisSampleN a = axis_sample_n(start_w, bin_w, t / gw, t % gw, gw, W);
        a.lo = min(max(a.lo - x0, 0), ww - 1) * kWinPitch;
        a.hi = min(max(a.hi - x0, 0), ww - 1) * kWinPitch;
        xtab[t] = a;
    }
#pragma unroll
    for (int i = 0; i < kWinMaxPasses; i++) {
        const int p = p0 + i * PPP;
        if (p < npx) *reinterpret_cast<float4 *>(win + p * kWinPitch + qq * 16) = stage[i];
    }
    __syncthreads();

    // 3. every bin of this thread out of the window, torchvision's sample order, un-fused: the arithmetic of the direct form
    const int ns = gh * gw;
    const float inv_pw = 1.0f / (float)PW;
    const int icount = prod > 1 ? prod : 1;
    const bool count_pow2 = (icount & (icount - 1)) == 0;     // wave-uniform
    const float inv_count = 1.0f / count;                     // exact when count is a power of two
    const char *wq = win + q * 16;
    float4 res[kWinMaxPasses];
#pragma unroll
    for (int k = 0; k < kWinMaxPasses; k++) {
        const int bin = k * PPP + wave * BPW + sub;
        const bool bin_ok = bin < bins;
        const int ph = bin_ok ? (int)(((float)bin + 0.5f) * inv_pw) : 0, pw = bin_ok ? bin - ph * PW : 0;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        if (bin_ok && c_ok) {
            int iy = 0, ix = 0;
            for (int sidx = 0; sidx < ns; sidx++) {
                const AxisSampleN ys = ytab[ph * gh + iy], xs = xtab[pw * gw + ix];
                const float w1 = ys.wh * xs.wh, w2 = ys.wh * xs.wl, w3 = ys.wl * xs.wh, w4 = ys.wl * xs.wl;
                const float4 v1 = *reinterpret_cast<const float4 *>(wq + ys.lo + xs.lo);
                const float4 v2 = *reinterpret_cast<const float4 *>(wq + ys.lo + xs.hi);
                const float4 v3 = *reinterpret_cast<const float4 *>(wq + ys.hi + xs.lo);
                const float4 v4 = *reinterpret_cast<const float4 *>(wq + ys.hi + xs.hi);
                // ((w1*v1 + w2*v2) + w3*v3) + w4*v4, then accumulate -- un-fused (file built with -ffp-contract=off)
                acc.x = acc.x + (((w1 * v1.x + w2 * v2.x) + w3 * v3.x) + w4 * v4.x);
                acc.y = acc.y + (((w1 * v1.y + w2 * v2.y) + w3 * v3.y) + w4 * v4.y);
                acc.z = acc.z + (((w1 * v1.z + w2 * v2.z) + w3 * v3.z) + w4 * v4.z);
                acc.w = acc.w + (((w1 * v1.w + w2 * v2.w) + w3 * v3.w) + w4 * v4.w);
                if (++ix == gw) {
                    ix = 0;
                    iy++;
                }
            }
        }
        if (count_pow2) {              // x / 2^k == x * 2^-k bit for bit (both are the correctly rounded quotient)
            acc.x *= inv_count; acc.y *= inv_count; acc.z *= inv_count; acc.w *= inv_count;
        } else {
            acc.x /= count; acc.y /= count; acc.z /= count; acc.w /= count;
        }
        res[k] = acc;
    }
    __syncthreads();                                          // every tap has been read: the window's bytes become the tile
#pragma unroll
    for (int k = 0; k < kWinMaxPasses; k++) {
        const int bin = k * PPP + wave * BPW + sub;
        if (bin < bins) {
            float *t = tile + (4 * q) * ts + bin;
            t[0] = res[k].x;
            t[ts] = res[k].y;
            t[2 * ts] = res[k].z;
            t[3 * ts] = res[k].w;
        }
    }
    __syncthreads();
    t2_store_tile(tile, ts, bins, C, c0, r, out);
}

#ifndef LOCOV_T2_MINW
#define LOCOV_T2_MINW 4                                    // four waves per SIMD = four workgroups per CU (the register allocator's budget: 128)
#endif
__global__ __launch_bounds__(kT2Threads, LOCOV_T2_MINW) void roi_align_nhwc2nchw_kernel(
    const float *__restrict__ feat, int N, int H, int W, int C, const float *__restrict__ rois, int PH, int PW,
    float scale, int sampling_ratio, int aligned, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int bins = PH * PW;
    const int ts = bins | 1;                                  // odd row stride of the transpose tile
    float *tile = smem;                                       // [kT2Ch][ts]
    AxisSampleN *ytab = reinterpret_cast<AxisSampleN *>(smem + kT2Ch * ts + (4 - (kT2Ch * ts) % 4) % 4);
    AxisSampleN *xtab = ytab + kT2Axis;

    const int64_t r = blockIdx.x;
    const int c0 = blockIdx.y * kT2Ch;
    const float *roi = rois + r * 5;
    const int b = (int)roi[0];
    const RoiGeom g = roi_geom(roi, scale, PH, PW, sampling_ratio, aligned);
    const float start_h = g.start_h, start_w = g.start_w, bin_h = g.bin_h, bin_w = g.bin_w, count = g.count;
    const int prod = g.grid_h * g.grid_w;
    const bool valid_b = b >= 0 && b < N;
    {
        // a proposal whose pixel rectangle fits the LDS window takes every tap from there (roi_align_window_path)
        int wy0, wx0, wwh, www;
        if (roi_window_rect(start_h, start_w, bin_h, bin_w, g.grid_h, g.grid_w, PH, PW, H, W, (kT2Ch * (bins | 1) * 4) / kWinPitch, valid_b, wy0, wx0, wwh, www)) {
            roi_align_window_path(feat, b, H, W, C, g, PH, PW, out, smem, wy0, wx0, wwh, www);
            return;
        }
    }
    const int gh = (g.grid_h > 0 && valid_b) ? g.grid_h : 0, gw = (g.grid_w > 0 && valid_b) ? g.grid_w : 0;
    const int ny = PH * gh, nx = PW * gw;
    const bool use_lds = ny <= kT2Axis && nx <= kT2Axis;
    // the tables hold BYTE offsets into the image (row offset for y, pixel offset for x): a tap address is
    // then two 32-bit adds on top of a wave-uniform buffer descriptor instead of 64-bit multiplies per tap
    const unsigned ystride = (unsigned)W * C * (unsigned)sizeof(float), xstride = (unsigned)C * (unsigned)sizeof(float);
    auto as_offsets = [](AxisSampleN a, unsigned stride) {
        a.lo = (int)((unsigned)a.lo * stride);
        a.hi = (int)((unsigned)a.hi * stride);
        return a;
    };
    if (use_lds) {
        for (int t = threadIdx.x; t < ny; t += kT2Threads)
            ytab[t] = as_offsets(axis_sample_n(start_h, bin_h, t / gh, t % gh, gh, H), ystride);
        for (int t = threadIdx.x; t < nx; t += kT2Threads)
            xtab[t] = as_offsets(axis_sample_n(start_w, bin_w, t / gw, t % gw, gw, W), xstride);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int QN = kT2Ch / 4;                             // lanes (channel quads) per bin
    constexpr int BPW = 64 / QN;                              // bins per wave instruction
    const int q = lane % QN, sub = lane / QN;
    const int cq = c0 + 4 * q;
    const bool c_ok = cq < C;                                 // C % 4 == 0: a quad is all-in or all-out
    const float *img = feat + (int64_t)(valid_b ? b : 0) * H * W * C;
    const __amdgpu_buffer_rsrc_t img_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(img), 0, (unsigned)H * ystride, 0x00020000);
    const unsigned ch_off = (unsigned)(c_ok ? cq : 0) * (unsigned)sizeof(float);
    auto tap = [&](unsigned off) {
        return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(img_rsrc, off, 0, 0));
    };
    const int ns = gh * gw;                                   // samples per bin
#ifndef LOCOV_T2_U
#define LOCOV_T2_U 2                                       // (4 until the row form took the 2-4-sample rows: 2 leaves it the registers -- mix 2.62 -> 2.50 ms)
#endif
    constexpr int U = LOCOV_T2_U;                             // samples in flight per lane on the plain path (4 x 16-byte loads each)
    const float inv_pw = 1.0f / (float)PW;
    const int icount = prod > 1 ? prod : 1;
    const bool count_pow2 = (icount & (icount - 1)) == 0;     // wave-uniform
    const float inv_count = 1.0f / count;                     // exact when count is a power of two
    for (int g0 = 0; g0 < bins; g0 += 4 * BPW) {
        const int bin = g0 + wave * BPW + sub;
        const bool bin_ok = bin < bins;
        // bin -> (ph, pw): exact for these small integers, and far cheaper than an integer division
        const int ph = bin_ok ? (int)(((float)bin + 0.5f) * inv_pw) : 0, pw = bin_ok ? bin - ph * PW : 0;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        if (bin_ok && c_ok) {
            // The gather is latency-bound (taps come from L1 / L2), so the loads of up to U samples are
            // issued back to back before any of them is consumed; the accumulation still runs in sample
            // order (iy outer, ix inner), i.e. the oracle's order.  Groups are sized exactly (ns is
            // uniform per ROI): most ROIs have 1-4 samples per bin and padded groups would spend the
            // texture-address unit and the vector ALU -- both ~80 % busy here -- on duplicates.
            int iy = 0, ix = 0;                                  // sample counters (wave-uniform: scalar registers)
            auto group = [&](auto nu_tag) __attribute__((always_inline)) {
                constexpr int NU = decltype(nu_tag)::value;
                float4 v[NU][4];
                float w[NU][4];
#pragma unroll
                for (int u = 0; u < NU; u++) {
                    const AxisSampleN ys = use_lds ? ytab[ph * gh + iy]
                                                   : as_offsets(axis_sample_n(start_h, bin_h, ph, iy, gh, H), ystride);
                    const AxisSampleN xs = use_lds ? xtab[pw * gw + ix]
                                                   : as_offsets(axis_sample_n(start_w, bin_w, pw, ix, gw, W), xstride);
                    const unsigned xlo = (unsigned)xs.lo + ch_off, xhi = (unsigned)xs.hi + ch_off;
                    w[u][0] = ys.wh * xs.wh; w[u][1] = ys.wh * xs.wl; w[u][2] = ys.wl * xs.wh; w[u][3] = ys.wl * xs.wl;
                    v[u][0] = tap((unsigned)ys.lo + xlo);
                    v[u][1] = tap((unsigned)ys.lo + xhi);
                    v[u][2] = tap((unsigned)ys.hi + xlo);
                    v[u][3] = tap((unsigned)ys.hi + xhi);
                    if (++ix == gw) {
                        ix = 0;
                        iy++;
                    }
                }
#pragma unroll
                for (int u = 0; u < NU; u++) {
                    // ((w1*v1 + w2*v2) + w3*v3) + w4*v4, then accumulate -- un-fused (file built
                    // with -ffp-contract=off)
                    acc.x = acc.x + (((w[u][0] * v[u][0].x + w[u][1] * v[u][1].x) + w[u][2] * v[u][2].x) + w[u][3] * v[u][3].x);
                    acc.y = acc.y + (((w[u][0] * v[u][0].y + w[u][1] * v[u][1].y) + w[u][2] * v[u][2].y) + w[u][3] * v[u][3].y);
                    acc.z = acc.z + (((w[u][0] * v[u][0].z + w[u][1] * v[u][1].z) + w[u][2] * v[u][2].z) + w[u][3] * v[u][3].z);
                    acc.w = acc.w + (((w[u][0] * v[u][0].w + w[u][1] * v[u][1].w) + w[u][2] * v[u][2].w) + w[u][3] * v[u][3].w);
                }
            };
            // Rows of 2-4 samples: consecutive samples of a bin row are at most one pixel apart (grid = ceil(bin size)), so sample
            // ix + 1 re-uses one of sample ix's two pixel columns -- its left column IS the previous left or the previous right one.
            // A row of GW samples then needs GW + 1 columns x 2 rows of loads instead of 4 GW taps (6 / 8 / 10 instead of 8 / 12 / 16):
            // a quarter to three eighths fewer bytes through the texture path, which is what bounds the large proposals.  Which column is
            // re-used differs per lane group (= per bin): a select on already loaded registers, the SAME values in the same sample
            // order -- bit-identical.  Checked per row from the tables alone (all lanes must be able to re-use); otherwise the row
            // takes the four taps per sample.
            auto row_group = [&](auto gw_tag, auto rp_tag) __attribute__((always_inline)) {
                constexpr int GW = decltype(gw_tag)::value, RP = decltype(rp_tag)::value;
                AxisSampleN xs[GW];
                bool ok = true;
#pragma unroll
                for (int i = 0; i < GW; i++) {
                    xs[i] = xtab[pw * gw + i];
                    if (i > 0) ok = ok && (xs[i].lo == xs[i - 1].lo || xs[i].lo == xs[i - 1].hi);
                }
                if (!__all(ok)) {                              // (wave-uniform: a lane group whose samples jump takes the plain form with it)
                    for (int t = 0; t < RP * GW; t++) group(std::integral_constant<int, 1>{});
                    return;
                }
                float4 L[RP][GW + 1], Hh[RP][GW + 1];
                AxisSampleN ys[RP];
#pragma unroll
                for (int r = 0; r < RP; r++) {
                    ys[r] = ytab[ph * gh + iy + r];
                    const unsigned ylo = (unsigned)ys[r].lo + ch_off, yhi = (unsigned)ys[r].hi + ch_off;
                    L[r][0] = tap(ylo + (unsigned)xs[0].lo);
                    Hh[r][0] = tap(yhi + (unsigned)xs[0].lo);
#pragma unroll
                    for (int i = 0; i < GW; i++) {
                        L[r][i + 1] = tap(ylo + (unsigned)xs[i].hi);
                        Hh[r][i + 1] = tap(yhi + (unsigned)xs[i].hi);
                    }
                }
#pragma unroll
                for (int r = 0; r < RP; r++) {
                    float4 a0 = L[r][0], a2 = Hh[r][0], a1 = L[r][1], a3 = Hh[r][1];
#pragma unroll
                    for (int i = 0; i < GW; i++) {
                        if (i > 0) {
                            const bool same = xs[i].lo == xs[i - 1].lo;      // else the previous right column
                            a0.x = same ? a0.x : a1.x; a0.y = same ? a0.y : a1.y; a0.z = same ? a0.z : a1.z; a0.w = same ? a0.w : a1.w;
                            a2.x = same ? a2.x : a3.x; a2.y = same ? a2.y : a3.y; a2.z = same ? a2.z : a3.z; a2.w = same ? a2.w : a3.w;
                            a1 = L[r][i + 1];
                            a3 = Hh[r][i + 1];
                        }
                        const float w0 = ys[r].wh * xs[i].wh, w1 = ys[r].wh * xs[i].wl, w2 = ys[r].wl * xs[i].wh, w3 = ys[r].wl * xs[i].wl;
                        acc.x = acc.x + (((w0 * a0.x + w1 * a1.x) + w2 * a2.x) + w3 * a3.x);
                        acc.y = acc.y + (((w0 * a0.y + w1 * a1.y) + w2 * a2.y) + w3 * a3.y);
                        acc.z = acc.z + (((w0 * a0.z + w1 * a1.z) + w2 * a2.z) + w3 * a3.z);
                        acc.w = acc.w + (((w0 * a0.w + w1 * a1.w) + w2 * a2.w) + w3 * a3.w);
                    }
                }
                iy += RP;                                      // (ix stays 0: whole rows)
            };
            // (Sharing a pixel ROW between two consecutive sample rows the same way -- 3 (GW + 1) loads per row pair instead of
            //  4 (GW + 1) -- was built too: bit-identical and 15-40 % SLOWER, 22 spilled registers at four waves per SIMD; R4.8.)
#ifndef LOCOV_T2_DEDUPE
#define LOCOV_T2_DEDUPE 1                                  // developer A/B: 0 = four taps per sample everywhere
#endif
            using std::integral_constant;
            if (LOCOV_T2_DEDUPE && use_lds && gw >= 2 && gw <= 4) {
                while (iy < gh) {
                    // (two rows in flight only at GW = 2: 12 loads; three samples x two rows asked for 140 registers = a wave per SIMD less)
                    if (gw == 2) {
                        if (iy + 1 < gh) row_group(integral_constant<int, 2>{}, integral_constant<int, 2>{});
                        else row_group(integral_constant<int, 2>{}, integral_constant<int, 1>{});
                    } else if (gw == 3) {
                        row_group(integral_constant<int, 3>{}, integral_constant<int, 1>{});
                    } else {
                        row_group(integral_constant<int, 4>{}, integral_constant<int, 1>{});
                    }
                }
            } else {
                int s0 = 0;
                for (; s0 + U <= ns; s0 += U) group(std::integral_constant<int, U>{});
                switch (ns - s0) {                                   // wave-uniform remainder, 0..U-1 samples
                case 3: group(std::integral_constant<int, (U > 3 ? 3 : 1)>{}); break;
                case 2: group(std::integral_constant<int, (U > 2 ? 2 : 1)>{}); break;
                case 1: group(std::integral_constant<int, 1>{}); break;
                default: break;
                }
            }
        }
        if (bin_ok) {
            float *t = tile + (4 * q) * ts + bin;
            if (count_pow2) {          // x / 2^k == x * 2^-k bit for bit (both are the correctly rounded quotient)
                t[0] = acc.x * inv_count;
                t[ts] = acc.y * inv_count;
                t[2 * ts] = acc.z * inv_count;
                t[3 * ts] = acc.w * inv_count;
            } else {
                t[0] = acc.x / count;
                t[ts] = acc.y / count;
                t[2 * ts] = acc.z / count;
                t[3 * ts] = acc.w / count;
            }
        }
    }
    __syncthreads();
    t2_store_tile(tile, ts, bins, C, c0, r, out);
}

}  // namespace locov

using namespace locov;

extern "C" {

int64_t locov_roi_align_plan_bytes(int64_t R) { return R > 0 ? roi_align_tiles_plan_bytes(R) : 0; }

int locov_roi_align_from_nhwc_fwd_ex(const float *feat_nhwc, int N, int H, int W, int C, const float *rois, int64_t R,
                                     int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio, int aligned,
                                     int mode, void *workspace, int64_t workspace_bytes, float *out, locov_stream_t stream)
{
    LOCOV_REQUIRE(mode == LOCOV_ROIALIGN_EXACT || mode == LOCOV_ROIALIGN_FAST, "locov_roi_align_from_nhwc_fwd: bad mode %d", mode);
    LOCOV_REQUIRE(R >= 0, "locov_roi_align_from_nhwc_fwd: R < 0");
    LOCOV_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "locov_roi_align_from_nhwc_fwd: bad feature shape");
    LOCOV_REQUIRE(pooled_h > 0 && pooled_w > 0, "locov_roi_align_from_nhwc_fwd: bad pooled size");
    LOCOV_REQUIRE(spatial_scale > 0.f, "locov_roi_align_from_nhwc_fwd: spatial_scale must be > 0");
    LOCOV_REQUIRE(C % 4 == 0, "locov_roi_align_from_nhwc_fwd: C must be a multiple of 4");
    if (R == 0) return LOCOV_OK;
    LOCOV_REQUIRE(feat_nhwc && rois && out, "locov_roi_align_from_nhwc_fwd: null pointer");
    LOCOV_REQUIRE(R <= 0x7fffffffLL, "locov_roi_align_from_nhwc_fwd: R too large");
    LOCOV_REQUIRE((int64_t)H * W * C * 4 < 0xffffffffLL, "locov_roi_align_from_nhwc_fwd: one image must stay below 4 GiB");
    if (mode == LOCOV_ROIALIGN_FAST) {
        LOCOV_REQUIRE(workspace && workspace_bytes >= locov_roi_align_plan_bytes(R) && (uintptr_t)workspace % 16 == 0,
                      "locov_roi_align_from_nhwc_fwd: the fast form needs locov_roi_align_plan_bytes(R) bytes of 16-byte aligned workspace");
        return launch_roi_align_tiles(feat_nhwc, N, H, W, C, rois, R, pooled_h, pooled_w, spatial_scale, sampling_ratio, aligned, workspace,
                                      out, as_stream(stream));
    }
    const int bins = pooled_h * pooled_w, ts = bins | 1;
    const size_t lds = ((size_t)kT2Ch * ts + 4) * sizeof(float) + 2 * kT2Axis * sizeof(AxisSampleN);
    LOCOV_REQUIRE(lds <= 150 * 1024, "locov_roi_align_from_nhwc_fwd: pooled size %dx%d too large for the LDS tile", pooled_h,
                  pooled_w);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(roi_align_nhwc2nchw_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return set_error(LOCOV_ERR_LAUNCH, "locov_roi_align_from_nhwc_fwd: cannot raise the dynamic LDS limit to %zu bytes", (size_t)lds);
    dim3 grid((unsigned)R, (unsigned)ceil_div(C, kT2Ch));
    hipLaunchKernelGGL(roi_align_nhwc2nchw_kernel, grid, dim3(kT2Threads), lds, as_stream(stream), feat_nhwc, N, H, W, C,
                       rois, pooled_h, pooled_w, spatial_scale, sampling_ratio, aligned, out);
    return check_launch("locov_roi_align_from_nhwc_fwd");
}

int locov_roi_align_from_nhwc_fwd(const float *feat_nhwc, int N, int H, int W, int C, const float *rois, int64_t R,
                                  int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio, int aligned,
                                  float *out, locov_stream_t stream)
{
    return locov_roi_align_from_nhwc_fwd_ex(feat_nhwc, N, H, W, C, rois, R, pooled_h, pooled_w, spatial_scale, sampling_ratio,
                                            aligned, LOCOV_ROIALIGN_EXACT, nullptr, 0, out, stream);
}

}  // extern "C"
