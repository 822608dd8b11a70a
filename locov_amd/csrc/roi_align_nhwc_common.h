// What the channels-last ROIAlign sources share (roi_align_nhwc.hip: the even-grid pooler; roi_align_nhwc_bwd.hip: its two backward
// kernels; roi_align_contract.hip: the pooler contract): 4-channel taps and stores, the pooler's workgroup frame (slice decode,
// geometry, sampling tables, separable per-pixel weights) and the launchers that cross the files.
#pragma once
#include "roi_align_common.h"

namespace locov {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
// The pooled rows are consumed by a LATER kernel (GBs of other traffic in between), while the map slice they were gathered from
// is re-read by every ROI of the image: `sc1` stores leave no copy of the written line in the XCD's L2 (MI355X_MICROARCH.md,
// stores of each flavour), so the 3.2 GB of output no longer push the 2-4 MB map slice out of it.
// Measured on the 2 048-channel launch of block 0's shortcut (8 x 1000 proposals; tools/ab_pool.sh, docs/experiments.md R4):
// plain stores 1.17 ms with 3.9 GB of fabric reads for a 0.28 GB map; `sc1` 1.18 ms / 1.6 GB; `nt` 1.06 ms / 1.8 GB -- nt it is.
#ifndef LOCOV_POOL_STORE_AUX
#define LOCOV_POOL_STORE_AUX 2                             // 0 = plain, 2 = nt, 16 = sc1, 17 = sc0 sc1 (developer A/B)
#endif
template <int AUX>
__device__ __forceinline__ void store4_policy(float *p, const float4 &v)
{
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const f32x4_t d = {v.x, v.y, v.z, v.w};
    if (AUX == 16) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(d) : "memory");
    else if (AUX == 17) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(d) : "memory");
    else if (AUX == 2) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(p), "v"(d) : "memory");
    else *reinterpret_cast<float4 *>(p) = v;
}
#ifndef LOCOV_POOL_NO_STORE
#define LOCOV_POOL_NO_STORE 0                              // developer timing (tools/ab_pool_nostore.sh): 1 = the gather alone (wrong results)
#endif
__device__ __forceinline__ void store4_out(float *p, const float4 &v)
{
    if (LOCOV_POOL_NO_STORE && v.x != 1234.56789f) return;       // (a value nothing takes: the loads stay, the store goes)
    store4_policy<LOCOV_POOL_STORE_AUX>(p, v);
}
__device__ __forceinline__ void store4_out(__bf16 *p, const float4 &v)
{
    bf16x4 o;
    o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
    *reinterpret_cast<bf16x4 *>(p) = o;
}

// one tap = 4 consecutive channels through a raw buffer descriptor (byte offset in a VGPR, base in SGPRs)
__device__ __forceinline__ float4 tap4(__amdgpu_buffer_rsrc_t r, unsigned off, float *)
{
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ float4 tap4(__amdgpu_buffer_rsrc_t r, unsigned off, __bf16 *)
{
    const bf16x4 v = __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
    return float4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// (the sampling tables hold BYTE offsets into the image -- row offset for y, pixel offset for x -- so that a tap address is two
// 32-bit adds on top of a wave-uniform buffer descriptor instead of 64-bit multiplies per tap)
__device__ __forceinline__ AxisSampleN as_offsets(AxisSampleN a, unsigned stride)
{
    a.lo = (int)((unsigned)a.lo * stride);
    a.hi = (int)((unsigned)a.hi * stride);
    return a;
}

constexpr int kNhwcThreads = 256;
constexpr int kMaxAxisN = 192;     // per-axis LDS table entries (7 x up to 27 samples; larger grids are computed on the fly): keeps the kernel at 6+ workgroups per CU
constexpr int kSepGrid = 16, kSepCols = 32;   // the separable form: sampling grids up to 16 per axis, up to 32 bin rows / columns

// ---- the workgroup frame of the even-grid pooler, forward (roi_align_nhwc_kernel) and scatter backward (roi_align_nhwc_bwd_kernel) ----
// The LDS arrays a workgroup builds before its bin loop.  They are DECLARED in the kernels (each kernel's LDS layout is its own) and
// handed to nhwc_roi_frame.
struct NhwcRoiLds {
    AxisSampleN *ytab, *xtab;      // [kMaxAxisN]: every (strided) bin row's y samples / every (strided) column's x samples
    float *ypw, *xpw;              // [kSepCols * (kSepGrid + 1)]: per bin row / column, the per-PIXEL sums of the samples' bilinear weights
    int (*ypix)[2], (*xpix)[2];    // [kSepCols]: per bin row / column {byte offset of the first pixel row / column, number of them}
    int *sep_bad;
};

// What the bin loops read of their (proposal, channel slice).
struct NhwcRoiFrame {
    int64_t r;                     // the proposal
    int b; bool valid_b;           // its batch index; whether that names an image
    float start_h, start_w, bin_h, bin_w, inv_count;
    int gh, gw;                    // sampling grid, clamped to >= 0
    unsigned xstride, ystride;     // bytes between pixels / pixel rows of the map
    bool use_lds, separable;       // the samples are in ytab / xtab; the bins are in ypw / xpw / ypix / xpix
    int q_lo, q_hi;                // this workgroup's channel slice [4 q_lo, 4 q_hi): multiples of 4 channels
};

// grid = R * nslices (1-D): one workgroup = one ROI x one CHANNEL SLICE, all OH x OW bins.
//
// Why slices: workgroups are dealt round-robin over the 8 XCDs, each with its own 4 MB L2.  With one workgroup per
// (ROI, bin row) and all channels, every XCD touched every channel of every image: on the map path (2 560 pooled channels,
// 43 MB per 1333x800 image) each bin's pixels came from beyond L2 -- 11.2 GB of fabric reads per launch pair for 4 GB of
// output (rocprofv3 FETCH_SIZE, profiles/r01l).  Now blockIdx % nslices selects the slice, i.e. (nslices = 8) the XCD: an
// XCD only ever reads ITS slice of the channels -- 4 200 pixels x C/8 channels of the image being pooled, 1.3 MB (512
// channels) to 5.4 MB (2 560) -- and consecutive ROIs (same image) run back to back on it, so the footprints of an image's
// proposals, which overlap heavily, are served by that XCD's L2.  The per-ROI sampling tables are built once per workgroup
// for all OH bin rows (they used to be rebuilt per bin row).
//
// elem_bytes / feat_ld: bytes per map element, elements between consecutive pixels of the map.  Every thread of the workgroup calls
// this (it holds barriers).
__device__ __forceinline__ NhwcRoiFrame nhwc_roi_frame(const float *__restrict__ rois, int N, int H, int W, int C, int PH, int PW, float scale,
                                                       int sampling_ratio, int aligned, int bin_stride, int OH, int OW, int64_t feat_ld,
                                                       unsigned elem_bytes, int nslices, int64_t R, const NhwcRoiLds &lds)
{
    NhwcRoiFrame f;
    // up to 8 slices: blockIdx % nslices = the slice = (round-robin dispatch) the XCD.  More than 8 (developer A/B,
    // LOCOV_ROIALIGN_SLICES): passes of 8 slices, every ROI of pass p before any of pass p + 1, so that an XCD still works on ONE
    // slice at a time.  The LAST pass may be ragged (nslices = 9, 12, ...: C = 576, 1536 on 64- / 128-channel slices): it holds
    // the remaining nslices - 8 * pass slices, every ROI of each
    const unsigned per = nslices > 8 ? 8u : (unsigned)nslices, per_pass = per * (unsigned)R;
    const unsigned pass = blockIdx.x / per_pass, rem = blockIdx.x - pass * per_pass;
    const unsigned left = (unsigned)nslices - pass * per, per_here = left < per ? left : per;
    const int slice = (int)(rem % per_here + pass * per);
    f.r = rem / per_here;
    const float *roi = rois + f.r * 5;
    f.b = (int)roi[0];
    f.valid_b = f.b >= 0 && f.b < N;
    const RoiGeom g = roi_geom(roi, scale, PH, PW, sampling_ratio, aligned);
    f.start_h = g.start_h; f.start_w = g.start_w; f.bin_h = g.bin_h; f.bin_w = g.bin_w;
    f.inv_count = 1.f / g.count;
    const int gh = f.gh = g.grid_h > 0 ? g.grid_h : 0;
    const int gw = f.gw = g.grid_w > 0 ? g.grid_w : 0;
    const int ny = OH * gh, nx = OW * gw;
    const bool use_lds = f.use_lds = ny <= kMaxAxisN && nx <= kMaxAxisN;
    const unsigned xstride = f.xstride = (unsigned)feat_ld * elem_bytes, ystride = f.ystride = (unsigned)W * xstride;
    if (use_lds) {
        for (int t = threadIdx.x; t < ny; t += kNhwcThreads)
            lds.ytab[t] = as_offsets(axis_sample_n(g.start_h, g.bin_h, (t / gh) * bin_stride, t % gh, gh, H), ystride);
        for (int t = threadIdx.x; t < nx; t += kNhwcThreads)
            lds.xtab[t] = as_offsets(axis_sample_n(g.start_w, g.bin_w, (t / gw) * bin_stride, t % gw, gw, W), xstride);
    }
    __syncthreads();

    // Separable form.  The bin value is sum_samples sum_taps wy*wx*F = sum_{pixel rows} sum_{pixel cols} Wy[y] Wx[x] F[y][x]
    // with Wy / Wx the per-PIXEL sums of the samples' bilinear weights.  Samples are at most one pixel apart
    // (grid = ceil(bin size)), so a bin touches at most (gh+1) x (gw+1) distinct pixels instead of 4*gh*gw taps:
    // 9 instead of 16 loads at a 2x2 grid, 25 instead of 64 at 4x4.  Same sum, re-associated (fp32 rounding only).
    const bool sep_try = use_lds && gh >= 1 && gw >= 1 && gh <= kSepGrid && gw <= kSepGrid && OW <= kSepCols && OH <= kSepCols;
    if (threadIdx.x == 0) *lds.sep_bad = 0;
    __syncthreads();
    if (sep_try && (int)threadIdx.x < OH + OW) {
        // thread oh: the y axis of bin row oh; thread OH + ow: the x axis of output column ow
        const bool is_y = (int)threadIdx.x < OH;
        const int idx_t = is_y ? (int)threadIdx.x : (int)threadIdx.x - OH, n = is_y ? gh : gw;
        const AxisSampleN *tab = is_y ? lds.ytab + idx_t * gh : lds.xtab + idx_t * gw;
        const unsigned stride = is_y ? ystride : xstride;
        float *pw = (is_y ? lds.ypw : lds.xpw) + idx_t * (kSepGrid + 1);
        int base = 0x7fffffff;
        for (int t = 0; t < n; t++)
            if (tab[t].wl != 0.f || tab[t].wh != 0.f) base = min(base, tab[t].lo);
        int num = 0;
        if (base != 0x7fffffff) {
            for (int k = 0; k <= n; k++) pw[k] = 0.f;
            for (int t = 0; t < n; t++) {
                const AxisSampleN sm = tab[t];
                if (sm.wl == 0.f && sm.wh == 0.f) continue;
                const int klo = (int)((unsigned)(sm.lo - base) / stride), khi = (int)((unsigned)(sm.hi - base) / stride);
                if (khi > n) {
                    *lds.sep_bad = 1;
                    break;
                }
                pw[klo] += sm.wh;
                pw[khi] += sm.wl;
                num = max(num, khi + 1);
            }
        }
        int (*pix)[2] = is_y ? lds.ypix : lds.xpix;
        pix[idx_t][0] = base == 0x7fffffff ? 0 : base;
        pix[idx_t][1] = num;
    }
    __syncthreads();
    f.separable = sep_try && !*lds.sep_bad;

    const int c4_all = C >> 2, c4s = (c4_all + nslices - 1) / nslices;
    f.q_lo = slice * c4s;
    f.q_hi = min(f.q_lo + c4s, c4_all);
    return f;
}

// channel slices per ROI of the even-grid pooler (roi_align_nhwc.hip)
int nhwc_slices(int C);

// roi_align_tiles.hip: the LDS-staged form of the contract (mode LOCOV_ROIALIGN_FAST)
int64_t roi_align_tiles_plan_bytes(int64_t R);
int launch_roi_align_tiles(const float *feat_nhwc, int N, int H, int W, int C, const float *rois, int64_t R, int PH, int PW,
                           float scale, int sampling_ratio, int aligned, void *plan_ws, float *out, hipStream_t s);

}  // namespace locov
