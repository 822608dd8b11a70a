// Channels-last ROIAlign for gfx950: channels on the lanes.
//
// Same arithmetic as roi_align.hip (torchvision roi_align semantics, reached from
// ovr/modeling/roi_heads/roi_emb_heads.py:243-245) but on an [N,H,W,C] feature map: the four
// bilinear taps of a sample are then four contiguous C-vectors, so every wave-level load is a
// fully coalesced run of 16 B (fp32) / 8 B (bf16) per lane and the interpolation weights are
// wave-uniform LDS broadcasts.  The output [R, oh, ow, C] is row-major "pixels x channels" --
// directly the A operand of Res5's first 1x1 convolutions as an NT GEMM.
//
// bin_stride = 2 evaluates only even bins (ph, pw even): with STRIDE_IN_1X1=True both stride-2
// 1x1 convs of Res5 block 0 (roi_emb_heads.py:217-241) read exactly those positions of the
// 14x14 tile, so 3/4 of the pooler's output bytes are never produced.
#include "roi_align_nhwc_common.h"
#include "winograd_transform.h"

#include <cstdlib>
#include <type_traits>

namespace locov {

#ifndef LOCOV_POOLWINO_NT
#define LOCOV_POOLWINO_NT 0                                // the WINO pooler's transform-domain stores (developer A/B)
#endif

// The even-grid pooler, forward: one workgroup = one ROI x one channel slice, all OH x OW bins (nhwc_roi_frame of
// roi_align_nhwc_common.h has the why of the slices; the adjoint with the same frame is roi_align_nhwc_bwd_kernel).
// feat_ld = elements between consecutive pixels of the map (>= C: the C channels may be a column block
// of a wider per-pixel vector).  ch_scale / ch_shift / relu: optional per-channel affine + ReLU applied to
// the pooled value -- ROIAlign is linear, so a 1x1 convolution can run on the MAP (once per pixel instead
// of once per ROI bin) and its FrozenBN + ReLU are applied here, after the pooling.
// WINO = true (fp32, 7 x 7 strided bins, slices of at most 64 channels): the pooled + FrozenBN + ReLU values are the input of a 3x3
// convolution evaluated in the Winograd domain (block 0's conv2).  They are kept in LDS ([49][64]) instead of being stored, and
// the workgroup writes their input transform V [121][R][C] (`out`, split layout x v_scale) itself -- wino_in_fy of
// winograd_transform.h, the bits wino_input_kernel<false, true> would have produced from the stored rows.
// WINO = the slice width in channels (0: not the WINO form).  128 where C allows it: the transform phase's lane = channel pair then
// fills its waves (64 pairs), a wave's store is a 512-byte run, and a 512-channel map makes 4 slices (two XCDs share one: 2.15 MB per
// image, still inside L2) -- block 0's pooler + conv2 2.73 -> 2.60 ms at 8 000 proposals (tools/attic/dbg_fuse_pool.py); 64 otherwise.
template <typename TIn, typename TOut, int WINO = 0>
__global__ __launch_bounds__(kNhwcThreads, WINO == 64 ? 6 : WINO ? 4 : 1) void roi_align_nhwc_kernel(
    const TIn *__restrict__ feat, int N, int H, int W, int C, const float *__restrict__ rois, int PH, int PW,
    float scale, int sampling_ratio, int aligned, int bin_stride, int OH, int OW, int pos_major,
    TOut *__restrict__ out, int64_t out_ld, int64_t feat_ld, const float *__restrict__ ch_scale,
    const float *__restrict__ ch_shift, int relu, int nslices, int64_t R, float v_scale = 1.f, unsigned *overflow = nullptr)
{
    constexpr int kWinoPitch = WINO + 4;
    __shared__ float wino_tile_s[WINO ? 49 * kWinoPitch : 1];
    float *const wino_tile = wino_tile_s;
    __shared__ AxisSampleN ytab[kMaxAxisN];
    __shared__ AxisSampleN xtab[kMaxAxisN];
    __shared__ float ypw[kSepCols * (kSepGrid + 1)];
    __shared__ float xpw[kSepCols * (kSepGrid + 1)];
    __shared__ int ypix[kSepCols][2];
    __shared__ int xpix[kSepCols][2];
    __shared__ int sep_bad;
    const NhwcRoiFrame f = nhwc_roi_frame(rois, N, H, W, C, PH, PW, scale, sampling_ratio, aligned, bin_stride, OH, OW, feat_ld,
                                          (unsigned)sizeof(TIn), nslices, R, NhwcRoiLds{ytab, xtab, ypw, xpw, ypix, xpix, &sep_bad});
    const float start_h = f.start_h, start_w = f.start_w, bin_h = f.bin_h, bin_w = f.bin_w, inv_count = f.inv_count;
    const int gh = f.gh, gw = f.gw, q_lo = f.q_lo;
    const unsigned xstride = f.xstride, ystride = f.ystride;
    const bool use_lds = f.use_lds, separable = f.separable, valid_b = f.valid_b;
    const int c4n = f.q_hi - q_lo;                               // channel quads of this workgroup's slice
    if (c4n <= 0) return;
    const TIn *img = feat + (int64_t)(valid_b ? f.b : 0) * H * W * feat_ld;
    const __amdgpu_buffer_rsrc_t img_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<TIn *>(img), 0, (unsigned)H * ystride, 0x00020000);
    // ROI-major: out[r][oh][ow][c]; position-major: out[oh][ow][r][c] (R rows per position)
    // (out_ld = elements between consecutive pixel rows, >= C: the rows may be a column block of a wider matrix)
    const int64_t bin_stride_out = pos_major ? R * out_ld : out_ld;
    TOut *obase = pos_major ? out + f.r * out_ld : out + (f.r * OH * (int64_t)OW) * out_ld;
    const int nbins = OH * OW;
    // (bin, channel quad) of this thread: advanced incrementally, no integer division in the loop
    int bin = 0, oh = 0, ow = 0, cq = threadIdx.x;
    auto normalise = [&]() {
        while (cq >= c4n) {
            cq -= c4n;
            bin++;
            if (++ow == OW) {
                ow = 0;
                oh++;
            }
        }
    };
    normalise();
    while (bin < nbins) {
        const int c = (q_lo + cq) << 2;
        const unsigned ch_off = (unsigned)c * (unsigned)sizeof(TIn);
        TOut *optr = obase + (int64_t)bin * bin_stride_out + c;
        const float *yw = ypw + oh * (kSepGrid + 1);
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        if (valid_b && separable) {
            const int nyp = ypix[oh][1], nxp = xpix[ow][1];
            const unsigned x0 = (unsigned)xpix[ow][0] + ch_off;
            const float *xw = xpw + ow * (kSepGrid + 1);
            // the gather is latency-bound: up to 8 pixels are in flight per lane before any is consumed
            // (pixel counters are wave-uniform -> scalar registers)
            const unsigned y0 = (unsigned)ypix[oh][0] + x0;
            const int npix = nyp * nxp;
            int ky = 0, kx = 0;
            auto group = [&](auto nu_tag) __attribute__((always_inline)) {
                constexpr int NU = decltype(nu_tag)::value;
                float4 v[NU];
                float wgt[NU];
#pragma unroll
                for (int u = 0; u < NU; u++) {
                    wgt[u] = yw[ky] * xw[kx];
                    v[u] = tap4(img_rsrc, y0 + (unsigned)ky * ystride + (unsigned)kx * xstride, (TIn *)nullptr);
                    if (++kx == nxp) {
                        kx = 0;
                        ky++;
                    }
                }
#pragma unroll
                for (int u = 0; u < NU; u++) {
                    acc.x = fmaf(wgt[u], v[u].x, acc.x);
                    acc.y = fmaf(wgt[u], v[u].y, acc.y);
                    acc.z = fmaf(wgt[u], v[u].z, acc.z);
                    acc.w = fmaf(wgt[u], v[u].w, acc.w);
                }
            };
            int p = 0;
            for (; p + 8 <= npix; p += 8) group(std::integral_constant<int, 8>{});
            const int rem = npix - p;                            // 0..7: binary decomposition
            if (rem & 4) group(std::integral_constant<int, 4>{});
            if (rem & 2) group(std::integral_constant<int, 2>{});
            if (rem & 1) group(std::integral_constant<int, 1>{});
        } else if (valid_b) {
            for (int iy = 0; iy < gh; iy++) {
                const AxisSampleN ys = use_lds ? ytab[oh * gh + iy]
                                               : as_offsets(axis_sample_n(start_h, bin_h, oh * bin_stride, iy, gh, H), ystride);
                const unsigned ylo = (unsigned)ys.lo + ch_off, yhi = (unsigned)ys.hi + ch_off;
                for (int ix = 0; ix < gw; ix++) {
                    const AxisSampleN xs = use_lds ? xtab[ow * gw + ix]
                                                   : as_offsets(axis_sample_n(start_w, bin_w, ow * bin_stride, ix, gw, W), xstride);
                    const float w1 = ys.wh * xs.wh, w2 = ys.wh * xs.wl, w3 = ys.wl * xs.wh, w4 = ys.wl * xs.wl;
                    const float4 v1 = tap4(img_rsrc, ylo + (unsigned)xs.lo, (TIn *)nullptr);
                    const float4 v2 = tap4(img_rsrc, ylo + (unsigned)xs.hi, (TIn *)nullptr);
                    const float4 v3 = tap4(img_rsrc, yhi + (unsigned)xs.lo, (TIn *)nullptr);
                    const float4 v4 = tap4(img_rsrc, yhi + (unsigned)xs.hi, (TIn *)nullptr);
                    // this file is built with -ffp-contract=off (exact coordinates); the
                    // accumulation asks for FMA explicitly
                    acc.x = fmaf(w4, v4.x, fmaf(w3, v3.x, fmaf(w2, v2.x, fmaf(w1, v1.x, acc.x))));
                    acc.y = fmaf(w4, v4.y, fmaf(w3, v3.y, fmaf(w2, v2.y, fmaf(w1, v1.y, acc.y))));
                    acc.z = fmaf(w4, v4.z, fmaf(w3, v3.z, fmaf(w2, v2.z, fmaf(w1, v1.z, acc.z))));
                    acc.w = fmaf(w4, v4.w, fmaf(w3, v3.w, fmaf(w2, v2.w, fmaf(w1, v1.w, acc.w))));
                }
            }
        }
        acc.x *= inv_count; acc.y *= inv_count; acc.z *= inv_count; acc.w *= inv_count;
        if (ch_scale) {
            const float4 sc = *reinterpret_cast<const float4 *>(ch_scale + c);
            acc.x *= sc.x; acc.y *= sc.y; acc.z *= sc.z; acc.w *= sc.w;
        }
        if (ch_shift) {
            const float4 sh = *reinterpret_cast<const float4 *>(ch_shift + c);
            acc.x += sh.x; acc.y += sh.y; acc.z += sh.z; acc.w += sh.w;
        }
        if (relu) {
            acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
        }
        if constexpr (WINO)
            *reinterpret_cast<float4 *>(wino_tile + bin * kWinoPitch + 4 * cq) = acc;
        else
            store4_out(optr, acc);
        cq += kNhwcThreads;
        normalise();
    }
    if constexpr (WINO != 0 && std::is_same<TOut, float>::value) {
        __syncthreads();
        // wave w takes the rows fy = w, w + 4, w + 8 of the transform; lane = channel pair of the slice (a slice has an even
        // number of pairs: lanes trade words in pairs)
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int npairs = 2 * c4n;
        float amax = 0.f;
        if (lane < npairs) {
            const int c = (q_lo << 2) + 2 * lane;
            const float *patch = wino_tile + 2 * lane;
            const int64_t fstride = R * C;
            float *vrow = reinterpret_cast<float *>(out) + f.r * C;
            auto load = [&](int y, int xx) __attribute__((always_inline)) {
                return *reinterpret_cast<const f32x2 *>(patch + (y * 7 + xx) * kWinoPitch);
            };
            auto unit = [&](auto fy_tag) __attribute__((always_inline)) {
                constexpr int FY = decltype(fy_tag)::value;
                wino_in_fy<false, FY>(load, [&](int fx, f32x2 a) __attribute__((always_inline)) {
                    amax = fmaxf(fmaxf(amax, fabsf(a[0])), fabsf(a[1]));
                    store_split_pair_policy<LOCOV_POOLWINO_NT != 0>(vrow + (int64_t)(FY * wino::NF + fx) * fstride, c, a, v_scale);
                });
                __builtin_amdgcn_sched_barrier(0);             // one row of the transform at a time: ~80 live registers, not 11 rows' worth
            };
            using std::integral_constant;
            if (wave == 0) {
                unit(integral_constant<int, 0>{}); unit(integral_constant<int, 4>{}); unit(integral_constant<int, 8>{});
            } else if (wave == 1) {
                unit(integral_constant<int, 1>{}); unit(integral_constant<int, 5>{}); unit(integral_constant<int, 9>{});
            } else if (wave == 2) {
                unit(integral_constant<int, 2>{}); unit(integral_constant<int, 6>{}); unit(integral_constant<int, 10>{});
            } else {
                unit(integral_constant<int, 3>{}); unit(integral_constant<int, 7>{});
            }
        }
        if (overflow != nullptr && amax * v_scale >= 65504.f) atomicOr(overflow, 1u);
    }
}

// [N,C,H,W] f32 -> [N,H,W,C] (f32 / bf16): 64x64 LDS-tiled transpose of the [C, HW] matrix of
// each image (coalesced on both sides; +1 padding keeps the column reads conflict-free).
template <typename TOut>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float *__restrict__ in, int C, int HW,
                                                           TOut *__restrict__ out)
{
    __shared__ float tile[64][65];
    const int n = blockIdx.z;
    const int c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
    const float *src = in + (int64_t)n * C * HW;
    TOut *dst = out + (int64_t)n * C * HW;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, p = p0 + tx;
        tile[i][tx] = (c < C && p < HW) ? src[(int64_t)c * HW + p] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int p = p0 + i, c = c0 + tx;
        if (p < HW && c < C) dst[(int64_t)p * C + c] = (TOut)tile[tx][i];
    }
}

// channel slices per ROI of roi_align_nhwc_kernel: a power of two up to 8 (= one per XCD, see the kernel) that still leaves a
// slice at least 64 channel quads wide, so that a wave stays inside one bin (wave-uniform pixel loops): 2 048+ channels -> 8,
// 1 024 -> 4, 512 -> 2, fewer -> 1
int nhwc_slices(int C)
{
    static const int forced = [] { const char *e = getenv("LOCOV_ROIALIGN_SLICES"); return e ? atoi(e) : 0; }();
    if (forced > 0) return forced;
    int n = 1;
    while (n < 8 && (C >> 2) / (2 * n) >= 64) n *= 2;
    return n;
}

// ROIAlign (even bins of a 14 x 14 pooler = 7 x 7, ROI-major) + per-channel affine + ReLU + Winograd input transform in one launch
bool roi_align_nhwc_wino_applicable(int C, int64_t R)
{
    const char *fe = getenv("LOCOV_WINO_FUSE");            // developer A/B / tests (read per launch): 0 = never
    if (fe && atoi(fe) == 0) return false;
    return C % 64 == 0 && R * (C / 64) <= 0x7fffffffLL;
}

int launch_roi_align_nhwc_wino(const float *feat, int N, int H, int W, int C, int64_t feat_ld, const float *rois, int64_t R, int pooled,
                               float spatial_scale, int sampling_ratio, int aligned, const float *ch_scale, const float *ch_shift, int relu,
                               float *V, float v_scale, unsigned *overflow, hipStream_t s)
{
    // (LOCOV_WINO_SLICE_CH: developer A/B of the slice width)
    static const int forced = [] { const char *e = getenv("LOCOV_WINO_SLICE_CH"); return e ? atoi(e) : 0; }();
    const int width = forced == 64 || forced == 128 ? (C % forced == 0 ? forced : 64) : (C % 128 == 0 ? 128 : 64);
    const int nslices = C / width;
    if (width == 128)
        hipLaunchKernelGGL((roi_align_nhwc_kernel<float, float, 128>), dim3((unsigned)(R * nslices)), dim3(kNhwcThreads), 0, s, feat, N, H, W, C,
                           rois, pooled, pooled, spatial_scale, sampling_ratio, aligned, 2, (pooled + 1) / 2, (pooled + 1) / 2, 0, V, (int64_t)C, feat_ld,
                           ch_scale, ch_shift, relu, nslices, R, v_scale, overflow);
    else
        hipLaunchKernelGGL((roi_align_nhwc_kernel<float, float, 64>), dim3((unsigned)(R * nslices)), dim3(kNhwcThreads), 0, s, feat, N, H, W, C,
                           rois, pooled, pooled, spatial_scale, sampling_ratio, aligned, 2, (pooled + 1) / 2, (pooled + 1) / 2, 0, V, (int64_t)C, feat_ld,
                           ch_scale, ch_shift, relu, nslices, R, v_scale, overflow);
    return check_launch("locov_roi_align_winograd_conv3x3_f32_split (ROIAlign + input transform)");
}

}  // namespace locov

using namespace locov;

extern "C" {

int locov_nchw_to_nhwc(const float *in, int N, int C, int H, int W, void *out, int out_dtype, locov_stream_t stream)
{
    LOCOV_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "locov_nchw_to_nhwc: bad shape");
    LOCOV_REQUIRE(in && out, "locov_nchw_to_nhwc: null pointer");
    LOCOV_REQUIRE(out_dtype == LOCOV_F32 || out_dtype == LOCOV_BF16, "locov_nchw_to_nhwc: bad out_dtype %d", out_dtype);
    const int HW = H * W;
    dim3 grid((unsigned)ceil_div(HW, 64), (unsigned)ceil_div(C, 64), (unsigned)N);
    if (out_dtype == LOCOV_F32)
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, grid, dim3(256), 0, as_stream(stream), in, C, HW, (float *)out);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<__bf16>, grid, dim3(256), 0, as_stream(stream), in, C, HW,
                           (__bf16 *)out);
    return check_launch("locov_nchw_to_nhwc");
}

int locov_roi_align_nhwc_fwd(const void *feat, int feat_dtype, int N, int H, int W, int C, const float *rois,
                             int64_t R, int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio,
                             int aligned, int bin_stride, int pos_major, void *out, int out_dtype, locov_stream_t stream)
{
    return locov_roi_align_nhwc_ld_fwd(feat, feat_dtype, N, H, W, C, rois, R, pooled_h, pooled_w, spatial_scale,
                                       sampling_ratio, aligned, bin_stride, pos_major, out, (int64_t)C, out_dtype, stream);
}

int locov_roi_align_nhwc_ld_fwd(const void *feat, int feat_dtype, int N, int H, int W, int C, const float *rois,
                                int64_t R, int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio,
                                int aligned, int bin_stride, int pos_major, void *out, int64_t out_ld, int out_dtype,
                                locov_stream_t stream)
{
    return locov_roi_align_nhwc_affine_fwd(feat, feat_dtype, N, H, W, C, (int64_t)C, rois, R, pooled_h, pooled_w,
                                           spatial_scale, sampling_ratio, aligned, bin_stride, pos_major, nullptr, nullptr, 0,
                                           out, out_ld, out_dtype, stream);
}

int locov_roi_align_nhwc_affine_fwd(const void *feat, int feat_dtype, int N, int H, int W, int C, int64_t feat_ld,
                                    const float *rois, int64_t R, int pooled_h, int pooled_w, float spatial_scale,
                                    int sampling_ratio, int aligned, int bin_stride, int pos_major, const float *ch_scale,
                                    const float *ch_shift, int relu, void *out, int64_t out_ld, int out_dtype,
                                    locov_stream_t stream)
{
    LOCOV_REQUIRE(out_ld >= C && out_ld % 4 == 0, "locov_roi_align_nhwc_fwd: out_ld must be >= C and a multiple of 4");
    LOCOV_REQUIRE(feat_ld >= C && feat_ld % 4 == 0, "locov_roi_align_nhwc_fwd: feat_ld must be >= C and a multiple of 4");
    LOCOV_REQUIRE((int64_t)H * W * feat_ld * 4 < 0xffffffffLL, "locov_roi_align_nhwc_fwd: one image must stay below 4 GiB");
    LOCOV_REQUIRE(R >= 0, "locov_roi_align_nhwc_fwd: R < 0");
    LOCOV_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "locov_roi_align_nhwc_fwd: bad feature shape");
    LOCOV_REQUIRE(pooled_h > 0 && pooled_w > 0, "locov_roi_align_nhwc_fwd: bad pooled size");
    LOCOV_REQUIRE(spatial_scale > 0.f, "locov_roi_align_nhwc_fwd: spatial_scale must be > 0");
    LOCOV_REQUIRE(bin_stride == 1 || bin_stride == 2, "locov_roi_align_nhwc_fwd: bin_stride must be 1 or 2");
    LOCOV_REQUIRE(C % 4 == 0, "locov_roi_align_nhwc_fwd: C must be a multiple of 4");
    LOCOV_REQUIRE((feat_dtype == LOCOV_F32 || feat_dtype == LOCOV_BF16) && (out_dtype == LOCOV_F32 || out_dtype == LOCOV_BF16),
                  "locov_roi_align_nhwc_fwd: bad dtype");
    if (R == 0) return LOCOV_OK;
    LOCOV_REQUIRE(feat && rois && out, "locov_roi_align_nhwc_fwd: null pointer");
    LOCOV_REQUIRE(R <= 0x7fffffffLL, "locov_roi_align_nhwc_fwd: R too large");
    const int OH = (pooled_h + bin_stride - 1) / bin_stride, OW = (pooled_w + bin_stride - 1) / bin_stride;
    const int nslices = nhwc_slices(C);
    LOCOV_REQUIRE(R * nslices <= 0x7fffffffLL, "locov_roi_align_nhwc_fwd: R too large");
    dim3 grid((unsigned)(R * nslices));
    hipStream_t s = as_stream(stream);
#define LOCOV_LAUNCH_NHWC(TI, TO)                                                                                   \
    hipLaunchKernelGGL((roi_align_nhwc_kernel<TI, TO>), grid, dim3(kNhwcThreads), 0, s, (const TI *)feat, N, H, W, C, \
                       rois, pooled_h, pooled_w, spatial_scale, sampling_ratio, aligned, bin_stride, OH, OW, pos_major, (TO *)out, out_ld, \
                       feat_ld, ch_scale, ch_shift, relu, nslices, R)
    if (feat_dtype == LOCOV_F32 && out_dtype == LOCOV_F32) LOCOV_LAUNCH_NHWC(float, float);
    else if (feat_dtype == LOCOV_F32 && out_dtype == LOCOV_BF16) LOCOV_LAUNCH_NHWC(float, __bf16);
    else if (feat_dtype == LOCOV_BF16 && out_dtype == LOCOV_F32) LOCOV_LAUNCH_NHWC(__bf16, float);
    else LOCOV_LAUNCH_NHWC(__bf16, __bf16);
#undef LOCOV_LAUNCH_NHWC
    return check_launch("locov_roi_align_nhwc_fwd");
}

}  // extern "C"
