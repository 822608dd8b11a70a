// The backward of the channels-last even-grid pooler (roi_align_nhwc.hip) for gfx950, two kernels behind locov_roi_align_nhwc_bwd:
// the scatter with fp32 atomics (any pooled size; roi_align_nhwc_bwd_kernel) and the ownership form without atomics (7 x 7 bins,
// ROI-major rows, multiples of 128 channels; roi_align_even_bwd_tiles_kernel), which is the default where it applies.
#include "roi_align_nhwc_common.h"

#include <cstdlib>

namespace locov {

// The adjoint of roi_align_nhwc_kernel (roi_align_nhwc.hip), on the same workgroup frame and sampling geometry: grad_rows holds the
// GRADIENT of the pooled rows (read; grad_ld elements between consecutive rows) and grad_feat the gradient of the channels-last fp32
// map [N,H,W,C], accumulated with fp32 hardware atomics (the caller zeroes it) -- what autograd needs when the LSM head trains
// through the even-grid pooler (roi_emb_heads.py:343 under autograd).
// Dynamic LDS of bwd_win_floats floats: the gradient window of a SMALL proposal (below).
__global__ __launch_bounds__(kNhwcThreads) void roi_align_nhwc_bwd_kernel(
    const float *__restrict__ grad_rows, int64_t grad_ld, float *__restrict__ grad_feat, int N, int H, int W, int C,
    const float *__restrict__ rois, int PH, int PW, float scale, int sampling_ratio, int aligned, int bin_stride, int OH, int OW,
    int pos_major, int nslices, int64_t R, int bwd_win_floats)
{
    extern __shared__ float bwd_win[];
    __shared__ AxisSampleN ytab[kMaxAxisN];
    __shared__ AxisSampleN xtab[kMaxAxisN];
    __shared__ float ypw[kSepCols * (kSepGrid + 1)];
    __shared__ float xpw[kSepCols * (kSepGrid + 1)];
    __shared__ int ypix[kSepCols][2];
    __shared__ int xpix[kSepCols][2];
    __shared__ int sep_bad;
    const NhwcRoiFrame f = nhwc_roi_frame(rois, N, H, W, C, PH, PW, scale, sampling_ratio, aligned, bin_stride, OH, OW, (int64_t)C,
                                          (unsigned)sizeof(float), nslices, R, NhwcRoiLds{ytab, xtab, ypw, xpw, ypix, xpix, &sep_bad});
    const float start_h = f.start_h, start_w = f.start_w, bin_h = f.bin_h, bin_w = f.bin_w, inv_count = f.inv_count;
    const int gh = f.gh, gw = f.gw, q_lo = f.q_lo;
    const unsigned xstride = f.xstride, ystride = f.ystride;
    const bool use_lds = f.use_lds, separable = f.separable, valid_b = f.valid_b;
    // (single channels, not quads: a wave's atomic instruction then covers 256 contiguous bytes = four full
    // 64-byte memory-side atomic requests instead of sixteen quarter-used ones)
    const int cn = 4 * (f.q_hi - q_lo);
    if (cn <= 0) return;
    char *gimg = reinterpret_cast<char *>(grad_feat + (int64_t)(valid_b ? f.b : 0) * H * W * C);
    // ROI-major: grad_rows[r][oh][ow][c]; position-major: grad_rows[oh][ow][r][c] (R rows per position)
    const int64_t bin_stride_out = pos_major ? R * grad_ld : grad_ld;
    const float *obase = pos_major ? grad_rows + f.r * grad_ld : grad_rows + (f.r * OH * (int64_t)OW) * grad_ld;
    const int nbins = OH * OW;
    // SMALL proposals (the 49 bins of a proposal below ~70 px land on at most 40 distinct map pixels, 4 pixels each): the bins'
    // contributions are first added up per pixel in an LDS window over the proposal's pixel rectangle (ds_add_f32), then every
    // touched (pixel, channel) costs ONE memory-side atomic instead of five to fifty on the same line.  The scatter of the LARGE
    // proposals, which bounds the launch, gets the atomic units the small ones no longer occupy: LSM step's launch 0.77 -> 0.60 ms,
    // STT's 1.44 -> 1.08 ms (the launcher's comment has the window-size sweep).
    __shared__ int rect[4];                            // {y0 (byte offset), x0 (byte offset), rows, columns}
    if (threadIdx.x == 0) {
        int ya = 0x7fffffff, yb = -1, xa = 0x7fffffff, xb = -1;
        if (separable && valid_b) {
            for (int i = 0; i < OH; i++)
                if (ypix[i][1] > 0) {
                    ya = min(ya, ypix[i][0]);
                    yb = max(yb, ypix[i][0] + (ypix[i][1] - 1) * (int)ystride);
                }
            for (int i = 0; i < OW; i++)
                if (xpix[i][1] > 0) {
                    xa = min(xa, xpix[i][0]);
                    xb = max(xb, xpix[i][0] + (xpix[i][1] - 1) * (int)xstride);
                }
        }
        const bool any = yb >= 0 && xb >= 0;
        rect[0] = ya;
        rect[1] = xa;
        rect[2] = any ? (yb - ya) / (int)ystride + 1 : 0;
        rect[3] = any ? (xb - xa) / (int)xstride + 1 : 0;
    }
    __syncthreads();
    // thread = (bin, channel), bins advanced incrementally (cn channels per bin): no integer division in the loops
    int bin = 0, oh = 0, ow = 0, cq = threadIdx.x;
    auto normalise = [&]() {
        while (cq >= cn) {
            cq -= cn;
            bin++;
            if (++ow == OW) {
                ow = 0;
                oh++;
            }
        }
    };
    const int wh = rect[2], ww = rect[3];
    if (wh > 0 && (int64_t)wh * ww * cn <= bwd_win_floats) {
        const int y0 = rect[0], x0 = rect[1];
        const int nwin = wh * ww * cn;
        for (int i = threadIdx.x; i < nwin; i += kNhwcThreads) bwd_win[i] = 0.f;
        __syncthreads();
        normalise();
        while (bin < nbins) {
            const float g = obase[(int64_t)bin * bin_stride_out + ((q_lo << 2) + cq)] * inv_count;
            const int nyp = ypix[oh][1], nxp = xpix[ow][1];
            const float *yw = ypw + oh * (kSepGrid + 1), *xw = xpw + ow * (kSepGrid + 1);
            const int py0 = (ypix[oh][0] - y0) / (int)ystride, px0 = (xpix[ow][0] - x0) / (int)xstride;
            for (int ky = 0; ky < nyp; ky++)
                for (int kx = 0; kx < nxp; kx++) {
                    const float w = yw[ky] * xw[kx];
                    if (w != 0.f)      // (the native LDS float add, ds_add_f32: the generic atomicAdd compiles to a compare-and-swap loop)
                        __builtin_amdgcn_ds_faddf((__attribute__((address_space(3))) float *)&bwd_win[((py0 + ky) * ww + px0 + kx) * cn + cq],
                                                  w * g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP, false);
                }
            cq += kNhwcThreads;
            normalise();
        }
        __syncthreads();
        // flush: consecutive threads = consecutive channels of one pixel (256-byte atomic instructions per wave)
        int pix = 0, c = threadIdx.x;
        while (true) {
            while (c >= cn) {
                c -= cn;
                pix++;
            }
            if (pix >= wh * ww) break;
            const float v = bwd_win[pix * cn + c];
            if (v != 0.f) {
                const int py = pix / ww, px = pix - py * ww;
                unsafeAtomicAdd(reinterpret_cast<float *>(gimg + (unsigned)y0 + (unsigned)py * ystride + (unsigned)x0 + (unsigned)px * xstride +
                                                          (unsigned)((q_lo << 2) + c) * (unsigned)sizeof(float)),
                                v);
            }
            c += kNhwcThreads;
        }
        return;
    }
    if (!valid_b) return;                              // (no image to add to)
    // every other proposal: each bin's contributions go straight to the map
    normalise();
    while (bin < nbins) {
        const int c = (q_lo << 2) + cq;
        const unsigned ch_off = (unsigned)c * (unsigned)sizeof(float);
        const float g = obase[(int64_t)bin * bin_stride_out + c] * inv_count;
        auto scatter = [&](unsigned off, float w) {
            if (w == 0.f) return;
            unsafeAtomicAdd(reinterpret_cast<float *>(gimg + off), w * g);
        };
        if (separable) {
            const int nyp = ypix[oh][1], nxp = xpix[ow][1];
            const unsigned y0 = (unsigned)ypix[oh][0] + (unsigned)xpix[ow][0] + ch_off;
            const float *yw = ypw + oh * (kSepGrid + 1), *xw = xpw + ow * (kSepGrid + 1);
            for (int ky = 0; ky < nyp; ky++)
                for (int kx = 0; kx < nxp; kx++) scatter(y0 + (unsigned)ky * ystride + (unsigned)kx * xstride, yw[ky] * xw[kx]);
        } else {
            for (int iy = 0; iy < gh; iy++) {
                const AxisSampleN ys = use_lds ? ytab[oh * gh + iy]
                                               : as_offsets(axis_sample_n(start_h, bin_h, oh * bin_stride, iy, gh, H), ystride);
                for (int ix = 0; ix < gw; ix++) {
                    const AxisSampleN xs = use_lds ? xtab[ow * gw + ix]
                                                   : as_offsets(axis_sample_n(start_w, bin_w, ow * bin_stride, ix, gw, W), xstride);
                    scatter((unsigned)ys.lo + (unsigned)xs.lo + ch_off, ys.wh * xs.wh);
                    scatter((unsigned)ys.lo + (unsigned)xs.hi + ch_off, ys.wh * xs.wl);
                    scatter((unsigned)ys.hi + (unsigned)xs.lo + ch_off, ys.wl * xs.wh);
                    scatter((unsigned)ys.hi + (unsigned)xs.hi + ch_off, ys.wl * xs.wl);
                }
            }
        }
        cq += kNhwcThreads;
        normalise();
    }
}

// ---- the even-grid pooler's backward by OWNERSHIP: one workgroup = one 8 x 8 pixel tile of one image x one 128-channel slice ---------
//
// roi_align_nhwc_bwd_kernel gives every (proposal, slice) a workgroup and adds each bin's contributions to the map with fp32
// memory-side atomics: 0.9-1.5 T atomic lanes per second, four times the scattered rate of the units (docs/experiments.md R5.23), and
// still 0.64 / 1.15 ms of the LSM / STT step for 0.16 / 0.3 GB of gradient rows.  Here the map is cut into tiles and a workgroup
// COLLECTS: it lists (in proposal order) the proposals of its image whose footprint reaches its tile, and for each of them every wave
// builds the separable per-pixel weights of the seven bin rows / columns on ITS eight pixel rows / four pixel columns (the sums of the
// samples' bilinear weights, as in the forward's separable form; no barrier between the waves inside the list), reads the gradient
// rows of the bins that reach the tile (its 128 channels: 512 contiguous bytes per bin) and adds  sum_oh w_y[oh][py] (sum_ow w_x[ow][px] g[oh][ow])  to REGISTER accumulators: a thread owns one
// channel and the 8 x 4 pixels of its column parity (two small dense products per proposal, at most 420 FMAs, instead of sparse updates).
// The tile is written (added to what the map gradient already holds) once: no atomics, and a sum whose order is the proposals'
// order -- the result is reproducible bit for bit.
constexpr int kBT = 8, kBwdCh = 128, kBwdList = 2048;

__global__ __launch_bounds__(256, 3) void roi_align_even_bwd_tiles_kernel(const float *__restrict__ grad_rows, int64_t grad_ld,
                                                                      const float *__restrict__ rois, int R, int N, int H, int W, int C, int PH,
                                                                      int PW, float scale, int sampling_ratio, int aligned, int bin_stride,
                                                                      float *__restrict__ grad_feat, int nslices, int tiles_x, int tiles_y)
{
    constexpr int OB = 7;
    __shared__ float wy[4][OB][kBT];                              // per WAVE: weights of the bin rows on the tile's pixel rows
    __shared__ float4 wx[4][OB];                                  // per wave: weights of the bin columns on the four tile columns of its parity
    __shared__ unsigned short list[kBwdList];
    __shared__ int wave_cnt[4], list_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t = blockIdx.x;
    const int slice = t % nslices;                                // (= the XCD under round-robin dispatch: an XCD reads ONE channel slice)
    t /= nslices;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, img = t / tiles_y;
    const int ty0 = ty * kBT, tx0 = tx * kBT, c0 = slice * kBwdCh;
    // this thread's accumulators: channel c, the 8 pixel rows x the 4 pixel columns of its parity
    float acc_r[kBT][kBT / 2];
#pragma unroll
    for (int py = 0; py < kBT; py++)
#pragma unroll
        for (int q = 0; q < kBT / 2; q++) acc_r[py][q] = 0.f;

    const int c = tid & (kBwdCh - 1), half = tid >> 7;

    for (int base = 0; base < R; base += kBwdList) {
        // ---- the proposals of this image whose footprint (conservatively: the box in map pixels, two pixels wider) reaches the tile,
        //      in proposal order (ballots + prefix counts: the order of the sums below must not depend on timing)
        if (tid == 0) list_n = 0;
        __syncthreads();
        const int stop = min(R, base + kBwdList);
        for (int r0 = base; r0 < stop; r0 += 256) {
            const int r = r0 + tid;
            bool ok = false;
            if (r < stop) {
                const float *roi = rois + (int64_t)r * 5;
                if ((int)roi[0] == img) {
                    const RoiGeom g = roi_geom(roi, scale, PH, PW, sampling_ratio, aligned);
                    // a, b: the box's two edges on an axis.  An inverted box under a fixed sampling ratio has a NEGATIVE bin size: its samples
                    // run from the start BACK to the end, so the footprint is [min, max] of the two, not [a, b].
                    // (NaN coordinates fail every comparison: such a proposal contributes nothing here, as its samples are invalid there)
                    auto reaches = [](float a, float b, int t0) {
                        const float lo = a <= b ? a : b, hi = a <= b ? b : a;
                        return hi + 2.f >= (float)t0 && lo - 2.f <= (float)(t0 + kBT);
                    };
                    ok = reaches(g.start_h, g.start_h + g.bin_h * (float)PH, ty0) && reaches(g.start_w, g.start_w + g.bin_w * (float)PW, tx0) &&
                         g.grid_h > 0 && g.grid_w > 0;
                }
            }
            const unsigned long long b = __ballot(ok);
            if (lane == 0) wave_cnt[wave] = __popcll(b);
            __syncthreads();
            int pos = list_n;
            for (int w = 0; w < wave; w++) pos += wave_cnt[w];
            if (ok) list[pos + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)(r - base);
            __syncthreads();
            if (tid == 0) list_n += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
            __syncthreads();
        }
        const int n_list = list_n;
        // Every WAVE builds the tables it uses (lanes 0-55: the rows, then the columns of its parity) in its own corner of LDS: the
        // four waves of the workgroup never wait for each other inside the list.  my / mx: bit 8 o + p set when bin row / column o has
        // a weight on tile row / column p (ballots: they stay in scalar registers).
        float (*wyw)[kBT] = wy[wave];
        float4 *wxw = wx[wave];
        for (int li = 0; li < n_list; li++) {
            const int r = base + (int)list[li];
            const RoiGeom g = roi_geom(rois + (int64_t)r * 5, scale, PH, PW, sampling_ratio, aligned);
            unsigned long long my, mx;
            {
                const int o = lane / kBT, p = lane % kBT;
                float w = 0.f;
                if (lane < OB * kBT)
                    for (int i = 0; i < g.grid_h; i++) {
                        const AxisSampleN sm = axis_sample_n(g.start_h, g.bin_h, o * bin_stride, i, g.grid_h, H);
                        w += (sm.lo == ty0 + p ? sm.wh : 0.f) + (sm.hi == ty0 + p ? sm.wl : 0.f);
                    }
                my = __ballot(w != 0.f);
                if (lane < OB * kBT) wyw[o][p] = w;
                w = 0.f;
                if (lane < OB * kBT)
                    for (int i = 0; i < g.grid_w; i++) {
                        const AxisSampleN sm = axis_sample_n(g.start_w, g.bin_w, o * bin_stride, i, g.grid_w, W);
                        w += (sm.lo == tx0 + p ? sm.wh : 0.f) + (sm.hi == tx0 + p ? sm.wl : 0.f);
                    }
                mx = __ballot(w != 0.f);
                if (lane < OB * kBT && (p & 1) == half) reinterpret_cast<float *>(&wxw[o])[p >> 1] = w;
            }
            // (the tables are read by OTHER lanes of this wave: order the LDS writes above and the reads below for the wave)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (my == 0 || mx == 0) continue;                      // (the conservative box reached the tile, no sample did)
            // ---- the gradient rows of the bins that reach the tile: all requested before any is used
            const float inv_count = 1.f / g.count;
            const float *grow = grad_rows + (int64_t)r * (OB * OB) * grad_ld + c0 + c;
            float gv[OB * OB];
#pragma unroll
            for (int oh = 0; oh < OB; oh++)
#pragma unroll
                for (int ow = 0; ow < OB; ow++)
                    gv[oh * OB + ow] = ((my >> (8 * oh)) & 0xffull) != 0 && ((mx >> (8 * ow)) & 0xffull) != 0 ? grow[(int64_t)(oh * OB + ow) * grad_ld] : 0.f;
            // ---- in registers:  acc[py][px] += sum_oh wy[oh][py] * (sum_ow wx[ow][px] * g[oh][ow])   for this thread's 8 x 4 pixels
#pragma unroll
            for (int oh = 0; oh < OB; oh++) {
                if (((my >> (8 * oh)) & 0xffull) == 0) continue;     // (wave-uniform: a bin row without a weight on this tile)
                float tq[kBT / 2] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ow = 0; ow < OB; ow++) {
                    const float4 w4 = wxw[ow];                        // this wave's four columns (its parity) of the column weights
                    const float gq = gv[oh * OB + ow];
                    tq[0] = fmaf(w4.x, gq, tq[0]);
                    tq[1] = fmaf(w4.y, gq, tq[1]);
                    tq[2] = fmaf(w4.z, gq, tq[2]);
                    tq[3] = fmaf(w4.w, gq, tq[3]);
                }
#pragma unroll
                for (int q = 0; q < kBT / 2; q++) tq[q] *= inv_count;
#pragma unroll
                for (int py = 0; py < kBT; py++) {
                    const float w = wyw[oh][py];
#pragma unroll
                    for (int q = 0; q < kBT / 2; q++) acc_r[py][q] = fmaf(w, tq[q], acc_r[py][q]);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next proposal's tables overwrite these)
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();                                            // (the list is rebuilt by the next pass)
    }
    __syncthreads();
    // ---- the tile, added to what the map gradient holds (a wave writes 256 contiguous bytes per pixel)
#pragma unroll
    for (int py = 0; py < kBT; py++)
#pragma unroll
        for (int q = 0; q < kBT / 2; q++) {
            const int y = ty0 + py, x = tx0 + 2 * q + half;
            const float v = acc_r[py][q];
            if (y < H && x < W && v != 0.f) grad_feat[(((int64_t)img * H + y) * W + x) * C + c0 + c] += v;
        }
}

}  // namespace locov

using namespace locov;

extern "C" {

int locov_roi_align_nhwc_bwd(const float *grad_rows, int64_t grad_ld, int N, int H, int W, int C, const float *rois, int64_t R,
                             int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio, int aligned, int bin_stride,
                             int pos_major, float *grad_feat, locov_stream_t stream)
{
    LOCOV_REQUIRE(grad_ld >= C && grad_ld % 4 == 0, "locov_roi_align_nhwc_bwd: grad_ld must be >= C and a multiple of 4");
    LOCOV_REQUIRE((int64_t)H * W * C * 4 < 0xffffffffLL, "locov_roi_align_nhwc_bwd: one image must stay below 4 GiB");
    LOCOV_REQUIRE(R >= 0 && N > 0 && C > 0 && H > 0 && W > 0 && pooled_h > 0 && pooled_w > 0, "locov_roi_align_nhwc_bwd: bad shape");
    LOCOV_REQUIRE(spatial_scale > 0.f, "locov_roi_align_nhwc_bwd: spatial_scale must be > 0");
    LOCOV_REQUIRE(bin_stride == 1 || bin_stride == 2, "locov_roi_align_nhwc_bwd: bin_stride must be 1 or 2");
    LOCOV_REQUIRE(C % 4 == 0, "locov_roi_align_nhwc_bwd: C must be a multiple of 4");
    if (R == 0) return LOCOV_OK;
    LOCOV_REQUIRE(grad_rows && rois && grad_feat, "locov_roi_align_nhwc_bwd: null pointer");
    LOCOV_REQUIRE(R <= 0x7fffffffLL, "locov_roi_align_nhwc_bwd: R too large");
    LOCOV_REQUIRE(((uintptr_t)grad_rows | (uintptr_t)grad_feat) % 16 == 0, "locov_roi_align_nhwc_bwd: misaligned pointer");
    const int OH = (pooled_h + bin_stride - 1) / bin_stride, OW = (pooled_w + bin_stride - 1) / bin_stride;
    // the ownership form (7 x 7 bins, ROI-major rows, 128-channel slices): developer A/B LOCOV_POOL_BWD_TILES=0 -> the scatter below
    {
        const char *te = getenv("LOCOV_POOL_BWD_TILES");      // (read per launch: tests flip it)
        if ((!te || atoi(te) != 0) && OH == 7 && OW == 7 && !pos_major && C % kBwdCh == 0) {
            const int tiles_x = (W + kBT - 1) / kBT, tiles_y = (H + kBT - 1) / kBT, ns = C / kBwdCh;
            const int64_t wgs = (int64_t)N * tiles_x * tiles_y * ns;
            LOCOV_REQUIRE(wgs <= 0x7fffffffLL, "locov_roi_align_nhwc_bwd: map too large");
            hipLaunchKernelGGL(roi_align_even_bwd_tiles_kernel, dim3((unsigned)wgs), dim3(256), 0, as_stream(stream), grad_rows, grad_ld, rois, (int)R,
                               N, H, W, C, pooled_h, pooled_w, spatial_scale, sampling_ratio, aligned, bin_stride, grad_feat, ns, tiles_x, tiles_y);
            return check_launch("locov_roi_align_nhwc_bwd (tiles)");
        }
    }
    // (slices of at most 128 channels where C allows: the 20 KB gradient window then holds the 40 pixels of a proposal below ~70 px)
    int nslices = nhwc_slices(C);
    while (nslices < 8 && C / (2 * nslices) >= 128 && (C >> 2) % (2 * nslices) == 0) nslices *= 2;
    LOCOV_REQUIRE(R * nslices <= 0x7fffffffLL, "locov_roi_align_nhwc_bwd: R too large");
    dim3 grid((unsigned)(R * nslices));
    // Window size: measured on the LSM step's launch (800 proposals, 4 images, 1024 channels) / the STT step's (1536 proposals, 3 images),
    // tools/ab_pool_bwd_sizes.py: none 0.771 / 1.437 ms, 16 KB 0.615 / 1.111, 20 KB 0.603 / 1.084, 24 KB 0.608 / 1.101, 32 KB 0.667 / 1.234,
    // 64 KB 0.835 -- a larger window takes more proposals but fewer workgroups per CU, and the window path needs the occupancy its two
    // barriers cost.  (Proposals of one small size class ALONE run slower through the window, 0.55 -> 0.71 ms: what it buys is room at the
    // memory-side atomic units for the large proposals' scatter, which bounds the launch.)
    // developer A/B: LOCOV_POOL_BWD_WINDOW=<bytes>, 0 -> every proposal scatters straight to memory
    const char *we = getenv("LOCOV_POOL_BWD_WINDOW");          // (read per launch: tests flip it)
    const int win_bytes = we ? atoi(we) : 20480;
    // (a refusal is no error here -- every proposal then scatters straight to memory -- so the error text stays as it is: no `who`)
    static std::atomic<int> window_lds[kMaxDevices];
    const bool attr_ok = raise_dynamic_lds(window_lds, reinterpret_cast<const void *>(&roi_align_nhwc_bwd_kernel), 65536, nullptr) == LOCOV_OK;
    const int wb = attr_ok && win_bytes > 0 ? (win_bytes < 65536 ? win_bytes : 65536) : 0;
    hipLaunchKernelGGL(roi_align_nhwc_bwd_kernel, grid, dim3(kNhwcThreads), (size_t)wb, as_stream(stream), grad_rows, grad_ld, grad_feat, N, H,
                       W, C, rois, pooled_h, pooled_w, spatial_scale, sampling_ratio, aligned, bin_stride, OH, OW, pos_major, nslices, R, wb / 4);
    return check_launch("locov_roi_align_nhwc_bwd");
}

}  // extern "C"
