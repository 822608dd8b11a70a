// Device pieces shared by the two detection post-processing pipelines: detect.hip (candidates sorted in LDS, COCO-style
// thresholds) and detect_wide.hip (any candidate count, LVIS-style thresholds).  Both files are compiled with -ffp-contract=off:
// the box decoding and the IoU must round as the torch ops do.  The IoU test, the scans and the key layout are select_common.h's.
#pragma once
#include "select_common.h"

namespace locov {
namespace {     // (each pipeline's translation unit keeps its own copy of the kernel)

struct DetGeom {
    int n_img;
    int roff[LOCOV_LABEL_MAX_IMAGES + 1];                       // proposals of image i: rows [roff[i], roff[i + 1])
    float h[LOCOV_LABEL_MAX_IMAGES], w[LOCOV_LABEL_MAX_IMAGES];
};

__device__ __forceinline__ int det_image_of(const DetGeom &g, int r)
{
    int lo = 0, hi = g.n_img - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g.roff[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool det_finite(float v) { return fabsf(v) <= 3.402823466e38f; }        // false for NaN / inf

// Box2BoxTransform.apply_deltas of one delta quadruple on its proposal, rounded as the torch ops round (pre-clip)
__device__ __forceinline__ float4 det_apply_deltas(const float4 d, const float4 b, float inv_wx, float inv_wy, float inv_ww, float inv_wh,
                                                   float scale_clamp)
{
    const float widths = __fsub_rn(b.z, b.x), heights = __fsub_rn(b.w, b.y);
    const float ctr_x = __fadd_rn(b.x, __fmul_rn(0.5f, widths)), ctr_y = __fadd_rn(b.y, __fmul_rn(0.5f, heights));
    const float dx = __fmul_rn(d.x, inv_wx), dy = __fmul_rn(d.y, inv_wy);
    float dw = __fmul_rn(d.z, inv_ww), dh = __fmul_rn(d.w, inv_wh);
    dw = dw > scale_clamp ? scale_clamp : dw;                     // torch.clamp(max=): NaN stays NaN
    dh = dh > scale_clamp ? scale_clamp : dh;
    const float pcx = __fadd_rn(__fmul_rn(dx, widths), ctr_x), pcy = __fadd_rn(__fmul_rn(dy, heights), ctr_y);
    const float pw = __fmul_rn(expf(dw), widths), ph = __fmul_rn(expf(dh), heights);
    float4 o;
    o.x = __fsub_rn(pcx, __fmul_rn(0.5f, pw));
    o.y = __fsub_rn(pcy, __fmul_rn(0.5f, ph));
    o.z = __fadd_rn(pcx, __fmul_rn(0.5f, pw));
    o.w = __fadd_rn(pcy, __fmul_rn(0.5f, ph));
    return o;
}

__device__ __forceinline__ float4 det_clip(float4 o, float W, float H)         // Boxes.clip
{
    o.x = fminf(fmaxf(o.x, 0.f), W);
    o.y = fminf(fmaxf(o.y, 0.f), H);
    o.z = fminf(fmaxf(o.z, 0.f), W);
    o.w = fminf(fmaxf(o.w, 0.f), H);
    return o;
}

// Box2BoxTransform.apply_deltas (class-agnostic: one box per proposal) + Boxes.clip, rounded as the torch ops round
__global__ __launch_bounds__(256) void det_decode_clip_kernel(const float4 *__restrict__ deltas, const float4 *__restrict__ props, int R,
                                                              DetGeom g, float inv_wx, float inv_wy, float inv_ww, float inv_wh,
                                                              float scale_clamp, float4 *__restrict__ boxes, int *__restrict__ flags)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float4 o = det_apply_deltas(deltas[r], props[r], inv_wx, inv_wy, inv_ww, inv_wh, scale_clamp);
    if (!(det_finite(o.x) && det_finite(o.y) && det_finite(o.z) && det_finite(o.w))) atomicOr(flags, LOCOV_DETECT_FLAG_NONFINITE);
    const int img = det_image_of(g, r);
    boxes[r] = det_clip(o, g.w[img], g.h[img]);
}

// The same with a box per (proposal, class): deltas [R, ld] holds K quadruples a row, boxes [R, K].  A thread per (r, c); EVERY
// decoded box is checked for inf / NaN, a candidate's or not (the torch chain tests the whole [R, 4K] tensor).  R x K < 2^31.
__global__ __launch_bounds__(256) void det_decode_clip_cs_kernel(const float *__restrict__ deltas, int64_t ld, const float4 *__restrict__ props,
                                                                 int R, int K, DetGeom g, float inv_wx, float inv_wy, float inv_ww,
                                                                 float inv_wh, float scale_clamp, float4 *__restrict__ boxes,
                                                                 int *__restrict__ flags)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (unsigned)R * (unsigned)K) return;
    const int r = (int)(t / (unsigned)K), c = (int)(t - (unsigned)r * (unsigned)K);
    const float4 d = *reinterpret_cast<const float4 *>(deltas + (int64_t)r * ld + 4 * c);
    const float4 o = det_apply_deltas(d, props[r], inv_wx, inv_wy, inv_ww, inv_wh, scale_clamp);
    if (!(det_finite(o.x) && det_finite(o.y) && det_finite(o.z) && det_finite(o.w))) atomicOr(flags, LOCOV_DETECT_FLAG_NONFINITE);
    const int img = det_image_of(g, r);
    boxes[t] = det_clip(o, g.w[img], g.h[img]);
}

template <int kThreads>
__device__ __forceinline__ void det_bitonic_sort(unsigned long long *key, int P, int tid)
{
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += kThreads) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool ascending = (lo & size) == 0;
                const unsigned long long a = key[lo], b = key[hi];
                if ((a > b) == ascending) {
                    key[lo] = b;
                    key[hi] = a;
                }
            }
            __syncthreads();
        }
}

}  // namespace
// A call without a single proposal launches nothing: its n_images * topk slots are written as empty here (box 0, score 0, class -1,
// row -1), as the last kernel writes the slots behind an image's detections.  Null outputs (allowed when R == 0) are skipped.
static int det_fill_empty(const char *who, int n_images, int topk, float *out_boxes, float *out_scores, int64_t *out_classes, int64_t *out_rows,
                          hipStream_t s)
{
    const size_t n = (size_t)n_images * (size_t)topk;
    hipError_t e = hipSuccess;
    if (out_boxes && e == hipSuccess) e = hipMemsetAsync(out_boxes, 0, n * 16, s);
    if (out_scores && e == hipSuccess) e = hipMemsetAsync(out_scores, 0, n * 4, s);
    if (out_classes && e == hipSuccess) e = hipMemsetAsync(out_classes, 0xFF, n * 8, s);
    if (out_rows && e == hipSuccess) e = hipMemsetAsync(out_rows, 0xFF, n * 8, s);
    if (e != hipSuccess) return set_error(LOCOV_ERR_LAUNCH, "%s: memset: %s", who, hipGetErrorString(e));
    return LOCOV_OK;
}

}  // namespace locov
