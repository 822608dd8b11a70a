// The RPN's training half on the device: anchor labelling, the 256-sample draw and the two losses with their gradients -- five
// launches for a batch, fixed output shapes, no host read.
//
// What Detectron2's RPN.label_and_sample_anchors / RPN.losses do per image with torch ops (a [num_gt, HWA] IoU matrix, the Matcher
// with allow_low_quality_matches, Boxes.inside_box, subsample_labels' two nonzero + randperm pairs, boolean-mask gathers for
// binary_cross_entropy_with_logits and smooth_l1_loss), stated as three operations in include/locov_hip.h.  The anchors of a feature
// level are the same for every image of the batch: [hwa, 4], flat index i = (y W + x) A + a.
//
//   rpn_gt_max_kernel   phase A of the labelling: per ground-truth box the maximum IoU over ALL anchors (what the low-quality rule
//                       compares against).  A block holds 1 024 anchors in registers and walks the boxes; per box a wave maximum, an
//                       LDS maximum per block, ONE global atomic max per (block, box) on the IoU's bit pattern (IoU >= 0: the unsigned
//                       order is the float order; a maximum does not depend on the order of arrival)
//   rpn_label_kernel    phase B: a thread per (image, anchor) walks ITS image's boxes: first maximum, the Matcher's interval label, the
//                       promotion (iou == a box's phase-A maximum), the boundary test; writes the pre-sampling label, the matched box
//                       and the per-image sizes of the two populations (a wave ballot, one integer atomic add per wave)
//   rpn_sample_kernel   a workgroup per (image, population): radix select (11 bits a pass) of the k-th smallest key among the
//                       population's float64 uniforms -- positive doubles order as their bit patterns -- and one ordered sweep that
//                       keeps the keys below the cut and the first of the keys on it in anchor order; everything else becomes -1
//   rpn_loss_kernel     a thread per (image, anchor): the objectness term and its gradient for labels >= 0, get_deltas + smooth-L1
//                       and its gradient for labels == 1, zeros elsewhere; fp64 partials per block, summed in block order by
//                       rpn_loss_finish_kernel (no float atomics: the same inputs give the same bits)
//
// Both phases of the labelling take the IoU from select_common.h's box_pairwise_iou (the promotion's `==` needs the two to round
// identically; this file is built with -ffp-contract=off), and the sampler's digit pick is that header's radix_pick.
#include "box_delta_common.h"
#include "reduce_common.h"
#include "select_common.h"

namespace locov {

constexpr int kRtThreads = 256;
constexpr int kRtPerThread = 4;                                  // anchors a thread of phase A holds
constexpr int kRtGtChunk = 256;                                  // ground-truth boxes per LDS round of phase A
constexpr int kRtMaxAnchors = 1 << 22;
constexpr int kRtSelThreads = 1024, kRtSelWaves = kRtSelThreads / kWave;
constexpr int kRtDigit = 11, kRtBins = 1 << kRtDigit, kRtPasses = 6;             // 64-bit keys: 9 + 5 x 11 bits

__global__ __launch_bounds__(kRtThreads) void rpn_gt_max_kernel(const float4 *__restrict__ anchors, int hwa, const float4 *__restrict__ gt,
                                                                int n_gt, unsigned *__restrict__ slots)
{
    __shared__ unsigned smax[kRtGtChunk];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int i0 = blockIdx.x * (kRtThreads * kRtPerThread);
    float4 b[kRtPerThread];
    bool live[kRtPerThread];
#pragma unroll
    for (int k = 0; k < kRtPerThread; k++) {
        const int i = i0 + k * kRtThreads + tid;
        live[k] = i < hwa;
        b[k] = live[k] ? anchors[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int g0 = 0; g0 < n_gt; g0 += kRtGtChunk) {
        const int ng = n_gt - g0 < kRtGtChunk ? n_gt - g0 : kRtGtChunk;
        smax[tid] = 0u;
        __syncthreads();
        for (int j = 0; j < ng; j++) {
            const float4 a = gt[g0 + j];
            unsigned m = 0u;
#pragma unroll
            for (int k = 0; k < kRtPerThread; k++) {
                const unsigned q = live[k] ? __float_as_uint(box_pairwise_iou(a, b[k])) : 0u;
                m = q > m ? q : m;
            }
            m = wave_reduce(m, MaxOp());
            if (lane == 0 && m != 0u) atomicMax(&smax[j], m);            // (an LDS integer maximum: the order does not matter)
        }
        __syncthreads();
        if (tid < ng && smax[tid] != 0u) atomicMax(&slots[g0 + tid], smax[tid]);
        __syncthreads();
    }
}

struct RpnLabelGeom {
    int goff[LOCOV_LABEL_MAX_IMAGES + 1];            // ground truth of image i: rows [goff[i], goff[i+1]) of the concatenated boxes
    float lim_x[LOCOV_LABEL_MAX_IMAGES], lim_y[LOCOV_LABEL_MAX_IMAGES];      // Boxes.inside_box: x2 < w + thresh, y2 < h + thresh
    float neg_thr;                                   // ... and x1, y1 >= -thresh
    int use_boundary, allow_lq;
    int n_thr;                                       // Matcher: n_thr intervals [lo[k], hi[k]) with label lab[k] in {-1, 0, 1}
    float lo[LOCOV_LABEL_MAX_THRESHOLDS], hi[LOCOV_LABEL_MAX_THRESHOLDS];
    int lab[LOCOV_LABEL_MAX_THRESHOLDS];
};

// grid (ceil(hwa / 256), images)
__global__ __launch_bounds__(kRtThreads) void rpn_label_kernel(const float4 *__restrict__ anchors, int hwa, const float4 *__restrict__ gt,
                                                               const unsigned *__restrict__ slots, RpnLabelGeom g,
                                                               signed char *__restrict__ labels, float4 *__restrict__ matched,
                                                               int *__restrict__ counts)
{
    const int img = blockIdx.y, i = blockIdx.x * kRtThreads + threadIdx.x, lane = threadIdx.x & (kWave - 1);
    int label = -2;                                              // (a thread past the end: in neither population)
    if (i < hwa) {
        const float4 b = anchors[i];
        const int g0 = g.goff[img], g1 = g.goff[img + 1];
        // matched_vals, matches = quality.max(dim=0): strict >, the FIRST maximum; NaN counts as the maximum
        float best = -1.f;
        int best_j = g0;
        bool promote = false;
        for (int j = g0; j < g1; j++) {
            const float q = box_pairwise_iou(gt[j], b);
            if (j == g0 || q > best || (q != q && best == best)) {
                best = q;
                best_j = j;
            }
            promote |= q == __uint_as_float(slots[j]);           // quality == highest[:, None] (a box's maximum of 0 promotes every
                                                                 // anchor that does not touch it, as upstream)
        }
        int ml = 1;                                              // Matcher: match_labels start at 1, every interval that holds overwrites
        for (int k = 0; k < g.n_thr; k++)
            if (best >= g.lo[k] && best < g.hi[k]) ml = g.lab[k];
        if (g.allow_lq && promote) ml = 1;                       // (the promoted anchor keeps its argmax box as its target)
        if (g1 == g0) ml = 0;                                    // an image without ground truth: all background
        if (g.use_boundary && !(b.x >= g.neg_thr && b.y >= g.neg_thr && b.z < g.lim_x[img] && b.w < g.lim_y[img])) ml = -1;
        label = ml;
        const int64_t at = (int64_t)img * hwa + i;
        labels[at] = (signed char)ml;
        matched[at] = g1 > g0 ? gt[best_j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const unsigned long long bp = __ballot(label == 1), bn = __ballot(label == 0);
    if (lane == 0) {
        if (bp) atomicAdd(&counts[4 * img + 0], (int)__popcll(bp));
        if (bn) atomicAdd(&counts[4 * img + 1], (int)__popcll(bn));
    }
}

// grid (images, 2): workgroup (i, 0) draws image i's positives (label 1, keys rnd[0, i]), (i, 1) its negatives (label 0, keys rnd[1, i]).
// Workgroup (i, 0) also writes the anchors whose pre-sampling label is -1, so the two write every anchor exactly once.
__global__ __launch_bounds__(kRtSelThreads) void rpn_sample_kernel(const signed char *__restrict__ labels, const double *__restrict__ rnd,
                                                                   int hwa, int n_images, int budget, int max_pos, int *__restrict__ counts,
                                                                   signed char *__restrict__ out)
{
    __shared__ int hist[kRtBins];
    __shared__ int wave_sum[kRtSelWaves];
    __shared__ int ctl[3];                                       // picked bin, keys before it, keys in it
    const int img = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
    const signed char target = part == 0 ? 1 : 0;
    const signed char *L = labels + (int64_t)img * hwa;
    const unsigned long long *K = reinterpret_cast<const unsigned long long *>(rnd) + ((int64_t)part * n_images + img) * hwa;
    signed char *O = out + (int64_t)img * hwa;
    // subsample_labels' counts
    const int pop_pos = counts[4 * img + 0], pop_neg = counts[4 * img + 1];
    const int num_pos = pop_pos < max_pos ? pop_pos : max_pos;
    const int num_neg = pop_neg < budget - num_pos ? pop_neg : budget - num_pos;
    const int k = part == 0 ? num_pos : num_neg, pop = part == 0 ? pop_pos : pop_neg;
    if (tid == 0) counts[4 * img + 2 + part] = k;

    // ---- the k-th smallest key of the population: its leading bits `pre` down to bit `shift`, and how many of the keys that carry
    //      exactly those bits are taken (`need`; they are taken in anchor order)
    unsigned long long pre = 0;
    int need = k, shift = 0;
    if (k > 0 && k < pop) {
        for (int pass = 0; pass < kRtPasses; pass++) {
            shift = kRtDigit * (kRtPasses - 1 - pass);
            for (int b = tid; b < kRtBins; b += kRtSelThreads) hist[b] = 0;
            __syncthreads();
#pragma unroll 4
            for (int i = tid; i < hwa; i += kRtSelThreads) {
                if (L[i] != target) continue;
                const unsigned long long key = K[i];
                if (pass == 0 || (key >> (shift + kRtDigit)) == pre)
                    atomicAdd(&hist[(int)(key >> shift) & (kRtBins - 1)], 1);                  // (integer counts in LDS: order-independent)
            }
            __syncthreads();
            const int v[2] = {hist[2 * tid], hist[2 * tid + 1]};
            radix_pick<kRtSelThreads>(v, need, wave_sum, ctl);
            pre = (pre << kRtDigit) | (unsigned long long)ctl[0];
            need -= ctl[1];
            const int in_bin = ctl[2];
            __syncthreads();                                     // (ctl and hist are written again in the next pass)
            if (in_bin == need) break;                           // the whole bin is taken: no key of it has to be told from another
        }
    }

    // ---- one ordered sweep: keys below the cut, and the first `need` of the keys on it in anchor order
    const bool all = k >= pop, none = k <= 0;
    int ties_seen = 0;                                           // keys on the cut in the chunks before this one (uniform)
    for (int i0 = 0; i0 < hwa; i0 += kRtSelThreads) {
        const int i = i0 + tid;
        signed char l = -2;
        bool take = false, tie = false;
        if (i < hwa) {
            l = L[i];
            if (l == target && !none) {
                if (all) {
                    take = true;
                } else {
                    const unsigned long long top = K[i] >> shift;
                    take = top < pre;
                    tie = top == pre;
                }
            }
        }
        if (!all && !none) {                                     // (uniform)
            int total;
            const int before = ties_seen + block_ballot_rank<kRtSelThreads>(tie, wave_sum, total);
            if (__builtin_expect(tie, false)) take = before < need;         // (rare; the hint keeps the rank's sum a branch most waves skip)
            ties_seen += total;
            __syncthreads();
        }
        if (i < hwa) {
            if (l == target) O[i] = take ? target : (signed char)-1;
            else if (part == 0 && l != 0) O[i] = -1;
        }
    }
}

// grid (ceil(hwa / 256), images); partials[blockIdx.y * gridDim.x + blockIdx.x] = this block's (objectness, localisation) sums
__global__ __launch_bounds__(kRtThreads) void rpn_loss_kernel(const float *__restrict__ logits, const float4 *__restrict__ deltas,
                                                              const signed char *__restrict__ labels, const float4 *__restrict__ anchors,
                                                              const float4 *__restrict__ matched, int hwa, float wx, float wy, float ww,
                                                              float wh, float beta, float cls_scale, float loc_scale,
                                                              double2 *__restrict__ partials, float *__restrict__ dlogits,
                                                              float4 *__restrict__ ddeltas, int *__restrict__ flags)
{
    __shared__ double red[2][kRtThreads / kWave];
    const int img = blockIdx.y, i = blockIdx.x * kRtThreads + threadIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    double sc = 0.0, sl = 0.0;
    bool degenerate = false;
    if (i < hwa) {
        const int64_t at = (int64_t)img * hwa + i;
        const int label = labels[at];
        float gl = 0.f;
        float gd[4] = {0.f, 0.f, 0.f, 0.f};
        if (label >= 0) {
            // bce(x, y) = max(x, 0) - x y + log1p(exp(-|x|));  sigmoid(x) = 1 / (1 + e) or e / (1 + e) with e = exp(-|x|)
            const float x = logits[at];
            const float e = expf(-fabsf(x));
            const bool hot = label == 1;
            sc = ((double)fmaxf(x, 0.f) - (hot ? (double)x : 0.0)) + (double)log1pf(e);
            const double sig = (x >= 0.f ? 1.0 : (double)e) / (1.0 + (double)e);
            gl = (float)((sig - (hot ? 1.0 : 0.0)) * (double)cls_scale);              // one rounding to fp32
        }
        if (label == 1) {
            const float4 s = anchors[i], p4 = deltas[at];
            degenerate = !((s.z - s.x) > 0.f && (s.w - s.y) > 0.f);                   // Box2BoxTransform's assert
            float d[4];
            box_get_deltas(s, matched[at], wx, wy, ww, wh, d);
            const float p[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float l, de;
                smooth_l1_term(p[j] - d[j], beta, l, de);
                sl += (double)l;
                gd[j] = de * loc_scale;
            }
        }
        dlogits[at] = gl;
        ddeltas[at] = make_float4(gd[0], gd[1], gd[2], gd[3]);
    }
    sc = wave_reduce(sc, SumOp());                               // a fixed tree over the wave, then the waves in order
    sl = wave_reduce(sl, SumOp());
    if (lane == 0) {
        red[0][wave] = sc;
        red[1][wave] = sl;
    }
    if (__ballot(degenerate) != 0ull && lane == 0) atomicOr(flags, LOCOV_RPN_LOSS_FLAG_DEGENERATE);
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int q = 0; q < kRtThreads / kWave; q++) {
            a += red[0][q];
            b += red[1][q];
        }
        partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = make_double2(a, b);
    }
}

__global__ __launch_bounds__(kRtThreads) void rpn_loss_finish_kernel(const double2 *__restrict__ partials, int64_t n, float cls_scale,
                                                                     float loc_scale, float *__restrict__ loss)
{
    __shared__ double red[2][kRtThreads];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t k = t; k < n; k += kRtThreads) {                // block order inside the thread, a fixed tree over the threads
        const double2 p = partials[k];
        a += p.x;
        b += p.y;
    }
    red[0][t] = a;
    red[1][t] = b;
    __syncthreads();
    for (int s = kRtThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] += red[0][t + s];
            red[1][t] += red[1][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        loss[0] = (float)(red[0][0] * (double)cls_scale);
        loss[1] = (float)(red[1][0] * (double)loc_scale);
    }
}

// the limits every entry point of this file shares; < 0 on an argument error (set_error has run)
static int rpn_train_limits(int n_images, int64_t hwa, const char *who)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= LOCOV_LABEL_MAX_IMAGES, "%s: too many images (0..%d per call)", who, LOCOV_LABEL_MAX_IMAGES);
    LOCOV_REQUIRE(hwa >= 0 && hwa < kRtMaxAnchors, "%s: too many anchors (fewer than %d per image)", who, kRtMaxAnchors);
    return LOCOV_OK;
}

}  // namespace locov

using namespace locov;

extern "C" {

int64_t locov_rpn_label_anchors_workspace_bytes(int n_images, int64_t hwa, int64_t n_gt)
{
    const int rc = rpn_train_limits(n_images, hwa, "locov_rpn_label_anchors_workspace_bytes");
    if (rc < 0) return rc;
    LOCOV_REQUIRE(n_gt >= 0 && n_gt <= INT32_MAX / 4, "locov_rpn_label_anchors_workspace_bytes: ground-truth count out of range");
    if (n_images == 0 || hwa == 0) return 0;
    return 16 * ceil_div(n_gt, 4);
}

int locov_rpn_label_anchors(const float *anchors, int64_t hwa, const float *gt_boxes, const int *gt_offsets_host, const float *image_hw_host,
                            int n_images, const float *thr_lo_host, const float *thr_hi_host, const int *thr_label_host, int n_thresholds,
                            int allow_low_quality, float boundary_thresh, void *workspace, int64_t workspace_bytes, int8_t *labels,
                            float *matched_boxes, int *counts, locov_stream_t stream)
{
    const char *who = "locov_rpn_label_anchors";
    const int rc = rpn_train_limits(n_images, hwa, who);
    if (rc < 0) return rc;
    LOCOV_REQUIRE(n_thresholds >= 0 && n_thresholds <= LOCOV_LABEL_MAX_THRESHOLDS, "%s: at most %d matcher intervals", who,
                  LOCOV_LABEL_MAX_THRESHOLDS);
    if (n_images == 0 || hwa == 0) return LOCOV_OK;
    LOCOV_REQUIRE(gt_offsets_host && image_hw_host && (n_thresholds == 0 || (thr_lo_host && thr_hi_host && thr_label_host)),
                  "%s: null host array", who);
    RpnLabelGeom g{};
    for (int i = 0; i <= n_images; i++) {
        g.goff[i] = gt_offsets_host[i];
        LOCOV_REQUIRE(g.goff[i] >= 0 && (i == 0 || g.goff[i] >= g.goff[i - 1]), "%s: offsets must be non-decreasing", who);
    }
    LOCOV_REQUIRE(g.goff[0] == 0, "%s: offsets start at 0", who);
    const int n_gt = g.goff[n_images];
    LOCOV_REQUIRE(n_gt <= INT32_MAX / 4, "%s: ground-truth count out of range", who);
    for (int k = 0; k < n_thresholds; k++) {
        g.lo[k] = thr_lo_host[k];
        g.hi[k] = thr_hi_host[k];
        g.lab[k] = thr_label_host[k];
        LOCOV_REQUIRE(g.lab[k] >= -1 && g.lab[k] <= 1, "%s: matcher labels are -1, 0 or 1", who);
    }
    g.n_thr = n_thresholds;
    g.allow_lq = allow_low_quality != 0;
    g.use_boundary = boundary_thresh >= 0.f;
    g.neg_thr = -boundary_thresh;
    for (int i = 0; i < n_images; i++) {                         // (Boxes.inside_box forms w + thresh on the host)
        g.lim_y[i] = (float)((double)image_hw_host[2 * i] + (double)boundary_thresh);
        g.lim_x[i] = (float)((double)image_hw_host[2 * i + 1] + (double)boundary_thresh);
    }
    const int64_t need = 16 * ceil_div(n_gt, 4);
    LOCOV_REQUIRE(anchors && labels && matched_boxes && counts && (n_gt == 0 || (gt_boxes && workspace)), "%s: null pointer", who);
    LOCOV_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld bytes, need %lld)", who, (long long)workspace_bytes, (long long)need);
    LOCOV_REQUIRE(((uintptr_t)anchors | (uintptr_t)gt_boxes | (uintptr_t)matched_boxes | (uintptr_t)workspace) % 16 == 0,
                  "%s: anchors / gt_boxes / matched_boxes / workspace must be 16-byte aligned", who);
    hipStream_t s = as_stream(stream);
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * 4 * (size_t)n_images, s);
    if (e == hipSuccess && n_gt > 0) e = hipMemsetAsync(workspace, 0, (size_t)need, s);
    if (e != hipSuccess) return set_error(LOCOV_ERR_LAUNCH, "%s: memset: %s", who, hipGetErrorString(e));
    unsigned *slots = static_cast<unsigned *>(workspace);
    if (n_gt > 0 && g.allow_lq)
        hipLaunchKernelGGL(rpn_gt_max_kernel, dim3((unsigned)ceil_div(hwa, kRtThreads * kRtPerThread)), dim3(kRtThreads), 0, s,
                           reinterpret_cast<const float4 *>(anchors), (int)hwa, reinterpret_cast<const float4 *>(gt_boxes), n_gt, slots);
    hipLaunchKernelGGL(rpn_label_kernel, dim3((unsigned)ceil_div(hwa, kRtThreads), (unsigned)n_images), dim3(kRtThreads), 0, s,
                       reinterpret_cast<const float4 *>(anchors), (int)hwa, reinterpret_cast<const float4 *>(gt_boxes), slots, g,
                       reinterpret_cast<signed char *>(labels), reinterpret_cast<float4 *>(matched_boxes), counts);
    return check_launch(who);
}

int locov_rpn_sample_anchors(const int8_t *labels, const double *rnd, int64_t hwa, int n_images, int budget, int max_pos, int *counts,
                             int8_t *out_labels, locov_stream_t stream)
{
    const char *who = "locov_rpn_sample_anchors";
    const int rc = rpn_train_limits(n_images, hwa, who);
    if (rc < 0) return rc;
    LOCOV_REQUIRE(budget >= 0 && max_pos >= 0 && max_pos <= budget, "%s: 0 <= max_pos <= budget", who);
    if (n_images == 0 || hwa == 0) return LOCOV_OK;
    LOCOV_REQUIRE(labels && rnd && counts && out_labels, "%s: null pointer", who);
    LOCOV_REQUIRE(labels != out_labels, "%s: out_labels must not alias labels", who);
    hipLaunchKernelGGL(rpn_sample_kernel, dim3((unsigned)n_images, 2), dim3(kRtSelThreads), 0, as_stream(stream),
                       reinterpret_cast<const signed char *>(labels), rnd, (int)hwa, n_images, budget, max_pos, counts,
                       reinterpret_cast<signed char *>(out_labels));
    return check_launch(who);
}

int64_t locov_rpn_loss_workspace_bytes(int n_images, int64_t hwa)
{
    const int rc = rpn_train_limits(n_images, hwa, "locov_rpn_loss_workspace_bytes");
    if (rc < 0) return rc;
    return 16 * (int64_t)n_images * ceil_div(hwa, kRtThreads);
}

int locov_rpn_loss(const float *logits, const float *deltas, const int8_t *labels, const float *anchors, const float *matched_boxes,
                   int64_t hwa, int n_images, float wx, float wy, float ww, float wh, float smooth_l1_beta, float cls_scale, float loc_scale,
                   void *workspace, int64_t workspace_bytes, float *loss, float *dlogits, float *ddeltas, int *flags, locov_stream_t stream)
{
    const char *who = "locov_rpn_loss";
    const int rc = rpn_train_limits(n_images, hwa, who);
    if (rc < 0) return rc;
    LOCOV_REQUIRE(smooth_l1_beta >= 0.f, "%s: smooth_l1_beta must be >= 0", who);
    if (n_images == 0 || hwa == 0) return LOCOV_OK;
    hipStream_t s = as_stream(stream);
    const int64_t blocks = (int64_t)n_images * ceil_div(hwa, kRtThreads), need = 16 * blocks;
    LOCOV_REQUIRE(logits && deltas && labels && anchors && matched_boxes && workspace && loss && dlogits && ddeltas && flags,
                  "%s: null pointer", who);
    LOCOV_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld bytes, need %lld)", who, (long long)workspace_bytes, (long long)need);
    LOCOV_REQUIRE(((uintptr_t)deltas | (uintptr_t)anchors | (uintptr_t)matched_boxes | (uintptr_t)workspace | (uintptr_t)ddeltas) % 16 == 0,
                  "%s: deltas / anchors / matched_boxes / workspace / ddeltas must be 16-byte aligned", who);
    const hipError_t e = hipMemsetAsync(flags, 0, sizeof(int), s);
    if (e != hipSuccess) return set_error(LOCOV_ERR_LAUNCH, "%s: memset: %s", who, hipGetErrorString(e));
    double2 *partials = static_cast<double2 *>(workspace);
    hipLaunchKernelGGL(rpn_loss_kernel, dim3((unsigned)ceil_div(hwa, kRtThreads), (unsigned)n_images), dim3(kRtThreads), 0, s, logits,
                       reinterpret_cast<const float4 *>(deltas), reinterpret_cast<const signed char *>(labels),
                       reinterpret_cast<const float4 *>(anchors), reinterpret_cast<const float4 *>(matched_boxes), (int)hwa, wx, wy, ww, wh,
                       smooth_l1_beta, cls_scale, loc_scale, partials, dlogits, reinterpret_cast<float4 *>(ddeltas), flags);
    hipLaunchKernelGGL(rpn_loss_finish_kernel, dim3(1), dim3(kRtThreads), 0, s, partials, blocks, cls_scale, loc_scale, loss);
    return check_launch(who);
}

}  // extern "C"
