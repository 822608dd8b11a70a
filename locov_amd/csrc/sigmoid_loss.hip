// The LVIS-style classification loss of the training heads: per-class sigmoid cross-entropy, optionally restricted to a federated
// class set, both formed on the device without a host read.
//
//   * locov_fed_loss_classes -- [D2-upstream, unverified] FastRCNNOutputLayers.get_fed_loss_classes: the classes present among the
//     labels plus classes sampled by weight without replacement up to a budget.  One launch of one block: a presence bitmap in LDS,
//     then a radix select over the keys weights[c] / rnd[c] (rnd ~ Exp(1): the top n of these keys are a weighted sample without
//     replacement, torch.multinomial's distribution).  The keys are formed again in every pass from the two L2-resident inputs rather
//     than kept in LDS: 32 767 of them would take 128 KB, and a pass reads two floats per class.
//   * locov_sigmoid_cls_loss -- [D2-upstream, unverified] FastRCNNOutputLayers.sigmoid_cross_entropy_loss together with the counts of
//     _log_classification_stats, from ONE pass over the logits (a sigmoid needs no row maximum first): the loss terms, the gradient
//     mask * (sigmoid - onehot) / R and the argmax of the row.  The launch structure -- the row loop, the partials, the finishing launch,
//     the host checks -- is the frame of cls_loss_common.h, shared with locov_cls_loss (cls_loss.hip); this file holds the sigmoid
//     mathematics of one row and the rule for which rows count.
#include "cls_loss_common.h"

namespace locov {

namespace {

// ------------------------------------------------------------------------------------------------ the federated class set

constexpr int kFedThreads = 1024;
constexpr int kFedWaves = kFedThreads / kWave;
constexpr int kFedWords = (LOCOV_FED_LOSS_MAX_CLASSES + 1 + 31) / 32;   // presence bits of the classes 0..K (K: the background label)
static_assert(kFedWords <= kFedThreads, "one bitmap word per thread");

// the sum of v over the block, in every thread (red: kFedWaves ints; safe to call back to back)
__device__ __forceinline__ int fed_block_sum(int v, int *red)
{
    v = wave_reduce(v, SumOp());
    __syncthreads();                                                 // (the previous call's readers are done)
    if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < kFedWaves; w++) s += red[w];
    return s;
}

// The sort key of class c as an unsigned integer whose order is the order of the fp32 keys: 0 for a class that cannot be sampled
// (present, or a weight that is not finite and > 0), else 1 + the bits of the positive key weights[c] / rnd[c] (a correctly rounded
// fp32 division: __fdiv_rn).  A key that is not positive (rnd outside its contract) ranks below every positive one.
__device__ __forceinline__ unsigned fed_key(int c, const unsigned *present, const float *__restrict__ weights, const float *__restrict__ rnd)
{
    if ((present[c >> 5] >> (c & 31)) & 1u) return 0u;
    const float w = weights[c];
    if (!(w > 0.f) || !(w < INFINITY)) return 0u;
    const float key = __fdiv_rn(w, rnd[c]);
    return key > 0.f ? __float_as_uint(key) + 1u : 1u;
}

}  // namespace

__global__ __launch_bounds__(kFedThreads) void fed_loss_classes_kernel(const int64_t *__restrict__ labels, int64_t R,
                                                                       const float *__restrict__ weights, const float *__restrict__ rnd,
                                                                       int K, int num_fed, unsigned char *__restrict__ mask,
                                                                       int *__restrict__ counts)
{
    __shared__ unsigned present[kFedWords];
    __shared__ int hist[256];
    __shared__ int red[kFedWaves];
    __shared__ int scan[kFedThreads];
    __shared__ unsigned sel_prefix;
    __shared__ int sel_remaining;
    const int t = threadIdx.x;
    const int words = (K + 1 + 31) / 32;

    if (t < kFedWords) present[t] = 0u;
    __syncthreads();
    for (int64_t r = t; r < R; r += kFedThreads) {
        const int64_t y = labels[r];
        if (y >= 0 && y <= K) atomicOr(&present[(int)y >> 5], 1u << ((int)y & 31));      // (an LDS bit-or: the order does not matter)
    }
    __syncthreads();
    const int n_present = fed_block_sum(t < words ? __popc(present[t]) : 0, red);

    int n_cand = 0;
    for (int c = t; c < K; c += kFedThreads) n_cand += fed_key(c, present, weights, rnd) != 0u ? 1 : 0;
    n_cand = fed_block_sum(n_cand, red);
    int n_take = num_fed - n_present;
    n_take = n_take < 0 ? 0 : n_take;
    n_take = n_take < n_cand ? n_take : n_cand;                      // fewer candidates than asked for: all of them

    // The n_take-th largest key, one byte per pass from the top: `prefix` holds the bytes found so far, `remaining` how many of the
    // keys that share them are still to be taken.  (n_take <= n_cand, so the key found is a candidate's: > 0.)
    unsigned cut = 0xffffffffu;                                      // nothing to sample: no key is above it ...
    int take_equal = 0;                                              // ... and none of the keys equal to it is taken
    if (n_take > 0) {
        unsigned prefix = 0u;
        int remaining = n_take;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (t < 256) hist[t] = 0;
            __syncthreads();
            const unsigned high = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
            for (int c = t; c < K; c += kFedThreads) {
                const unsigned u = fed_key(c, present, weights, rnd);
                if ((u & high) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);      // (integer counts in LDS: order-independent)
            }
            __syncthreads();
            if (t == 0) {
                int above = 0, b = 255;
                for (; b > 0; b--) {
                    if (above + hist[b] >= remaining) break;
                    above += hist[b];
                }
                sel_prefix = prefix | ((unsigned)b << shift);
                sel_remaining = remaining - above;
            }
            __syncthreads();
            prefix = sel_prefix;
            remaining = sel_remaining;
        }
        cut = prefix;
        take_equal = remaining;
    }

    // every key above the cut, and the first take_equal of the keys equal to it in class order (equal keys: the lower index wins);
    // thread t owns the classes [t * per, (t + 1) * per)
    const int per = (K + kFedThreads - 1) / kFedThreads;
    const int c0 = t * per < K ? t * per : K, c1 = c0 + per < K ? c0 + per : K;
    int n_equal = 0;
    for (int c = c0; c < c1; c++) n_equal += fed_key(c, present, weights, rnd) == cut ? 1 : 0;
    scan[t] = n_equal;
    __syncthreads();
    for (int s = 1; s < kFedThreads; s <<= 1) {                      // inclusive scan over the threads' counts
        const int other = t >= s ? scan[t - s] : 0;
        __syncthreads();
        scan[t] += other;
        __syncthreads();
    }
    int rank = scan[t] - n_equal;                                    // keys equal to the cut in the classes below c0
    for (int c = c0; c < c1; c++) {
        const unsigned u = fed_key(c, present, weights, rnd);
        bool on = ((present[c >> 5] >> (c & 31)) & 1u) != 0u || u > cut;
        if (u == cut) {
            on = on || rank < take_equal;
            rank++;
        }
        mask[c] = on ? 1 : 0;
    }
    if (t == 0) {
        counts[0] = n_present;
        counts[1] = n_take;
    }
}

// ------------------------------------------------------------------------------------------------ the loss

namespace {

struct SigmoidLoss {
    const unsigned char *__restrict__ class_mask;                    // [K] or null: every class
    double inv_r;                                                    // the gradient's 1 / R

    // out of range (counted; upstream's index-put would fail); the sigmoid loss has no ignore index
    __device__ __forceinline__ bool counts(int64_t y, int C) const { return y >= 0 && y <= C - 1; }
    __device__ __forceinline__ bool invalid(int64_t) const { return true; }

    // (label K: a background row, every target 0)
    template <bool VEC>
    __device__ __forceinline__ double row_term(const float *__restrict__ row, float *__restrict__ drow, int label, int C, int lane,
                                               int chunks, int &arg) const
    {
        const int K = C - 1;                                         // the background column, which never enters the loss
        float m = -INFINITY;
        arg = 0x7fffffff;
        double sum = 0.0;                                            // this lane's terms, fp64 accumulation in a fixed order
        for (int k = lane; k < chunks; k += kWave) {
            const float4 v = load_chunk<VEC>(row, k, C);
            const float x[4] = {v.x, v.y, v.z, v.w};
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c = k * 4 + j;
                if (x[j] > m) {                                      // (strict: the lane's lowest index among equal maxima)
                    m = x[j];
                    arg = c;
                }
                g[j] = 0.f;
                if (c < K && (!class_mask || class_mask[c])) {
                    // bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|));  sigmoid(x) = 1 / (1 + e) or e / (1 + e) with e = exp(-|x|)
                    const float e = expf(-fabsf(x[j]));
                    const bool hot = c == label;
                    sum += ((double)fmaxf(x[j], 0.f) - (hot ? (double)x[j] : 0.0)) + (double)log1pf(e);
                    const double sig = (x[j] >= 0.f ? 1.0 : (double)e) / (1.0 + (double)e);
                    g[j] = (float)((sig - (hot ? 1.0 : 0.0)) * inv_r);       // one rounding to fp32
                }
            }
            if (drow) store_chunk<VEC>(drow, k, C, make_float4(g[0], g[1], g[2], g[3]));
        }
        wave_argmax(m, arg);
        return wave_reduce(sum, SumOp());
    }
};

}  // namespace

template <bool VEC>
__global__ __launch_bounds__(kClsThreads) void sigmoid_loss_rows_kernel(const float *__restrict__ scores, int64_t ld,
                                                                        const int64_t *__restrict__ labels,
                                                                        const unsigned char *__restrict__ class_mask, int64_t R, int C,
                                                                        float *__restrict__ dscores, ClsPartial *__restrict__ partials)
{
    cls_loss_rows<VEC>(SigmoidLoss{class_mask, 1.0 / (double)R}, scores, ld, labels, R, C, dscores, partials);
}

}  // namespace locov

using namespace locov;

extern "C" int locov_fed_loss_classes(const int64_t *gt_classes, int64_t R, const float *weights, const float *rnd, int K, int num_fed,
                                      unsigned char *mask, int *counts, locov_stream_t stream)
{
    LOCOV_REQUIRE(K >= 1 && K <= LOCOV_FED_LOSS_MAX_CLASSES, "locov_fed_loss_classes: 1 <= K <= %d required (K %d)",
                  LOCOV_FED_LOSS_MAX_CLASSES, K);
    LOCOV_REQUIRE(R >= 0 && num_fed >= 0, "locov_fed_loss_classes: R >= 0 and num_fed >= 0 required (R %lld, num_fed %d)", (long long)R,
                  num_fed);
    LOCOV_REQUIRE(weights && rnd && mask && counts && (R == 0 || gt_classes), "locov_fed_loss_classes: null pointer");
    hipLaunchKernelGGL(fed_loss_classes_kernel, dim3(1), dim3(kFedThreads), 0, as_stream(stream), gt_classes, R, weights, rnd, K, num_fed,
                       mask, counts);
    return check_launch("locov_fed_loss_classes");
}

extern "C" int64_t locov_sigmoid_cls_loss_workspace_bytes(int64_t R) { return cls_workspace_bytes(R); }

extern "C" int locov_sigmoid_cls_loss(const float *scores, int64_t ld, const int64_t *gt_classes, const unsigned char *class_mask, int64_t R,
                                      int C, void *workspace, int64_t workspace_bytes, float *loss, float *dscores, int64_t *stats,
                                      locov_stream_t stream)
{
    LOCOV_REQUIRE(R >= 0 && C >= 2, "locov_sigmoid_cls_loss: R >= 0 and K = C - 1 >= 1 required (R %lld, C %d)", (long long)R, C);
    return cls_loss_launch<false>("locov_sigmoid_cls_loss", scores, ld, gt_classes, R, C, workspace, workspace_bytes, loss, dscores, stats,
                                  stream, [&](bool vec, int blocks, ClsPartial *partials) {
                                      hipLaunchKernelGGL(vec ? sigmoid_loss_rows_kernel<true> : sigmoid_loss_rows_kernel<false>,
                                                         dim3(blocks), dim3(kClsThreads), 0, as_stream(stream), scores, ld, gt_classes,
                                                         class_mask, R, C, dscores, partials);
                                  });
}
