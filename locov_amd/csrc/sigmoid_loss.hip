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
//     mask * (sigmoid - onehot) / R and the argmax of the row.  Launch structure of locov_cls_loss (cls_loss.hip): one wave per row,
//     kSigRowsPerBlock rows per block, grid-stride over the row groups, one double partial per block, a finishing launch that adds the
//     partials in block order.  No atomics there: the same inputs give the same bits, and a row's element -> lane assignment is the
//     same with 16-byte loads and with scalar ones, so a column slice of a wider matrix gives the bits of its contiguous copy.
#include "common.h"

#include <cmath>

namespace locov {

namespace {

// ------------------------------------------------------------------------------------------------ the federated class set

constexpr int kFedThreads = 1024;
constexpr int kFedWaves = kFedThreads / kWave;
constexpr int kFedWords = (LOCOV_FED_LOSS_MAX_CLASSES + 1 + 31) / 32;   // presence bits of the classes 0..K (K: the background label)
static_assert(kFedWords <= kFedThreads, "one bitmap word per thread");

__device__ __forceinline__ int wave_sum_int(int v)
{
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, kWave);
    return v;
}

// the sum of v over the block, in every thread (red: kFedWaves ints; safe to call back to back)
__device__ __forceinline__ int fed_block_sum(int v, int *red)
{
    v = wave_sum_int(v);
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

constexpr int kSigRowsPerBlock = 4;
constexpr int kSigThreads = kSigRowsPerBlock * kWave;
constexpr int kSigMaxBlocks = 1024;
constexpr int kSigFinishThreads = 256;

// what a block hands to the finishing launch (32 bytes)
struct SigPartial {
    double loss;                                                     // sum of the rows' loss terms
    int n_fg, n_accurate, n_fg_accurate, n_false_negative, n_invalid, pad;
};

inline int sig_blocks(int64_t R)
{
    const int64_t groups = ceil_div(R, kSigRowsPerBlock);
    return (int)(groups < kSigMaxBlocks ? groups : kSigMaxBlocks);
}

// elements [4 * chunk, 4 * chunk + 4) of a row of C logits; past the end: -inf (no weight in the maximum; the loss stops at K < C)
template <bool VEC>
__device__ __forceinline__ float4 load_chunk(const float *__restrict__ row, int chunk, int C)
{
    if constexpr (VEC) {
        return reinterpret_cast<const float4 *>(row)[chunk];
    } else {
        const int c = chunk * 4;
        float4 v;
        v.x = row[c];                                                // (c < C: the caller's loop bound)
        v.y = c + 1 < C ? row[c + 1] : -INFINITY;
        v.z = c + 2 < C ? row[c + 2] : -INFINITY;
        v.w = c + 3 < C ? row[c + 3] : -INFINITY;
        return v;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_chunk(float *__restrict__ row, int chunk, int C, float4 v)
{
    if constexpr (VEC) {
        reinterpret_cast<float4 *>(row)[chunk] = v;
    } else {
        const int c = chunk * 4;
        row[c] = v.x;
        if (c + 1 < C) row[c + 1] = v.y;
        if (c + 2 < C) row[c + 2] = v.z;
        if (c + 3 < C) row[c + 3] = v.w;
    }
}

}  // namespace

template <bool VEC>
__global__ __launch_bounds__(kSigThreads) void sigmoid_loss_rows_kernel(const float *__restrict__ scores, int64_t ld,
                                                                        const int64_t *__restrict__ labels,
                                                                        const unsigned char *__restrict__ class_mask, int64_t R, int C,
                                                                        float *__restrict__ dscores, SigPartial *__restrict__ partials)
{
    __shared__ SigPartial red_p[kSigRowsPerBlock];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int K = C - 1, chunks = (C + 3) / 4;                       // K: the background column, which never enters the loss
    const double inv_r = 1.0 / (double)R;

    SigPartial acc = {0.0, 0, 0, 0, 0, 0, 0};                        // this wave's rows, in row order (every lane holds the same)
    for (int64_t r = (int64_t)blockIdx.x * kSigRowsPerBlock + wave; r < R; r += (int64_t)gridDim.x * kSigRowsPerBlock) {
        const int64_t y = labels[r];
        float *drow = dscores ? dscores + r * (int64_t)C : nullptr;
        if (y < 0 || y > K) {
            // out of range (counted; upstream's index-put would fail): no loss terms, an exactly zero gradient, and no prediction
            // can equal such a label, so the row's logits are not read
            acc.n_invalid += 1;
            if (drow)
                for (int k = lane; k < chunks; k += kWave) store_chunk<VEC>(drow, k, C, make_float4(0.f, 0.f, 0.f, 0.f));
            continue;
        }
        const float *row = scores + r * ld;
        const int label = (int)y;                                    // (K: a background row, every target 0)

        float m = -INFINITY;
        int arg = 0x7fffffff;
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
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1) {
            const float om = __shfl_xor(m, s, kWave);
            const int oa = __shfl_xor(arg, s, kWave);
            if (om > m || (om == m && oa < arg)) {
                m = om;
                arg = oa;
            }
            sum += __shfl_xor(sum, s, kWave);
        }

        acc.loss += sum;
        const bool fg = label < K, hit = arg == label;
        acc.n_fg += fg ? 1 : 0;
        acc.n_accurate += hit ? 1 : 0;
        acc.n_fg_accurate += fg && hit ? 1 : 0;
        acc.n_false_negative += fg && arg == K ? 1 : 0;
    }

    if (lane == 0) red_p[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        SigPartial p = red_p[0];
#pragma unroll
        for (int w = 1; w < kSigRowsPerBlock; w++) {
            p.loss += red_p[w].loss;
            p.n_fg += red_p[w].n_fg;
            p.n_accurate += red_p[w].n_accurate;
            p.n_fg_accurate += red_p[w].n_fg_accurate;
            p.n_false_negative += red_p[w].n_false_negative;
            p.n_invalid += red_p[w].n_invalid;
        }
        partials[blockIdx.x] = p;
    }
}

// one block: thread t adds partials t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(kSigFinishThreads) void sigmoid_loss_finish_kernel(const SigPartial *__restrict__ partials, int n_partials,
                                                                                int64_t R, float *__restrict__ loss,
                                                                                int64_t *__restrict__ stats)
{
    __shared__ double red_loss[kSigFinishThreads];
    __shared__ int64_t red_cnt[kSigFinishThreads][5];
    const int t = threadIdx.x;
    double l = 0.0;
    int64_t c[5] = {0, 0, 0, 0, 0};
    for (int i = t; i < n_partials; i += kSigFinishThreads) {
        const SigPartial p = partials[i];
        l += p.loss;
        c[0] += p.n_fg;
        c[1] += p.n_accurate;
        c[2] += p.n_fg_accurate;
        c[3] += p.n_false_negative;
        c[4] += p.n_invalid;
    }
    red_loss[t] = l;
#pragma unroll
    for (int j = 0; j < 5; j++) red_cnt[t][j] = c[j];
    __syncthreads();
    for (int s = kSigFinishThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            red_loss[t] += red_loss[t + s];
#pragma unroll
            for (int j = 0; j < 5; j++) red_cnt[t][j] += red_cnt[t + s][j];
        }
        __syncthreads();
    }
    if (t == 0) {
        loss[0] = R > 0 ? (float)(red_loss[0] / (double)R) : 0.f;   // the divisor is R, whatever the labels
        if (stats) {
            stats[0] = R;                                            // num_instances
            stats[1] = red_cnt[0][0];                                // num_fg
            stats[2] = red_cnt[0][1];                                // num_accurate
            stats[3] = red_cnt[0][2];                                // fg_num_accurate
            stats[4] = red_cnt[0][3];                                // num_false_negative
            stats[5] = red_cnt[0][4];                                // num_invalid
        }
    }
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

extern "C" int64_t locov_sigmoid_cls_loss_workspace_bytes(int64_t R)
{
    return R > 0 ? (int64_t)sig_blocks(R) * (int64_t)sizeof(SigPartial) : 0;
}

extern "C" int locov_sigmoid_cls_loss(const float *scores, int64_t ld, const int64_t *gt_classes, const unsigned char *class_mask, int64_t R,
                                      int C, void *workspace, int64_t workspace_bytes, float *loss, float *dscores, int64_t *stats,
                                      locov_stream_t stream)
{
    LOCOV_REQUIRE(R >= 0 && C >= 2, "locov_sigmoid_cls_loss: R >= 0 and K = C - 1 >= 1 required (R %lld, C %d)", (long long)R, C);
    LOCOV_REQUIRE(ld >= C, "locov_sigmoid_cls_loss: row stride ld %lld is smaller than C %d", (long long)ld, C);
    LOCOV_REQUIRE(loss && (R == 0 || (scores && gt_classes)), "locov_sigmoid_cls_loss: null pointer");
    LOCOV_REQUIRE(workspace_bytes >= locov_sigmoid_cls_loss_workspace_bytes(R) && (R == 0 || workspace),
                  "locov_sigmoid_cls_loss: workspace too small (%lld bytes, %lld needed)", (long long)workspace_bytes,
                  (long long)locov_sigmoid_cls_loss_workspace_bytes(R));
    LOCOV_REQUIRE((uintptr_t)workspace % 8 == 0, "locov_sigmoid_cls_loss: workspace must be 8-byte aligned");
    SigPartial *partials = static_cast<SigPartial *>(workspace);
    const int blocks = R > 0 ? sig_blocks(R) : 0;
    if (blocks > 0) {
        // 16-byte loads and stores when every row of both matrices starts on a 16-byte boundary and holds whole chunks
        const bool vec = C % 4 == 0 && ld % 4 == 0 && (uintptr_t)scores % 16 == 0 && (uintptr_t)dscores % 16 == 0;
        hipLaunchKernelGGL(vec ? sigmoid_loss_rows_kernel<true> : sigmoid_loss_rows_kernel<false>, dim3(blocks), dim3(kSigThreads), 0,
                           as_stream(stream), scores, ld, gt_classes, class_mask, R, C, dscores, partials);
        const int rc = check_launch("locov_sigmoid_cls_loss (rows)");
        if (rc != LOCOV_OK) return rc;
    }
    hipLaunchKernelGGL(sigmoid_loss_finish_kernel, dim3(1), dim3(kSigFinishThreads), 0, as_stream(stream), partials, blocks, R, loss,
                       stats);
    return check_launch("locov_sigmoid_cls_loss (finish)");
}
