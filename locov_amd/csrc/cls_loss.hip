// The classification loss of the training heads and its training statistics, from ONE pass over the logits.
//
//   * locov_cls_loss -- [D2-upstream] FastRCNNOutputLayers.losses' `cross_entropy(scores, gt_classes, reduction="mean")` (the reference
//     inherits it: ovr/modeling/roi_heads/box_emb_head.py:60 EmbeddingFastRCNNOutputLayers(FastRCNNOutputLayers), box_emb_grounding_head.py:259)
//     together with the counts of [D2-upstream, unverified] _log_classification_stats: argmax, foreground rule and the five counters
//     restated from public Detectron2.  The gradient of the logits comes out of the same pass, already divided by the number of rows
//     that count, so backward is one multiplication by the incoming gradient.
//
// Two launches: cls_loss_rows_kernel (one wave per row, kClsRowsPerBlock rows per block, grid-stride over the row groups) writes the
// gradient and one partial per block; cls_loss_finish_kernel (one block) adds the partials in block-index order.  No atomics: the same
// inputs give the same bits.  A row's element -> lane assignment is the same with 16-byte loads and with scalar ones, so a column slice
// of a wider matrix gives the bits of its contiguous copy.
#include "common.h"

#include <cmath>

namespace locov {

namespace {

constexpr int kClsRowsPerBlock = 4;
constexpr int kClsThreads = kClsRowsPerBlock * kWave;
constexpr int kClsMaxBlocks = 1024;
constexpr int kClsFinishThreads = 256;

// what a block hands to the finishing launch (32 bytes)
struct ClsPartial {
    double loss;                                                     // sum of the rows' losses
    int n_valid, n_fg, n_accurate, n_fg_accurate, n_false_negative, n_invalid;
};

inline int cls_blocks(int64_t R)
{
    const int64_t groups = ceil_div(R, kClsRowsPerBlock);
    return (int)(groups < kClsMaxBlocks ? groups : kClsMaxBlocks);
}

// elements [4 * chunk, 4 * chunk + 4) of a row of C logits; past the end: -inf (no weight in the maximum or in the sum)
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

__device__ __forceinline__ int wave_sum_int(int v)
{
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, kWave);
    return v;
}

}  // namespace

template <bool VEC>
__global__ __launch_bounds__(kClsThreads) void cls_loss_rows_kernel(const float *__restrict__ scores, int64_t ld,
                                                                    const int64_t *__restrict__ labels, int64_t R, int C,
                                                                    int64_t ignore_index, float *__restrict__ dscores,
                                                                    ClsPartial *__restrict__ partials)
{
    __shared__ int red_n[kClsRowsPerBlock];
    __shared__ ClsPartial red_p[kClsRowsPerBlock];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int bg = C - 1, chunks = (C + 3) / 4;

    // the gradient's 1 / n_valid: every block counts the rows that count (integers: the same in every block and every run)
    double inv_n = 0.0;
    if (dscores) {
        int n = 0;
        for (int64_t r = threadIdx.x; r < R; r += kClsThreads) {
            const int64_t y = labels[r];
            n += (y >= 0 && y < C && y != ignore_index) ? 1 : 0;
        }
        n = wave_sum_int(n);
        if (lane == 0) red_n[wave] = n;
        __syncthreads();
        n = 0;
#pragma unroll
        for (int w = 0; w < kClsRowsPerBlock; w++) n += red_n[w];
        inv_n = n > 0 ? 1.0 / (double)n : 0.0;
    }

    ClsPartial acc = {0.0, 0, 0, 0, 0, 0, 0};                        // this wave's rows, in row order (every lane holds the same)
    for (int64_t r = (int64_t)blockIdx.x * kClsRowsPerBlock + wave; r < R; r += (int64_t)gridDim.x * kClsRowsPerBlock) {
        const int64_t y = labels[r];
        const bool valid = y >= 0 && y < C && y != ignore_index;
        float *drow = dscores ? dscores + r * (int64_t)C : nullptr;
        if (!valid) {
            // ignored (ignore_index) or out of range (counted; torch asserts on the device): no loss, an exactly zero gradient, and
            // no prediction can equal such a label, so the row's logits are not read
            acc.n_invalid += y != ignore_index ? 1 : 0;
            if (drow)
                for (int k = lane; k < chunks; k += kWave) store_chunk<VEC>(drow, k, C, make_float4(0.f, 0.f, 0.f, 0.f));
            continue;
        }
        const float *row = scores + r * ld;

        // pass 1: the maximum and its lowest index
        float m = -INFINITY;
        int arg = 0x7fffffff;
        for (int k = lane; k < chunks; k += kWave) {
            const float4 v = load_chunk<VEC>(row, k, C);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (e[j] > m) {                                      // (strict: the lane's lowest index among equal maxima)
                    m = e[j];
                    arg = k * 4 + j;
                }
        }
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1) {
            const float om = __shfl_xor(m, s, kWave);
            const int oa = __shfl_xor(arg, s, kWave);
            if (om > m || (om == m && oa < arg)) {
                m = om;
                arg = oa;
            }
        }

        // pass 2 (the row is in cache): sum exp(x - max), fp64 accumulation in a fixed order
        double sum = 0.0;
        for (int k = lane; k < chunks; k += kWave) {
            const float4 v = load_chunk<VEC>(row, k, C);
            sum += (double)expf(v.x - m);
            sum += (double)expf(v.y - m);
            sum += (double)expf(v.z - m);
            sum += (double)expf(v.w - m);
        }
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1) sum += __shfl_xor(sum, s, kWave);

        const int label = (int)y;
        const float xl = row[label];
        acc.loss += ((double)m + log(sum)) - (double)xl;
        acc.n_valid += 1;
        const bool fg = label < bg, hit = arg == label;
        acc.n_fg += fg ? 1 : 0;
        acc.n_accurate += hit ? 1 : 0;
        acc.n_fg_accurate += fg && hit ? 1 : 0;
        acc.n_false_negative += fg && arg == bg ? 1 : 0;

        // pass 3: (softmax - onehot) / n_valid, one rounding to fp32
        if (drow) {
            const double scale = inv_n / sum;
            for (int k = lane; k < chunks; k += kWave) {
                const float4 v = load_chunk<VEC>(row, k, C);
                const float x[4] = {v.x, v.y, v.z, v.w};
                float g[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double e = (double)expf(x[j] - m);
                    g[j] = (float)((k * 4 + j == label ? e - sum : e) * scale);
                }
                store_chunk<VEC>(drow, k, C, make_float4(g[0], g[1], g[2], g[3]));
            }
        }
    }

    if (lane == 0) red_p[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        ClsPartial p = red_p[0];
#pragma unroll
        for (int w = 1; w < kClsRowsPerBlock; w++) {
            p.loss += red_p[w].loss;
            p.n_valid += red_p[w].n_valid;
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
__global__ __launch_bounds__(kClsFinishThreads) void cls_loss_finish_kernel(const ClsPartial *__restrict__ partials, int n_partials,
                                                                            int64_t R, float *__restrict__ loss,
                                                                            int64_t *__restrict__ stats)
{
    __shared__ double red_loss[kClsFinishThreads];
    __shared__ int64_t red_cnt[kClsFinishThreads][6];
    const int t = threadIdx.x;
    double l = 0.0;
    int64_t c[6] = {0, 0, 0, 0, 0, 0};
    for (int i = t; i < n_partials; i += kClsFinishThreads) {
        const ClsPartial p = partials[i];
        l += p.loss;
        c[0] += p.n_valid;
        c[1] += p.n_fg;
        c[2] += p.n_accurate;
        c[3] += p.n_fg_accurate;
        c[4] += p.n_false_negative;
        c[5] += p.n_invalid;
    }
    red_loss[t] = l;
#pragma unroll
    for (int j = 0; j < 6; j++) red_cnt[t][j] = c[j];
    __syncthreads();
    for (int s = kClsFinishThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            red_loss[t] += red_loss[t + s];
#pragma unroll
            for (int j = 0; j < 6; j++) red_cnt[t][j] += red_cnt[t + s][j];
        }
        __syncthreads();
    }
    if (t == 0) {
        loss[0] = (float)(red_loss[0] / (double)red_cnt[0][0]);     // no row counts: 0 / 0 = NaN, as torch's mean
        if (stats) {
            stats[0] = R;                                            // num_instances
            stats[1] = red_cnt[0][1];                                // num_fg
            stats[2] = red_cnt[0][2];                                // num_accurate
            stats[3] = red_cnt[0][3];                                // fg_num_accurate
            stats[4] = red_cnt[0][4];                                // num_false_negative
            stats[5] = red_cnt[0][5];                                // num_invalid
        }
    }
}

}  // namespace locov

using namespace locov;

extern "C" int64_t locov_cls_loss_workspace_bytes(int64_t R)
{
    return R > 0 ? (int64_t)cls_blocks(R) * (int64_t)sizeof(ClsPartial) : 0;
}

extern "C" int locov_cls_loss(const float *scores, int64_t ld, const int64_t *gt_classes, int64_t R, int C, int64_t ignore_index,
                              void *workspace, int64_t workspace_bytes, float *loss, float *dscores, int64_t *stats,
                              locov_stream_t stream)
{
    LOCOV_REQUIRE(R >= 0 && C >= 1, "locov_cls_loss: R >= 0 and C >= 1 required (R %lld, C %d)", (long long)R, C);
    LOCOV_REQUIRE(ld >= C, "locov_cls_loss: row stride ld %lld is smaller than C %d", (long long)ld, C);
    LOCOV_REQUIRE(loss && (R == 0 || (scores && gt_classes)), "locov_cls_loss: null pointer");
    LOCOV_REQUIRE(workspace_bytes >= locov_cls_loss_workspace_bytes(R) && (R == 0 || workspace),
                  "locov_cls_loss: workspace too small (%lld bytes, %lld needed)", (long long)workspace_bytes,
                  (long long)locov_cls_loss_workspace_bytes(R));
    LOCOV_REQUIRE((uintptr_t)workspace % 8 == 0, "locov_cls_loss: workspace must be 8-byte aligned");
    ClsPartial *partials = static_cast<ClsPartial *>(workspace);
    const int blocks = R > 0 ? cls_blocks(R) : 0;
    if (blocks > 0) {
        // 16-byte loads and stores when every row of both matrices starts on a 16-byte boundary and holds whole chunks
        const bool vec = C % 4 == 0 && ld % 4 == 0 && (uintptr_t)scores % 16 == 0 && (uintptr_t)dscores % 16 == 0;
        hipLaunchKernelGGL(vec ? cls_loss_rows_kernel<true> : cls_loss_rows_kernel<false>, dim3(blocks), dim3(kClsThreads), 0,
                           as_stream(stream), scores, ld, gt_classes, R, C, ignore_index, dscores, partials);
        const int rc = check_launch("locov_cls_loss (rows)");
        if (rc != LOCOV_OK) return rc;
    }
    hipLaunchKernelGGL(cls_loss_finish_kernel, dim3(1), dim3(kClsFinishThreads), 0, as_stream(stream), partials, blocks, R, loss, stats);
    return check_launch("locov_cls_loss (finish)");
}
