// The classification loss of the training heads and its training statistics, from ONE pass over the logits.
//
//   * locov_cls_loss -- [D2-upstream] FastRCNNOutputLayers.losses' `cross_entropy(scores, gt_classes, reduction="mean")` (the reference
//     inherits it: ovr/modeling/roi_heads/box_emb_head.py:60 EmbeddingFastRCNNOutputLayers(FastRCNNOutputLayers), box_emb_grounding_head.py:259)
//     together with the counts of [D2-upstream, unverified] _log_classification_stats: argmax, foreground rule and the five counters
//     restated from public Detectron2.  The gradient of the logits comes out of the same pass, already divided by the number of rows
//     that count, so backward is one multiplication by the incoming gradient.
//
// The launch structure -- the row loop, the partials, the finishing launch, the host checks -- is the frame of cls_loss_common.h; this
// file holds the softmax mathematics of one row and the rule for which rows count.
#include "cls_loss_common.h"

namespace locov {

namespace {

struct SoftmaxLoss {
    int64_t ignore_index;
    double inv_n;                                                    // the gradient's 1 / n_valid (0 where no gradient is asked for)

    // ignored (ignore_index) or out of range (counted; torch asserts on the device)
    __device__ __forceinline__ bool counts(int64_t y, int C) const { return y >= 0 && y < C && y != ignore_index; }
    __device__ __forceinline__ bool invalid(int64_t y) const { return y != ignore_index; }

    template <bool VEC>
    __device__ __forceinline__ double row_term(const float *__restrict__ row, float *__restrict__ drow, int label, int C, int lane,
                                               int chunks, int &arg) const
    {
        // pass 1: the maximum and its lowest index
        float m = -INFINITY;
        arg = 0x7fffffff;
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
        wave_argmax(m, arg);

        // pass 2 (the row is in cache): sum exp(x - max), fp64 accumulation in a fixed order
        double sum = 0.0;
        for (int k = lane; k < chunks; k += kWave) {
            const float4 v = load_chunk<VEC>(row, k, C);
            sum += (double)expf(v.x - m);
            sum += (double)expf(v.y - m);
            sum += (double)expf(v.z - m);
            sum += (double)expf(v.w - m);
        }
        sum = wave_reduce(sum, SumOp());
        const float xl = row[label];
        const double term = ((double)m + log(sum)) - (double)xl;

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
        return term;
    }
};

}  // namespace

template <bool VEC>
__global__ __launch_bounds__(kClsThreads) void cls_loss_rows_kernel(const float *__restrict__ scores, int64_t ld,
                                                                    const int64_t *__restrict__ labels, int64_t R, int C,
                                                                    int64_t ignore_index, float *__restrict__ dscores,
                                                                    ClsPartial *__restrict__ partials)
{
    __shared__ int red_n[kClsRowsPerBlock];
    SoftmaxLoss policy = {ignore_index, 0.0};

    // the gradient's 1 / n_valid: every block counts the rows that count (integers: the same in every block and every run)
    if (dscores) {
        const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
        int n = 0;
        for (int64_t r = threadIdx.x; r < R; r += kClsThreads) n += policy.counts(labels[r], C) ? 1 : 0;
        n = wave_reduce(n, SumOp());
        if (lane == 0) red_n[wave] = n;
        __syncthreads();
        n = 0;
#pragma unroll
        for (int w = 0; w < kClsRowsPerBlock; w++) n += red_n[w];
        policy.inv_n = n > 0 ? 1.0 / (double)n : 0.0;
    }
    cls_loss_rows<VEC>(policy, scores, ld, labels, R, C, dscores, partials);
}

}  // namespace locov

using namespace locov;

extern "C" int64_t locov_cls_loss_workspace_bytes(int64_t R) { return cls_workspace_bytes(R); }

extern "C" int locov_cls_loss(const float *scores, int64_t ld, const int64_t *gt_classes, int64_t R, int C, int64_t ignore_index,
                              void *workspace, int64_t workspace_bytes, float *loss, float *dscores, int64_t *stats,
                              locov_stream_t stream)
{
    LOCOV_REQUIRE(R >= 0 && C >= 1, "locov_cls_loss: R >= 0 and C >= 1 required (R %lld, C %d)", (long long)R, C);
    return cls_loss_launch<true>("locov_cls_loss", scores, ld, gt_classes, R, C, workspace, workspace_bytes, loss, dscores, stats, stream,
                                 [&](bool vec, int blocks, ClsPartial *partials) {
                                     hipLaunchKernelGGL(vec ? cls_loss_rows_kernel<true> : cls_loss_rows_kernel<false>, dim3(blocks),
                                                        dim3(kClsThreads), 0, as_stream(stream), scores, ld, gt_classes, R, C,
                                                        ignore_index, dscores, partials);
                                 });
}
