// The frame the classification-loss kernels share (cls_loss.hip: softmax cross-entropy; sigmoid_loss.hip: per-class sigmoid with an
// optional class mask).  Two launches: a row kernel (one wave per row, kClsRowsPerBlock rows per block, grid-stride over the row
// groups) writes the gradient and one partial per block; cls_loss_finish_kernel (one block) adds the partials in block-index order.
// No atomics: the same inputs give the same bits.  A row's element -> lane assignment is the same with 16-byte loads and with scalar
// ones, so a column slice of a wider matrix gives the bits of its contiguous copy.
//
// A loss is a policy type with
//   bool counts(int64_t y, int C) const     -- does a row with the label y enter the loss
//   bool invalid(int64_t y) const           -- (asked of a row that does not count) is it counted in num_invalid
//   template <bool VEC> double row_term(const float *row, float *drow, int label, int C, int lane, int chunks, int &arg) const
//                                           -- one counted row: returns its loss term and in `arg` its lowest argmax (both the same in
//                                              every lane), and writes its gradient to drow unless that is null
// Neither file has per-file compile flags (build.py FILE_FLAGS): the contraction setting is part of the bits.
#pragma once
#include "reduce_common.h"

#include <cmath>

namespace locov {

constexpr int kClsRowsPerBlock = 4;
constexpr int kClsThreads = kClsRowsPerBlock * kWave;
constexpr int kClsMaxBlocks = 1024;
constexpr int kClsFinishThreads = 256;

// what a block hands to the finishing launch (32 bytes)
struct ClsPartial {
    double loss;                                                     // sum of the rows' loss terms
    int n_valid, n_fg, n_accurate, n_fg_accurate, n_false_negative, n_invalid;
};

inline int cls_blocks(int64_t R)
{
    const int64_t groups = ceil_div(R, kClsRowsPerBlock);
    return (int)(groups < kClsMaxBlocks ? groups : kClsMaxBlocks);
}

inline int64_t cls_workspace_bytes(int64_t R) { return R > 0 ? (int64_t)cls_blocks(R) * (int64_t)sizeof(ClsPartial) : 0; }

// elements [4 * chunk, 4 * chunk + 4) of a row of C logits; past the end: -inf (no weight in a maximum or in a softmax sum)
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

// [D2-upstream, unverified] _log_classification_stats for one counted row: label < bg is foreground, arg the predicted class
__device__ __forceinline__ void tally_row(ClsPartial &acc, int label, int arg, int bg)
{
    const bool fg = label < bg, hit = arg == label;
    acc.n_fg += fg ? 1 : 0;
    acc.n_accurate += hit ? 1 : 0;
    acc.n_fg_accurate += fg && hit ? 1 : 0;
    acc.n_false_negative += fg && arg == bg ? 1 : 0;
}

// the exactly zero gradient of a row that does not count
template <bool VEC>
__device__ __forceinline__ void zero_row(float *__restrict__ drow, int C, int lane, int chunks)
{
    for (int k = lane; k < chunks; k += kWave) store_chunk<VEC>(drow, k, C, make_float4(0.f, 0.f, 0.f, 0.f));
}

// The body of a row kernel (kClsThreads threads): this block's rows through the policy, then partials[blockIdx.x].
template <bool VEC, class Policy>
__device__ __forceinline__ void cls_loss_rows(const Policy &policy, const float *__restrict__ scores, int64_t ld,
                                              const int64_t *__restrict__ labels, int64_t R, int C, float *__restrict__ dscores,
                                              ClsPartial *__restrict__ partials)
{
    __shared__ ClsPartial red_p[kClsRowsPerBlock];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int bg = C - 1, chunks = (C + 3) / 4;

    ClsPartial acc = {0.0, 0, 0, 0, 0, 0, 0};                        // this wave's rows, in row order (every lane holds the same)
    for (int64_t r = (int64_t)blockIdx.x * kClsRowsPerBlock + wave; r < R; r += (int64_t)gridDim.x * kClsRowsPerBlock) {
        const int64_t y = labels[r];
        float *drow = dscores ? dscores + r * (int64_t)C : nullptr;
        if (!policy.counts(y, C)) {
            // no loss, an exactly zero gradient, and no prediction can equal such a label, so the row's logits are not read
            acc.n_invalid += policy.invalid(y) ? 1 : 0;
            if (drow) zero_row<VEC>(drow, C, lane, chunks);
            continue;
        }
        const int label = (int)y;
        int arg;
        acc.loss += policy.template row_term<VEC>(scores + r * ld, drow, label, C, lane, chunks, arg);
        acc.n_valid += 1;
        tally_row(acc, label, arg, bg);
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

// One block: thread t adds partials t, t + 256, ... in that order, then a fixed tree.  MEAN_OVER_VALID: the loss is the mean over the
// rows that count (none: 0 / 0 = NaN, as torch's mean); else the sum over R, whatever the labels (0 at R == 0).
template <bool MEAN_OVER_VALID>
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
        if constexpr (MEAN_OVER_VALID)
            loss[0] = (float)(red_loss[0] / (double)red_cnt[0][0]);
        else
            loss[0] = R > 0 ? (float)(red_loss[0] / (double)R) : 0.f;
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

// The host side of an entry `name` after its own check of R and C: the shared argument checks, then the two launches.
// launch_rows(vec, blocks, partials) enqueues the entry's row kernel, with 16-byte loads and stores where vec.
template <bool MEAN_OVER_VALID, class LaunchRows>
int cls_loss_launch(const char *name, const float *scores, int64_t ld, const int64_t *gt_classes, int64_t R, int C, void *workspace,
                    int64_t workspace_bytes, float *loss, float *dscores, int64_t *stats, locov_stream_t stream,
                    LaunchRows launch_rows)
{
    LOCOV_REQUIRE(ld >= C, "%s: row stride ld %lld is smaller than C %d", name, (long long)ld, C);
    LOCOV_REQUIRE(loss && (R == 0 || (scores && gt_classes)), "%s: null pointer", name);
    LOCOV_REQUIRE(workspace_bytes >= cls_workspace_bytes(R) && (R == 0 || workspace), "%s: workspace too small (%lld bytes, %lld needed)",
                  name, (long long)workspace_bytes, (long long)cls_workspace_bytes(R));
    LOCOV_REQUIRE((uintptr_t)workspace % 8 == 0, "%s: workspace must be 8-byte aligned", name);
    ClsPartial *partials = static_cast<ClsPartial *>(workspace);
    const int blocks = R > 0 ? cls_blocks(R) : 0;
    char what[64];
    if (blocks > 0) {
        // 16-byte loads and stores when every row of both matrices starts on a 16-byte boundary and holds whole chunks
        const bool vec = C % 4 == 0 && ld % 4 == 0 && (uintptr_t)scores % 16 == 0 && (uintptr_t)dscores % 16 == 0;
        launch_rows(vec, blocks, partials);
        snprintf(what, sizeof what, "%s (rows)", name);
        const int rc = check_launch(what);
        if (rc != LOCOV_OK) return rc;
    }
    hipLaunchKernelGGL(cls_loss_finish_kernel<MEAN_OVER_VALID>, dim3(1), dim3(kClsFinishThreads), 0, as_stream(stream), partials, blocks,
                       R, loss, stats);
    snprintf(what, sizeof what, "%s (finish)", name);
    return check_launch(what);
}

}  // namespace locov
