// The building blocks of every box-selection pipeline, ONE copy each: the IoU predicates, the block-wide scan and the radix digit
// pick on top of it, the wave-level compacting append, the candidate key layout and the small index helpers.  Users: nms.hip,
// detect.hip, detect_wide.hip, rpn.hip, rpn_train.hip, label.hip, image_batch.hip, proposal_map.hip (rpn_select_kernel alone keeps its own text of the scan, the pick
// and the append: see the comment there).  Only __forceinline__ functions and constants live here -- no
// kernels, no global state -- and a new selection kernel starts from these instead of copying a neighbour.
//
// The IoU functions reproduce torch ops rounding by rounding: a file that calls them is built with -ffp-contract=off (build.py).
// The wave-level helpers assume one-dimensional workgroups of whole 64-lane waves.
#pragma once
#include "common.h"

namespace locov {

// ---- IoU ------------------------------------------------------------------------------------------------------------------------------

// torchvision nms's test "IoU(a, b) > thr" on XYXY boxes: inter / (area_a + area_b - inter), every step rounded on its own.  Each
// NMS of the library decides with this function, which is what makes their keep lists agree bit for bit.
__device__ __forceinline__ bool box_iou_gt(const float4 a, const float4 b, float thr)
{
    const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
    const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
    const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
    const float inter = w * h;
    const float sa = (a.z - a.x) * (a.w - a.y), sb = (b.z - b.x) * (b.w - b.y);
    return inter / (sa + sb - inter) > thr;
}

// Detectron2's pairwise_iou of (ground-truth box a, box b): torch's ops, each rounded on its own.  The proposal labelling and both
// phases of the anchor labelling call it (the low-quality promotion's `==` needs the phases to round identically).
__device__ __forceinline__ float box_pairwise_iou(const float4 a, const float4 b)
{
    const float area_a = (a.z - a.x) * (a.w - a.y);
    const float area_b = (b.z - b.x) * (b.w - b.y);
    float w = fminf(a.z, b.z) - fmaxf(a.x, b.x), h = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    // torch.min / torch.max propagate NaN (fminf / fmaxf do not); clamp_(min=0) keeps it
    if (a.z != a.z || b.z != b.z || a.x != a.x || b.x != b.x) w = __builtin_nanf("");
    if (a.w != a.w || b.w != b.w || a.y != a.y || b.y != b.y) h = __builtin_nanf("");
    w = w < 0.f ? 0.f : w;
    h = h < 0.f ? 0.f : h;
    const float inter = w * h;
    return inter > 0.f ? inter / ((area_a + area_b) - inter) : 0.f;
}

// ---- wave level (the reductions -- wave_reduce, wave_argmax, block_tree_reduce -- are reduce_common.h's) ------------------------------

// how many of the lanes below this one have their bit set in a ballot
__device__ __forceinline__ int lanes_below(unsigned long long ballot)
{
    return __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// Compacting append, called by a whole wave: the lanes with `take` get consecutive slots behind *cursor (one atomic add per wave
// that has a taker, in lane order inside the wave); the value returned to the other lanes means nothing.
__device__ __forceinline__ int wave_append(bool take, int *cursor)
{
    const unsigned long long b = __ballot(take);
    if (!b) return 0;                           // (uniform: most waves of a sparse gather leave here)
    int at = 0;
    if ((threadIdx.x & 63) == 0) at = atomicAdd(cursor, __popcll(b));
    return __shfl(at, 0) + lanes_below(b);
}

// lane j's box (j uniform over the wave)
__device__ __forceinline__ float4 lane_box(const float4 v, int j)
{
    float4 e;
    e.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), j));
    e.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), j));
    e.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.z), j));
    e.w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.w), j));
    return e;
}

// ---- block level ----------------------------------------------------------------------------------------------------------------------

// Exclusive scan over a workgroup of kThreads threads: returns the sum of v over the threads below this one.  ONE __syncthreads()
// inside, between the write of wave_sum[] (one int per wave: the wave's total) and its reads.  The workgroup's total is what the
// LAST thread gets plus its own v (the carry of a chunked scan).  Before the next call the caller needs a barrier of its own:
// wave_sum[] is still being read when the first thread returns.
template <int kThreads>
__device__ __forceinline__ int block_exclusive_scan(int v, int (&wave_sum)[kThreads / 64])
{
    static_assert(kThreads % 64 == 0, "block_exclusive_scan: whole waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = incl - v;
    for (int w = 0; w < wave; w++) before += wave_sum[w];
    return before;
}

// Ordered rank over a workgroup of kThreads threads: returns how many of the threads below this one have `flag` set, and leaves the
// workgroup's number of flagged threads in `total` (the same in every thread).  One ballot per wave and ONE __syncthreads() inside,
// between the write of wave_count[] (one int per wave: its flagged lanes) and its reads; as with block_exclusive_scan the caller
// owns the barrier before wave_count[] is written again (it is still being read when the first thread returns).
template <int kThreads>
__device__ __forceinline__ int block_ballot_rank(bool flag, int (&wave_count)[kThreads / 64], int &total)
{
    static_assert(kThreads % 64 == 0, "block_ballot_rank: whole waves");
    const int wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0) wave_count[wave] = __popcll(b);
    __syncthreads();
    int below = lanes_below(b);
    total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        const int c = wave_count[w];
        below += w < wave ? c : 0;
        total += c;
    }
    return below;
}

// One digit of a radix select by a workgroup of kThreads threads.  Thread t holds the counts v[] of bins t * kPer .. t * kPer + kPer - 1 of the digit's histogram; the
// need-th key (1 <= need <= keys counted) lies in exactly one bin, whose owner leaves  ctl[0] = the bin, ctl[1] = keys in the bins
// before it, ctl[2] = keys in it.  TWO __syncthreads() inside: the scan's, and one behind the write of ctl[], so every thread may
// read ctl[] on return.  Filling the histogram, the prefix / threshold bookkeeping and the stop rule stay with the kernel, and so
// does the barrier in front of the next pass (ctl[] and wave_sum[] are written again there).
template <int kThreads, int kPer>
__device__ __forceinline__ void radix_pick(const int (&v)[kPer], int need, int (&wave_sum)[kThreads / 64], int *ctl)
{
    int sum = 0;
#pragma unroll
    for (int q = 0; q < kPer; q++) sum += v[q];
    int cum = block_exclusive_scan<kThreads>(sum, wave_sum);
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        if (cum < need && need <= cum + v[q]) {
            ctl[0] = (int)threadIdx.x * kPer + q;
            ctl[1] = cum;
            ctl[2] = v[q];
        }
        cum += v[q];
    }
    __syncthreads();
}

// ---- candidate keys -------------------------------------------------------------------------------------------------------------------

// A candidate's row (proposal of its image) takes kKeyRowBits and its class kKeyClsBits of a 64-bit key, beside the 32 bits of
// ~score: the documented limits of the detection entry points (ops.py states them as DETECT_MAX_ROWS_PER_IMAGE / DETECT_MAX_CLASSES).
constexpr int kKeyRowBits = 14, kKeyScoreBits = 32, kKeyClsBits = 15;
constexpr unsigned long long kKeyRowMask = (1ull << kKeyRowBits) - 1ull, kKeyClsMask = (1ull << kKeyClsBits) - 1ull;

// segment key  ~score << 14 | row  (the order inside a class: descending score, ties by row; nothing above the score's 32 bits) ->
// merge key  ~score << 29 | row << 15 | class  (the order of the detections: descending score, ties by row, then class)
__device__ __forceinline__ unsigned long long merge_key(unsigned long long sort_key, int cls)
{
    return ((sort_key >> kKeyRowBits) << (kKeyRowBits + kKeyClsBits)) | ((sort_key & kKeyRowMask) << kKeyClsBits) | (unsigned long long)cls;
}

// Slots img * topk + j for j in [from, topk): no detection -- box 0, score 0, class -1, row -1 (every slot of a call is written).
template <int kThreads>
__device__ __forceinline__ void empty_detections_write_out(int from, int img, int topk, float4 *out_boxes, float *out_scores,
                                                           int64_t *out_classes, int64_t *out_rows)
{
    for (int j = from + threadIdx.x; j < topk; j += kThreads) {
        const int64_t slot = (int64_t)img * topk + j;
        out_boxes[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
        out_scores[slot] = 0.f;
        out_classes[slot] = -1;
        out_rows[slot] = -1;
    }
}

// The first `count` of an image's sorted merge keys as detections: box (of candidate (row, class): gbox[row * bk + class * cs]),
// score, class and row into slots img * topk + j; the slots behind them are written as empty.
template <int kThreads>
__device__ __forceinline__ void merge_keys_write_out(const unsigned long long *key, int count, const float4 *gbox, int bk, int cs, int img,
                                                     int topk, float4 *out_boxes, float *out_scores, int64_t *out_classes,
                                                     int64_t *out_rows)
{
    for (int j = threadIdx.x; j < count; j += kThreads) {
        const unsigned long long k = key[j];
        const int cls = (int)(k & kKeyClsMask), row = (int)((k >> kKeyClsBits) & kKeyRowMask);
        const int64_t slot = (int64_t)img * topk + j;
        out_boxes[slot] = gbox[row * bk + cls * cs];
        out_scores[slot] = __uint_as_float(~(unsigned)(k >> (kKeyRowBits + kKeyClsBits)));
        out_classes[slot] = cls;
        out_rows[slot] = row;
    }
    empty_detections_write_out<kThreads>(count, img, topk, out_boxes, out_scores, out_classes, out_rows);
}

// ---- small things ---------------------------------------------------------------------------------------------------------------------

// the smallest floor * 2^k at or above n (floor a power of two: the result is one)
__host__ __device__ __forceinline__ int next_pow2(int n, int floor)
{
    int p = floor;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace locov
