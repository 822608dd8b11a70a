// Class-agnostic proposal recall, AR at a few proposal limits and area ranges (Detectron2's _evaluate_box_proposals, which its
// COCOEvaluator and LVISEvaluator report as "box_proposals").  locov_amd/evaluation.py states the protocol; proposal_recall_host
// there is the definition, and everything here is fp32 rounded step by step (the file is compiled with -ffp-contract=off) and
// integers, so the outputs equal it bit for bit.
//
// locov_proposal_recall: one workgroup of 256 threads per (image, area range, limit).
//   The image's first `limit` proposals (they arrive in descending objectness) go into LDS.  A gt of the image is a COLUMN, a
//   proposal a ROW.  No IoU matrix is kept: per column the workgroup caches (the largest IoU over the unused rows, its lowest
//   row) as one 64-bit word, IoU bits above ~row -- a non-negative fp32 orders like its bits, so the largest word is the largest
//   IoU at the lowest row.  Waves take columns, lanes stride rows, a wave reduction fills the cache.
//   A step of the greedy matching is a workgroup argmax over the unused columns of (IoU bits, ~column): the largest IoU, at the
//   lowest gt, at that gt's lowest row.  The row and the column get a bit in the used masks, and only the columns whose cached
//   row was the one just taken are formed again, over the rows still unused.  A column whose cached IoU is 0 is never formed
//   again: its value cannot rise, and the walk ends at the first step whose maximum is 0 (the rest of the overlaps are 0).
//   That is P * G + (columns formed again) * P IoUs per workgroup where the literal loop reads min(P, G) * P * G.
//   The gts outside the area range, and the ones the caller leaves out (gt_skip: COCO's crowd), start as used columns.
#include "reduce_common.h"
#include "select_common.h"

namespace locov {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxGt = LOCOV_PROPOSAL_RECALL_MAX_GT;
constexpr int kMaxLimit = LOCOV_PROPOSAL_RECALL_MAX_LIMIT;

typedef unsigned long long u64;

struct RecallArgs {
    float lo[LOCOV_COCO_MAX_AREAS], hi[LOCOV_COCO_MAX_AREAS], thr[LOCOV_COCO_MAX_THRESHOLDS];
    int limit[LOCOV_PROPOSAL_RECALL_MAX_LIMITS];
    int A, L, T;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ u64 wave_max(u64 v) { return wave_reduce(v, MaxOp()); }

__device__ __forceinline__ bool bit_set(const unsigned *mask, int i) { return (mask[i >> 5] >> (i & 31)) & 1u; }

// (the largest IoU of gt box `g` over the unused rows, its lowest row) as one word, by a whole wave; 0 with no unused row
__device__ __forceinline__ u64 column_key(const float4 g, const float4 *rows, int P, const unsigned *row_used, int lane)
{
    u64 key = 0;
    for (int r = lane; r < P; r += kWave) {
        if (bit_set(row_used, r)) continue;
        const u64 k = ((u64)__float_as_uint(box_pairwise_iou(g, rows[r])) << 32) | (u64)(0xffffffffu - (unsigned)r);
        key = k > key ? k : key;
    }
    return wave_max(key);
}

__global__ __launch_bounds__(kThreads) void proposal_recall_kernel(const int *__restrict__ prop_off, const int *__restrict__ gt_off,
                                                                   int n_prop, int n_gt, int max_gt,
                                                                   const float4 *__restrict__ prop_box,
                                                                   const float4 *__restrict__ gt_box, const float *__restrict__ gt_area,
                                                                   const uint8_t *__restrict__ gt_skip, RecallArgs args,
                                                                   float *__restrict__ gt_overlaps, int *__restrict__ counts)
{
    extern __shared__ float4 s_box[];                      // the image's first `limit` proposals
    __shared__ u64 s_col[kMaxGt];                          // per gt: IoU bits << 32 | ~row
    __shared__ unsigned s_row_used[kMaxLimit / 32], s_col_used[kMaxGt / 32];
    __shared__ u64 s_wmax[kWaves];
    __shared__ int s_n[2];                                 // the image's gts that count at all / in this range
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int A = args.A, L = args.L, T = args.T;
    int b = blockIdx.x;
    const int l = b % L;
    b /= L;
    const int a = b % A;
    const int img = b / A;
    const float lo = args.lo[a], hi = args.hi[a];

    // the offsets are device data the entry point cannot check: clamped, a descending pair is an empty image
    const int p0 = clampi(prop_off[img], 0, n_prop);
    const int P = min(clampi(prop_off[img + 1], p0, n_prop) - p0, args.limit[l]);
    const int g0 = clampi(gt_off[img], 0, n_gt);
    const int seg = clampi(gt_off[img + 1], g0, n_gt) - g0;
    const int G = min(seg, max_gt);                        // (max_gt <= kMaxGt: the entry point's check)
    float *out = gt_overlaps + (int64_t)(a * L + l) * n_gt + g0;
    int *cnt = counts + ((int64_t)img * A * L + a * L + l) * (T + 1);

    for (int w = tid; w < kMaxLimit / 32; w += kThreads) s_row_used[w] = 0u;
    if (tid < 2) s_n[tid] = 0;
    __syncthreads();
    for (int base = 0; base < kMaxGt; base += kThreads) {  // a column outside the range, or left out, is used from the start
        const int c = base + tid;
        bool counted = false, in_range = false;
        if (c < G) {
            counted = !(gt_skip && gt_skip[g0 + c]);
            const float ar = gt_area[g0 + c];
            in_range = counted && ar >= lo && ar <= hi;
        }
        const u64 bc = __ballot(counted), br = __ballot(in_range);
        if (lane == 0) {
            s_col_used[(base >> 5) + 2 * wave] = ~(unsigned)br;
            s_col_used[(base >> 5) + 2 * wave + 1] = ~(unsigned)(br >> 32);
            if (bc) atomicAdd(&s_n[0], __popcll(bc));
            if (br) atomicAdd(&s_n[1], __popcll(br));
        }
    }
    for (int r = tid; r < P; r += kThreads) s_box[r] = prop_box[p0 + r];
    __syncthreads();
    const int n_all = s_n[0], n_in = s_n[1];
    if (n_all == 0 || P == 0) {                            // a skipped image: it adds nothing, not even to num_pos
        for (int j = tid; j < seg; j += kThreads) out[j] = 0.f;
        if (tid <= T) cnt[tid] = 0;
        return;
    }

    for (int c = wave; c < G; c += kWaves) {               // (uniform per wave)
        if (bit_set(s_col_used, c)) continue;
        const u64 key = column_key(gt_box[g0 + c], s_box, P, s_row_used, lane);
        if (lane == 0) s_col[c] = key;
    }
    __syncthreads();

    const int steps = P < n_in ? P : n_in;
    const float thr = tid < T ? args.thr[tid] : 0.f;
    int reached = 0, done = 0;
    for (; done < steps; done++) {
        u64 best = 0;                                      // (an unused column's word is never 0: its low half is ~column)
        for (int c = tid; c < G; c += kThreads)
            if (!bit_set(s_col_used, c)) {
                const u64 k = (s_col[c] & 0xffffffff00000000ull) | (u64)(0xffffffffu - (unsigned)c);
                best = k > best ? k : best;
            }
        best = wave_max(best);
        if (lane == 0) s_wmax[wave] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; w++) best = s_wmax[w] > best ? s_wmax[w] : best;
        const float v = __uint_as_float((unsigned)(best >> 32));
        if (!(v > 0.f)) break;                             // (uniform) the maxima never rise: every later overlap is 0
        const int c = (int)(0xffffffffu - (unsigned)best);
        const int r = (int)(0xffffffffu - (unsigned)s_col[c]);
        reached += v >= thr ? 1 : 0;
        if (tid == 0) {
            out[done] = v;
            s_row_used[r >> 5] |= 1u << (r & 31);
            s_col_used[c >> 5] |= 1u << (c & 31);
        }
        __syncthreads();                                   // the two bits are set; s_wmax and s_col[c] have been read
        for (int k = wave; k < G; k += kWaves) {           // the columns that lost their cached row
            if (bit_set(s_col_used, k)) continue;
            const u64 old = s_col[k];
            if ((int)(0xffffffffu - (unsigned)old) != r || (old >> 32) == 0) continue;
            const u64 key = column_key(gt_box[g0 + k], s_box, P, s_row_used, lane);
            if (lane == 0) s_col[k] = key;
        }
        __syncthreads();
    }
    for (int j = done + tid; j < seg; j += kThreads) out[j] = 0.f;
    if (tid < T) cnt[tid] = reached;
    if (tid == T) cnt[T] = n_in;
}

}  // namespace

}  // namespace locov

using namespace locov;

extern "C" int locov_proposal_recall(const int *prop_offsets, const int *gt_offsets, int n_images, int n_prop, int n_gt,
                                     int max_gt_per_image, const float *prop_boxes, const float *gt_boxes, const float *gt_area,
                                     const uint8_t *gt_skip, const float *area_ranges_host, int n_areas, const int *limits_host,
                                     int n_limits, const float *iou_thresholds_host, int n_thresholds, float *gt_overlaps,
                                     int *counts, locov_stream_t stream)
{
    const char *who = "locov_proposal_recall";
    LOCOV_REQUIRE(n_images >= 0 && n_prop >= 0 && n_gt >= 0 && max_gt_per_image >= 0, "%s: negative count", who);
    LOCOV_REQUIRE(n_areas >= 1 && n_areas <= LOCOV_COCO_MAX_AREAS, "%s: 1..%d area ranges", who, LOCOV_COCO_MAX_AREAS);
    LOCOV_REQUIRE(n_limits >= 1 && n_limits <= LOCOV_PROPOSAL_RECALL_MAX_LIMITS, "%s: 1..%d proposal limits", who,
                  LOCOV_PROPOSAL_RECALL_MAX_LIMITS);
    LOCOV_REQUIRE(n_thresholds >= 1 && n_thresholds <= LOCOV_COCO_MAX_THRESHOLDS, "%s: 1..%d IoU thresholds", who,
                  LOCOV_COCO_MAX_THRESHOLDS);
    LOCOV_REQUIRE(area_ranges_host && limits_host && iou_thresholds_host, "%s: null area range, limit or threshold list", who);
    for (int a = 0; a < n_areas; a++)
        LOCOV_REQUIRE(area_ranges_host[2 * a] <= area_ranges_host[2 * a + 1], "%s: area range %d is not ascending", who, a);
    for (int l = 0; l < n_limits; l++)
        LOCOV_REQUIRE(limits_host[l] >= 1 && (l == 0 || limits_host[l] > limits_host[l - 1]),
                      "%s: the proposal limits must be positive and ascending", who);
    if (n_images == 0 || (n_prop == 0 && n_gt == 0)) return LOCOV_OK;
    const int64_t blocks = (int64_t)n_images * n_areas * n_limits;
    if (limits_host[n_limits - 1] > LOCOV_PROPOSAL_RECALL_MAX_LIMIT || max_gt_per_image > LOCOV_PROPOSAL_RECALL_MAX_GT ||
        blocks > LOCOV_COCO_MAX_BLOCKS)
        return set_error(LOCOV_ERR_UNSUPPORTED, "%s: at most %d proposals and %d gts per image, images x ranges x limits at most %d",
                         who, LOCOV_PROPOSAL_RECALL_MAX_LIMIT, LOCOV_PROPOSAL_RECALL_MAX_GT, LOCOV_COCO_MAX_BLOCKS);
    LOCOV_REQUIRE(prop_offsets && gt_offsets && counts, "%s: null offsets or counts", who);
    LOCOV_REQUIRE(n_prop == 0 || prop_boxes, "%s: null proposal pointer", who);
    LOCOV_REQUIRE(n_gt == 0 || (gt_boxes && gt_area && gt_overlaps), "%s: null gt pointer", who);
    LOCOV_REQUIRE((uintptr_t)prop_boxes % 16 == 0 && (uintptr_t)gt_boxes % 16 == 0 && (uintptr_t)gt_area % 4 == 0 &&
                      (uintptr_t)prop_offsets % 4 == 0 && (uintptr_t)gt_offsets % 4 == 0 && (uintptr_t)gt_overlaps % 4 == 0 &&
                      (uintptr_t)counts % 4 == 0,
                  "%s: misaligned pointer", who);
    RecallArgs args{};
    for (int a = 0; a < n_areas; a++) {
        args.lo[a] = area_ranges_host[2 * a];
        args.hi[a] = area_ranges_host[2 * a + 1];
    }
    for (int l = 0; l < n_limits; l++) args.limit[l] = limits_host[l];
    for (int t = 0; t < n_thresholds; t++) args.thr[t] = iou_thresholds_host[t];
    args.A = n_areas;
    args.L = n_limits;
    args.T = n_thresholds;
    const size_t lds = (size_t)limits_host[n_limits - 1] * sizeof(float4);      // at most 32 KiB beside 9 KiB of static LDS
    hipLaunchKernelGGL(proposal_recall_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, as_stream(stream), prop_offsets, gt_offsets,
                       n_prop, n_gt, max_gt_per_image, reinterpret_cast<const float4 *>(prop_boxes),
                       reinterpret_cast<const float4 *>(gt_boxes), gt_area, gt_skip, args, gt_overlaps, counts);
    return check_launch(who);
}
