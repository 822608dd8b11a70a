// The proposal side of the dataset mapper as ONE launch for the whole batch (data.py: transform_proposals, change_proposals_as_gt):
//   locov_map_proposals : the images' precomputed proposals, read in place from the device store, through the resize factor and the
//                         flip (Transform.apply_box: the corners, then their min / max, per transform), rounded to fp32, clipped, the
//                         empty boxes dropped, the first topk kept; and of those the rows with logit > thr as the pseudo ground truth.
// Compiled with -ffp-contract=off: every product and difference rounds on its own, in the rows' dtype, as the numpy ops they stand for.
// The per-image tables travel in a by-value argument struct (the idiom of image_batch.hip): no H2D copy, no workspace.
#include "box_clip_common.h"
#include "select_common.h"

namespace locov {
namespace {

struct ProposalMapArgs {
    int64_t row_start[LOCOV_LABEL_MAX_IMAGES];                   // image i reads store rows [row_start[i], row_start[i] + n_rows[i])
    double fx[LOCOV_LABEL_MAX_IMAGES], fy[LOCOV_LABEL_MAX_IMAGES];       // new_w * 1.0 / w, new_h * 1.0 / h as the host's doubles
    int n_rows[LOCOV_LABEL_MAX_IMAGES], out_off[LOCOV_LABEL_MAX_IMAGES]; // its output segment: [out_off[i], out_off[i] + n_rows[i])
    int new_h[LOCOV_LABEL_MAX_IMAGES], new_w[LOCOV_LABEL_MAX_IMAGES];
    uint8_t flip[LOCOV_LABEL_MAX_IMAGES];
};

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }

// ndarray.min / .max over the corners of one axis: a NaN end makes both NaN (the row is then empty)
template <typename T>
__device__ __forceinline__ void ordered(T a, T b, T &lo, T &hi)
{
    if (a != a || b != b) {
        lo = hi = a != a ? a : b;
    } else {
        lo = a < b ? a : b;
        hi = a < b ? b : a;
    }
}

// One axis of one row: ResizeTransform.apply_box, the flip's apply_box when this is the flipped axis, Boxes' fp32, Boxes.clip.
template <typename T>
__device__ __forceinline__ void map_axis(T a, T b, T factor, bool flipped, int size, float &lo32, float &hi32)
{
    T lo, hi;
    ordered(mul_rn(a, factor), mul_rn(b, factor), lo, hi);
    if (flipped) ordered(sub_rn((T)size, lo), sub_rn((T)size, hi), lo, hi);
    lo32 = clamp_like_torch((float)lo, (float)size);
    hi32 = clamp_like_torch((float)hi, (float)size);
}

// One workgroup per image, 256 rows at a time.  Two block_ballot_ranks give every kept row its place in the proposal list and,
// behind the cut at topk, every row above the threshold its place in the pseudo-GT list.  The counts are carried from chunk to chunk,
// the same in every lane; the LDS counts alternate between two buffers, so a chunk needs the ranks' two barriers and no third.
template <typename T>
__global__ __launch_bounds__(256) void map_proposals_kernel(const T *__restrict__ rows, ProposalMapArgs a, int topk, float thr,
                                                            float4 *__restrict__ prop_boxes, float *__restrict__ prop_logits,
                                                            int64_t *__restrict__ prop_src, float4 *__restrict__ gt_boxes,
                                                            float *__restrict__ gt_logits, int64_t *__restrict__ gt_classes,
                                                            int64_t *__restrict__ gt_src, int *__restrict__ counts)
{
    __shared__ int wave_count[2][2][4];                           // [chunk parity][proposals, pseudo-GT][wave]
    const int img = blockIdx.x, n = a.n_rows[img];
    const int64_t out = a.out_off[img];
    const T *src = rows + a.row_start[img] * 5;
    const T fx = (T)a.fx[img], fy = (T)a.fy[img];                 // (the weak Python scalar, rounded ONCE to the array's dtype)
    const int flip = a.flip[img], W = a.new_w[img], H = a.new_h[img];
    const int tid = threadIdx.x;
    int kept = 0, gt_kept = 0, parity = 0;
    for (int base = 0; base < n && kept < topk; base += 256, parity ^= 1) {
        const int r = base + tid;
        bool keep = false;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        float logit = 0.f;
        if (r < n) {
            const T *p = src + (int64_t)r * 5;
            map_axis<T>(p[0], p[2], fx, flip == LOCOV_FLIP_HORIZONTAL, W, b.x, b.z);
            map_axis<T>(p[1], p[3], fy, flip == LOCOV_FLIP_VERTICAL, H, b.y, b.w);
            logit = (float)p[4];
            keep = (__fsub_rn(b.z, b.x) > 0.f) && (__fsub_rn(b.w, b.y) > 0.f);
        }
        int all, gt_all;
        const int at = kept + block_ballot_rank<256>(keep, wave_count[parity][0], all);
        const bool take = keep && at < topk;
        const bool as_gt = take && logit > thr;
        const int gt_at = gt_kept + block_ballot_rank<256>(as_gt, wave_count[parity][1], gt_all);
        if (take) {
            prop_boxes[out + at] = b;
            prop_logits[out + at] = logit;
            prop_src[out + at] = r;
        }
        if (as_gt) {
            gt_boxes[out + gt_at] = b;
            gt_logits[out + gt_at] = logit;
            gt_classes[out + gt_at] = 1;
            gt_src[out + gt_at] = r;
        }
        kept += all;
        gt_kept += gt_all;
    }
    kept = kept < topk ? kept : topk;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = kept + tid; r < n; r += 256) {
        prop_boxes[out + r] = zero;
        prop_logits[out + r] = 0.f;
        prop_src[out + r] = -1;
    }
    for (int r = gt_kept + tid; r < n; r += 256) {
        gt_boxes[out + r] = zero;
        gt_logits[out + r] = 0.f;
        gt_classes[out + r] = 0;
        gt_src[out + r] = -1;
    }
    if (tid == 0) {
        counts[2 * img] = kept;
        counts[2 * img + 1] = gt_kept;
    }
}

}  // namespace
}  // namespace locov

using namespace locov;

extern "C" {

int locov_map_proposals(const void *rows, int64_t n_store_rows, int dtype, const int64_t *row_start_host, const int *n_rows_host,
                        const double *fx_host, const double *fy_host, const int *flips_host, const int *new_h_host,
                        const int *new_w_host, int n_images, int topk, float thr, float *prop_boxes, float *prop_logits,
                        int64_t *prop_src, float *gt_boxes, float *gt_logits, int64_t *gt_classes, int64_t *gt_src, int *counts,
                        locov_stream_t stream)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= LOCOV_LABEL_MAX_IMAGES, "locov_map_proposals: 0..%d images per call", LOCOV_LABEL_MAX_IMAGES);
    if (n_images == 0) return LOCOV_OK;
    LOCOV_REQUIRE(dtype == LOCOV_PROPOSAL_F32 || dtype == LOCOV_PROPOSAL_F64, "locov_map_proposals: unknown dtype %d", dtype);
    LOCOV_REQUIRE(topk >= 0, "locov_map_proposals: topk must not be negative, got %d", topk);
    LOCOV_REQUIRE(n_store_rows >= 0, "locov_map_proposals: the store cannot have %lld rows", (long long)n_store_rows);
    LOCOV_REQUIRE(row_start_host && n_rows_host && fx_host && fy_host && flips_host && new_h_host && new_w_host && counts,
                  "locov_map_proposals: null pointer");
    LOCOV_REQUIRE((uintptr_t)counts % 4 == 0, "locov_map_proposals: counts must be 4-byte aligned");
    ProposalMapArgs a{};
    int64_t total = 0;
    for (int i = 0; i < n_images; i++) {
        const int n = n_rows_host[i], flip = flips_host[i];
        LOCOV_REQUIRE(n >= 0, "locov_map_proposals: image %d: a negative row count %d", i, n);
        LOCOV_REQUIRE(row_start_host[i] >= 0 && row_start_host[i] <= n_store_rows - n,
                      "locov_map_proposals: image %d: rows [%lld, %lld + %d) leave the store's %lld rows", i, (long long)row_start_host[i],
                      (long long)row_start_host[i], n, (long long)n_store_rows);
        LOCOV_REQUIRE(flip == LOCOV_FLIP_NONE || flip == LOCOV_FLIP_HORIZONTAL || flip == LOCOV_FLIP_VERTICAL,
                      "locov_map_proposals: image %d: unknown flip %d", i, flip);
        LOCOV_REQUIRE(new_h_host[i] >= 0 && new_w_host[i] >= 0, "locov_map_proposals: image %d: a negative size %d x %d", i, new_h_host[i],
                      new_w_host[i]);
        LOCOV_REQUIRE(total + n <= INT32_MAX, "locov_map_proposals: the batch's rows leave int32 at image %d", i);
        a.row_start[i] = row_start_host[i];
        a.fx[i] = fx_host[i];
        a.fy[i] = fy_host[i];
        a.n_rows[i] = n;
        a.out_off[i] = (int)total;
        a.new_h[i] = new_h_host[i];
        a.new_w[i] = new_w_host[i];
        a.flip[i] = (uint8_t)flip;
        total += n;
    }
    if (total > 0) {
        LOCOV_REQUIRE(rows && prop_boxes && prop_logits && prop_src && gt_boxes && gt_logits && gt_classes && gt_src,
                      "locov_map_proposals: null pointer");
        LOCOV_REQUIRE((uintptr_t)rows % (dtype == LOCOV_PROPOSAL_F32 ? 4 : 8) == 0, "locov_map_proposals: rows must be aligned to its element size");
        LOCOV_REQUIRE((uintptr_t)prop_boxes % 16 == 0 && (uintptr_t)gt_boxes % 16 == 0 && (uintptr_t)prop_logits % 4 == 0 &&
                          (uintptr_t)gt_logits % 4 == 0 && (uintptr_t)prop_src % 8 == 0 && (uintptr_t)gt_src % 8 == 0 &&
                          (uintptr_t)gt_classes % 8 == 0,
                      "locov_map_proposals: the box outputs must be 16-byte aligned, the int64 outputs 8-byte, the logits 4-byte aligned");
    }
    if (dtype == LOCOV_PROPOSAL_F32)
        hipLaunchKernelGGL(map_proposals_kernel<float>, dim3((unsigned)n_images), dim3(256), 0, as_stream(stream),
                           static_cast<const float *>(rows), a, topk, thr, reinterpret_cast<float4 *>(prop_boxes), prop_logits, prop_src,
                           reinterpret_cast<float4 *>(gt_boxes), gt_logits, gt_classes, gt_src, counts);
    else
        hipLaunchKernelGGL(map_proposals_kernel<double>, dim3((unsigned)n_images), dim3(256), 0, as_stream(stream),
                           static_cast<const double *>(rows), a, topk, thr, reinterpret_cast<float4 *>(prop_boxes), prop_logits, prop_src,
                           reinterpret_cast<float4 *>(gt_boxes), gt_logits, gt_classes, gt_src, counts);
    return check_launch("locov_map_proposals");
}

}  // extern "C"
