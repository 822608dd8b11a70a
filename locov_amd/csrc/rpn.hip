// RPN proposal generation of one feature level on the device: select, decode, NMS, top-k -- three launches, no host read.
//
// What Detectron2's find_top_rpn_proposals does per image with torch ops and torchvision's batched_nms (top-k of the objectness
// logits, gather, Box2BoxTransform.apply_deltas, the finite test, Boxes.clip, nonempty(min_box_size), NMS, slice), stated as one
// operation in include/locov_hip.h.  The order is fixed where torch.topk leaves it open: descending logit, ties by ascending anchor
// index (-0.0 and +0.0 tie).  ops.nms sweeps one box per barrier, which at 12 000 boxes is 12 000 barriers; here the greedy sweep
// resolves 64 boxes per barrier and stops as soon as post_nms_topk survivors exist (the greedy prefix is final).
//
//   rpn_select_kernel    a workgroup per image: radix select (11 bits a pass) of the P-th key  ~ordered(logit) << 22 | index  with
//                        the histograms in LDS; ends as soon as the keys below a threshold number at least P and fit the sort
//                        buffer; those keys are gathered and sorted in LDS (bitonic); the first P are decoded (det_apply_deltas),
//                        tested for inf / NaN, clipped (det_clip) and size-filtered: boxes, logits, indices in selection order and
//                        one bit per position (1 = passed the size filter)
//   rpn_overlap_kernel   the upper triangle of the P x ceil(P / 64) bit matrix: bit k of word wd of row j = box_iou_gt(box j,
//                        box 64 wd + k); a wave per (64 rows, one word column), the column's boxes handed round from their lanes
//   rpn_sweep_kernel     a workgroup per image, thread t owns word t of the removed set (filtered boxes start removed: they are
//                        never kept, so they suppress nothing).  Per 64 positions: every wave walks the diagonal 64 x 64 block in
//                        registers (the same result in all four, which saves a barrier), each thread ORs the kept rows' words into
//                        its own, wave 0 writes the survivors out.  One barrier per 64 positions; the loop ends at post_nms_topk.
//
// The select is one workgroup per image: five passes over an image's logits at most (usually two), each read coalesced from L2.
// Every cross-workgroup hand-off is a kernel boundary.
#include "detect_common.h"

namespace locov {

constexpr int kRpnIdxBits = 22;                 // anchors per image < 2^22
constexpr int kRpnMaxPre = 16384;               // keys the select's workgroup sorts in LDS (128 KB)
constexpr int kRpnDigit = 11, kRpnBins = 1 << kRpnDigit, kRpnPasses = 5;        // 54-bit keys: 10 + 4 x 11 bits
constexpr int kRpnSelThreads = 1024;
constexpr int kRpnMaxImages = LOCOV_LABEL_MAX_IMAGES;

struct RpnGeom {
    float h[kRpnMaxImages], w[kRpnMaxImages];
};

struct RpnWork {                                // per image: Pa = 64 W positions, W = ceil(P / 64) words
    float4 *boxes;                              // [n_img][Pa] decoded, clipped, in selection order
    unsigned long long *M;                      // [n_img][Pa][W] overlap bits (words wd >= row / 64 are written)
    float *slog;                                // [n_img][Pa] the selected logits (original bits)
    int *sidx;                                  // [n_img][Pa] their anchor indices
    unsigned long long *valid;                  // [n_img][W] bit = the position passed the size filter
    int *flags;
};

// ascending key order = descending logit (-0 folded onto +0), then ascending anchor index
__device__ __forceinline__ unsigned long long rpn_key(float v, int i)
{
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    const unsigned u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)(~u) << kRpnIdxBits) | (unsigned long long)(unsigned)i;
}

__global__ __launch_bounds__(kRpnSelThreads) void rpn_select_kernel(const float *__restrict__ logits, const float4 *__restrict__ deltas,
                                                                    const float4 *__restrict__ anchors, int hwa, int P, int cap, RpnGeom g,
                                                                    float inv_wx, float inv_wy, float inv_ww, float inv_wh, float scale_clamp,
                                                                    float min_size, RpnWork w)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long rpn_lds[];
    unsigned long long *skey = rpn_lds;                          // [cap]
    int *hist = reinterpret_cast<int *>(skey + cap);             // [kRpnBins]
    int *wave_sum = hist + kRpnBins;                             // [16]
    int *ctl = wave_sum + 16;                                    // picked bin, keys before it, keys in it, gather cursor
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *L = logits + (int64_t)img * hwa;

    // ---- radix select: the smallest threshold with P <= #(keys < thresh) <= cap (pre, below, thresh are uniform)
    unsigned long long pre = 0, thresh = 0;
    int below = 0;
    bool bad = false;
    for (int pass = 0; pass < kRpnPasses; pass++) {
        const int shift = kRpnDigit * (kRpnPasses - 1 - pass);
        for (int b = tid; b < kRpnBins; b += kRpnSelThreads) hist[b] = 0;
        __syncthreads();
#pragma unroll 4
        for (int i = tid; i < hwa; i += kRpnSelThreads) {
            const float v = L[i];
            if (pass == 0) bad |= !det_finite(v);
            const unsigned long long key = rpn_key(v, i);
            if ((key >> (shift + kRpnDigit)) == pre) atomicAdd(&hist[(int)(key >> shift) & (kRpnBins - 1)], 1);
        }
        __syncthreads();
        // (The scan, the pick and the gather's append below are this kernel's own text, not select_common.h's radix_pick and
        //  wave_append: with the helpers the compiler ordered the same instructions differently and the kernel measured 1 % slower
        //  at 4 x 63 000 anchors -- docs/experiments.md.  With this text its machine code is what it was before the header existed.)
        const int v0 = hist[2 * tid], v1 = hist[2 * tid + 1], sum = v0 + v1;
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int cum = incl - sum;
        for (int q = 0; q < wave; q++) cum += wave_sum[q];
        const int need = P - below;                             // >= 1: the need-th key under the prefix is the P-th of all
        if (cum < need && need <= cum + v0) {
            ctl[0] = 2 * tid;
            ctl[1] = cum;
            ctl[2] = v0;
        }
        cum += v0;
        if (cum < need && need <= cum + v1) {
            ctl[0] = 2 * tid + 1;
            ctl[1] = cum;
            ctl[2] = v1;
        }
        __syncthreads();
        const int before = below + ctl[1], in_bin = ctl[2];
        const unsigned long long np = (pre << kRpnDigit) | (unsigned long long)ctl[0];
        if (before + in_bin <= cap) {                            // (the last pass always ends here: its bins hold one key each)
            thresh = (np + 1ull) << shift;
            break;
        }
        pre = np;
        below = before;
        __syncthreads();
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(w.flags, LOCOV_RPN_FLAG_NONFINITE);        // (conservative: any logit of the image)

    // ---- gather the keys below the threshold, sort them: positions 0 .. P - 1 are the selection in order
    if (tid == 0) ctl[3] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < hwa; i0 += kRpnSelThreads) {
        const int i = i0 + tid;
        const unsigned long long key = i < hwa ? rpn_key(L[i], i) : ~0ull;
        const bool take = i < hwa && key < thresh;
        const unsigned long long b = __ballot(take);
        if (!b) continue;
        int at = 0;
        if (lane == 0) at = atomicAdd(&ctl[3], __popcll(b));
        at = __shfl(at, 0);
        if (take) skey[at + __popcll(b & ((1ull << lane) - 1ull))] = key;
    }
    __syncthreads();
    const int n = ctl[3];                                        // P <= n <= cap
    const int P2 = next_pow2(n, 2);
    for (int i = n + tid; i < P2; i += kRpnSelThreads) skey[i] = ~0ull;
    __syncthreads();
    det_bitonic_sort<kRpnSelThreads>(skey, P2, tid);

    // ---- decode, finite test (before the clip), clip, size filter
    const int W = (P + 63) >> 6, Pa = W << 6;
    const int64_t base = (int64_t)img * Pa;
    const float4 *D = deltas + (int64_t)img * hwa;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    bool nonfinite = false;
    for (int p0 = 0; p0 < Pa; p0 += kRpnSelThreads) {
        const int p = p0 + tid;                                  // (whole waves: Pa and the stride are multiples of 64)
        if (p >= Pa) break;
        bool ok = false;
        float4 box = zero;
        float v = 0.f;
        int i = -1;
        if (p < P) {
            i = (int)(skey[p] & ((1ull << kRpnIdxBits) - 1ull));
            v = L[i];
            const float4 o = det_apply_deltas(D[i], anchors[i], inv_wx, inv_wy, inv_ww, inv_wh, scale_clamp);
            nonfinite |= !(det_finite(v) && det_finite(o.x) && det_finite(o.y) && det_finite(o.z) && det_finite(o.w));
            box = det_clip(o, g.w[img], g.h[img]);
            ok = (box.z - box.x) > min_size && (box.w - box.y) > min_size;          // Boxes.nonempty(threshold)
        }
        w.boxes[base + p] = box;
        w.slog[base + p] = v;
        w.sidx[base + p] = i;
        const unsigned long long okw = __ballot(ok);
        if (lane == 0) w.valid[(int64_t)img * W + (p >> 6)] = okw;
    }
    if (__ballot(nonfinite) != 0ull && lane == 0) atomicOr(w.flags, LOCOV_RPN_FLAG_NONFINITE);
}

// grid (row chunks, ceil(W / 4), images): wave `wave` of a workgroup has word column 4 blockIdx.y + wave of the 64 rows
__global__ __launch_bounds__(256) void rpn_overlap_kernel(int P, float nms_thr, RpnWork w)
{
    const int W = (P + 63) >> 6, Pa = W << 6;
    const int lane = threadIdx.x & 63, rc = blockIdx.x, wd = blockIdx.y * 4 + (threadIdx.x >> 6), img = blockIdx.z;
    if (wd < rc || wd >= W) return;                              // (the lower triangle is never read)
    const float4 *gb = w.boxes + (int64_t)img * Pa;
    const int row = 64 * rc + lane;
    const float4 a = gb[row], col = gb[64 * wd + lane];          // (rows P .. Pa - 1 hold zero boxes)
    const int lim = min(64, P - 64 * wd);
    unsigned long long bits = 0;
    for (int k = 0; k < lim; k++) bits |= (unsigned long long)box_iou_gt(a, lane_box(col, k), nms_thr) << k;
    w.M[((int64_t)img * Pa + row) * W + wd] = bits;
}

__global__ __launch_bounds__(256) void rpn_sweep_kernel(int P, int post, RpnWork w, float4 *__restrict__ out_boxes,
                                                        float *__restrict__ out_logits, int64_t *__restrict__ out_index,
                                                        int *__restrict__ counts)
{
    __shared__ unsigned long long cur[2];                        // the removed word of the chunk being resolved (two slots: one barrier)
    const int W = (P + 63) >> 6, Pa = W << 6;
    const int img = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const int64_t base = (int64_t)img * Pa;
    const unsigned long long *Mi = w.M + base * W;
    unsigned long long removed = t < W ? ~w.valid[(int64_t)img * W + t] : ~0ull;
    int nk = 0;
    for (int c = 0; c < W && nk < post; c++) {
        if (t == c) cur[c & 1] = removed;
        __syncthreads();
        const unsigned long long rem = cur[c & 1];
        const unsigned long long diag = Mi[(int64_t)(64 * c + lane) * W + c];
        const int dlo = (int)(unsigned)diag, dhi = (int)(unsigned)(diag >> 32);
        unsigned long long alive = ~(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rem >> 32)) << 32) |
                                     (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)rem));
        unsigned long long keep = 0;
        while (alive) {                                          // greedy, in position order: the first alive box is kept
            const int j = __ffsll((long long)alive) - 1;
            keep |= 1ull << j;
            const unsigned long long dj = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, j) << 32) |
                                          (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, j);
            alive &= ~(dj | (1ull << j));
        }
        if (t > c && t < W) {                                    // the kept rows' overlaps into this thread's word, four loads in flight
            const unsigned long long *col = Mi + (int64_t)(64 * c) * W + t;
            unsigned long long m = keep;
            while (m) {
                const int j0 = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                const int j1 = m ? __ffsll((long long)m) - 1 : j0;
                m &= m - 1ull;
                const int j2 = m ? __ffsll((long long)m) - 1 : j0;
                m &= m - 1ull;
                const int j3 = m ? __ffsll((long long)m) - 1 : j0;
                m &= m - 1ull;
                const unsigned long long a0 = col[(int64_t)j0 * W], a1 = col[(int64_t)j1 * W], a2 = col[(int64_t)j2 * W],
                                         a3 = col[(int64_t)j3 * W];
                removed |= a0 | a1 | a2 | a3;
            }
        }
        if (t < 64 && ((keep >> lane) & 1ull)) {
            const int slot = nk + lanes_below(keep);
            if (slot < post) {
                const int64_t src = base + 64 * c + lane, dst = (int64_t)img * post + slot;
                out_boxes[dst] = w.boxes[src];
                out_logits[dst] = w.slog[src];
                out_index[dst] = w.sidx[src];
            }
        }
        nk += __popcll(keep);
    }
    const int cnt = min(nk, post);
    for (int j = cnt + t; j < post; j += 256) {
        const int64_t dst = (int64_t)img * post + j;
        out_boxes[dst] = make_float4(0.f, 0.f, 0.f, 0.f);
        out_logits[dst] = 0.f;
        out_index[dst] = -1;
    }
    if (t == 0) counts[img] = cnt;
}

// the limits of a call and its workspace size, from host data only; < 0 on an argument error (set_error has run)
static int64_t rpn_plan(int n_images, int64_t hwa, int pre_nms_topk, const char *who)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= kRpnMaxImages, "%s: too many images (0..%d per call)", who, kRpnMaxImages);
    LOCOV_REQUIRE(hwa >= 0 && hwa < (1 << kRpnIdxBits), "%s: too many anchors (fewer than %d per image)", who, 1 << kRpnIdxBits);
    LOCOV_REQUIRE(pre_nms_topk >= 1 && pre_nms_topk <= kRpnMaxPre, "%s: pre_nms_topk out of range (1..%d)", who, kRpnMaxPre);
    if (n_images == 0 || hwa == 0) return 0;
    const int64_t P = hwa < pre_nms_topk ? hwa : pre_nms_topk, W = (P + 63) / 64;
    return (int64_t)n_images * (512 * W * W + 1544 * W);
}

}  // namespace locov

using namespace locov;

extern "C" {

int64_t locov_rpn_proposals_workspace_bytes(int n_images, int64_t hwa, int pre_nms_topk)
{
    return rpn_plan(n_images, hwa, pre_nms_topk, "locov_rpn_proposals_workspace_bytes");
}

int locov_rpn_proposals(const float *logits, const float *deltas, const float *anchors, int64_t hwa, const float *image_hw, int n_images,
                        float wx, float wy, float ww, float wh, float scale_clamp, int pre_nms_topk, int post_nms_topk, float min_box_size,
                        float nms_thresh, void *workspace, int64_t workspace_bytes, float *out_boxes, float *out_logits, int64_t *out_index,
                        int *counts_and_flags, locov_stream_t stream)
{
    const char *who = "locov_rpn_proposals";
    const int64_t need = rpn_plan(n_images, hwa, pre_nms_topk, who);
    if (need < 0) return (int)need;
    LOCOV_REQUIRE(post_nms_topk >= 1 && post_nms_topk <= pre_nms_topk, "%s: post_nms_topk out of range (1..pre_nms_topk = %d)", who,
                  pre_nms_topk);
    LOCOV_REQUIRE(wx != 0.f && wy != 0.f && ww != 0.f && wh != 0.f, "%s: zero box weight", who);
    if (n_images == 0 || hwa == 0) return LOCOV_OK;
    LOCOV_REQUIRE(logits && deltas && anchors && image_hw && workspace && out_boxes && out_logits && out_index && counts_and_flags,
                  "%s: null pointer", who);
    LOCOV_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld bytes, need %lld)", who, (long long)workspace_bytes, (long long)need);
    LOCOV_REQUIRE(((uintptr_t)deltas | (uintptr_t)anchors | (uintptr_t)workspace | (uintptr_t)out_boxes) % 16 == 0,
                  "%s: deltas / anchors / workspace / out_boxes must be 16-byte aligned", who);
    const int P = (int)(hwa < pre_nms_topk ? hwa : pre_nms_topk), W = (P + 63) / 64, Pa = 64 * W;
    const int cap = next_pow2(P, 64);                            // the sort buffer: the next power of two at or above P
    RpnGeom g{};
    for (int i = 0; i < n_images; i++) {
        g.h[i] = image_hw[2 * i];
        g.w[i] = image_hw[2 * i + 1];
    }
    const int64_t n = n_images;
    char *ws = static_cast<char *>(workspace);
    RpnWork w;
    w.boxes = reinterpret_cast<float4 *>(ws);
    ws += 16 * n * Pa;
    w.M = reinterpret_cast<unsigned long long *>(ws);
    ws += 8 * n * Pa * W;
    w.valid = reinterpret_cast<unsigned long long *>(ws);
    ws += 8 * n * W;
    w.slog = reinterpret_cast<float *>(ws);
    ws += 4 * n * Pa;
    w.sidx = reinterpret_cast<int *>(ws);
    w.flags = counts_and_flags + n_images;

    static std::atomic<int> select_lds[kMaxDevices];
    if (int rc = raise_dynamic_lds(select_lds, reinterpret_cast<const void *>(rpn_select_kernel), kRpnMaxPre * 8 + kRpnBins * 4 + 128, who))
        return rc;
    hipStream_t s = as_stream(stream);
    hipError_t e = hipMemsetAsync(counts_and_flags, 0, sizeof(int) * (size_t)(n_images + 1), s);
    if (e != hipSuccess) return set_error(LOCOV_ERR_LAUNCH, "%s: memset: %s", who, hipGetErrorString(e));

    hipLaunchKernelGGL(rpn_select_kernel, dim3((unsigned)n_images), dim3(kRpnSelThreads), (size_t)cap * 8 + kRpnBins * 4 + 128, s, logits,
                       reinterpret_cast<const float4 *>(deltas), reinterpret_cast<const float4 *>(anchors), (int)hwa, P, cap, g, 1.0f / wx,
                       1.0f / wy, 1.0f / ww, 1.0f / wh, scale_clamp, min_box_size, w);
    hipLaunchKernelGGL(rpn_overlap_kernel, dim3((unsigned)W, (unsigned)ceil_div(W, 4), (unsigned)n_images), dim3(256), 0, s, P, nms_thresh, w);
    hipLaunchKernelGGL(rpn_sweep_kernel, dim3((unsigned)n_images), dim3(256), 0, s, P, post_nms_topk, w, reinterpret_cast<float4 *>(out_boxes),
                       out_logits, out_index, counts_and_flags);
    return check_launch(who);
}

}  // extern "C"
