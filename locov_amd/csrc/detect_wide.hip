// Detection post-processing of the evaluation call for any candidate count (LVIS-style thresholds), on the device, ONE host read.
//
// detect.hip sorts an image's candidates in LDS and so takes at most LOCOV_DETECT_MAX_CANDIDATES of them: enough at COCO's
// SCORE_THRESH_TEST 0.05, far too few at Detectron2's LVIS setting (SCORE_THRESH_TEST 1e-4, DETECTIONS_PER_IMAGE 300), where one
// image of 1 000 proposals x 1 203 classes has 2e5..1.2e6 candidates.  The torch chain then takes batched_nms's per-class Python loop
// (thousands of launches, host waits per class).  This file computes the same detections, bit for bit, with the structure that
// class-agnostic box regression gives: every class's candidate of proposal j has the SAME box, proposal j's.
//
// What the chain does per image (roi_heads/box_emb_head.py: fast_rcnn_inference -> batched_nms), which is what this file reproduces:
//   n < per_class_above candidates: ONE NMS over boxes shifted by class * (max coordinate over the image's candidates + 1); the IoU
//       is taken on the shifted fp32 coordinates (classes never suppress each other, so the greedy sweep runs per class segment);
//   n >= per_class_above: a separate NMS per class on the unshifted boxes -- the IoU of two candidates is then the IoU of their two
//       proposals, one R x R bit matrix per image serves every class;
//   inside a class: descending score, ties by row; survivors merged by (descending score, row, class), the first `topk` kept.
//
// Class-specific regression (locov_detect_postprocess_wide_cs with box_classes = K: deltas [R, 4K], boxes [R, K]) keeps the segments,
// the orders and the top-k and changes which box a candidate has -- its OWN: the shift unit is the maximum over the candidates' own
// boxes; the shifted branch reads each candidate's own box; the per-class branch has no matrix to share and tests its pairs inside the
// sweep (dw_sweep_cs_kernel).  The class-agnostic kernels are template instances of their own and run as before.
//
//   det_decode_clip_kernel   (detect_common.h) apply_deltas + clip, one thread per proposal (_cs: per (proposal, class))
//   dw_count_kernel          a workgroup per (64 rows of an image, 256 columns): candidates per (image, class); non-finite
//                            probabilities; the max coordinate over the image's candidate boxes (batched_nms's shift unit)
//   dw_scan_kernel           one workgroup: segment offsets per (image, class), candidates per image, the branch of each image
//   dw_emit_kernel           same tiling as the count: keys  ~score << 14 | row  into the (image, class) segments
//   dw_segsort_kernel        a workgroup per segment: bitonic sort in LDS (descending score, ties by row)
//   dw_overlap_kernel        per-class images: the row x row IoU bit matrix; shifted images: per candidate, which earlier candidates
//                            of its class overlap it (IoU on the SHIFTED boxes)
//   dw_sweep_kernel          a wave per segment: the greedy sweep over the segment with the kept set in registers; survivors are
//                            compacted to the segment's front as  ~score << 29 | row << 15 | class  (the merge order)
//   dw_sweep_cs_kernel       class-specific boxes, per-class images: a wave per segment, 64 candidates a step -- IoU against the
//                            survivors so far, then among themselves, resolved in candidate order; same survivor layout
//   dw_select_kernel x 6     radix select, 11 bits a pass, chip-wide histograms; the last workgroup of an image picks the digit:
//                            ends as soon as the keys below a threshold number at least top-k and at most kDwCap
//   dw_gather_kernel         those keys into one buffer per image
//   dw_topk_kernel           a workgroup per image: bitonic sort of the <= kDwCap winners in LDS, the first top-k out.
// The IoU test, the block scan, the radix digit pick, the compacting append and the key layout are select_common.h's.
#include "detect_common.h"
#include "reduce_common.h"

namespace locov {

constexpr int kDwChunkRows = 64;                // rows per count / emit workgroup
constexpr int kDwCap = 16384;                   // winners the last launch sorts in LDS (128 KB)
constexpr int kDwDigit = 11, kDwBins = 1 << kDwDigit, kDwPasses = 6;     // 61-bit merge keys: 5 x 11 + 6 bits
constexpr int kDwClassChunk = 32;               // classes per select / gather workgroup
constexpr int kDwMaxImages = LOCOV_LABEL_MAX_IMAGES;

struct DwPlan {
    int n_img, K, pca;
    int bk, cs;                                 // boxes per proposal (1 or K) and 0 / 1: candidate (row, class) has box row * bk + class * cs
    int cbase[kDwMaxImages + 1];                // row chunks of image i: [cbase[i], cbase[i + 1])
    int W[kDwMaxImages];                        // 64-bit words of a row / candidate overlap set of image i: ceil(rows / 64)
    int64_t mbase[kDwMaxImages];                // word offset of image i's row x row matrix (rows * W words)
    int64_t ovbase[kDwMaxImages];               // word offset of image i's candidate overlap words (cap * W words)
};

struct DwImage {                                // per image, zeroed at the start of a call
    int n;                                      // candidates
    int base;                                   // first candidate slot of the image
    int per_class;                              // n >= per_class_above
    unsigned umax;                              // bits of the max coordinate over the candidate boxes (+0.0 start)
    int surv;                                   // survivors of the NMS
    int done;                                   // the select has found its threshold
    int below;                                  // keys below the current prefix (all winners)
    int gcount;                                 // keys gathered
    unsigned long long pre, thresh;             // radix prefix; winners are the keys < thresh
    int arrive[kDwPasses];                      // select workgroups finished, per pass
    int pad[14];
};
static_assert(sizeof(DwImage) == 128, "DwImage: 128 bytes per image (the documented workspace formula)");

struct DwWork {
    float4 *boxes;                              // [R, bk] decoded, clipped
    DwImage *info;                              // [n_img]
    int *hist;                                  // [kDwPasses][n_img][kDwBins]
    int *cnt, *kept, *seg_off, *cursor;         // [n_img * K] candidates / survivors / first slot / emit cursor per segment
    unsigned long long *gbuf;                   // [n_img][kDwCap]
    unsigned long long *M, *ov, *keys;
    int *flags;
};

__device__ __forceinline__ int dw_chunk_image(const DwPlan &p, int chunk)
{
    int lo = 0, hi = p.n_img - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.cbase[mid] <= chunk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// a workgroup per (64 rows, 256 columns); every one of the K + 1 columns must be finite.  CS: class-specific boxes (an instance of
// its own, so that the class-agnostic loop stays as it was)
template <bool CS>
__global__ __launch_bounds__(256) void dw_count_kernel(const float *__restrict__ probs, int64_t ld, float thr, DetGeom g, DwPlan p, DwWork w)
{
    __shared__ unsigned long long rows_hit;
    const int tid = threadIdx.x, lane = tid & 63, chunk = blockIdx.x, c = blockIdx.y * 256 + tid, K = p.K;
    const int img = dw_chunk_image(p, chunk);
    const int r0 = g.roff[img] + (chunk - p.cbase[img]) * kDwChunkRows, r1 = min(r0 + kDwChunkRows, g.roff[img + 1]);
    if (tid == 0) rows_hit = 0;
    __syncthreads();
    int n = 0;
    unsigned long long mask = 0;
    bool bad = false;
    float own = -__builtin_inff();              // class-specific boxes: the max coordinate over this thread's candidates' OWN boxes
    if (c <= K)
        for (int r = r0; r < r1; r++) {
            const float v = probs[(int64_t)r * ld + c];
            bad |= !det_finite(v);
            if (c < K && v > thr) {
                n++;
                mask |= 1ull << (r - r0);
                if constexpr (CS) {
                    const float4 b = w.boxes[(int64_t)r * K + c];
                    own = fmaxf(own, fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)) + 0.f);
                }
            }
        }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(w.flags, LOCOV_DETECT_FLAG_NONFINITE);
    if (n) atomicAdd(&w.cnt[img * K + c], n);
    if constexpr (CS) {                         // (a row has K different boxes: the maximum is over candidates, not over rows)
        own = wave_reduce(own, FmaxOp());
        if (lane == 0 && own >= 0.f) atomicMax(&w.info[img].umax, __float_as_uint(own));
        return;
    }
    mask = wave_reduce(mask, OrOp());
    if (lane == 0 && mask) atomicOr(&rows_hit, mask);
    __syncthreads();
    if (tid < 64) {                             // batched_nms's max coordinate: over the boxes of rows with a candidate
        float mx = -__builtin_inff();
        if (tid < r1 - r0 && ((rows_hit >> tid) & 1ull)) {
            const float4 b = w.boxes[r0 + tid];
            mx = fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)) + 0.f;       // (+ 0: a -0 max becomes +0; max + 1 is the same)
        }
        mx = wave_reduce(mx, FmaxOp());
        if (tid == 0 && mx >= 0.f) atomicMax(&w.info[img].umax, __float_as_uint(mx));
    }
}

// one workgroup: per image, the exclusive scan of its class counts (segments in (image, class) order), its candidates and branch
__global__ __launch_bounds__(1024) void dw_scan_kernel(DwPlan p, DwWork w)
{
    __shared__ int wave_sum[16];
    __shared__ int carry;
    const int tid = threadIdx.x, K = p.K;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int img = 0; img < p.n_img; img++) {
        const int base = carry;
        for (int c0 = 0; c0 < K; c0 += 1024) {
            const int c = c0 + tid;
            const int v = c < K ? w.cnt[img * K + c] : 0;
            // (carry is read in front of the scan's barrier and written behind it: the barrier that used to separate the two is gone)
            const int before = carry;
            const int at = before + block_exclusive_scan<1024>(v, wave_sum);
            if (c < K) w.seg_off[img * K + c] = w.cursor[img * K + c] = at;
            if (tid == 1023) carry = at + v;
            __syncthreads();
        }
        if (tid == 0) {
            const int n = carry - base;
            w.info[img].n = n;
            w.info[img].base = base;
            w.info[img].per_class = n >= p.pca ? 1 : 0;
        }
    }
}

// same tiling as dw_count_kernel: a thread's candidates of its column (class) in the 64 rows, behind a per-class cursor
__global__ __launch_bounds__(256) void dw_emit_kernel(const float *__restrict__ probs, int64_t ld, float thr, DetGeom g, DwPlan p, DwWork w)
{
    const int tid = threadIdx.x, chunk = blockIdx.x, c = blockIdx.y * 256 + tid, K = p.K;
    if (c >= K) return;
    const int img = dw_chunk_image(p, chunk);
    const int r0 = g.roff[img] + (chunk - p.cbase[img]) * kDwChunkRows, r1 = min(r0 + kDwChunkRows, g.roff[img + 1]);
    unsigned long long mask = 0;
    for (int r = r0; r < r1; r++)
        if (probs[(int64_t)r * ld + c] > thr) mask |= 1ull << (r - r0);
    if (!mask) return;
    int at = atomicAdd(&w.cursor[img * K + c], __popcll(mask));
    while (mask) {
        const int j = __ffsll((long long)mask) - 1;
        mask &= mask - 1ull;
        const float v = probs[(int64_t)(r0 + j) * ld + c];
        w.keys[at++] = ((unsigned long long)(~__float_as_uint(v)) << kKeyRowBits) | (unsigned long long)(r0 + j - g.roff[img]);
    }
}

// a workgroup per (image, class) segment; the LDS holds the next power of two above the largest image's rows
__global__ __launch_bounds__(256) void dw_segsort_kernel(DwWork w)
{
    extern __shared__ unsigned long long skey[];
    const int seg = blockIdx.x, tid = threadIdx.x;
    const int m = w.cnt[seg];
    if (m <= 1) return;
    const int P = next_pow2(m, 2);
    unsigned long long *keys = w.keys + w.seg_off[seg];
    for (int i = tid; i < P; i += 256) skey[i] = i < m ? keys[i] : ~0ull;
    __syncthreads();
    det_bitonic_sort<256>(skey, P, tid);
    for (int i = tid; i < m; i += 256) keys[i] = skey[i];
}

// per-class images: bit k of word wd of row j = IoU(box j, box 64 wd + k) > thr (the unshifted boxes; IoU is symmetric bit for bit).
// shifted images: a thread per candidate: bit j of its word wd = its class's candidate 64 wd + j (an earlier one) overlaps it on
// the shifted boxes.
template <bool CS>
__global__ __launch_bounds__(256) void dw_overlap_kernel(DetGeom g, DwPlan p, DwWork w, float nms_thr)
{
    const int bk = CS ? p.K : 1;                // candidate (row, class) has box row * bk + (CS ? class : 0)
    const int img = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x, W = p.W[img], K = p.K;
    const int rows = g.roff[img + 1] - g.roff[img];
    const float4 *gb = w.boxes + (int64_t)g.roff[img] * bk;
    const DwImage &inf = w.info[img];
    if (inf.per_class) {
        if (CS || t >= rows * W) return;      // (class-specific boxes: no row x row matrix, dw_sweep_cs_kernel tests the pairs itself)
        const int j = t / W, wd = t - j * W;
        const float4 a = gb[j];
        const int lim = min(64, rows - 64 * wd);
        unsigned long long bits = 0;
        for (int k = 0; k < lim; k++) bits |= (unsigned long long)box_iou_gt(a, gb[64 * wd + k], nms_thr) << k;
        w.M[p.mbase[img] + (int64_t)j * W + wd] = bits;
        return;
    }
    if (t >= inf.n) return;
    const int idx = inf.base + t;
    const int *so = w.seg_off + img * K;
    int lo = 0, hi = K - 1;                     // the segment of candidate idx: the last class starting at or before it
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (so[mid] <= idx) lo = mid;
        else hi = mid - 1;
    }
    const int s = so[lo], pos = idx - s;
    const float off = (float)lo * (__uint_as_float(inf.umax) + 1.f);
    float4 b = gb[(int)(w.keys[idx] & kKeyRowMask) * bk + (CS ? lo : 0)];
    b.x += off;
    b.y += off;
    b.z += off;
    b.w += off;
    unsigned long long *out = w.ov + p.ovbase[img] + (int64_t)t * W;
    for (int wd = 0; 64 * wd < pos; wd++) {
        const int lim = min(64, pos - 64 * wd);
        unsigned long long bits = 0;
        for (int j = 0; j < lim; j++) {
            float4 e = gb[(int)(w.keys[s + 64 * wd + j] & kKeyRowMask) * bk + (CS ? lo : 0)];
            e.x += off;
            e.y += off;
            e.z += off;
            e.w += off;
            bits |= (unsigned long long)box_iou_gt(e, b, nms_thr) << j;
        }
        out[wd] = bits;
    }
}

// a wave per segment: the greedy sweep in the segment's order.  Candidate a is kept iff none of the KEPT candidates overlaps it:
// the kept set lives in registers (lane l holds words l, l + 64, ...: bits by row for per-class images, by segment position for
// shifted ones), a candidate's overlap words are loaded 8 candidates ahead.  Survivors go to the segment's front in merge-key form.
template <int NQ, bool CS>
__global__ __launch_bounds__(256) void dw_sweep_kernel(DwPlan p, DwWork w)
{
    const int lane = threadIdx.x & 63;
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= p.n_img * p.K) return;
    const int m = w.cnt[seg];
    if (m == 0) return;                         // (kept[] starts at zero)
    const int img = seg / p.K, cls = seg - img * p.K, s = w.seg_off[seg], W = p.W[img];
    const bool per_class = w.info[img].per_class != 0;
    if (CS && per_class) return;                // (dw_sweep_cs_kernel's segment)
    const unsigned long long *Mi = w.M + p.mbase[img];
    const unsigned long long *ovs = w.ov + p.ovbase[img] + (int64_t)(s - w.info[img].base) * W;
    unsigned long long *keys = w.keys + s;
    unsigned long long kept[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) kept[q] = 0;
    int nk = 0;
    for (int a0 = 0; a0 < m; a0 += 64) {
        const int nb = min(64, m - a0);
        const unsigned long long mykey = lane < nb ? keys[a0 + lane] : 0ull;
        for (int b0 = 0; b0 < nb; b0 += 8) {
            unsigned long long v[8][NQ];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int a = a0 + b0 + i;
                const unsigned long long ka = __shfl(mykey, (b0 + i) & 63);
                const int row = (int)(ka & kKeyRowMask);
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const int wd = lane + 64 * q;
                    v[i][q] = 0;
                    if (b0 + i < nb) {
                        if (per_class) {
                            if (wd < W) v[i][q] = Mi[(int64_t)row * W + wd];
                        } else if (64 * wd < a) {
                            v[i][q] = ovs[(int64_t)a * W + wd];
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if (b0 + i >= nb) break;
                bool hit = false;
#pragma unroll
                for (int q = 0; q < NQ; q++) hit |= (v[i][q] & kept[q]) != 0ull;
                if (__ballot(hit) == 0ull) {
                    const unsigned long long ka = __shfl(mykey, b0 + i);
                    const int idx = per_class ? (int)(ka & kKeyRowMask) : a0 + b0 + i;
#pragma unroll
                    for (int q = 0; q < NQ; q++)
                        if ((idx >> 6) == lane + 64 * q) kept[q] |= 1ull << (idx & 63);
                    if (lane == 0) keys[nk] = merge_key(ka, cls);
                    nk++;
                }
            }
        }
    }
    if (lane == 0) {
        w.kept[seg] = nk;
        atomicAdd(&w.info[img].surv, nk);
    }
}

// Class-specific boxes, per-class images: a wave per segment, the greedy sweep with the pair tests inside (every candidate has its own
// box, so no matrix is shared between the classes).  64 candidates a step, one per lane: first against the survivors of the earlier
// steps (64 at a time, a survivor's box handed round from its lane), then among themselves -- lane l's bit set of the step's earlier
// candidates that overlap it, resolved in candidate order with one ballot per survivor.  The IoU is taken on the unshifted boxes.
// Survivors go to the segment's front in merge-key form, as dw_sweep_kernel leaves them; the wave reads them back from there.
__global__ __launch_bounds__(256) void dw_sweep_cs_kernel(DetGeom g, DwPlan p, DwWork w, float nms_thr)
{
    const int lane = threadIdx.x & 63;
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= p.n_img * p.K) return;
    const int m = w.cnt[seg];
    if (m == 0) return;
    const int img = seg / p.K, cls = seg - img * p.K, K = p.K;
    if (!w.info[img].per_class) return;
    const float4 *gb = w.boxes + (int64_t)g.roff[img] * K + cls;          // the class's box of row r: gb[r * K]
    unsigned long long *keys = w.keys + w.seg_off[seg];
    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    int nk = 0;
    for (int a0 = 0; a0 < m; a0 += 64) {
        const int nb = min(64, m - a0);
        const bool have = lane < nb;
        const unsigned long long mykey = have ? keys[a0 + lane] : 0ull;
        const float4 mine = have ? gb[(int64_t)(int)(mykey & kKeyRowMask) * K] : none;
        bool dead = !have;
        for (int k0 = 0; k0 < nk && __ballot(!dead) != 0ull; k0 += 64) {
            const int nkk = min(64, nk - k0);
            float4 kb = none;
            if (lane < nkk) {
                const unsigned long long kk = __hip_atomic_load(&keys[k0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                kb = gb[(int64_t)(int)((kk >> kKeyClsBits) & kKeyRowMask) * K];
            }
            for (int j = 0; j < nkk; j++) dead |= box_iou_gt(lane_box(kb, j), mine, nms_thr);
        }
        unsigned long long earlier = 0;         // bit j: the step's candidate j < lane overlaps mine
        for (int j = 0; j < nb - 1; j++) earlier |= (unsigned long long)(j < lane && box_iou_gt(lane_box(mine, j), mine, nms_thr)) << j;
        unsigned long long alive = __ballot(!dead), keep = 0;
        while (alive) {
            const int j = __ffsll((long long)alive) - 1;
            keep |= 1ull << j;
            alive &= ~(1ull << j) & ~__ballot(((earlier >> j) & 1ull) != 0ull);
        }
        if ((keep >> lane) & 1ull)              // (slot <= a0 + lane: never a candidate that is still to be read)
            __hip_atomic_store(&keys[nk + lanes_below(keep)], merge_key(mykey, cls), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nk += __popcll(keep);
        __threadfence();                        // the next step's lanes read what other lanes wrote here
    }
    if (lane == 0) {
        w.kept[seg] = nk;
        atomicAdd(&w.info[img].surv, nk);
    }
}

__device__ __forceinline__ int dw_lo_bit(int pass) { return pass < kDwPasses - 1 ? 61 - kDwDigit * (pass + 1) : 0; }
__device__ __forceinline__ int dw_digits(int pass) { return pass < kDwPasses - 1 ? kDwDigit : 61 - kDwDigit * (kDwPasses - 1); }

// pass `pass` of the radix select of an image's top-k (only images with more than kDwCap survivors): a histogram of the next digit
// of the keys under the current prefix, chip-wide; the last workgroup of the image to finish reads it and picks the digit
__global__ __launch_bounds__(256) void dw_select_kernel(DwPlan p, DwWork w, int topk, int pass)
{
    __shared__ int h[kDwBins];
    __shared__ int wave_sum[4];
    __shared__ int last, ctl[3];                          // ctl: picked bin, keys before it, keys in it (radix_pick)
    const int img = blockIdx.y, tid = threadIdx.x, K = p.K;
    DwImage &inf = w.info[img];
    if (inf.surv <= kDwCap || inf.done) return;           // (uniform over the image's workgroups)
    const int lo = dw_lo_bit(pass), nd = dw_digits(pass);
    const unsigned long long pre = inf.pre;
    for (int b = tid; b < kDwBins; b += 256) h[b] = 0;
    __syncthreads();
    const int c1 = min(K, (int)(blockIdx.x + 1) * kDwClassChunk);
    for (int c = blockIdx.x * kDwClassChunk; c < c1; c++) {
        const int n = w.kept[img * K + c];
        const unsigned long long *keys = w.keys + w.seg_off[img * K + c];
        for (int j = tid; j < n; j += 256) {
            const unsigned long long k = keys[j];
            if ((k >> (lo + nd)) == pre) atomicAdd(&h[(int)(k >> lo) & ((1 << nd) - 1)], 1);
        }
    }
    __syncthreads();
    int *gh = w.hist + ((int64_t)pass * p.n_img + img) * kDwBins;
    for (int b = tid; b < kDwBins; b += 256)
        if (h[b]) atomicAdd(&gh[b], h[b]);
    __threadfence();
    __syncthreads();
    if (tid == 0) last = atomicAdd(&inf.arrive[pass], 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    // the last workgroup: find the bin of the need-th key under the prefix
    constexpr int kPer = kDwBins / 256;
    int v[kPer];
#pragma unroll
    for (int q = 0; q < kPer; q++) v[q] = __hip_atomic_load(&gh[tid * kPer + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    radix_pick<256>(v, min(topk, inf.surv) - inf.below, wave_sum, ctl);
    if (tid == 0) {
        const int below = inf.below + ctl[1];
        const unsigned long long np = (pre << nd) | (unsigned long long)ctl[0];
        if (below + ctl[2] <= kDwCap) {
            inf.thresh = (np + 1ull) << lo;
            inf.done = 1;
        } else {
            inf.pre = np;
            inf.below = below;
        }
    }
}

// the winners' candidates: every survivor (at most kDwCap of them) or the survivors below the select's threshold
__global__ __launch_bounds__(256) void dw_gather_kernel(DwPlan p, DwWork w)
{
    const int img = blockIdx.y, tid = threadIdx.x, K = p.K;
    DwImage &inf = w.info[img];
    const unsigned long long T = inf.surv <= kDwCap ? ~0ull : inf.thresh;
    unsigned long long *out = w.gbuf + (int64_t)img * kDwCap;
    const int c1 = min(K, (int)(blockIdx.x + 1) * kDwClassChunk);
    for (int c = blockIdx.x * kDwClassChunk; c < c1; c++) {
        const int n = w.kept[img * K + c];
        const unsigned long long *keys = w.keys + w.seg_off[img * K + c];
        for (int j0 = 0; j0 < n; j0 += 256) {
            const int j = j0 + tid;
            const unsigned long long k = j < n ? keys[j] : ~0ull;
            const bool take = j < n && k < T;
            const int at = wave_append(take, &inf.gcount);
            if (take) out[at] = k;
        }
    }
}

__global__ __launch_bounds__(1024) void dw_topk_kernel(DetGeom g, DwWork w, int w_bk, int w_cs, int topk, float4 *__restrict__ out_boxes, float *__restrict__ out_scores,
                                                       int64_t *__restrict__ out_classes, int64_t *__restrict__ out_rows, int *__restrict__ counts)
{
    extern __shared__ unsigned long long tkey[];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int n = w.info[img].gcount, k = min(topk, w.info[img].surv);
    if (n == 0) {
        empty_detections_write_out<1024>(0, img, topk, out_boxes, out_scores, out_classes, out_rows);
        if (tid == 0) counts[img] = 0;
        return;
    }
    const int P = next_pow2(n, 2);
    const unsigned long long *in = w.gbuf + (int64_t)img * kDwCap;
    for (int i = tid; i < P; i += 1024) tkey[i] = i < n ? in[i] : ~0ull;
    __syncthreads();
    det_bitonic_sort<1024>(tkey, P, tid);
    merge_keys_write_out<1024>(tkey, k, w.boxes + (int64_t)g.roff[img] * w_bk, w_bk, w_cs, img, topk, out_boxes, out_scores, out_classes,
                               out_rows);
    if (tid == 0) counts[img] = k;
}

// the plan of a call and its workspace size, from host data only; < 0 on an argument error (set_error has run)
static int64_t dw_plan(const int *row_offsets, int n_images, int K, int per_class_above, int64_t ld_deltas, int box_classes, DwPlan *p,
                       const char *who)
{
    LOCOV_REQUIRE(n_images >= 0 && n_images <= kDwMaxImages, "%s: too many images (0..%d per call)", who, kDwMaxImages);
    if (n_images == 0) return 0;
    LOCOV_REQUIRE(row_offsets, "%s: null row_offsets", who);
    LOCOV_REQUIRE(K >= 1 && K < (1 << kKeyClsBits), "%s: too many classes (1..%d)", who, (1 << kKeyClsBits) - 1);
    LOCOV_REQUIRE(box_classes == 1 || box_classes == K, "%s: box_classes must be 1 or num_classes (%d), got %d", who, K, box_classes);
    LOCOV_REQUIRE(ld_deltas >= 4 * (int64_t)box_classes && ld_deltas % 4 == 0,
                  "%s: ld_deltas must cover the 4 x box_classes columns and be a multiple of 4", who);
    LOCOV_REQUIRE(row_offsets[0] == 0, "%s: offsets start at 0", who);
    p->n_img = n_images;
    p->bk = box_classes;
    p->cs = box_classes > 1 ? 1 : 0;
    p->K = K;
    p->pca = per_class_above;
    p->cbase[0] = 0;
    int64_t R = 0, mw = 0, ow = 0;
    for (int i = 0; i < n_images; i++) {
        const int64_t rows = (int64_t)row_offsets[i + 1] - row_offsets[i];
        LOCOV_REQUIRE(rows >= 0, "%s: offsets must be non-decreasing", who);
        LOCOV_REQUIRE(rows < (1 << kKeyRowBits), "%s: too many rows (at most %d proposals per image)", who, (1 << kKeyRowBits) - 1);
        const int64_t W = (rows + 63) / 64;
        const int64_t cap = per_class_above <= 0 ? 0 : (per_class_above - 1 < rows * K ? per_class_above - 1 : rows * K);
        p->W[i] = (int)W;
        p->mbase[i] = mw;
        p->ovbase[i] = ow;
        mw += p->cs ? 0 : rows * W;             // (class-specific boxes: no row x row matrix)
        ow += cap * W;
        p->cbase[i + 1] = p->cbase[i] + (int)((rows + kDwChunkRows - 1) / kDwChunkRows);
        R += rows;
    }
    LOCOV_REQUIRE(R * K <= 0x7fffffff, "%s: too many candidate slots (rows x classes must stay below 2^31)", who);
    if (R == 0) return 0;
    const int64_t nK = (int64_t)n_images * K;
    return 16 * R * p->bk + 16 * nK + (int64_t)n_images * (128 + 4 * kDwPasses * kDwBins + 8 * kDwCap) + 8 * (mw + ow + R * K);
}

}  // namespace locov

using namespace locov;

static int dw_run(const char *who, const float *probs, int64_t ld_probs, int num_classes, const float *deltas, int64_t ld_deltas,
                  int box_classes, const float *proposal_boxes, const int *row_offsets, const float *image_hw, int n_images, float wx, float wy,
                  float ww, float wh, float scale_clamp, float score_thresh, float nms_thresh, int topk, int per_class_above, void *workspace,
                  int64_t workspace_bytes, float *out_boxes, float *out_scores, int64_t *out_classes, int64_t *out_rows, int *counts_and_flags,
                  locov_stream_t stream)
{
    DwPlan p;
    const int64_t need = dw_plan(row_offsets, n_images, num_classes, per_class_above, ld_deltas, box_classes, &p, who);
    if (need < 0) return (int)need;
    if (n_images == 0) return LOCOV_OK;
    LOCOV_REQUIRE(image_hw, "%s: null image_hw", who);
    LOCOV_REQUIRE(topk >= 1 && topk <= LOCOV_DETECT_MAX_CANDIDATES, "%s: topk out of range (1..%d)", who, LOCOV_DETECT_MAX_CANDIDATES);
    LOCOV_REQUIRE(ld_probs >= (int64_t)num_classes + 1, "%s: ld_probs must cover the K + 1 columns", who);
    LOCOV_REQUIRE(wx != 0.f && wy != 0.f && ww != 0.f && wh != 0.f, "%s: zero box weight", who);
    LOCOV_REQUIRE(counts_and_flags, "%s: null pointer (counts_and_flags)", who);
    const int64_t R = row_offsets[n_images];
    LOCOV_REQUIRE(R == 0 || (probs && deltas && proposal_boxes && workspace && out_boxes && out_scores && out_classes && out_rows),
                  "%s: null pointer", who);
    LOCOV_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld bytes, need %lld)", who, (long long)workspace_bytes, (long long)need);
    LOCOV_REQUIRE(((uintptr_t)deltas | (uintptr_t)proposal_boxes | (uintptr_t)workspace | (uintptr_t)out_boxes) % 16 == 0,
                  "%s: boxes / workspace must be 16-byte aligned", who);
    DetGeom g{};
    g.n_img = n_images;
    for (int i = 0; i <= n_images; i++) g.roff[i] = row_offsets[i];
    for (int i = 0; i < n_images; i++) {
        g.h[i] = image_hw[2 * i];
        g.w[i] = image_hw[2 * i + 1];
    }
    hipStream_t s = as_stream(stream);
    hipError_t e = hipMemsetAsync(counts_and_flags, 0, sizeof(int) * (size_t)(n_images + 1), s);
    if (e != hipSuccess) return set_error(LOCOV_ERR_LAUNCH, "%s: memset: %s", who, hipGetErrorString(e));
    if (R == 0) return det_fill_empty(who, n_images, topk, out_boxes, out_scores, out_classes, out_rows, s);
    const int K = num_classes;
    const int64_t nK = (int64_t)n_images * K;
    char *ws = static_cast<char *>(workspace);
    DwWork w;
    w.boxes = reinterpret_cast<float4 *>(ws);
    ws += 16 * R * p.bk;
    char *zero0 = ws;                                            // info, histograms, class counts, survivors: zeroed per call
    w.info = reinterpret_cast<DwImage *>(ws);
    ws += 128 * (int64_t)n_images;
    w.hist = reinterpret_cast<int *>(ws);
    ws += (int64_t)4 * kDwPasses * kDwBins * n_images;
    w.cnt = reinterpret_cast<int *>(ws);
    w.kept = w.cnt + nK;
    const size_t zero_bytes = (size_t)(reinterpret_cast<char *>(w.kept + nK) - zero0);
    w.seg_off = w.kept + nK;
    w.cursor = w.seg_off + nK;
    ws = reinterpret_cast<char *>(w.cursor + nK);
    w.gbuf = reinterpret_cast<unsigned long long *>(ws);
    ws += (int64_t)8 * kDwCap * n_images;
    w.M = reinterpret_cast<unsigned long long *>(ws);
    int64_t mw = 0, ow = 0;
    for (int i = 0; i < n_images; i++) {
        const int64_t rows = g.roff[i + 1] - g.roff[i];
        mw += p.cs ? 0 : rows * p.W[i];
        const int64_t cap = per_class_above <= 0 ? 0 : (per_class_above - 1 < rows * K ? per_class_above - 1 : rows * K);
        ow += cap * p.W[i];
    }
    w.ov = w.M + mw;
    w.keys = w.ov + ow;
    w.flags = counts_and_flags + n_images;
    e = hipMemsetAsync(zero0, 0, zero_bytes, s);
    if (e != hipSuccess) return set_error(LOCOV_ERR_LAUNCH, "%s: memset: %s", who, hipGetErrorString(e));

    const int lds_max = kDwCap * 8;
    static std::atomic<int> segsort_lds[kMaxDevices], topk_lds[kMaxDevices];
    if (int rc = raise_dynamic_lds(segsort_lds, reinterpret_cast<const void *>(dw_segsort_kernel), lds_max, who)) return rc;
    if (int rc = raise_dynamic_lds(topk_lds, reinterpret_cast<const void *>(dw_topk_kernel), lds_max, who)) return rc;

    const float inv_wx = 1.0f / wx, inv_wy = 1.0f / wy, inv_ww = 1.0f / ww, inv_wh = 1.0f / wh;
    if (p.bk == 1 && ld_deltas == 4)
        hipLaunchKernelGGL(det_decode_clip_kernel, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, s, reinterpret_cast<const float4 *>(deltas),
                           reinterpret_cast<const float4 *>(proposal_boxes), (int)R, g, inv_wx, inv_wy, inv_ww, inv_wh, scale_clamp, w.boxes,
                           w.flags);
    else
        hipLaunchKernelGGL(det_decode_clip_cs_kernel, dim3((unsigned)ceil_div(R * p.bk, 256)), dim3(256), 0, s, deltas, ld_deltas,
                           reinterpret_cast<const float4 *>(proposal_boxes), (int)R, p.bk, g, inv_wx, inv_wy, inv_ww, inv_wh, scale_clamp,
                           w.boxes, w.flags);
    const dim3 tiles((unsigned)p.cbase[n_images], (unsigned)ceil_div(K + 1, 256));
    if (p.cs)
        hipLaunchKernelGGL(dw_count_kernel<true>, tiles, dim3(256), 0, s, probs, ld_probs, score_thresh, g, p, w);
    else
        hipLaunchKernelGGL(dw_count_kernel<false>, tiles, dim3(256), 0, s, probs, ld_probs, score_thresh, g, p, w);
    hipLaunchKernelGGL(dw_scan_kernel, dim3(1), dim3(1024), 0, s, p, w);
    hipLaunchKernelGGL(dw_emit_kernel, tiles, dim3(256), 0, s, probs, ld_probs, score_thresh, g, p, w);
    int max_rows = 0;
    int64_t max_items = 0;
    for (int i = 0; i < n_images; i++) {
        const int rows = g.roff[i + 1] - g.roff[i];
        max_rows = rows > max_rows ? rows : max_rows;
        const int64_t cap = per_class_above <= 0 ? 0 : (per_class_above - 1 < (int64_t)rows * K ? per_class_above - 1 : (int64_t)rows * K);
        const int64_t cells = p.cs ? 0 : (int64_t)rows * p.W[i];
        const int64_t items = cells > cap ? cells : cap;
        max_items = items > max_items ? items : max_items;
    }
    hipLaunchKernelGGL(dw_segsort_kernel, dim3((unsigned)nK), dim3(256), (size_t)next_pow2(max_rows, 2) * 8, s, w);
    const dim3 ov_grid((unsigned)ceil_div(max_items, 256), (unsigned)n_images), sweep_grid((unsigned)ceil_div(nK, 4));
    if (!p.cs) {
        if (max_items > 0) hipLaunchKernelGGL(dw_overlap_kernel<false>, ov_grid, dim3(256), 0, s, g, p, w, nms_thresh);
        if (max_rows <= 64 * 64)
            hipLaunchKernelGGL((dw_sweep_kernel<1, false>), sweep_grid, dim3(256), 0, s, p, w);
        else
            hipLaunchKernelGGL((dw_sweep_kernel<4, false>), sweep_grid, dim3(256), 0, s, p, w);
    } else {                                                     // (shifted images, then the per-class images' segments)
        if (max_items > 0) hipLaunchKernelGGL(dw_overlap_kernel<true>, ov_grid, dim3(256), 0, s, g, p, w, nms_thresh);
        if (max_rows <= 64 * 64)
            hipLaunchKernelGGL((dw_sweep_kernel<1, true>), sweep_grid, dim3(256), 0, s, p, w);
        else
            hipLaunchKernelGGL((dw_sweep_kernel<4, true>), sweep_grid, dim3(256), 0, s, p, w);
        hipLaunchKernelGGL(dw_sweep_cs_kernel, sweep_grid, dim3(256), 0, s, g, p, w, nms_thresh);
    }
    const dim3 class_chunks((unsigned)ceil_div(K, kDwClassChunk), (unsigned)n_images);
    for (int pass = 0; pass < kDwPasses; pass++) hipLaunchKernelGGL(dw_select_kernel, class_chunks, dim3(256), 0, s, p, w, topk, pass);
    hipLaunchKernelGGL(dw_gather_kernel, class_chunks, dim3(256), 0, s, p, w);
    hipLaunchKernelGGL(dw_topk_kernel, dim3((unsigned)n_images), dim3(1024), (size_t)lds_max, s, g, w, p.bk, p.cs, topk,
                       reinterpret_cast<float4 *>(out_boxes), out_scores, out_classes, out_rows, counts_and_flags);
    return check_launch(who);
}

extern "C" {

int64_t locov_detect_postprocess_wide_workspace_bytes(const int *row_offsets, int n_images, int num_classes, int per_class_above)
{
    DwPlan p;
    return dw_plan(row_offsets, n_images, num_classes, per_class_above, 4, 1, &p, "locov_detect_postprocess_wide_workspace_bytes");
}

int64_t locov_detect_postprocess_wide_cs_workspace_bytes(const int *row_offsets, int n_images, int num_classes, int per_class_above,
                                                         int64_t ld_deltas, int box_classes)
{
    DwPlan p;
    return dw_plan(row_offsets, n_images, num_classes, per_class_above, ld_deltas, box_classes, &p,
                   "locov_detect_postprocess_wide_cs_workspace_bytes");
}

int locov_detect_postprocess_wide(const float *probs, int64_t ld_probs, int num_classes, const float *deltas, const float *proposal_boxes,
                                  const int *row_offsets, const float *image_hw, int n_images, float wx, float wy, float ww, float wh,
                                  float scale_clamp, float score_thresh, float nms_thresh, int topk, int per_class_above, void *workspace,
                                  int64_t workspace_bytes, float *out_boxes, float *out_scores, int64_t *out_classes, int64_t *out_rows,
                                  int *counts_and_flags, locov_stream_t stream)
{
    return dw_run("locov_detect_postprocess_wide", probs, ld_probs, num_classes, deltas, 4, 1, proposal_boxes, row_offsets, image_hw, n_images,
                  wx, wy, ww, wh, scale_clamp, score_thresh, nms_thresh, topk, per_class_above, workspace, workspace_bytes, out_boxes,
                  out_scores, out_classes, out_rows, counts_and_flags, stream);
}

int locov_detect_postprocess_wide_cs(const float *probs, int64_t ld_probs, int num_classes, const float *deltas, int64_t ld_deltas,
                                     int box_classes, const float *proposal_boxes, const int *row_offsets, const float *image_hw, int n_images,
                                     float wx, float wy, float ww, float wh, float scale_clamp, float score_thresh, float nms_thresh, int topk,
                                     int per_class_above, void *workspace, int64_t workspace_bytes, float *out_boxes, float *out_scores,
                                     int64_t *out_classes, int64_t *out_rows, int *counts_and_flags, locov_stream_t stream)
{
    return dw_run("locov_detect_postprocess_wide_cs", probs, ld_probs, num_classes, deltas, ld_deltas, box_classes, proposal_boxes,
                  row_offsets, image_hw, n_images, wx, wy, ww, wh, scale_clamp, score_thresh, nms_thresh, topk, per_class_above, workspace,
                  workspace_bytes, out_boxes, out_scores, out_classes, out_rows, counts_and_flags, stream);
}

}  // extern "C"
