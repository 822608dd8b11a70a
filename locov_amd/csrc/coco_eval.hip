// COCO-protocol bounding-box evaluation (the public COCOeval with iouType = "bbox", useCats = 1, which the reference's
// CustomCOCOEvaluator sits on: ovr/evaluation/custom_coco_eval.py).  Everything is fp64 and integer, each step rounded on its
// own (this file is compiled with -ffp-contract=off), so the result equals the numpy definition in locov_amd/evaluation.py
// bit for bit.
//
// locov_coco_match: one wave per (image, category) cell, one lane per (area range, IoU threshold).
//   The cell's dets arrive in descending-score order (ties in input order); only the first max_det take part.
//   IoU of det (x, y, w, h) and gt (x, y, w, h), in double:  w = min(dx + dw, gx + gw) - max(dx, gx), h likewise; 0 if w <= 0 or
//   h <= 0; else i = w * h, u = crowd ? dw * dh : dw * dh + gw * gh - i, IoU = i / u.  The det's w / h are x2 - x1 / y2 - y1
//   formed in fp32 and then widened.  The D x G matrix is formed once per cell by all 64 lanes -- in the wave's LDS slice where
//   D * G * 8 + G * 64 <= kCellLds, else in the caller's workspace at a slot that depends only on the cell's gt offset.
//   Per (range, threshold) lane the dets are taken in order: best = min(t, 1 - 1e-10), m = none; first over the gts that are NOT
//   ignored in this range (ignored = crowd or area outside [lo, hi]), skipping one already matched at this threshold, a gt with
//   iou >= best becomes m and raises best (equal IoU moves to the later gt); only if that found nothing, the same over the IGNORED
//   gts, where a matched crowd gt may be taken again.  This is COCOeval's single loop over the gts sorted non-ignored first.  A
//   matched det takes its gt's ignore flag; an unmatched det whose own area (dw * dh) is outside the range is ignored.
//
// locov_lvis_match: the same kernel under the LVIS protocol (the public LVISEval, which Detectron2's LVISEvaluator sits on).
//   The gt's own `ignore` flag stands where crowd stood in the ignore test and nowhere else: the IoU is always the non-crowd one
//   and a matched gt is never taken again.  A byte per cell carries the image's federated lists: an unmatched det of a cell
//   marked NOT_EXHAUSTIVE is ignored whatever its area, and a cell with no gt and no NEG mark is UNLISTED -- its dets are neither
//   true nor false positives, and are written as unmatched and ignored (2), which the accumulation passes over.
//
// locov_coco_accumulate: one workgroup per (category, range, cap, threshold), walking the category's dets (descending score, ties
//   in image then in-cell order) in chunks of kAccChunk, in ascending order, with integer carries -- no atomics, no float carry
//   but a running maximum, so two runs give equal bits.  Over the dets whose in-cell rank is below the cap:  tp / fp are the
//   cumulative counts of the non-ignored matched / unmatched dets, rc = tp / npig, pr = tp / (fp + tp + 2^-52), pr is made
//   non-increasing from the right, and for every recall threshold the first det with rc >= it gives precision and score (0 once
//   no det reaches it).  recall is the last rc (0 with no det).  npig == 0: precision, recall and scores are WRITTEN as -1.
#include "common.h"

namespace locov {

namespace {

constexpr int kThreads = 256;
constexpr int kCellsPerBlock = kThreads / kWave;
constexpr int kCellLds = 8192;                      // bytes of LDS per cell (wave)
constexpr int kGtmStride = kWave;                   // matched flags: one byte per (gt, lane)
constexpr int kAccChunk = 1024;
constexpr int kPerThread = kAccChunk / kThreads;

struct MatchArgs {
    double lo[LOCOV_COCO_MAX_AREAS], hi[LOCOV_COCO_MAX_AREAS], thr[LOCOV_COCO_MAX_THRESHOLDS];
    int A, T;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bytes of workspace one gt owns: its column of the largest IoU matrix and its matched flags
__host__ __device__ inline int64_t gt_slot_bytes(int max_det) { return (int64_t)max_det * 8 + kGtmStride; }

// kLvis false: gt_flag is iscrowd and cell_flags is not read.  kLvis true: gt_flag is the gt's own ignore field.
template <bool kLvis>
__global__ __launch_bounds__(kThreads) void match_kernel(const int *__restrict__ det_off, const int *__restrict__ gt_off,
                                                         const uint8_t *__restrict__ cell_flags, int64_t n_cells, int n_det, int n_gt,
                                                         int max_det, const float *__restrict__ det_box,
                                                         const double *__restrict__ gt_box, const double *__restrict__ gt_area,
                                                         const uint8_t *__restrict__ gt_flag, MatchArgs args,
                                                         uint8_t *__restrict__ det_bits, uint8_t *__restrict__ gt_ignore,
                                                         char *__restrict__ ws)
{
    __shared__ double lds[kCellsPerBlock][kCellLds / 8];
    __shared__ double s_lo[LOCOV_COCO_MAX_AREAS], s_hi[LOCOV_COCO_MAX_AREAS], s_thr[LOCOV_COCO_MAX_THRESHOLDS];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int A = args.A, T = args.T, AT = A * T;
    if (threadIdx.x < LOCOV_COCO_MAX_AREAS) {
        s_lo[threadIdx.x] = args.lo[threadIdx.x];
        s_hi[threadIdx.x] = args.hi[threadIdx.x];
    }
    if (threadIdx.x < LOCOV_COCO_MAX_THRESHOLDS) s_thr[threadIdx.x] = args.thr[threadIdx.x];
    __syncthreads();

    const int64_t cell = (int64_t)blockIdx.x * kCellsPerBlock + wave;
    int d0 = 0, D = 0, g0 = 0, G = 0, flags = 0;
    double *iou = nullptr;
    uint8_t *gtm = nullptr;
    if (cell < n_cells) {
        // the offsets are device data the entry point cannot check: clamped, a descending pair is an empty cell
        d0 = clampi(det_off[cell], 0, n_det);
        const int d1 = clampi(det_off[cell + 1], d0, n_det);
        g0 = clampi(gt_off[cell], 0, n_gt);
        G = clampi(gt_off[cell + 1], g0, n_gt) - g0;
        D = d1 - d0 < max_det ? d1 - d0 : max_det;
        if constexpr (kLvis) flags = cell_flags[cell];
        // the dets past the cap take no part: their bits are written as zero
        const int64_t extra = (int64_t)(d1 - d0 - D) * AT;
        uint8_t *tail = det_bits + (int64_t)(d0 + D) * AT;
        for (int64_t i = lane; i < extra; i += kWave) tail[i] = 0;
        for (int64_t i = lane; i < (int64_t)A * G; i += kWave) {
            const int a = (int)(i / G), g = g0 + (int)(i % G);
            const double ar = gt_area[g];
            gt_ignore[(int64_t)a * n_gt + g] = (gt_flag[g] != 0 || ar < s_lo[a] || ar > s_hi[a]) ? 1 : 0;
        }
        if (D > 0 && G > 0) {
            if ((int64_t)D * G * 8 + (int64_t)G * kGtmStride <= kCellLds) {
                iou = lds[wave];
                gtm = reinterpret_cast<uint8_t *>(lds[wave] + D * G);                           // (D * G <= 1024 here)
            } else {
                char *slot = ws + (int64_t)g0 * gt_slot_bytes(max_det);
                iou = reinterpret_cast<double *>(slot);
                gtm = reinterpret_cast<uint8_t *>(slot + (int64_t)G * max_det * 8);
            }
            for (int64_t p = lane; p < (int64_t)D * G; p += kWave) {
                const int d = (int)(p / G), g = (int)(p % G);
                const float *b = det_box + (int64_t)(d0 + d) * 4;
                const double dx = (double)b[0], dy = (double)b[1];
                const double dw = (double)(b[2] - b[0]), dh = (double)(b[3] - b[1]);          // XYXY -> XYWH in fp32, then widened
                const double *q = gt_box + (int64_t)(g0 + g) * 4;
                const double gx = q[0], gy = q[1], gw = q[2], gh = q[3];
                double v = 0.0;
                const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
                if (w > 0.0) {
                    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
                    if (h > 0.0) {
                        const double i = w * h;
                        const double da = dw * dh;
                        const double u = (!kLvis && gt_flag[g0 + g]) ? da : da + gw * gh - i;
                        v = i / u;
                    }
                }
                iou[p] = v;
            }
            for (int g = 0; g < G; g++) gtm[(int64_t)g * kGtmStride + lane] = 0;                         // (this lane's own column)
        }
    }
    __syncthreads();                                                                           // the matrix is complete
    if (lane >= AT || D == 0) return;
    if constexpr (kLvis) {
        if (G == 0 && !(flags & LOCOV_LVIS_CELL_NEG)) {                                        // an unlisted cell: no part
            for (int d = 0; d < D; d++) det_bits[(int64_t)(d0 + d) * AT + lane] = 2;
            return;
        }
    }

    const int a = lane / T;
    const double lo = s_lo[a], hi = s_hi[a];
    const double t = s_thr[lane % T];
    const double start = t < 1.0 - 1e-10 ? t : 1.0 - 1e-10;
    for (int d = 0; d < D; d++) {
        double best = start;
        int m = -1, m_ignored = 0;
        for (int g = 0; g < G; g++) {                                                          // the gts not ignored in this range
            const double ar = gt_area[g0 + g];
            if (gt_flag[g0 + g] || ar < lo || ar > hi) continue;
            if (gtm[(int64_t)g * kGtmStride + lane]) continue;
            const double v = iou[(int64_t)d * G + g];
            if (v < best) continue;
            best = v;
            m = g;
        }
        if (m < 0) {
            for (int g = 0; g < G; g++) {                                                      // nothing there: the ignored ones
                const double ar = gt_area[g0 + g];
                const bool flag = gt_flag[g0 + g] != 0;
                if (!(flag || ar < lo || ar > hi)) continue;
                if (gtm[(int64_t)g * kGtmStride + lane] && (kLvis || !flag)) continue;              // (only a crowd gt is taken again)
                const double v = iou[(int64_t)d * G + g];
                if (v < best) continue;
                best = v;
                m = g;
            }
            m_ignored = 1;
        }
        int bits;
        if (m >= 0) {
            gtm[(int64_t)m * kGtmStride + lane] = 1;
            bits = 1 | (m_ignored << 1);
        } else {
            const float *b = det_box + (int64_t)(d0 + d) * 4;
            const double da = (double)(b[2] - b[0]) * (double)(b[3] - b[1]);
            bits = (da < lo || da > hi || (kLvis && (flags & LOCOV_LVIS_CELL_NOT_EXHAUSTIVE))) ? 2 : 0;
        }
        det_bits[(int64_t)(d0 + d) * AT + lane] = (uint8_t)bits;
    }
}

struct AccArgs {
    double rec[LOCOV_COCO_MAX_RECALL_THRESHOLDS];
    int cap[LOCOV_COCO_MAX_CAPS];
    int K, A, M, T, R;
};

typedef unsigned long long u64;

// counts of (dets under the cap, true positives, false positives) travel as three 20-bit fields of one word
__device__ __forceinline__ u64 pack3(int q, int tp, int fp) { return (u64)q | ((u64)tp << 20) | ((u64)fp << 40); }
__device__ __forceinline__ int field(u64 v, int i) { return (int)((v >> (20 * i)) & 0xfffff); }

__global__ __launch_bounds__(kThreads) void coco_accumulate_kernel(const int *__restrict__ cat_off, const int *__restrict__ acc_idx,
                                                                   const int *__restrict__ acc_rank, const double *__restrict__ acc_score,
                                                                   int n_det, const uint8_t *__restrict__ det_bits,
                                                                   const int *__restrict__ npig, AccArgs args,
                                                                   double *__restrict__ precision, double *__restrict__ recall,
                                                                   double *__restrict__ scores)
{
    __shared__ int s_tp[kAccChunk];
    __shared__ double s_pr[kAccChunk];
    __shared__ double s_sc[kAccChunk];
    __shared__ u64 s_wsum[kThreads / kWave];
    __shared__ double s_wmax[kThreads / kWave];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int K = args.K, A = args.A, M = args.M, T = args.T, R = args.R;
    int b = blockIdx.x;
    const int t = b % T;
    b /= T;
    const int m = b % M;
    b /= M;
    const int a = b % A;
    const int k = b / A;
    const int cap = args.cap[m];
    const int AT = A * T, col = a * T + t;
    const int64_t rec_idx = (((int64_t)t * K + k) * A + a) * M + m;                            // recall [T,K,A,M]
    auto prec_idx = [&](int r) { return ((((int64_t)t * R + r) * K + k) * A + a) * M + m; };   // precision [T,R,K,A,M]

    const int np = npig[k * A + a];
    if (np <= 0) {
        if (tid < R) {
            precision[prec_idx(tid)] = -1.0;
            if (scores) scores[prec_idx(tid)] = -1.0;
        }
        if (tid == 0) recall[rec_idx] = -1.0;
        return;
    }
    const double npd = (double)np;
    const double thr = tid < R ? args.rec[tid] : 0.0;
    const int n0 = clampi(cat_off[k], 0, n_det), n1 = clampi(cat_off[k + 1], n0, n_det);
    const double kNegInf = -__builtin_inf();

    int q_before = 0, tp_before = 0, fp_before = 0;        // the carries: integers, every thread keeps the same copy
    double q = 0.0, ss = 0.0;                              // thread r's precision and score
    bool active = false;                                   // recall threshold r has been reached

    for (int base = n0; base < n1; base += kAccChunk) {
        int inc[kPerThread];                               // 0: over the cap; else 1 | tp << 1 | fp << 2
        double sc[kPerThread];
        int cq = 0, ctp = 0, cfp = 0;
#pragma unroll
        for (int e = 0; e < kPerThread; e++) {
            const int j = base + tid * kPerThread + e;
            inc[e] = 0;
            sc[e] = 0.0;
            if (j < n1 && acc_rank[j] < cap) {
                const int i = clampi(acc_idx[j], 0, n_det - 1);
                const int bits = det_bits[(int64_t)i * AT + col];
                const int tp = bits == 1, fp = bits == 0;  // matched and not ignored / unmatched and not ignored
                inc[e] = 1 | (tp << 1) | (fp << 2);
                sc[e] = acc_score[j];
                cq++;
                ctp += tp;
                cfp += fp;
            }
        }
        // the workgroup's exclusive scan of the three counts
        const u64 own = pack3(cq, ctp, cfp);
        u64 incl = own;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const u64 o = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += o;
        }
        if (lane == kWave - 1) s_wsum[wave] = incl;
        __syncthreads();
        u64 before = 0, total = 0;
        for (int w = 0; w < kThreads / kWave; w++) {
            if (w < wave) before += s_wsum[w];
            total += s_wsum[w];
        }
        const u64 excl = before + incl - own;
        int pq = field(excl, 0), ptp = tp_before + field(excl, 1), pfp = fp_before + field(excl, 2);
        const int L = field(total, 0);
#pragma unroll
        for (int e = 0; e < kPerThread; e++) {
            if (!inc[e]) continue;
            ptp += (inc[e] >> 1) & 1;
            pfp += (inc[e] >> 2) & 1;
            const double tp = (double)ptp, fp = (double)pfp;
            s_tp[pq] = ptp;
            s_pr[pq] = tp / (fp + tp + 2.220446049250313e-16);
            s_sc[pq] = sc[e];
            pq++;
        }
        __syncthreads();
        // pr non-increasing from the right: a suffix maximum over the chunk's L packed entries (a later chunk's entries come later
        // in the walk; the thresholds reached earlier take this chunk's maximum below)
        double v = kNegInf;
#pragma unroll
        for (int e = 0; e < kPerThread; e++) {
            const int s = tid * kPerThread + e;
            if (s < L) v = fmax(v, s_pr[s]);
        }
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const double o = __shfl_down(v, off, kWave);
            if (lane + off < kWave) v = fmax(v, o);
        }
        if (lane == 0) s_wmax[wave] = v;
        double right = __shfl_down(v, 1, kWave);
        if (lane == kWave - 1) right = kNegInf;
        __syncthreads();
        for (int w = wave + 1; w < kThreads / kWave; w++) right = fmax(right, s_wmax[w]);
#pragma unroll
        for (int e = kPerThread - 1; e >= 0; e--) {
            const int s = tid * kPerThread + e;
            if (s < L) {
                right = fmax(right, s_pr[s]);
                s_pr[s] = right;
            }
        }
        __syncthreads();
        if (tid < R && L > 0) {
            if (active) {
                q = fmax(q, s_pr[0]);
            } else if ((double)s_tp[L - 1] / npd >= thr) {
                int lo = 0, hi = L - 1;                    // the first entry with rc >= thr
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((double)s_tp[mid] / npd >= thr) hi = mid;
                    else lo = mid + 1;
                }
                q = s_pr[lo];
                ss = s_sc[lo];
                active = true;
            }
        }
        q_before += L;
        tp_before += field(total, 1);
        fp_before += field(total, 2);
        __syncthreads();                                   // the next chunk overwrites s_*
    }
    if (tid < R) {
        precision[prec_idx(tid)] = q;
        if (scores) scores[prec_idx(tid)] = ss;
    }
    if (tid == 0) recall[rec_idx] = q_before > 0 ? (double)tp_before / npd : 0.0;
}

}  // namespace

}  // namespace locov

using namespace locov;

extern "C" int64_t locov_coco_match_workspace_bytes(int n_gt, int max_det)
{
    if (n_gt <= 0 || max_det <= 0) return 0;
    return (int64_t)n_gt * gt_slot_bytes(max_det);
}

namespace {

// The one body of locov_coco_match (cell_flags unused, gt_flag = iscrowd) and locov_lvis_match (gt_flag = the gt's ignore field).
template <bool kLvis>
int match_entry(const char *who, const int *det_offsets, const int *gt_offsets, const uint8_t *cell_flags, int64_t n_cells, int n_det,
                int n_gt, int max_det, const float *det_boxes, const double *gt_boxes, const double *gt_area, const uint8_t *gt_flag,
                const double *area_ranges_host, int n_areas, const double *iou_thresholds_host, int n_thresholds, uint8_t *det_bits,
                uint8_t *gt_ignore, void *workspace, int64_t workspace_bytes, locov_stream_t stream)
{
    LOCOV_REQUIRE(n_cells >= 0 && n_det >= 0 && n_gt >= 0 && workspace_bytes >= 0, "%s: negative count or size", who);
    LOCOV_REQUIRE(max_det >= 1, "%s: max_det must be at least 1", who);
    LOCOV_REQUIRE(n_areas >= 1 && n_areas <= LOCOV_COCO_MAX_AREAS, "%s: 1..%d area ranges", who, LOCOV_COCO_MAX_AREAS);
    LOCOV_REQUIRE(n_thresholds >= 1 && n_thresholds <= LOCOV_COCO_MAX_THRESHOLDS, "%s: 1..%d IoU thresholds", who,
                  LOCOV_COCO_MAX_THRESHOLDS);
    LOCOV_REQUIRE(area_ranges_host && iou_thresholds_host, "%s: null area range or threshold list", who);
    for (int a = 0; a < n_areas; a++)
        LOCOV_REQUIRE(area_ranges_host[2 * a] <= area_ranges_host[2 * a + 1], "%s: area range %d is not ascending", who, a);
    if (n_cells == 0 || (n_det == 0 && n_gt == 0)) return LOCOV_OK;
    if (max_det > LOCOV_COCO_MAX_DET || n_cells > (int64_t)LOCOV_COCO_MAX_BLOCKS * kCellsPerBlock)
        return set_error(LOCOV_ERR_UNSUPPORTED, "%s: at most %d dets per cell and %lld cells", who, LOCOV_COCO_MAX_DET,
                         (long long)LOCOV_COCO_MAX_BLOCKS * kCellsPerBlock);
    LOCOV_REQUIRE(det_offsets && gt_offsets, "%s: null offsets", who);
    if (kLvis) LOCOV_REQUIRE(cell_flags, "%s: null cell flags", who);
    LOCOV_REQUIRE(n_det == 0 || (det_boxes && det_bits), "%s: null det pointer", who);
    LOCOV_REQUIRE(n_gt == 0 || (gt_boxes && gt_area && gt_flag && gt_ignore), "%s: null gt pointer", who);
    LOCOV_REQUIRE((uintptr_t)gt_boxes % 8 == 0 && (uintptr_t)gt_area % 8 == 0 && (uintptr_t)det_boxes % 4 == 0 &&
                      (uintptr_t)det_offsets % 4 == 0 && (uintptr_t)gt_offsets % 4 == 0,
                  "%s: misaligned pointer", who);
    if (n_det > 0 && n_gt > 0) {
        LOCOV_REQUIRE(workspace && (uintptr_t)workspace % 8 == 0, "%s: null or misaligned workspace", who);
        LOCOV_REQUIRE(workspace_bytes >= locov_coco_match_workspace_bytes(n_gt, max_det), "%s: workspace too small", who);
    }
    MatchArgs args{};
    for (int a = 0; a < n_areas; a++) {
        args.lo[a] = area_ranges_host[2 * a];
        args.hi[a] = area_ranges_host[2 * a + 1];
    }
    for (int t = 0; t < n_thresholds; t++) args.thr[t] = iou_thresholds_host[t];
    args.A = n_areas;
    args.T = n_thresholds;
    const int64_t grid = ceil_div(n_cells, kCellsPerBlock);
    hipLaunchKernelGGL(match_kernel<kLvis>, dim3((unsigned)grid), dim3(kThreads), 0, as_stream(stream), det_offsets, gt_offsets,
                       cell_flags, n_cells, n_det, n_gt, max_det, det_boxes, gt_boxes, gt_area, gt_flag, args, det_bits, gt_ignore,
                       static_cast<char *>(workspace));
    return check_launch(who);
}

}  // namespace

extern "C" int locov_coco_match(const int *det_offsets, const int *gt_offsets, int64_t n_cells, int n_det, int n_gt, int max_det,
                                const float *det_boxes, const double *gt_boxes, const double *gt_area, const uint8_t *gt_crowd,
                                const double *area_ranges_host, int n_areas, const double *iou_thresholds_host, int n_thresholds,
                                uint8_t *det_bits, uint8_t *gt_ignore, void *workspace, int64_t workspace_bytes,
                                locov_stream_t stream)
{
    return match_entry<false>("locov_coco_match", det_offsets, gt_offsets, nullptr, n_cells, n_det, n_gt, max_det, det_boxes, gt_boxes,
                              gt_area, gt_crowd, area_ranges_host, n_areas, iou_thresholds_host, n_thresholds, det_bits, gt_ignore,
                              workspace, workspace_bytes, stream);
}

extern "C" int locov_lvis_match(const int *det_offsets, const int *gt_offsets, const uint8_t *cell_flags, int64_t n_cells, int n_det,
                                int n_gt, int max_det, const float *det_boxes, const double *gt_boxes, const double *gt_area,
                                const uint8_t *gt_ignore_in, const double *area_ranges_host, int n_areas,
                                const double *iou_thresholds_host, int n_thresholds, uint8_t *det_bits, uint8_t *gt_ignore,
                                void *workspace, int64_t workspace_bytes, locov_stream_t stream)
{
    return match_entry<true>("locov_lvis_match", det_offsets, gt_offsets, cell_flags, n_cells, n_det, n_gt, max_det, det_boxes, gt_boxes,
                             gt_area, gt_ignore_in, area_ranges_host, n_areas, iou_thresholds_host, n_thresholds, det_bits, gt_ignore,
                             workspace, workspace_bytes, stream);
}

extern "C" int locov_coco_accumulate(const int *cat_offsets, int n_categories, const int *acc_index, const int *acc_rank,
                                     const double *acc_score, int n_det, const uint8_t *det_bits, const int *npig, int n_areas,
                                     int n_thresholds, const int *max_dets_host, int n_max_dets, const double *recall_thresholds_host,
                                     int n_recall_thresholds, double *precision, double *recall, double *scores, locov_stream_t stream)
{
    LOCOV_REQUIRE(n_categories >= 0 && n_det >= 0, "locov_coco_accumulate: negative count");
    LOCOV_REQUIRE(n_areas >= 1 && n_areas <= LOCOV_COCO_MAX_AREAS, "locov_coco_accumulate: 1..%d area ranges", LOCOV_COCO_MAX_AREAS);
    LOCOV_REQUIRE(n_thresholds >= 1 && n_thresholds <= LOCOV_COCO_MAX_THRESHOLDS, "locov_coco_accumulate: 1..%d IoU thresholds",
                  LOCOV_COCO_MAX_THRESHOLDS);
    LOCOV_REQUIRE(n_max_dets >= 1 && n_max_dets <= LOCOV_COCO_MAX_CAPS, "locov_coco_accumulate: 1..%d detection caps",
                  LOCOV_COCO_MAX_CAPS);
    LOCOV_REQUIRE(n_recall_thresholds >= 1 && n_recall_thresholds <= LOCOV_COCO_MAX_RECALL_THRESHOLDS,
                  "locov_coco_accumulate: 1..%d recall thresholds", LOCOV_COCO_MAX_RECALL_THRESHOLDS);
    LOCOV_REQUIRE(max_dets_host && recall_thresholds_host, "locov_coco_accumulate: null cap or recall threshold list");
    for (int m = 0; m < n_max_dets; m++)
        LOCOV_REQUIRE(max_dets_host[m] >= 1 && (m == 0 || max_dets_host[m] > max_dets_host[m - 1]),
                      "locov_coco_accumulate: the detection caps must be positive and ascending");
    for (int r = 1; r < n_recall_thresholds; r++)
        LOCOV_REQUIRE(recall_thresholds_host[r] >= recall_thresholds_host[r - 1],
                      "locov_coco_accumulate: the recall thresholds must be ascending");
    if (n_categories == 0) return LOCOV_OK;
    const int64_t blocks = (int64_t)n_categories * n_areas * n_max_dets * n_thresholds;
    if (blocks > LOCOV_COCO_MAX_BLOCKS)
        return set_error(LOCOV_ERR_UNSUPPORTED, "locov_coco_accumulate: categories x ranges x caps x thresholds above %d",
                         LOCOV_COCO_MAX_BLOCKS);
    LOCOV_REQUIRE(cat_offsets && npig && precision && recall, "locov_coco_accumulate: null pointer");
    LOCOV_REQUIRE(n_det == 0 || (acc_index && acc_rank && acc_score && det_bits), "locov_coco_accumulate: null det pointer");
    LOCOV_REQUIRE((uintptr_t)precision % 8 == 0 && (uintptr_t)recall % 8 == 0 && (uintptr_t)scores % 8 == 0 &&
                      (uintptr_t)acc_score % 8 == 0 && (uintptr_t)cat_offsets % 4 == 0 && (uintptr_t)acc_index % 4 == 0 &&
                      (uintptr_t)acc_rank % 4 == 0 && (uintptr_t)npig % 4 == 0,
                  "locov_coco_accumulate: misaligned pointer");
    AccArgs args{};
    for (int r = 0; r < n_recall_thresholds; r++) args.rec[r] = recall_thresholds_host[r];
    for (int m = 0; m < n_max_dets; m++) args.cap[m] = max_dets_host[m];
    args.K = n_categories;
    args.A = n_areas;
    args.M = n_max_dets;
    args.T = n_thresholds;
    args.R = n_recall_thresholds;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, as_stream(stream), cat_offsets, acc_index,
                       acc_rank, acc_score, n_det, det_bits, npig, args, precision, recall, scores);
    return check_launch("locov_coco_accumulate");
}
