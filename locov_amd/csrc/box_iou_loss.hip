// The IoU forms of the box-regression loss of a training step -- BBOX_REG_LOSS_TYPE "giou", "diou", "ciou" -- as ONE launch instead of
// Box2BoxTransform.apply_deltas + ~40 element-wise torch launches (and as many again in autograd's backward).
//
//   * locov_box_iou_loss -- [D2-upstream] FastRCNNOutputLayers.box_reg_loss for a loss type other than "smooth_l1" (the reference
//     imports giou_loss and documents the key: ovr/modeling/roi_heads/box_emb_head.py:5,102,165, box_emb_grounding_head.py:5,305,374;
//     [D2-upstream] _dense_box_regression_loss also takes "diou" and "ciou"): apply_deltas of the foreground rows' predictions onto
//     their proposals, [fvcore, unverified] giou_loss / diou_loss / ciou_loss against the matched ground truth, summed and divided by
//     the number of ALL rows; the gradient with respect to the predictions comes out of the same launch.
//
// A row is a hundred operations on twelve fp32 inputs, so the row's mathematics runs in fp64 and the loss and each gradient entry are
// rounded to fp32 once: the result sits within rounding of the float64 evaluation instead of at an fp32 chain's distance from it.
// One workgroup, a fixed tree for the sum, no atomics: the same inputs give the same bits.  Built with -ffp-contract=off.
#include "reduce_common.h"

namespace locov {

namespace {

constexpr int kIouThreads = 256;
constexpr double kIouEps = 1e-7;                                     // fvcore's eps, all three losses

// fixed-order sum over the workgroup (reduce_common.h: every thread returns the total)
__device__ __forceinline__ double block_sum(double v, double *red) { return block_tree_reduce<kIouThreads>(v, red, SumOp()); }

// d max(a, b) / d a and d min(a, b) / d a as torch.max / torch.min of two tensors define them: equal arguments share the gradient
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ __forceinline__ double dmin(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }

}  // namespace

// KIND: LOCOV_BOX_IOU_GIOU / _DIOU / _CIOU
template <int KIND>
__global__ __launch_bounds__(kIouThreads) void box_iou_loss_kernel(const float4 *__restrict__ src, const float4 *__restrict__ tgt,
                                                                   const float *__restrict__ pred, int64_t ld,
                                                                   const int64_t *__restrict__ cls, int64_t R, int64_t num_classes,
                                                                   double wx, double wy, double ww, double wh, double scale_clamp,
                                                                   float *__restrict__ loss, float *__restrict__ dpred)
{
    __shared__ double red[kIouThreads];
    const bool agnostic = ld == 4;
    const double n = (double)(R > 1 ? R : 1);
    double part = 0.0;
    for (int64_t r = threadIdx.x; r < R; r += kIouThreads) {
        const int64_t c = cls[r];
        const bool fg = c >= 0 && c < num_classes;
        const int64_t col = agnostic ? 0 : (fg ? c : 0) * 4;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (fg) {                                                     // (background / ignored rows: their predictions are never read)
            const float4 s = src[r], t = tgt[r];
            const float *p = pred + r * ld + col;
            // Box2BoxTransform.apply_deltas
            const double W = (double)s.z - (double)s.x, H = (double)s.w - (double)s.y;
            const double cx = (double)s.x + 0.5 * W, cy = (double)s.y + 0.5 * H;
            const double dx = (double)p[0] / wx, dy = (double)p[1] / wy;
            const double dw0 = (double)p[2] / ww, dh0 = (double)p[3] / wh;
            const bool cw = dw0 > scale_clamp, ch = dh0 > scale_clamp;   // torch.clamp(max=): equality passes the gradient
            const double dw = cw ? scale_clamp : dw0, dh = ch ? scale_clamp : dh0;
            const double pcx = dx * W + cx, pcy = dy * H + cy;
            const double pw = exp(dw) * W, ph = exp(dh) * H;
            const double x1 = pcx - 0.5 * pw, y1 = pcy - 0.5 * ph, x2 = pcx + 0.5 * pw, y2 = pcy + 0.5 * ph;
            const double gx1 = t.x, gy1 = t.y, gx2 = t.z, gy2 = t.w;

            // intersection, union, IoU
            const double xk1 = fmax(x1, gx1), yk1 = fmax(y1, gy1), xk2 = fmin(x2, gx2), yk2 = fmin(y2, gy2);
            const bool hit = yk2 > yk1 && xk2 > xk1;                  // (strict: boxes that only touch do not intersect)
            const double iw = xk2 - xk1, ih = yk2 - yk1;
            const double inter = hit ? iw * ih : 0.0;
            const double bw = x2 - x1, bh = y2 - y1, gw = gx2 - gx1, gh = gy2 - gy1;
            const double un = (bw * bh + gw * gh) - inter, ue = un + kIouEps;
            const double iou = inter / ue;
            // the smallest enclosing box
            const double xc1 = fmin(x1, gx1), yc1 = fmin(y1, gy1), xc2 = fmax(x2, gx2), yc2 = fmax(y2, gy2);
            const double ew = xc2 - xc1, eh = yc2 - yc1;

            // the row's loss and its derivatives in: the predicted box's area (through the union), the intersection (directly and
            // through the union), the enclosing box's corners, and directly in the predicted corners (gd: x1, y1, x2, y2)
            double l, d_area, d_inter, d_xc1, d_yc1, d_xc2, d_yc2;
            double gd[4] = {0.0, 0.0, 0.0, 0.0};
            if (KIND == LOCOV_BOX_IOU_GIOU) {
                const double area_c = ew * eh, ce = area_c + kIouEps;
                l = 1.0 - (iou - (area_c - un) / ce);
                const double d_un = inter / (ue * ue) - 1.0 / ce;     // d l / d union
                const double d_c = (ce - (area_c - un)) / (ce * ce);  // d l / d area_c
                d_area = d_un;
                d_inter = -1.0 / ue - d_un;
                d_xc1 = -d_c * eh;
                d_xc2 = d_c * eh;
                d_yc1 = -d_c * ew;
                d_yc2 = d_c * ew;
            } else {
                const double diag = (ew * ew + eh * eh) + kIouEps;
                const double ex = (x2 + x1) / 2.0 - (gx1 + gx2) / 2.0, ey = (y2 + y1) / 2.0 - (gy1 + gy2) / 2.0;
                const double dist = ex * ex + ey * ey;
                l = (1.0 - iou) + dist / diag;
                const double d_un = inter / (ue * ue);
                d_area = d_un;
                d_inter = -1.0 / ue - d_un;
                const double d_diag = -dist / (diag * diag);
                d_xc1 = -2.0 * ew * d_diag;
                d_xc2 = 2.0 * ew * d_diag;
                d_yc1 = -2.0 * eh * d_diag;
                d_yc2 = 2.0 * eh * d_diag;
                gd[0] = gd[2] = ex / diag;                            // d dist / d x1 = 2 ex / 2
                gd[1] = gd[3] = ey / diag;
                if (KIND == LOCOV_BOX_IOU_CIOU) {
                    const double q = bw / bh;
                    const double da = atan(gw / gh) - atan(q);
                    const double k = 4.0 / (M_PI * M_PI);
                    const double v = k * (da * da);
                    const double alpha = v / (((1.0 - iou) + v) + kIouEps);   // a constant of the gradient (fvcore: under no_grad)
                    l = l + alpha * v;
                    const double d_q = alpha * (2.0 * k * da) * (-1.0 / (1.0 + q * q));   // d (alpha v) / d (w / h)
                    const double d_bw = d_q / bh, d_bh = -d_q * q / bh;
                    gd[0] -= d_bw;
                    gd[2] += d_bw;
                    gd[1] -= d_bh;
                    gd[3] += d_bh;
                }
            }
            part = part + l;

            // back to the predicted corners: area = bw * bh, inter = iw * ih where the boxes intersect, max / min of the corners
            gd[0] += -d_area * bh + d_xc1 * dmin(x1, gx1);
            gd[1] += -d_area * bw + d_yc1 * dmin(y1, gy1);
            gd[2] += d_area * bh + d_xc2 * dmax(x2, gx2);
            gd[3] += d_area * bw + d_yc2 * dmax(y2, gy2);
            if (hit) {
                gd[0] += -d_inter * ih * dmax(x1, gx1);
                gd[1] += -d_inter * iw * dmax(y1, gy1);
                gd[2] += d_inter * ih * dmin(x2, gx2);
                gd[3] += d_inter * iw * dmin(y2, gy2);
            }
            // and through apply_deltas: centre = d * size + centre, size = exp(clamp(d)) * size (a clamped delta gets exactly zero)
            const double g_dx = (gd[0] + gd[2]) * W / wx, g_dy = (gd[1] + gd[3]) * H / wy;
            const double g_dw = 0.5 * (gd[2] - gd[0]) * pw / ww, g_dh = 0.5 * (gd[3] - gd[1]) * ph / wh;
            g[0] = (float)(g_dx / n);
            g[1] = (float)(g_dy / n);
            g[2] = cw ? 0.f : (float)(g_dw / n);
            g[3] = ch ? 0.f : (float)(g_dh / n);
        }
        if (dpred) {
            // class-agnostic: the whole [R, 4] gradient is written here; per-class predictions: the caller zeroed [R, 4 K] and the
            // four columns of the row's class are filled in (background / ignored rows: nothing, as the indexed upstream form)
            if (agnostic || fg) {
                float *q = dpred + r * ld + col;
#pragma unroll
                for (int j = 0; j < 4; j++) q[j] = g[j];
            }
        }
    }
    const double total = block_sum(part, red);
    if (threadIdx.x == 0) loss[0] = (float)(total / n);
}

}  // namespace locov

extern "C" int locov_box_iou_loss(const float *proposal_boxes, const float *gt_boxes, const float *pred_deltas, int64_t ld,
                                  const int64_t *gt_classes, int64_t R, int64_t num_classes, float wx, float wy, float ww, float wh,
                                  double scale_clamp, int kind, float *loss, float *dpred, locov_stream_t stream)
{
    using namespace locov;
    LOCOV_REQUIRE(R >= 0 && num_classes >= 1 && (ld == 4 || ld == 4 * num_classes),
                  "locov_box_iou_loss: pred_deltas must be [R, 4] or [R, 4 * num_classes] (R %lld, ld %lld, num_classes %lld)", (long long)R,
                  (long long)ld, (long long)num_classes);
    LOCOV_REQUIRE(kind == LOCOV_BOX_IOU_GIOU || kind == LOCOV_BOX_IOU_DIOU || kind == LOCOV_BOX_IOU_CIOU,
                  "locov_box_iou_loss: unknown kind %d", kind);
    LOCOV_REQUIRE(loss && (R == 0 || (proposal_boxes && gt_boxes && pred_deltas && gt_classes)), "locov_box_iou_loss: null pointer");
    LOCOV_REQUIRE(((uintptr_t)proposal_boxes | (uintptr_t)gt_boxes) % 16 == 0, "locov_box_iou_loss: boxes must be 16-byte aligned");
    auto kernel = kind == LOCOV_BOX_IOU_GIOU ? box_iou_loss_kernel<LOCOV_BOX_IOU_GIOU>
                  : kind == LOCOV_BOX_IOU_DIOU ? box_iou_loss_kernel<LOCOV_BOX_IOU_DIOU>
                                               : box_iou_loss_kernel<LOCOV_BOX_IOU_CIOU>;
    // (R == 0: the launch runs no row and writes loss = 0, as locov_box_reg_loss)
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kIouThreads), 0, as_stream(stream), reinterpret_cast<const float4 *>(proposal_boxes),
                       reinterpret_cast<const float4 *>(gt_boxes), pred_deltas, ld, gt_classes, R, num_classes, (double)wx, (double)wy,
                       (double)ww, (double)wh, scale_clamp, loss, dpred);
    return check_launch("locov_box_iou_loss");
}
