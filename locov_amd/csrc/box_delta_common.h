// The box-regression arithmetic shared by locov_box_reg_loss (losses.hip) and locov_rpn_loss (rpn_train.hip): [D2-upstream]
// Box2BoxTransform.get_deltas and fvcore's smooth_l1_loss, every step the torch op it replaces, rounded on its own -- a file that
// includes this header is built with -ffp-contract=off.
#pragma once
#include "common.h"

namespace locov {

// Box2BoxTransform.get_deltas of (source box s, target box t), op by op
__device__ __forceinline__ void box_get_deltas(const float4 s, const float4 t, float wx, float wy, float ww, float wh, float d[4])
{
    const float sw = s.z - s.x, sh = s.w - s.y;
    const float scx = s.x + 0.5f * sw, scy = s.y + 0.5f * sh;
    const float tw = t.z - t.x, th = t.w - t.y;
    const float tcx = t.x + 0.5f * tw, tcy = t.y + 0.5f * th;
    d[0] = wx * (tcx - scx) / sw;
    d[1] = wy * (tcy - scy) / sh;
    d[2] = ww * logf(tw / sw);
    d[3] = wh * logf(th / sh);
}

// fvcore smooth_l1_loss of one element e = input - target (beta < 1e-5: plain L1) and its derivative in e
__device__ __forceinline__ void smooth_l1_term(float e, float beta, float &l, float &de)
{
    const float a = fabsf(e);
    if (beta < 1e-5f) {
        l = a;
        de = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
    } else if (a < beta) {
        l = 0.5f * (a * a) / beta;
        de = e / beta;
    } else {
        l = a - 0.5f * beta;
        de = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
    }
}

}  // namespace locov
