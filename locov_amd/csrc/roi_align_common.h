// Sampling arithmetic shared by every ROIAlign kernel (roi_align.hip, roi_align_nhwc.hip, roi_align_nhwc_bwd.hip,
// roi_align_contract.hip, roi_align_tiles.hip): torchvision's roi_align as reached from
// ovr/modeling/roi_heads/roi_emb_heads.py:243-245, every step an explicitly rounded fp32 operation -- the coordinates must be the
// CPU oracle's (oracle/roi_ops_ref.c), bit for bit, whatever the including file's contraction flags are.
#pragma once
#include "common.h"

namespace locov {

// A proposal's geometry as torchvision computes it.  The grids are RAW: under `aligned` with sampling_ratio 0 a bin size <= -1
// makes them negative, and the callers differ in what they do then (clamp to 0, also zero them for an invalid batch index, refuse
// the proposal) -- every caller applies its own rule to the result.  count = max(grid_h * grid_w, 1) of the RAW product, kept a
// float because some callers divide by it (the bit-exact contract kernels) and others multiply by its reciprocal.
struct RoiGeom {
    float start_h, start_w, bin_h, bin_w, count;
    int grid_h, grid_w;
};

__device__ __forceinline__ RoiGeom roi_geom(const float *roi, float scale, int ph, int pw, int sampling_ratio, int aligned)
{
    RoiGeom g;
    const float off = aligned ? 0.5f : 0.0f;
    g.start_w = __fsub_rn(__fmul_rn(roi[1], scale), off);
    g.start_h = __fsub_rn(__fmul_rn(roi[2], scale), off);
    const float end_w = __fsub_rn(__fmul_rn(roi[3], scale), off);
    const float end_h = __fsub_rn(__fmul_rn(roi[4], scale), off);
    float rw = __fsub_rn(end_w, g.start_w), rh = __fsub_rn(end_h, g.start_h);
    if (!aligned) {
        rw = fmaxf(rw, 1.f);
        rh = fmaxf(rh, 1.f);
    }
    g.bin_h = __fdiv_rn(rh, (float)ph);
    g.bin_w = __fdiv_rn(rw, (float)pw);
    g.grid_h = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(g.bin_h);
    g.grid_w = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(g.bin_w);
    const int prod = g.grid_h * g.grid_w;
    g.count = (float)(prod > 1 ? prod : 1);
    return g;
}

struct AxisSampleN {
    int lo, hi;   // pixel index along the axis
    float wl, wh;
};

// sample i of bin p on one axis: coordinate, the [-1, size] rule (weights 0), the clamp at 0 and at the last pixel
__device__ __forceinline__ AxisSampleN axis_sample_n(float start, float bin, int p, int i, int grid, int size)
{
    float v = __fadd_rn(__fadd_rn(start, __fmul_rn((float)p, bin)),
                        __fdiv_rn(__fmul_rn(__fadd_rn((float)i, .5f), bin), (float)grid));
    AxisSampleN s;
    if (v < -1.0f || v > (float)size) {
        s.lo = 0; s.hi = 0; s.wl = 0.f; s.wh = 0.f;
        return s;
    }
    if (v <= 0.f) v = 0.f;
    int lo = (int)v, hi;
    if (lo >= size - 1) {
        hi = lo = size - 1;
        v = (float)lo;
    } else {
        hi = lo + 1;
    }
    const float l = __fsub_rn(v, (float)lo);
    s.lo = lo; s.hi = hi; s.wl = l; s.wh = __fsub_rn(1.f, l);
    return s;
}

}  // namespace locov
