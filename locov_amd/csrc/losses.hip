// The scalar-sized loss tails of a training step, each as ONE launch instead of a chain of ~40 small torch launches (and as many
// again in autograd's backward): what a step of the LSM / STT configurations spends on them is launch gaps, not work.
//
//   * locov_box_reg_loss -- [D2-upstream] FastRCNNOutputLayers.box_reg_loss as the reference's heads call it
//     (ovr/modeling/roi_heads/box_emb_grounding_head.py:278-279,370-374: smooth_l1, beta 0 by default): Box2BoxTransform.get_deltas
//     of (proposal, matched ground truth) for the foreground rows, smooth-L1 against the predicted deltas, summed and divided by the
//     number of ALL rows; the gradient with respect to the predictions comes out of the same launch.
//   * locov_grounding_ce_fwd / _bwd -- the cross-entropy tail of GroundingHead.forward (ovr/modeling/mmss_heads/grounding_head.py:
//     239-251 the "(max + 100)" replacement of pairs with neither words nor regions, :273-290 log_softmax over captions and over
//     images + the diagonal means, :357-377 the batch accuracies) on the [B, B] caption x image cost matrices of locov_grounding_fwd;
//     locov_grounding_ce_dist_fwd / _bwd the same launch when the head also returns the filled costs (DISTILLATION_LOSS).
//   * locov_grounding_triplet_fwd / _bwd -- the triplet tail of the same forward (:279-343: hardest / easiest / given negatives of
//     every caption and image, the hinge means) with the same fill, accuracies and optional distributions, one launch each way.
//   * locov_distill_loss_fwd / _bwd -- MultiDistillLoss / MultiDistillLossJS / MultiDistillLossL2 (ovr/modeling/meta_arch/
//     distill_mmss_gcnn.py:211-433) on the transformer's and the grounding head's [B, B] costs, one workgroup, all three staged in LDS.
//
// Built with -ffp-contract=off: each step is the torch op it replaces, rounded on its own; the sums run in a fixed order (one
// workgroup, a fixed tree), so a step's losses are reproducible run to run.
#include "box_delta_common.h"
#include "reduce_common.h"

namespace locov {

namespace {

constexpr int kLossThreads = 256;

// fixed-order sum / maximum over the workgroup (reduce_common.h: every thread returns it)
__device__ __forceinline__ float block_sum(float v, float *red) { return block_tree_reduce<kLossThreads>(v, red, SumOp()); }
__device__ __forceinline__ float block_max(float v, float *red) { return block_tree_reduce<kLossThreads>(v, red, FmaxOp()); }

}  // namespace

__global__ __launch_bounds__(kLossThreads) void box_reg_loss_kernel(const float4 *__restrict__ src, const float4 *__restrict__ tgt,
                                                                    const float *__restrict__ pred, int64_t ld,
                                                                    const int64_t *__restrict__ cls, int64_t R, int64_t num_classes,
                                                                    float wx, float wy, float ww, float wh, float beta,
                                                                    float *__restrict__ loss, float *__restrict__ dpred)
{
    __shared__ float red[kLossThreads];
    const bool agnostic = ld == 4;
    const float n = (float)(R > 1 ? R : 1);
    float part = 0.f;
    for (int64_t r = threadIdx.x; r < R; r += kLossThreads) {
        const int64_t c = cls[r];
        const bool fg = c >= 0 && c < num_classes;
        const int64_t col = agnostic ? 0 : (c < 0 ? 0 : (c >= num_classes ? num_classes - 1 : c)) * 4;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (fg) {
            // Box2BoxTransform.get_deltas and fvcore's smooth_l1_loss, op by op (box_delta_common.h)
            float d[4];
            box_get_deltas(src[r], tgt[r], wx, wy, ww, wh, d);
            const float *p = pred + r * ld + col;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float l, de;
                smooth_l1_term(p[j] - d[j], beta, l, de);
                part = part + l;
                g[j] = de / n;
            }
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
    const float total = block_sum(part, red);
    if (threadIdx.x == 0) loss[0] = total / n;
}

// ---- the grounding tail (locov_grounding_ce[_dist]_fwd / _bwd, locov_grounding_triplet_fwd / _bwd) ----
// Everything on the two [B, B] cost matrices after the alignment launch, one workgroup.  tag 0 = cost[0] ("Words": w2r), 1 = cost[1]
// ("Regions": r2w); an alignment that is off has a null cost.  Forward: out[tag * 4 + k], k: 0 = the loss choosing the caption (over
// dim 0), 1 = choosing the image (dim 1), 2 / 3 = the batch accuracies of the same two directions; pw[tag], where non-null (the head
// also returns its distributions), receives the filled cost.  Backward: d[tag] = d(sum_k up[tag * 2 + k] * loss_k) / d cost, plus
// gpw[tag] (pw's upstream gradient) where non-null, on the pairs that are not filled; a null up reads as 0.  mining, margin and
// neg_idx belong to the triplet loss alone.
struct TailArgs {
    const float *cost[2], *cmask, *rmask;
    int B, T, NR, mining;
    float margin;
    const int64_t *neg_idx;
    float *out, *pw[2];
    const float *up[4], *gpw[2];
    float *d[2];
};

namespace {

constexpr int kTailMaxB = LOCOV_GROUNDING_CE_MAX_B;

// nw[i] / nr[i]: the words of caption i / the regions of image i
__device__ __forceinline__ void tail_mask_counts(const TailArgs &a, float *nw, float *nr)
{
    for (int i = threadIdx.x; i < a.B; i += kLossThreads) {
        float w = 0.f, r = 0.f;
        for (int k = 0; k < a.T; k++) w = w + a.cmask[i * a.T + k];
        for (int k = 0; k < a.NR; k++) r = r + a.rmask[i * a.NR + k];
        nw[i] = w;
        nr[i] = r;
    }
    __syncthreads();
}

// pair e = (caption i, image j) keeps its cost unless it has neither words nor regions
__device__ __forceinline__ bool tail_ok(const float *nw, const float *nr, int B, int e)
{
    const int i = e / B, j = e - i * B;
    return nw[i] > 0.f || nr[j] > 0.f;
}

// cf = the cost with the pairs that are not ok replaced by max + 100 (:239-251), also written to pw when that is non-null
__device__ __forceinline__ void tail_fill(const float *cost, int B, const float *nw, const float *nr, float *red, float *cf, float *pw)
{
    const int t = threadIdx.x, BB = B * B;
    float m = -INFINITY;
    for (int e = t; e < BB; e += kLossThreads) m = fmaxf(m, cost[e]);
    const float fill = block_max(m, red) + 100.0f;
    for (int e = t; e < BB; e += kLossThreads) {
        const float c = tail_ok(nw, nr, B, e) ? cost[e] : fill;
        cf[e] = c;
        if (pw) pw[e] = c;
    }
    __syncthreads();
}

// an alignment that is off: its four outputs are zeros
__device__ __forceinline__ void tail_absent(float *out, int tag)
{
    if (threadIdx.x < 4) out[tag * 4 + threadIdx.x] = 0.f;
}

// the batch accuracies' terms of column k (choose caption) and row k (choose image): is the argmin, first index on ties, k itself
__device__ __forceinline__ void tail_accuracy(const float *cf, int B, int k, float &ac, float &ai)
{
    int bc = 0, bi = 0;
    for (int v = 1; v < B; v++) {
        if (cf[v * B + k] < cf[bc * B + k]) bc = v;
        if (cf[k * B + v] < cf[k * B + bi]) bi = v;
    }
    ac = bc == k ? 1.f : 0.f;
    ai = bi == k ? 1.f : 0.f;
}

// out[tag * 4 ..] = the four means over k (B <= kLossThreads: thread k holds the terms of k, every other thread zeros)
__device__ __forceinline__ void tail_store_means(float *out, int tag, int B, float lc, float li, float ac, float ai, float *red)
{
    const float slc = block_sum(lc, red), sli = block_sum(li, red), sac = block_sum(ac, red), sai = block_sum(ai, red);
    if (threadIdx.x == 0) {
        out[tag * 4 + 0] = slc / (float)B;
        out[tag * 4 + 1] = sli / (float)B;
        out[tag * 4 + 2] = sac / (float)B;
        out[tag * 4 + 3] = sai / (float)B;
    }
}

// what one loss term's mean passes down to each of its B terms
__device__ __forceinline__ float tail_upstream(const float *up, int B) { return (up ? up[0] : 0.f) / (float)B; }

// d[e] for the loss's own dc: pw's gradient joins it, and the replaced pairs are constants
__device__ __forceinline__ void tail_store_grad(float *d, const float *gp, int e, bool ok, float dc)
{
    if (gp) dc = dc + gp[e];
    d[e] = ok ? dc : 0.f;
}

// The cross-entropy tail (grounding_head.py:273-290): log_softmax of z = -cost' over captions and over images, the diagonal means.
template <bool GRAD>
__device__ __forceinline__ void grounding_ce_body(const TailArgs &a)
{
    __shared__ float red[kLossThreads];
    __shared__ float cf[kTailMaxB * kTailMaxB];               // the filled cost of the current tag
    __shared__ float nw[kTailMaxB], nr[kTailMaxB];
    __shared__ float cmx[kTailMaxB], cls_[kTailMaxB];         // per column: max, log-sum-exp term (softmax over dim 0)
    __shared__ float rmx[kTailMaxB], rls_[kTailMaxB];         // per row (softmax over dim 1)
    const int t = threadIdx.x, B = a.B, BB = B * B;
    tail_mask_counts(a, nw, nr);
    for (int tag = 0; tag < 2; tag++) {
        if (!a.cost[tag]) {                                   // (workgroup-uniform)
            if (!GRAD) tail_absent(a.out, tag);
            continue;
        }
        tail_fill(a.cost[tag], B, nw, nr, red, cf, a.pw[tag]);
        // log_softmax's pieces: x - max - log(sum exp(x - max)), per column (dim 0) and per row (dim 1)
        for (int u = t; u < 2 * B; u += kLossThreads) {
            const bool col = u < B;
            const int k = col ? u : u - B;
            float mx = -INFINITY;
            for (int v = 0; v < B; v++) mx = fmaxf(mx, -(col ? cf[v * B + k] : cf[k * B + v]));
            float s = 0.f;
            for (int v = 0; v < B; v++) s = s + expf(-(col ? cf[v * B + k] : cf[k * B + v]) - mx);
            (col ? cmx : rmx)[k] = mx;
            (col ? cls_ : rls_)[k] = logf(s);
        }
        __syncthreads();
        if (!GRAD) {
            float lc = 0.f, li = 0.f, ac = 0.f, ai = 0.f;
            if (t < B) {
                const float zkk = -cf[t * B + t];
                lc = -((zkk - cmx[t]) - cls_[t]);
                li = -((zkk - rmx[t]) - rls_[t]);
                tail_accuracy(cf, B, t, ac, ai);
            }
            tail_store_means(a.out, tag, B, lc, li, ac, ai, red);
        } else {
            const float gc = tail_upstream(a.up[tag * 2], B), gi = tail_upstream(a.up[tag * 2 + 1], B);
            for (int e = t; e < BB; e += kLossThreads) {
                const int i = e / B, j = e - i * B;
                const float z = -cf[e];
                const float pcol = expf((z - cmx[j]) - cls_[j]), prow = expf((z - rmx[i]) - rls_[i]);
                const float dz = gc * (pcol - (i == j ? 1.f : 0.f)) + gi * (prow - (i == j ? 1.f : 0.f));
                tail_store_grad(a.d[tag], a.gpw[tag], e, tail_ok(nw, nr, B, e), -dz);      // z = -cost'
            }
        }
        __syncthreads();
    }
}

// The triplet tail (grounding_head.py:279-343): positive = the diagonal; the negative of column j ("choose caption") / row i ("choose
// image") is the off-diagonal minimum (hardest), maximum (easiest) or the entry a given index names in the matrix without its
// diagonal (reduced index k -> k below the diagonal position, k + 1 from it on: what gather on remove_diag picks; an index outside
// [0, B - 1) is clamped into it, never followed out of the matrix).  The loss terms are mean(relu(positive - negative + margin)).
// B < 2: negative = positive + margin, no gradient.  GRAD: the hinge's gradient on the diagonal entry and on the selected negative.
template <bool GRAD>
__device__ __forceinline__ void grounding_triplet_body(const TailArgs &a)
{
    __shared__ float red[kLossThreads];
    __shared__ float cf[kTailMaxB * kTailMaxB];               // the filled cost of the current tag
    __shared__ float dacc[GRAD ? kTailMaxB * kTailMaxB : 1];
    __shared__ float nw[kTailMaxB], nr[kTailMaxB];
    const int t = threadIdx.x, B = a.B, BB = B * B;
    const float margin = a.margin;
    tail_mask_counts(a, nw, nr);
    for (int tag = 0; tag < 2; tag++) {
        if (!a.cost[tag]) {                                   // (workgroup-uniform)
            if (!GRAD) tail_absent(a.out, tag);
            continue;
        }
        if (GRAD)
            for (int e = t; e < BB; e += kLossThreads) dacc[e] = 0.f;
        tail_fill(a.cost[tag], B, nw, nr, red, cf, a.pw[tag]);
        // thread k: column k (choose caption) and row k (choose image)
        const int k = t;
        int nc = -1, ni = -1;                                 // the selected negatives: cf[nc * B + k], cf[k * B + ni]
        float hc = 0.f, hi = 0.f, ac = 0.f, ai = 0.f;
        if (k < B) {
            const float pos = cf[k * B + k];
            float negc, negi;
            if (B < 2) {
                negc = negi = pos + margin;
            } else if (a.mining == LOCOV_TRIPLET_GIVEN) {
                const int64_t *idx = a.neg_idx + (int64_t)tag * 2 * B;
                int64_t p = idx[k], q = idx[B + k];
                p = p < 0 ? 0 : (p > B - 2 ? B - 2 : p);
                q = q < 0 ? 0 : (q > B - 2 ? B - 2 : q);
                nc = (int)(p < k ? p : p + 1);
                ni = (int)(q < k ? q : q + 1);
                negc = cf[nc * B + k];
                negi = cf[k * B + ni];
            } else {
                const bool easiest = a.mining == LOCOV_TRIPLET_EASIEST;
                for (int v = 0; v < B; v++) {
                    if (v == k) continue;
                    const float xc = cf[v * B + k], xi = cf[k * B + v];
                    if (nc < 0 || (easiest ? xc > cf[nc * B + k] : xc < cf[nc * B + k])) nc = v;
                    if (ni < 0 || (easiest ? xi > cf[k * B + ni] : xi < cf[k * B + ni])) ni = v;
                }
                negc = cf[nc * B + k];
                negi = cf[k * B + ni];
            }
            hc = fmaxf((pos - negc) + margin, 0.f);
            hi = fmaxf((pos - negi) + margin, 0.f);
            if (B < 2) nc = ni = -1;
            if (!GRAD) tail_accuracy(cf, B, k, ac, ai);
        }
        if (!GRAD) {
            tail_store_means(a.out, tag, B, hc, hi, ac, ai, red);
        } else {
            const float gc = tail_upstream(a.up[tag * 2], B), gi = tail_upstream(a.up[tag * 2 + 1], B);
            // column k's two entries belong to thread k alone, row k's likewise; the two passes meet, so a barrier parts them
            if (k < B && nc >= 0 && hc > 0.f) {
                dacc[k * B + k] += gc;
                dacc[nc * B + k] -= gc;
            }
            __syncthreads();
            if (k < B && ni >= 0 && hi > 0.f) {
                dacc[k * B + k] += gi;
                dacc[k * B + ni] -= gi;
            }
            __syncthreads();
            for (int e = t; e < BB; e += kLossThreads) tail_store_grad(a.d[tag], a.gpw[tag], e, tail_ok(nw, nr, B, e), dacc[e]);
        }
        __syncthreads();
    }
}

}  // namespace

// The kernels: thin shells, one workgroup of kLossThreads each.  _ce and _ce_dist are the same body under the two names the entry
// points of include/locov_hip.h launch (without and with pw / gpw).
template <bool GRAD>
__global__ __launch_bounds__(kLossThreads) void grounding_ce_kernel(TailArgs a) { grounding_ce_body<GRAD>(a); }

template <bool GRAD>
__global__ __launch_bounds__(kLossThreads) void grounding_ce_dist_kernel(TailArgs a) { grounding_ce_body<GRAD>(a); }

template <bool GRAD>
__global__ __launch_bounds__(kLossThreads) void grounding_triplet_kernel(TailArgs a) { grounding_triplet_body<GRAD>(a); }


// ---- the distillation losses (locov_distill_loss_fwd / _bwd; include/locov_hip.h states the arithmetic) ----
constexpr int kDistMaxB = LOCOV_DISTILL_MAX_B;

// Matrix X = 0 trans, 1 w2r, 2 r2w, staged as z = -cost / temperature; per column (softmax over dim 0, the "cap" view) and per row
// (dim 1, "img"): max, sum of exp(z - max) and its log -- softmax = exp(z - max) / sum and log_softmax = (z - max) - log(sum), as
// torch's softmax / log_softmax epilogues round them.
struct DistillSmem {
    float z[3][kDistMaxB * kDistMaxB];
    float cmx[3][kDistMaxB], csum[3][kDistMaxB], clse[3][kDistMaxB];
    float rmx[3][kDistMaxB], rsum[3][kDistMaxB], rlse[3][kDistMaxB];
    float aux[6][kDistMaxB];                                  // per-slice sums of the backward
    float red[kLossThreads];
};

struct DistillView {
    const DistillSmem &s;
    int B;
    __device__ __forceinline__ float zz(int X, int i, int j) const { return s.z[X][i * B + j]; }
    __device__ __forceinline__ float pcol(int X, int i, int j) const { return expf(zz(X, i, j) - s.cmx[X][j]) / s.csum[X][j]; }
    __device__ __forceinline__ float lcol(int X, int i, int j) const { return (zz(X, i, j) - s.cmx[X][j]) - s.clse[X][j]; }
    __device__ __forceinline__ float prow(int X, int i, int j) const { return expf(zz(X, i, j) - s.rmx[X][i]) / s.rsum[X][i]; }
    __device__ __forceinline__ float lrow(int X, int i, int j) const { return (zz(X, i, j) - s.rmx[X][i]) - s.rlse[X][i]; }
    // JS: the "cap" mixture of trans and cost X, and d L / d M at (i, j) up to the scale k (0 where M == 0: every path from M
    // to the logits there is multiplied by a zero probability -- the finite limit of torch's 0 * (-inf))
    __device__ __forceinline__ float mix(int X, int i, int j) const { return 0.5f * (pcol(0, i, j) + pcol(X, i, j)); }
    __device__ __forceinline__ float js_gm(int X, int i, int j, float k) const
    {
        const float m = mix(X, i, j);
        if (m == 0.f) return 0.f;
        const float lsum = ((lcol(0, i, j) + lcol(X, i, j)) + lrow(0, j, i)) + lrow(X, j, i);
        return k * (4.f * logf(m) - lsum);
    }
};

// xlogy(x, x) as kl_div's target term forms it: 0 where x == 0
__device__ __forceinline__ float xlogx(float x) { return x == 0.f ? 0.f : x * logf(x); }

template <bool GRAD>
__global__ __launch_bounds__(kLossThreads) void distill_loss_kernel(const float *__restrict__ trans, const float *__restrict__ w2r,
                                                                    const float *__restrict__ r2w, int B, int kind, int tt,
                                                                    float temperature, float loss_weight, float *__restrict__ loss,
                                                                    const float *__restrict__ gloss, float *__restrict__ dtrans,
                                                                    float *__restrict__ dw2r, float *__restrict__ dr2w)
{
    __shared__ DistillSmem s;
    const int t = threadIdx.x, BB = B * B;
    const float nb = (float)B;
    const float g = GRAD ? gloss[0] * loss_weight : 0.f;       // d L / d (the sum before loss_weight)
    if (kind == LOCOV_DISTILL_MSE) {
        // mse(trans, S) + mse(trans^T, S^T): the same mean counted twice, for S = w2r then r2w
        const float n = (float)BB;
        float s1 = 0.f, s2 = 0.f;
        for (int e = t; e < BB; e += kLossThreads) {
            const float a = trans[e] - w2r[e], b = trans[e] - r2w[e];
            if (GRAD) {
                const float ga = (2.f / n) * a * g, gb = (2.f / n) * b * g;    // mse_loss_backward: 2 / N * (x - y) * grad
                if (dtrans) dtrans[e] = (ga + ga) + (gb + gb);
                if (dw2r) dw2r[e] = -(ga + ga);
                if (dr2w) dr2w[e] = -(gb + gb);
            } else {
                s1 = s1 + a * a;
                s2 = s2 + b * b;
            }
        }
        if (!GRAD) {
            const float m1 = block_sum(s1, s.red) / n, m2 = block_sum(s2, s.red) / n;
            if (t == 0) loss[0] = (((m1 + m1) + m2) + m2) * loss_weight;
        }
        return;
    }
    // stage z = -cost / temperature (torch on the device: a negation, then a multiplication by the fp32 reciprocal)
    const float inv_t = 1.0f / temperature;
    for (int e = t; e < 3 * BB; e += kLossThreads) {
        const int X = e / BB, k = e - X * BB;
        const float *src = X == 0 ? trans : (X == 1 ? w2r : r2w);
        s.z[X][k] = -src[k] * inv_t;
    }
    __syncthreads();
    for (int u = t; u < 6 * B; u += kLossThreads) {
        const int X = u / (2 * B), r = u - X * 2 * B;
        const bool col = r < B;
        const int k = col ? r : r - B;
        const float *zx = s.z[X];
        float mx = -INFINITY;
        for (int v = 0; v < B; v++) mx = fmaxf(mx, col ? zx[v * B + k] : zx[k * B + v]);
        float sm = 0.f;
        for (int v = 0; v < B; v++) sm = sm + expf((col ? zx[v * B + k] : zx[k * B + v]) - mx);
        (col ? s.cmx : s.rmx)[X][k] = mx;
        (col ? s.csum : s.rsum)[X][k] = sm;
        (col ? s.clse : s.rlse)[X][k] = logf(sm);
    }
    __syncthreads();
    const DistillView v{s, B};
    const bool js = kind == LOCOV_DISTILL_JS;
    const float t2 = temperature * temperature;
    if (!GRAD) {
        // KD: sum over the two (teacher, student) pairs and both views of p_t log p_t - p_t log q_s; JS: over both costs of the four
        // kl_div(log ., M) terms (cap and img view of trans and of the cost, all against the cap mixture M)
        float part = 0.f;
        for (int e = t; e < BB; e += kLossThreads) {
            const int i = e / B, j = e - i * B;
#pragma unroll
            for (int X = 1; X <= 2; X++) {
                if (js) {
                    const float m = v.mix(X, i, j), xm = xlogx(m);
                    part = part + ((((xm - m * v.lcol(0, i, j)) + (xm - m * v.lcol(X, i, j))) + (xm - m * v.lrow(0, j, i))) +
                                   (xm - m * v.lrow(X, j, i)));
                } else {
                    const int te = tt ? 0 : X, st = tt ? X : 0;
                    const float pc = v.pcol(te, i, j), pr = v.prow(te, i, j);
                    part = part + ((xlogx(pc) - pc * v.lcol(st, i, j)) + (xlogx(pr) - pr * v.lrow(st, i, j)));
                }
            }
        }
        const float total = block_sum(part, s.red) / nb;
        if (t == 0) loss[0] = (js ? 0.5f * (total * t2) : total * t2) * loss_weight;
        return;
    }
    const float k = (js ? 0.5f : 1.f) * g * t2 / nb;          // d L / d (each element's term)
    // per-slice sums.  KD: aux[2 p + 0][j] = sum_i p_t (l_t - l_s) over column j, aux[2 p + 1][i] the same over row i, for the pair
    // p = (teacher, student) of cost X = p + 1.  JS, cost X = c + 1: aux[3 c][j] = column sums of M, aux[3 c + 1][j] / aux[3 c + 2][j]
    // = column sums of p_cap(trans) * dP / p_cap(cost) * dP, dP = d L / d p_cap = 1/2 d L / d M.
    const int ntask = (js ? 6 : 4) * B;
    for (int u = t; u < ntask; u += kLossThreads) {
        const int a = u / B, q = u - a * B;
        float acc = 0.f;
        if (js) {
            const int X = a / 3 + 1, w = a % 3;
            for (int i = 0; i < B; i++) {
                if (w == 0) acc = acc + v.mix(X, i, q);
                else acc = acc + v.pcol(w == 1 ? 0 : X, i, q) * (0.5f * v.js_gm(X, i, q, k));
            }
        } else {
            const int X = a / 2 + 1, te = tt ? 0 : X, st = tt ? X : 0;
            for (int r = 0; r < B; r++) {
                if ((a & 1) == 0) acc = acc + v.pcol(te, r, q) * (v.lcol(te, r, q) - v.lcol(st, r, q));
                else acc = acc + v.prow(te, q, r) * (v.lrow(te, q, r) - v.lrow(st, q, r));
            }
        }
        s.aux[a][q] = acc;
    }
    __syncthreads();
    for (int e = t; e < BB; e += kLossThreads) {
        const int i = e / B, j = e - i * B;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;                    // d L / d z of trans, w2r, r2w
#pragma unroll
        for (int X = 1; X <= 2; X++) {
            float &dx = X == 1 ? d1 : d2;
            if (js) {
                const int c = X - 1;
                const float dp = 0.5f * v.js_gm(X, i, j, k);
                const float mij = v.mix(X, i, j), mji = v.mix(X, j, i);
                const float *cm = s.aux[3 * c];
                // through p_cap (softmax over dim 0), log_softmax over dim 0 (cap view), log_softmax over dim 1 read transposed (img)
                const float pa = v.pcol(0, i, j), px = v.pcol(X, i, j);
                d0 = d0 + ((pa * (dp - s.aux[3 * c + 1][j]) + (-k * mij + pa * (k * cm[j]))) + (-k * mji + v.prow(0, i, j) * (k * cm[i])));
                dx = dx + ((px * (dp - s.aux[3 * c + 2][j]) + (-k * mij + px * (k * cm[j]))) + (-k * mji + v.prow(X, i, j) * (k * cm[i])));
            } else {
                const int te = tt ? 0 : X, st = tt ? X : 0;
                const float pct = v.pcol(te, i, j), prt = v.prow(te, i, j);
                // teacher: p_t (l_t - l_s - sum_slice p_t (l_t - l_s)), 0 where p_t == 0; student: p_s - p_t
                const float gt = k * (pct * ((v.lcol(te, i, j) - v.lcol(st, i, j)) - s.aux[2 * (X - 1)][j]) +
                                      prt * ((v.lrow(te, i, j) - v.lrow(st, i, j)) - s.aux[2 * (X - 1) + 1][i]));
                const float gs = k * ((v.pcol(st, i, j) - pct) + (v.prow(st, i, j) - prt));
                if (tt) {
                    d0 = d0 + gt;
                    dx = dx + gs;
                } else {
                    d0 = d0 + gs;
                    dx = dx + gt;
                }
            }
        }
        // z = -cost / temperature
        if (dtrans) dtrans[e] = -(d0 * inv_t);
        if (dw2r) dw2r[e] = -(d1 * inv_t);
        if (dr2w) dr2w[e] = -(d2 * inv_t);
    }
}

}  // namespace locov

extern "C" int locov_box_reg_loss(const float *proposal_boxes, const float *gt_boxes, const float *pred_deltas, int64_t ld,
                                  const int64_t *gt_classes, int64_t R, int64_t num_classes, float wx, float wy, float ww, float wh,
                                  float smooth_l1_beta, float *loss, float *dpred, locov_stream_t stream)
{
    using namespace locov;
    LOCOV_REQUIRE(R >= 0 && num_classes >= 1 && (ld == 4 || ld == 4 * num_classes),
                  "locov_box_reg_loss: pred_deltas must be [R, 4] or [R, 4 * num_classes]");
    LOCOV_REQUIRE(loss && (R == 0 || (proposal_boxes && gt_boxes && pred_deltas && gt_classes)), "locov_box_reg_loss: null pointer");
    LOCOV_REQUIRE(((uintptr_t)proposal_boxes | (uintptr_t)gt_boxes) % 16 == 0, "locov_box_reg_loss: boxes must be 16-byte aligned");
    hipLaunchKernelGGL(box_reg_loss_kernel, dim3(1), dim3(kLossThreads), 0, as_stream(stream), reinterpret_cast<const float4 *>(proposal_boxes),
                       reinterpret_cast<const float4 *>(gt_boxes), pred_deltas, ld, gt_classes, R, num_classes, wx, wy, ww, wh, smooth_l1_beta,
                       loss, dpred);
    return check_launch("locov_box_reg_loss");
}

// The grounding tail's entry points: the checks they share under the family's name `who`, each one's own null-output requirement,
// one launch.  (The cross-entropy entries pass a valid mining, which their kernels do not read.)
static int tail_args(const char *who, const locov::TailArgs &a)
{
    using namespace locov;
    LOCOV_REQUIRE(a.B >= 1 && a.B <= LOCOV_GROUNDING_CE_MAX_B && a.T >= 0 && a.NR >= 0, "%s: 1 <= B <= %d", who, LOCOV_GROUNDING_CE_MAX_B);
    LOCOV_REQUIRE(a.mining == LOCOV_TRIPLET_HARDEST || a.mining == LOCOV_TRIPLET_EASIEST || a.mining == LOCOV_TRIPLET_GIVEN,
                  "%s: unknown mining %d", who, a.mining);
    LOCOV_REQUIRE(a.mining != LOCOV_TRIPLET_GIVEN || a.neg_idx, "%s: given negatives need their indices", who);
    LOCOV_REQUIRE((a.cost[0] || a.cost[1]) && a.cmask && a.rmask, "%s: null pointer", who);
    return LOCOV_OK;
}

template <class Kernel>
static int tail_launch(Kernel kernel, const char *what, const locov::TailArgs &a, locov_stream_t stream)
{
    using namespace locov;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kLossThreads), 0, as_stream(stream), a);
    return check_launch(what);
}

extern "C" int locov_grounding_ce_fwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask, int B,
                                      int T, int NR, float *out8, locov_stream_t stream)
{
    using namespace locov;
    const TailArgs a = {{cost_w2r, cost_r2w}, caption_mask, region_mask, B, T, NR, LOCOV_TRIPLET_HARDEST, 0.f, nullptr, out8};
    if (int rc = tail_args("locov_grounding_ce", a)) return rc;
    LOCOV_REQUIRE(out8, "locov_grounding_ce_fwd: null output");
    return tail_launch(grounding_ce_kernel<false>, "locov_grounding_ce_fwd", a, stream);
}

extern "C" int locov_grounding_ce_bwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask, int B,
                                      int T, int NR, const float *g_w2r_caption, const float *g_w2r_image, const float *g_r2w_caption,
                                      const float *g_r2w_image, float *dcost_w2r, float *dcost_r2w, locov_stream_t stream)
{
    using namespace locov;
    const TailArgs a = {{cost_w2r, cost_r2w}, caption_mask, region_mask, B, T, NR, LOCOV_TRIPLET_HARDEST, 0.f, nullptr, nullptr, {},
                        {g_w2r_caption, g_w2r_image, g_r2w_caption, g_r2w_image}, {}, {dcost_w2r, dcost_r2w}};
    if (int rc = tail_args("locov_grounding_ce", a)) return rc;
    LOCOV_REQUIRE((!cost_w2r || dcost_w2r) && (!cost_r2w || dcost_r2w), "locov_grounding_ce_bwd: null gradient output");
    return tail_launch(grounding_ce_kernel<true>, "locov_grounding_ce_bwd", a, stream);
}

extern "C" int locov_grounding_ce_dist_fwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask,
                                           int B, int T, int NR, float *out8, float *pw_w2r, float *pw_r2w, locov_stream_t stream)
{
    using namespace locov;
    const TailArgs a = {{cost_w2r, cost_r2w}, caption_mask, region_mask, B, T, NR, LOCOV_TRIPLET_HARDEST, 0.f, nullptr, out8,
                        {pw_w2r, pw_r2w}};
    if (int rc = tail_args("locov_grounding_ce_dist", a)) return rc;
    LOCOV_REQUIRE(out8 && (!cost_w2r || pw_w2r) && (!cost_r2w || pw_r2w), "locov_grounding_ce_dist_fwd: null output");
    return tail_launch(grounding_ce_dist_kernel<false>, "locov_grounding_ce_dist_fwd", a, stream);
}

extern "C" int locov_grounding_ce_dist_bwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask,
                                           int B, int T, int NR, const float *g_w2r_caption, const float *g_w2r_image,
                                           const float *g_r2w_caption, const float *g_r2w_image, const float *g_pw_w2r,
                                           const float *g_pw_r2w, float *dcost_w2r, float *dcost_r2w, locov_stream_t stream)
{
    using namespace locov;
    const TailArgs a = {{cost_w2r, cost_r2w}, caption_mask, region_mask, B, T, NR, LOCOV_TRIPLET_HARDEST, 0.f, nullptr, nullptr, {},
                        {g_w2r_caption, g_w2r_image, g_r2w_caption, g_r2w_image}, {g_pw_w2r, g_pw_r2w}, {dcost_w2r, dcost_r2w}};
    if (int rc = tail_args("locov_grounding_ce_dist", a)) return rc;
    LOCOV_REQUIRE((!cost_w2r || dcost_w2r) && (!cost_r2w || dcost_r2w), "locov_grounding_ce_dist_bwd: null gradient output");
    return tail_launch(grounding_ce_dist_kernel<true>, "locov_grounding_ce_dist_bwd", a, stream);
}

extern "C" int locov_grounding_triplet_fwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask,
                                           int B, int T, int NR, int mining, float margin, const int64_t *neg_idx, float *out8,
                                           float *pw_w2r, float *pw_r2w, locov_stream_t stream)
{
    using namespace locov;
    const TailArgs a = {{cost_w2r, cost_r2w}, caption_mask, region_mask, B, T, NR, mining, margin, neg_idx, out8, {pw_w2r, pw_r2w}};
    if (int rc = tail_args("locov_grounding_triplet", a)) return rc;
    LOCOV_REQUIRE(out8, "locov_grounding_triplet_fwd: null output");
    return tail_launch(grounding_triplet_kernel<false>, "locov_grounding_triplet_fwd", a, stream);
}

extern "C" int locov_grounding_triplet_bwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask,
                                           int B, int T, int NR, int mining, float margin, const int64_t *neg_idx,
                                           const float *g_w2r_caption, const float *g_w2r_image, const float *g_r2w_caption,
                                           const float *g_r2w_image, const float *g_pw_w2r, const float *g_pw_r2w, float *dcost_w2r,
                                           float *dcost_r2w, locov_stream_t stream)
{
    using namespace locov;
    const TailArgs a = {{cost_w2r, cost_r2w}, caption_mask, region_mask, B, T, NR, mining, margin, neg_idx, nullptr, {},
                        {g_w2r_caption, g_w2r_image, g_r2w_caption, g_r2w_image}, {g_pw_w2r, g_pw_r2w}, {dcost_w2r, dcost_r2w}};
    if (int rc = tail_args("locov_grounding_triplet", a)) return rc;
    LOCOV_REQUIRE((!cost_w2r || dcost_w2r) && (!cost_r2w || dcost_r2w), "locov_grounding_triplet_bwd: null gradient output");
    return tail_launch(grounding_triplet_kernel<true>, "locov_grounding_triplet_bwd", a, stream);
}


static int distill_args(const float *trans, const float *w2r, const float *r2w, int B, int kind, float temperature)
{
    using namespace locov;
    LOCOV_REQUIRE(B >= 1 && B <= LOCOV_DISTILL_MAX_B, "locov_distill_loss: 1 <= B <= %d", LOCOV_DISTILL_MAX_B);
    LOCOV_REQUIRE(kind == LOCOV_DISTILL_KD || kind == LOCOV_DISTILL_JS || kind == LOCOV_DISTILL_MSE, "locov_distill_loss: unknown kind %d",
                  kind);
    LOCOV_REQUIRE(temperature > 0.f, "locov_distill_loss: temperature must be > 0");
    LOCOV_REQUIRE(trans && w2r && r2w, "locov_distill_loss: null pointer");
    return LOCOV_OK;
}

extern "C" int locov_distill_loss_fwd(const float *trans, const float *w2r, const float *r2w, int B, int kind, int transformer_teacher,
                                      float temperature, float loss_weight, float *loss, locov_stream_t stream)
{
    using namespace locov;
    if (int rc = distill_args(trans, w2r, r2w, B, kind, temperature)) return rc;
    LOCOV_REQUIRE(loss, "locov_distill_loss_fwd: null output");
    hipLaunchKernelGGL(distill_loss_kernel<false>, dim3(1), dim3(kLossThreads), 0, as_stream(stream), trans, w2r, r2w, B, kind,
                       transformer_teacher ? 1 : 0, temperature, loss_weight, loss, nullptr, nullptr, nullptr, nullptr);
    return check_launch("locov_distill_loss_fwd");
}

extern "C" int locov_distill_loss_bwd(const float *trans, const float *w2r, const float *r2w, int B, int kind, int transformer_teacher,
                                      float temperature, float loss_weight, const float *grad_loss, float *grad_trans, float *grad_w2r,
                                      float *grad_r2w, locov_stream_t stream)
{
    using namespace locov;
    if (int rc = distill_args(trans, w2r, r2w, B, kind, temperature)) return rc;
    LOCOV_REQUIRE(grad_loss, "locov_distill_loss_bwd: null grad_loss");
    if (!grad_trans && !grad_w2r && !grad_r2w) return LOCOV_OK;      // nothing asks for a gradient
    hipLaunchKernelGGL(distill_loss_kernel<true>, dim3(1), dim3(kLossThreads), 0, as_stream(stream), trans, w2r, r2w, B, kind,
                       transformer_teacher ? 1 : 0, temperature, loss_weight, nullptr, grad_loss, grad_trans, grad_w2r, grad_r2w);
    return check_launch("locov_distill_loss_bwd");
}
