// Multi-token class scoring of the grounding predictor:
// ovr/modeling/roi_heads/box_emb_grounding_head.py:60-256 GroundingModule.forward after its
// token_score Linear (that GEMM is locov_gemm_nt_f32 on the concatenated token bank).
//
// Per region r and class k with n_k real tokens (the reference pads every class to Tmax slots):
//   s_t = sim[r, off_k + t] / temperature                      (cosine: NaN -> 0 first)
//   d_t = -s_t (dot)  |  (1 - sim) / temperature (cosine)
//   masked s_t = s_t for t < n_k, else gmin - 100               (gmin = min of the padded tensor)
//   a = softmax_t(masked s)  |  one_hot(argmax_t masked s)      over all Tmax slots
//   att_t = a_t * [t < n_k];   score = -sum_t att_t * d_t
// A class without tokens (the background row) keeps the one slot the reference's in-place
// `split_sizes[split_sizes == 0] = 1` gives it, but its mask row is zero: attention 0, score -0.
// One lane per (r, k); Tmax is small (<= 32), everything stays in registers.
#include "common.h"

namespace locov {

constexpr int kTokMax = 32;

// What both directions form per (r, k) from the class's columns of one row of sim: the distances d_t, the masked s_t, their first
// maximum, and under softmax exp(s_t - max) (left in s) with its sum over all Tmax slots.
__device__ __forceinline__ void token_terms(const float *__restrict__ row, int n, int Tmax, float temp, int cosine, int hardmax,
                                            float fill, float (&s)[kTokMax], float (&d)[kTokMax], int &arg, float &denom)
{
    float mx = -INFINITY;
    arg = 0;
#pragma unroll
    for (int t = 0; t < kTokMax; t++) {
        if (t >= Tmax) break;
        float v = t < n ? row[t] : 0.f;
        if (cosine && v != v) v = 0.f;
        d[t] = (cosine ? (1.0f - v) : -v) / temp;
        s[t] = t < n ? v / temp : fill;
        if (s[t] > mx) {                                      // first maximum, as torch.argmax
            mx = s[t];
            arg = t;
        }
    }
    denom = 0.f;
    if (!hardmax) {
#pragma unroll
        for (int t = 0; t < kTokMax; t++) {
            if (t >= Tmax) break;
            s[t] = expf(s[t] - mx);
            denom += s[t];
        }
    }
}

__global__ __launch_bounds__(256) void token_attention_kernel(const float *__restrict__ sim, int64_t R, int Ttot,
                                                              const int *__restrict__ tok_off,
                                                              const int *__restrict__ num_tok, int K1, int Tmax,
                                                              float temp, int cosine, int hardmax,
                                                              const float *__restrict__ gmin,
                                                              float *__restrict__ scores, float *__restrict__ att)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * K1) return;
    const int64_t r = idx / K1;
    const int k = (int)(idx - r * K1);
    const int n = num_tok[k], off = tok_off[k];
    const float fill = gmin[0] - 100.0f;
    const float *row = sim + r * Ttot + off;
    float s[kTokMax], d[kTokMax];
    int arg;
    float denom;
    token_terms(row, n, Tmax, temp, cosine, hardmax, fill, s, d, arg, denom);
    float dist = 0.f;
#pragma unroll
    for (int t = 0; t < kTokMax; t++) {
        if (t >= Tmax) break;
        float a = hardmax ? (t == arg ? 1.f : 0.f) : s[t] / denom;
        a = t < n ? a : 0.f;
        dist += a * d[t];
        if (att) att[idx * Tmax + t] = a;
    }
    scores[idx] = -dist;
}

// The way back (the reference's autograd through box_emb_grounding_head.py:152-183).  With att_t = a_t [t < n] and
// score = -sum_t att_t d_t, d d_t / d s_t = -1 in both metrics, for j < n:
//   softmax: dL/ds_j = g a_j (1 - d_j + sum_t att_t d_t) + a_j (ga_j - sum_{t<n} ga_t a_t)     (g = grad_scores, ga = grad_att)
//   hardmax: dL/ds_j = g [j == argmax]                                       (the one-hot attention is a constant)
//   dL/dsim_j = dL/ds_j / temperature;  0 where the cosine branch replaced a NaN similarity;  gmin is detached.
// One lane per (r, k), as the forward: class k owns the columns [off_k, off_k + max(n_k, 1)) of a row and the classes' ranges
// partition [0, Ttot), so this lane is the only writer of its elements and every element has a writer -- no atomics, no
// zeroed buffer.  Adjacent lanes own adjacent ranges (classes in bank order): a wave reads and writes one contiguous span.
__global__ __launch_bounds__(256) void token_attention_bwd_kernel(const float *__restrict__ sim, int64_t R, int Ttot,
                                                                  const int *__restrict__ tok_off,
                                                                  const int *__restrict__ num_tok, int K1, int Tmax,
                                                                  float temp, int cosine, int hardmax,
                                                                  const float *__restrict__ gmin,
                                                                  const float *__restrict__ grad_scores,
                                                                  const float *__restrict__ grad_att,
                                                                  float *__restrict__ grad_sim)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * K1) return;
    const int64_t r = idx / K1;
    const int k = (int)(idx - r * K1);
    const int n = num_tok[k], off = tok_off[k];
    if (off < 0 || off + (n > 0 ? n : 1) > Ttot) return;      // a layout that breaks the contract is never written out of bounds
    const float *row = sim + r * Ttot + off;
    float *out = grad_sim + r * Ttot + off;
    if (n <= 0) {                                             // the background row's one column
        out[0] = 0.f;
        return;
    }
    const float fill = gmin[0] - 100.0f;
    float s[kTokMax], d[kTokMax];
    int arg;
    float denom;
    token_terms(row, n, Tmax, temp, cosine, hardmax, fill, s, d, arg, denom);
    const float g = grad_scores[idx];
    if (hardmax) {
#pragma unroll
        for (int t = 0; t < kTokMax; t++) {
            if (t >= Tmax || t >= n) break;
            const float v = row[t];
            out[t] = (t == arg && !(cosine && v != v)) ? g / temp : 0.f;
        }
        return;
    }
    const float *ga = grad_att ? grad_att + idx * Tmax : nullptr;
    float dist = 0.f, gdot = 0.f;
#pragma unroll
    for (int t = 0; t < kTokMax; t++) {
        if (t >= Tmax || t >= n) break;
        s[t] = s[t] / denom;                                  // a_t
        dist += s[t] * d[t];
        if (ga) gdot += ga[t] * s[t];
    }
#pragma unroll
    for (int t = 0; t < kTokMax; t++) {
        if (t >= Tmax || t >= n) break;
        float ds = g * s[t] * (1.0f - d[t] + dist);
        if (ga) ds += s[t] * (ga[t] - gdot);
        const float v = row[t];
        out[t] = (cosine && v != v) ? 0.f : ds / temp;
    }
}

}  // namespace locov

using namespace locov;

extern "C" int locov_token_attention_fwd(const float *sim, int64_t R, int Ttot, const int *tok_off, const int *num_tok,
                                         int K1, int Tmax, float temperature, int cosine, int hardmax,
                                         const float *gmin, float *scores, float *att, locov_stream_t stream)
{
    LOCOV_REQUIRE(R >= 0 && Ttot > 0 && K1 > 0, "locov_token_attention_fwd: bad shape R=%lld Ttot=%d K1=%d", (long long)R, Ttot,
                  K1);
    LOCOV_REQUIRE(Tmax > 0 && Tmax <= kTokMax, "locov_token_attention_fwd: Tmax must be in [1, %d] (got %d)", kTokMax, Tmax);
    LOCOV_REQUIRE(temperature > 0.f, "locov_token_attention_fwd: temperature must be > 0");
    if (R == 0) return LOCOV_OK;
    LOCOV_REQUIRE(sim && tok_off && num_tok && gmin && scores, "locov_token_attention_fwd: null pointer");
    const int64_t total = R * K1;
    hipLaunchKernelGGL(token_attention_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, as_stream(stream), sim, R,
                       Ttot, tok_off, num_tok, K1, Tmax, temperature, cosine, hardmax, gmin, scores, att);
    return check_launch("locov_token_attention_fwd");
}

extern "C" int locov_token_attention_bwd(const float *sim, int64_t R, int Ttot, const int *tok_off, const int *num_tok,
                                         int K1, int Tmax, float temperature, int cosine, int hardmax,
                                         const float *gmin, const float *grad_scores, const float *grad_att,
                                         float *grad_sim, locov_stream_t stream)
{
    LOCOV_REQUIRE(R >= 0 && Ttot > 0 && K1 > 0, "locov_token_attention_bwd: bad shape R=%lld Ttot=%d K1=%d", (long long)R, Ttot,
                  K1);
    LOCOV_REQUIRE(Tmax > 0 && Tmax <= kTokMax, "locov_token_attention_bwd: Tmax must be in [1, %d] (got %d)", kTokMax, Tmax);
    LOCOV_REQUIRE(temperature > 0.f, "locov_token_attention_bwd: temperature must be > 0");
    if (R == 0) return LOCOV_OK;
    LOCOV_REQUIRE(sim, "locov_token_attention_bwd: null pointer sim");
    LOCOV_REQUIRE(tok_off && num_tok, "locov_token_attention_bwd: null pointer tok_off / num_tok");
    LOCOV_REQUIRE(gmin, "locov_token_attention_bwd: null pointer gmin");
    LOCOV_REQUIRE(grad_scores, "locov_token_attention_bwd: null pointer grad_scores");
    LOCOV_REQUIRE(grad_sim, "locov_token_attention_bwd: null pointer grad_sim");      // (grad_att may be null: attention unused)
    const int64_t total = R * K1;
    hipLaunchKernelGGL(token_attention_bwd_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, as_stream(stream), sim, R,
                       Ttot, tok_off, num_tok, K1, Tmax, temperature, cosine, hardmax, gmin, grad_scores, grad_att, grad_sim);
    return check_launch("locov_token_attention_bwd");
}
