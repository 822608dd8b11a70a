// The caption path of the LSM step: BertEmbedding's forward (ovr/modeling/language/transf_models.py:105-154) after the tokenizer.
//
// Replaces the host loop over B * T tokens that draws np.random.rand() per token (:114-137), the torch.tensor(v).cuda() per
// dictionary key (:139) and the index / embedding / LayerNorm / dropout launches behind them (:142-152) with ONE launch:
//
//   caption_embed_kernel    one 64-lane wave per token, four tokens per workgroup.  The wave reads the token's four tokenizer
//                           integers and its two float64 draws, applies the masked-language-modelling rule (every comparison in
//                           double, as numpy's float64 draw meets Python floats) -- a wave-uniform decision --, lane 0 writes the
//                           six int64 outputs, and all lanes copy row W[id] (input_embeddings).  With the position embedding on, the
//                           row (W[id] + Tt[type]) + P[j] stays in registers (H = 768: three float4 per lane), both LayerNorm
//                           reductions are wave shuffles (mean, then the biased variance of the centred row), and the normalised,
//                           scaled, dropped row is written as encoded_tokens with the token's mean and rstd.
//
// Backward (only word_embeddings.weight trains, :156-164), no atomics, fixed order, every row of dW written by the launch:
//   caption_rank_kernel     one workgroup: the ids go to LDS and token n counts the tokens with a smaller (id, n) pair -- the
//                           counting rank of regions_select_kernel -- giving the tokens ordered by (id, flat position).
//   caption_ln_bwd_kernel   LayerNorm path only, one wave per token: dx = LN-backward(g_enc * keep / (1 - p)) + g_in.
//   caption_scatter_kernel  grid-stride, one wave per vocabulary row: binary search of the row's run in the sorted ids, then
//                           0.0f + the gradient rows of its tokens in ascending flat position; an empty run writes zeros.
#include "reduce_common.h"

#include <cmath>

namespace locov {

constexpr int kCapThreads = 256;
constexpr int kCapRankThreads = 1024;
constexpr int kCapMaxTokens = LOCOV_CAPTION_MAX_TOKENS;

__device__ __forceinline__ float wave_sum(float v) { return wave_reduce(v, SumOp()); }

struct CaptionMlm {
    double p, p_mask, p_mask_noise;      // MASKED_LANGUAGE_MODELING_PROB, _PROB_MASK, _PROB_MASK + _PROB_NOISE (summed in double by the host)
    int mask_id, len_tok;
};

struct CaptionLn {                       // null P: ADD_POSITION_EMBEDDING off, encoded_tokens is input_embeddings
    const float *P, *Tt, *gamma, *beta;
    const uint8_t *keep;
    float eps, drop_scale;               // drop_scale = 1 / (1 - p_drop)
};

template <int VEC> struct Row;
template <> struct Row<4> { typedef float4 type; };
template <> struct Row<1> { typedef float type; };

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// VEC = 4: 16-byte lanes (H % 4 == 0, every pointer 16-byte aligned); VEC = 1 otherwise.  MAXC: register slots per lane,
// 64 * VEC * MAXC >= H.
template <int VEC, int MAXC>
__global__ __launch_bounds__(kCapThreads) void caption_embed_kernel(
    const int *__restrict__ packed, const double *__restrict__ draws, int N, int T, int H, const float *__restrict__ W, CaptionLn ln,
    CaptionMlm mlm, int int_rows, int64_t *__restrict__ ints, float *__restrict__ input_emb, float *__restrict__ encoded,
    float *__restrict__ mean_out, float *__restrict__ rstd_out)
{
    const int n = blockIdx.x * (kCapThreads / kWave) + (threadIdx.x >> 6);
    if (n >= N) return;
    const int lane = threadIdx.x & 63;
    int id = packed[n];
    const int type = packed[N + n], attn = packed[2 * N + n];
    int special = packed[3 * N + n];
    const int target = id;
    int selected = 0;
    if (draws != nullptr && !special && attn) {          // :120-124 (draws == nullptr: neither training nor MLM validation)
        const double u = draws[n];
        if (u < mlm.p) {                                 // :126
            selected = 1;
            const double q = u / mlm.p;                  // :128
            if (q < mlm.p_mask) {                        // :129-132
                id = mlm.mask_id;
                special = 1;
            } else if (q < mlm.p_mask_noise) {           // :133-134, np.random.randint(len(tokenizer)) from the second draw
                const long long r = (long long)(draws[N + n] * (double)mlm.len_tok);
                id = (int)(r < mlm.len_tok - 1 ? r : mlm.len_tok - 1);
            }
        }
    }
    if (lane == 0) {
        ints[n] = id;
        ints[(int64_t)N + n] = type;
        ints[(int64_t)2 * N + n] = attn;
        ints[(int64_t)3 * N + n] = special;
        if (int_rows == 6) {
            ints[(int64_t)4 * N + n] = target;
            ints[(int64_t)5 * N + n] = selected;
        }
    }

    typedef typename Row<VEC>::type vec;
    const int chunks = H / VEC;
    const vec *w = reinterpret_cast<const vec *>(W + (int64_t)id * H);
    vec *o_in = reinterpret_cast<vec *>(input_emb + (int64_t)n * H);
    vec x[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; k++) {
        const int c = lane + k * kWave;
        if (c < chunks) {
            x[k] = w[c];
            o_in[c] = x[k];
        }
    }
    if (ln.P == nullptr) return;

    const vec *pt = reinterpret_cast<const vec *>(ln.Tt + (int64_t)type * H);
    const vec *pp = reinterpret_cast<const vec *>(ln.P + (int64_t)(n % T) * H);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MAXC; k++) {
        const int c = lane + k * kWave;
        if (c < chunks) {
            if constexpr (VEC == 4) {
                x[k] = add4(add4(x[k], pt[c]), pp[c]);
                s += (x[k].x + x[k].y) + (x[k].z + x[k].w);
            } else {
                x[k] = (x[k] + pt[c]) + pp[c];
                s += x[k];
            }
        }
    }
    const float mean = wave_sum(s) / (float)H;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < MAXC; k++) {
        const int c = lane + k * kWave;
        if (c < chunks) {
            if constexpr (VEC == 4) {
                x[k] = make_float4(x[k].x - mean, x[k].y - mean, x[k].z - mean, x[k].w - mean);
                v += (x[k].x * x[k].x + x[k].y * x[k].y) + (x[k].z * x[k].z + x[k].w * x[k].w);
            } else {
                x[k] -= mean;
                v += x[k] * x[k];
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)H + ln.eps);
    if (lane == 0) {
        mean_out[n] = mean;
        rstd_out[n] = rstd;
    }
    const vec *ga = reinterpret_cast<const vec *>(ln.gamma), *be = reinterpret_cast<const vec *>(ln.beta);
    vec *o_enc = reinterpret_cast<vec *>(encoded + (int64_t)n * H);
    const uint8_t *keep = ln.keep ? ln.keep + (int64_t)n * H : nullptr;
#pragma unroll
    for (int k = 0; k < MAXC; k++) {
        const int c = lane + k * kWave;
        if (c < chunks) {
            if constexpr (VEC == 4) {
                const float4 g = ga[c], b = be[c];
                float4 y = make_float4(x[k].x * rstd * g.x + b.x, x[k].y * rstd * g.y + b.y, x[k].z * rstd * g.z + b.z,
                                       x[k].w * rstd * g.w + b.w);
                if (keep) {
                    const uchar4 m = reinterpret_cast<const uchar4 *>(keep)[c];
                    y = make_float4(m.x ? y.x * ln.drop_scale : 0.f, m.y ? y.y * ln.drop_scale : 0.f, m.z ? y.z * ln.drop_scale : 0.f,
                                    m.w ? y.w * ln.drop_scale : 0.f);
                }
                o_enc[c] = y;
            } else {
                float y = x[k] * rstd * ga[c] + be[c];
                if (keep) y = keep[c] ? y * ln.drop_scale : 0.f;
                o_enc[c] = y;
            }
        }
    }
}

// The N tokens ordered by (id, flat position): sorted_ids[r], order[r] = the id and the position of the token of rank r.
__global__ __launch_bounds__(kCapRankThreads) void caption_rank_kernel(const int64_t *__restrict__ ids, int N, int *__restrict__ sorted_ids,
                                                                       int *__restrict__ order)
{
    __shared__ int sid[kCapMaxTokens];
    for (int n = threadIdx.x; n < N; n += kCapRankThreads) sid[n] = (int)ids[n];
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += kCapRankThreads) {
        const int k = sid[n];
        int rank = 0;
        for (int o = 0; o < N; o++) {                    // (every lane reads the same LDS word: a broadcast)
            const int ko = sid[o];
            rank += (ko < k || (ko == k && o < n)) ? 1 : 0;
        }
        sorted_ids[rank] = k;                            // (rank is a permutation of 0 .. N-1: every slot is written once)
        order[rank] = n;
    }
}

// dx[n] = LN-backward(g_enc[n] * keep / (1 - p)) + g_in[n]; x and xhat are formed again from the tables, the mean and the rstd.
__global__ __launch_bounds__(kCapThreads) void caption_ln_bwd_kernel(
    const int64_t *__restrict__ ints, int N, int T, int H, const float *__restrict__ W, CaptionLn ln, const float *__restrict__ mean_in,
    const float *__restrict__ rstd_in, const float *__restrict__ g_enc, const float *__restrict__ g_in, float *__restrict__ dx)
{
    const int n = blockIdx.x * (kCapThreads / kWave) + (threadIdx.x >> 6);
    if (n >= N) return;
    const int lane = threadIdx.x & 63;
    const float *w = W + ints[n] * H, *pt = ln.Tt + ints[(int64_t)N + n] * H, *pp = ln.P + (int64_t)(n % T) * H;
    const float mean = mean_in[n], rstd = rstd_in[n];
    const float *ge = g_enc ? g_enc + (int64_t)n * H : nullptr, *gi = g_in ? g_in + (int64_t)n * H : nullptr;
    const uint8_t *keep = ln.keep ? ln.keep + (int64_t)n * H : nullptr;
    float *o = dx + (int64_t)n * H;
    float s1 = 0.f, s2 = 0.f;
    if (ge) {
        for (int c = lane; c < H; c += kWave) {
            float g = ge[c];
            if (keep) g = keep[c] ? g * ln.drop_scale : 0.f;
            const float gh = g * ln.gamma[c];
            const float xh = (((w[c] + pt[c]) + pp[c]) - mean) * rstd;
            s1 += gh;
            s2 += gh * xh;
        }
    }
    s1 = wave_sum(s1) / (float)H;
    s2 = wave_sum(s2) / (float)H;
    for (int c = lane; c < H; c += kWave) {
        float d = gi ? gi[c] : 0.f;
        if (ge) {
            float g = ge[c];
            if (keep) g = keep[c] ? g * ln.drop_scale : 0.f;
            const float gh = g * ln.gamma[c];
            const float xh = (((w[c] + pt[c]) + pp[c]) - mean) * rstd;
            d += rstd * ((gh - s1) - xh * s2);
        }
        o[c] = d;
    }
}

// dW[v] = 0.0f + g[order[lo]] + g[order[lo + 1]] + ... over the run [lo, end) of id v in sorted_ids, left to right.
template <int VEC>
__global__ __launch_bounds__(kCapThreads) void caption_scatter_kernel(const int *__restrict__ sorted_ids, const int *__restrict__ order, int N,
                                                                     int V, int H, const float *__restrict__ g, float *__restrict__ dW)
{
    typedef typename Row<VEC>::type vec;
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * (kCapThreads / kWave);
    const int chunks = H / VEC;
    for (int v = blockIdx.x * (kCapThreads / kWave) + (threadIdx.x >> 6); v < V; v += waves) {
        int lo = 0, hi = N;
        while (lo < hi) {                                // first rank whose id is >= v
            const int mid = (lo + hi) >> 1;
            if (sorted_ids[mid] < v) lo = mid + 1; else hi = mid;
        }
        int end = lo;
        while (end < N && sorted_ids[end] == v) end++;
        vec *o = reinterpret_cast<vec *>(dW + (int64_t)v * H);
        for (int c = lane; c < chunks; c += kWave) {
            vec acc;
            if constexpr (VEC == 4) acc = make_float4(0.f, 0.f, 0.f, 0.f); else acc = 0.f;
            for (int r = lo; r < end; r++) {
                const vec t = reinterpret_cast<const vec *>(g + (int64_t)order[r] * H)[c];
                if constexpr (VEC == 4) acc = add4(acc, t); else acc += t;
            }
            o[c] = acc;
        }
    }
}

static bool cap_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <int VEC, int MAXC>
static void launch_embed(const int *packed, const double *draws, int N, int T, int H, const float *W, const CaptionLn &ln, const CaptionMlm &mlm,
                         int int_rows, int64_t *ints, float *input_emb, float *encoded, float *mean, float *rstd, hipStream_t s)
{
    hipLaunchKernelGGL((caption_embed_kernel<VEC, MAXC>), dim3((unsigned)ceil_div(N, kCapThreads / kWave)), dim3(kCapThreads), 0, s, packed,
                       draws, N, T, H, W, ln, mlm, int_rows, ints, input_emb, encoded, mean, rstd);
}

}  // namespace locov

using namespace locov;

extern "C" {

int locov_caption_embed_fwd(const int *packed, const double *draws, int N, int T, int H, int V, const float *W, const float *P,
                            int max_pos, const float *Tt, int type_vocab, const float *gamma, const float *beta, float eps,
                            const uint8_t *keep, float p_drop, double p, double p_mask, double p_mask_noise, int mask_id, int len_tok,
                            int int_rows, int64_t *ints, float *input_emb, float *encoded, float *mean, float *rstd,
                            locov_stream_t stream)
{
    LOCOV_REQUIRE(N >= 0 && T >= 0 && H >= 0 && V >= 0, "locov_caption_embed_fwd: negative count (N=%d T=%d H=%d V=%d)", N, T, H, V);
    if (N > LOCOV_CAPTION_MAX_TOKENS || H > LOCOV_CAPTION_MAX_HIDDEN)
        return set_error(LOCOV_ERR_UNSUPPORTED, "locov_caption_embed_fwd: N = %d tokens / H = %d over the limits (%d, %d)", N, H,
                         LOCOV_CAPTION_MAX_TOKENS, LOCOV_CAPTION_MAX_HIDDEN);
    LOCOV_REQUIRE(int_rows == 4 || int_rows == 6, "locov_caption_embed_fwd: int_rows must be 4 or 6, got %d", int_rows);
    if (N == 0 || H == 0) return LOCOV_OK;
    LOCOV_REQUIRE(T >= 1 && N % T == 0, "locov_caption_embed_fwd: N = %d is not a multiple of T = %d", N, T);
    LOCOV_REQUIRE(V >= 1, "locov_caption_embed_fwd: empty word table");
    LOCOV_REQUIRE(packed && W && ints && input_emb, "locov_caption_embed_fwd: null pointer (packed / W / ints / input_emb)");
    if (draws) {
        LOCOV_REQUIRE(int_rows == 6, "locov_caption_embed_fwd: draws need int_rows == 6 (target_ids, mlm_mask)");
        LOCOV_REQUIRE(mask_id >= 0 && mask_id < V, "locov_caption_embed_fwd: mask_id %d outside the word table [0, %d)", mask_id, V);
        LOCOV_REQUIRE(len_tok >= 1 && len_tok <= V, "locov_caption_embed_fwd: len_tok %d outside [1, V = %d]", len_tok, V);
        LOCOV_REQUIRE(p > 0.0 && p <= 1.0 && p_mask >= 0.0 && p_mask_noise >= p_mask,
                      "locov_caption_embed_fwd: MLM probabilities must satisfy 0 < p <= 1, 0 <= p_mask <= p_mask + p_noise");
    }
    CaptionLn ln = {nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 1.f};
    if (P) {
        LOCOV_REQUIRE(Tt && gamma && beta && encoded && mean && rstd,
                      "locov_caption_embed_fwd: null pointer (the LayerNorm path needs Tt, gamma, beta, encoded, mean, rstd)");
        LOCOV_REQUIRE(T <= max_pos, "locov_caption_embed_fwd: T = %d exceeds the %d position embeddings", T, max_pos);
        LOCOV_REQUIRE(type_vocab >= 1, "locov_caption_embed_fwd: type_vocab must be >= 1");
        LOCOV_REQUIRE(eps >= 0.f, "locov_caption_embed_fwd: eps must be >= 0");
        if (keep) LOCOV_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "locov_caption_embed_fwd: p_drop must be in [0, 1)");
        ln = {P, Tt, gamma, beta, keep, eps, keep ? 1.0f / (1.0f - p_drop) : 1.f};
    }
    const CaptionMlm mlm = {p, p_mask, p_mask_noise, mask_id, len_tok};
    const hipStream_t s = as_stream(stream);
    const bool vec = H % 4 == 0 && cap_aligned16(W) && cap_aligned16(input_emb) &&
                     (!P || (cap_aligned16(P) && cap_aligned16(Tt) && cap_aligned16(gamma) && cap_aligned16(beta) && cap_aligned16(encoded) &&
                             (!keep || ((uintptr_t)keep & 3) == 0)));
#define CAP_LAUNCH(VEC, MAXC) launch_embed<VEC, MAXC>(packed, draws, N, T, H, W, ln, mlm, int_rows, ints, input_emb, encoded, mean, rstd, s)
    if (vec) {
        if (H <= 4 * kWave * 4) CAP_LAUNCH(4, 4); else CAP_LAUNCH(4, 16);
    } else {
        if (H <= kWave * 4) CAP_LAUNCH(1, 4); else if (H <= kWave * 16) CAP_LAUNCH(1, 16); else CAP_LAUNCH(1, 64);
    }
#undef CAP_LAUNCH
    return check_launch("locov_caption_embed_fwd");
}

int64_t locov_caption_embed_bwd_workspace_bytes(int N, int H, int layer_norm)
{
    if (N <= 0 || H <= 0) return 0;
    const int64_t ranks = (((int64_t)2 * N * 4) + 15) / 16 * 16;
    return ranks + (layer_norm ? (int64_t)N * H * 4 : 0);
}

int locov_caption_embed_bwd(const int64_t *ints, int N, int T, int H, int V, const float *W, const float *P, const float *Tt,
                            const float *gamma, const float *mean, const float *rstd, const uint8_t *keep, float p_drop,
                            const float *g_enc, const float *g_in, float *dW, void *workspace, int64_t workspace_bytes,
                            locov_stream_t stream)
{
    LOCOV_REQUIRE(N >= 0 && T >= 0 && H >= 0 && V >= 0, "locov_caption_embed_bwd: negative count (N=%d T=%d H=%d V=%d)", N, T, H, V);
    if (N > LOCOV_CAPTION_MAX_TOKENS || H > LOCOV_CAPTION_MAX_HIDDEN)
        return set_error(LOCOV_ERR_UNSUPPORTED, "locov_caption_embed_bwd: N = %d tokens / H = %d over the limits (%d, %d)", N, H,
                         LOCOV_CAPTION_MAX_TOKENS, LOCOV_CAPTION_MAX_HIDDEN);
    if (V == 0 || H == 0) return LOCOV_OK;
    LOCOV_REQUIRE(dW, "locov_caption_embed_bwd: null pointer (dW)");
    LOCOV_REQUIRE(N == 0 || (ints && workspace), "locov_caption_embed_bwd: null pointer (ints / workspace)");
    const bool layer_norm = P != nullptr;
    LOCOV_REQUIRE(N == 0 || g_in || (layer_norm && g_enc), "locov_caption_embed_bwd: null pointer (no gradient given)");
    LOCOV_REQUIRE(layer_norm || !g_enc, "locov_caption_embed_bwd: g_enc without the LayerNorm path (sum the two gradients into g_in)");
    LOCOV_REQUIRE(workspace_bytes >= locov_caption_embed_bwd_workspace_bytes(N, H, layer_norm),
                  "locov_caption_embed_bwd: workspace of %lld bytes is too small", (long long)workspace_bytes);
    LOCOV_REQUIRE(((uintptr_t)workspace & 15) == 0, "locov_caption_embed_bwd: misaligned workspace");
    if (N > 0 && layer_norm) {
        LOCOV_REQUIRE(T >= 1 && N % T == 0, "locov_caption_embed_bwd: N = %d is not a multiple of T = %d", N, T);
        LOCOV_REQUIRE(W && Tt && gamma && mean && rstd, "locov_caption_embed_bwd: null pointer (the LayerNorm path needs W, Tt, gamma, mean, rstd)");
        if (keep) LOCOV_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "locov_caption_embed_bwd: p_drop must be in [0, 1)");
    }
    const hipStream_t s = as_stream(stream);
    int *sorted_ids = static_cast<int *>(workspace), *order = sorted_ids + N;
    const float *g = g_in;
    if (N > 0) {
        hipLaunchKernelGGL(caption_rank_kernel, dim3(1), dim3(kCapRankThreads), 0, s, ints, N, sorted_ids, order);
        if (layer_norm) {
            float *dx = reinterpret_cast<float *>(static_cast<char *>(workspace) + (((int64_t)2 * N * 4) + 15) / 16 * 16);
            const CaptionLn ln = {P, Tt, gamma, nullptr, keep, 0.f, keep ? 1.0f / (1.0f - p_drop) : 1.f};
            hipLaunchKernelGGL(caption_ln_bwd_kernel, dim3((unsigned)ceil_div(N, kCapThreads / kWave)), dim3(kCapThreads), 0, s, ints, N, T, H, W,
                               ln, mean, rstd, g_enc, g_in, dx);
            g = dx;
        }
    }
    const int64_t blocks = ceil_div(V, kCapThreads / kWave);
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096)), block(kCapThreads);
    if (H % 4 == 0 && cap_aligned16(g) && cap_aligned16(dW))
        hipLaunchKernelGGL(caption_scatter_kernel<4>, grid, block, 0, s, sorted_ids, order, N, V, H, g, dW);
    else
        hipLaunchKernelGGL(caption_scatter_kernel<1>, grid, block, 0, s, sorted_ids, order, N, V, H, g, dW);
    return check_launch("locov_caption_embed_bwd");
}

}  // extern "C"
