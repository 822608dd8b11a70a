// Fused multi-head self-attention core for short padded sequences (TransformerHead's BERT layers), fp32 in / fp32 out on the
// f32-input MFMA (v_mfma_f32_32x32x2_f32), forward and backward:
//
//     ctx = dropout(softmax(Q K^T * scale + bias[n, key])) V          per (sequence n, head h)
//
// Q, K, V, ctx are [Nseq * S, H * d] row matrices with a row pitch each (column blocks of one [Nseq * S, 3 H d] matrix, or
// separate tensors); bias [Nseq, S] is added per key; the dropout keep mask, where given, is uint8 [Nseq, H, S, S] drawn by the
// caller (no RNG here).  No S x S tensor is written: the forward keeps a running maximum and sum per query row (online softmax
// over 32-key tiles) and stores a log-sum-exp per (n, h, query); the backward recomputes the probabilities from it.
//
// One shape for all three kernels.  A workgroup is 2 waves; a wave owns 32 "resident" rows (queries in the forward and the dQ
// kernel, keys in the dK/dV kernel) whose operands stay in registers for the whole sweep, and the workgroup streams the other
// side through LDS in tiles of 32 rows.  The products are oriented so that the resident row is the MFMA column = the lane
// (lane & 31) and the 32 streamed rows of the tile are the 16 accumulator registers of the two lane halves:
//   T[streamed][resident] = Y X^T      A operand = the LDS tile Y (one 16-byte LDS read per 4 MFMAs), B = the registers X
//   acc^T[dd][resident] += Y^T E       A operand = the LDS tile read by columns, B = the tile E just made, register t as it is
// (k step t of the second product takes streamed rows crow(t, 0) and crow(t, 1), which is exactly what register t of the two lane
// halves holds, so a score tile feeds the next product with no lane movement and no LDS).  The row statistics of the softmax are
// then per lane: 16 registers and one exchange with lane ^ 32 -- every lane works (no serial-lane softmax).
//
// Backward = two launches, no atomics, every sum in a fixed order (bitwise reproducible): the dQ kernel (resident queries) and the
// dK/dV kernel (resident keys), each recomputing S and dP.  delta = sum_k P dP of a query row is formed by a first sweep of the dQ
// kernel from the very products the second sweep and the next launch recompute bit for bit -- not as rowsum(dO * O), which rounds
// differently: where one key holds all of a row's weight, dP - delta must cancel to exactly 0, as it does in softmax's backward.
//
// Built with -ffp-contract=off (locov_amd/build.py): dP * keep / (1 - p) is rounded before delta is taken from it, so the two cancel
// exactly where they must; the multiply-adds that may fuse say fmaf().
//
// Budget (hipcc -O3, gfx950; DESIGN.md has the table): LDS 2 x 32 x (d + 4) x 4 B + <= 256 B = 25.1 KB at d = 96; registers: the
// dK/dV kernel at d = 128 is the largest (K, V, dK, dV resident: 4 x 64, plus two 16-register tiles).
#include "common.h"

namespace locov {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;                 // rows of one MFMA tile: resident rows per wave, streamed rows per LDS stage
constexpr int kMhaWaves = 2;
constexpr int kMhaThreads = kMhaWaves * kWave;
constexpr int kBlockRows = kMhaWaves * kTile;
constexpr int kPad = 4;                   // LDS row padding in floats (keeps rows 16-byte aligned)

// row of a 32x32 accumulator tile held by register r of lane half hi
__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// x[4u + j] = row[8u + 4hi + j]: the k order both operands of T = Y X^T use (any order serves, as long as they agree)
template <int D>
__device__ __forceinline__ void load_resident(const float *__restrict__ row, bool valid, int hi, float (&x)[D / 2])
{
#pragma unroll
    for (int u = 0; u < D / 8; ++u) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) v = *reinterpret_cast<const float4 *>(row + 8 * u + 4 * hi);
        x[4 * u + 0] = v.x; x[4 * u + 1] = v.y; x[4 * u + 2] = v.z; x[4 * u + 3] = v.w;
    }
}

// rows [t0, t0 + 32) of one (sequence, head) into an LDS tile, zeros past the sequence's end
template <int D>
__device__ __forceinline__ void stage_tile(const float *__restrict__ base, int64_t ld, int t0, int S, float (*y)[D + kPad])
{
    for (int idx = threadIdx.x; idx < kTile * (D / 4); idx += kMhaThreads) {
        const int r = idx / (D / 4), c4 = idx % (D / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 + r < S) v = *reinterpret_cast<const float4 *>(base + (int64_t)(t0 + r) * ld + 4 * c4);
        *reinterpret_cast<float4 *>(&y[r][4 * c4]) = v;
    }
}

// T[streamed][resident] = Y X^T
template <int D>
__device__ __forceinline__ f32x16 tile_product(const float (*y)[D + kPad], const float (&x)[D / 2], int c, int hi)
{
    f32x16 acc = {0};
#pragma unroll
    for (int u = 0; u < D / 8; ++u) {
        const float4 a = *reinterpret_cast<const float4 *>(&y[c][8 * u + 4 * hi]);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, x[4 * u + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, x[4 * u + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, x[4 * u + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, x[4 * u + 3], acc, 0, 0, 0);
    }
    return acc;
}

// acc^T[dd][resident] += sum over the tile's streamed rows of Y[row][dd] * E[row][resident]
template <int D>
__device__ __forceinline__ void tile_accumulate(const float (*y)[D + kPad], const f32x16 &e, int c, int hi, f32x16 (&acc)[D / 32])
{
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int row = crow(t, hi);
#pragma unroll
        for (int b = 0; b < D / 32; ++b)
            acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(y[row][32 * b + c], e[t], acc[b], 0, 0, 0);
    }
}

// acc^T[dd][resident] (times mul) -> out row of the resident: registers 4g .. 4g + 3 are columns 32b + 8g + 4hi + (0..3)
template <int D>
__device__ __forceinline__ void store_resident(float *__restrict__ row, int hi, const f32x16 (&acc)[D / 32], float mul)
{
#pragma unroll
    for (int b = 0; b < D / 32; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4 *>(row + 32 * b + 8 * g + 4 * hi) =
                make_float4(acc[b][4 * g] * mul, acc[b][4 * g + 1] * mul, acc[b][4 * g + 2] * mul, acc[b][4 * g + 3] * mul);
}

template <int D>
__global__ __launch_bounds__(kMhaThreads) void mha_fwd_kernel(const float *__restrict__ q, int64_t ldq, const float *__restrict__ k,
                                                               int64_t ldk, const float *__restrict__ v, int64_t ldv,
                                                               const float *__restrict__ bias, const uint8_t *__restrict__ keep,
                                                               float inv_keep, float scale, int S, int H, float *__restrict__ ctx,
                                                               int64_t ldo, float *__restrict__ lse)
{
    __shared__ __attribute__((aligned(16))) float yk[kTile][D + kPad];
    __shared__ __attribute__((aligned(16))) float yv[kTile][D + kPad];
    __shared__ float sbias[kTile];
    const int n = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int c = lane & 31, hi = lane >> 5;
    const int q0 = blockIdx.x * kBlockRows + wave * kTile;      // wave-uniform
    const int qrow = q0 + c;
    const bool valid_q = qrow < S;
    const int64_t row0 = (int64_t)n * S;
    const int64_t nh = (int64_t)n * H + h;

    float xq[D / 2];
    load_resident<D>(q + (row0 + qrow) * ldq + h * D, valid_q, hi, xq);
    f32x16 o[D / 32];
#pragma unroll
    for (int b = 0; b < D / 32; ++b) o[b] = f32x16{0};
    float m = -INFINITY, l = 0.f;                                // l: this lane half's share of the row sum

    for (int t0 = 0; t0 < S; t0 += kTile) {
        __syncthreads();                                         // the previous tile has been read
        stage_tile<D>(k + row0 * ldk + h * D, ldk, t0, S, yk);
        stage_tile<D>(v + row0 * ldv + h * D, ldv, t0, S, yv);
        if (threadIdx.x < kTile) sbias[threadIdx.x] = t0 + (int)threadIdx.x < S ? bias[row0 + t0 + threadIdx.x] : 0.f;
        __syncthreads();
        if (q0 >= S) continue;                                   // (a wave past the end only helps to stage)
        f32x16 s = tile_product<D>(yk, xq, c, hi);
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = crow(r, hi);
            s[r] = t0 + kk < S ? fmaf(s[r], scale, sbias[kk]) : -INFINITY;
            tmax = fmaxf(tmax, s[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float m_new = fmaxf(m, tmax);                      // finite: key t0 exists and the bias is finite
        const float alpha = expf(m - m_new);                     // (0 on the first tile)
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = expf(s[r] - m_new);
            sum += s[r];
        }
        l = fmaf(l, alpha, sum);
        m = m_new;
#pragma unroll
        for (int b = 0; b < D / 32; ++b) o[b] *= alpha;
        if (keep != nullptr) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = t0 + crow(r, hi);
                const bool on = valid_q && key < S && keep[(nh * S + qrow) * S + key] != 0;
                s[r] = on ? s[r] * inv_keep : 0.f;
            }
        }
        tile_accumulate<D>(yv, s, c, hi, o);
    }
    if (!valid_q) return;
    const float lsum = l + __shfl_xor(l, 32);
    store_resident<D>(ctx + (row0 + qrow) * ldo + h * D, hi, o, 1.f / lsum);
    if (hi == 0) lse[nh * S + qrow] = m + logf(lsum);
}

// KV = false: resident queries, X1 = Q, X2 = dO, streamed Y1 = K, Y2 = V; writes dQ and delta.
// KV = true : resident keys,    X1 = K, X2 = V,  streamed Y1 = Q, Y2 = dO; reads delta, writes dK and dV.
template <int D, bool KV>
__global__ __launch_bounds__(kMhaThreads) void mha_bwd_kernel(const float *__restrict__ q, int64_t ldq, const float *__restrict__ k,
                                                               int64_t ldk, const float *__restrict__ v, int64_t ldv,
                                                               const float *__restrict__ bias, const uint8_t *__restrict__ keep,
                                                               float inv_keep, float scale, int S, int H,
                                                               const float *__restrict__ dctx,
                                                               int64_t ldo, const float *__restrict__ lse, float *__restrict__ delta,
                                                               float *__restrict__ dq, int64_t lddq, float *__restrict__ dk,
                                                               int64_t lddk, float *__restrict__ dv, int64_t lddv)
{
    __shared__ __attribute__((aligned(16))) float y1[kTile][D + kPad];
    __shared__ __attribute__((aligned(16))) float y2[kTile][D + kPad];
    __shared__ float sa[kTile], sb[kTile];                      // per streamed row: bias (dQ kernel) | lse and delta (dK/dV kernel)
    const int n = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int c = lane & 31, hi = lane >> 5;
    const int r0 = blockIdx.x * kBlockRows + wave * kTile;      // wave-uniform
    const int res = r0 + c;
    const bool valid_res = res < S;
    const int64_t row0 = (int64_t)n * S;
    const int64_t nh = (int64_t)n * H + h;

    const float *x1p = KV ? k + (row0 + res) * ldk + h * D : q + (row0 + res) * ldq + h * D;
    const float *x2p = KV ? v + (row0 + res) * ldv + h * D : dctx + (row0 + res) * ldo + h * D;
    const float *y1p = KV ? q + row0 * ldq + h * D : k + row0 * ldk + h * D;
    const float *y2p = KV ? dctx + row0 * ldo + h * D : v + row0 * ldv + h * D;
    const int64_t ld1 = KV ? ldq : ldk, ld2 = KV ? ldo : ldv;

    float x1[D / 2], x2[D / 2];
    load_resident<D>(x1p, valid_res, hi, x1);
    load_resident<D>(x2p, valid_res, hi, x2);
    float ca = 0.f, cb = 0.f;                                    // per resident row: lse and delta (dQ kernel) | bias (dK/dV kernel)
    if (valid_res) ca = KV ? bias[row0 + res] : lse[nh * S + res];

    // one tile's probabilities and the gradient with respect to them, [streamed][resident]; the same instructions wherever called
    auto tile_terms = [&](int t0, f32x16 &pd, f32x16 &dpf, f32x16 &kpv) {
        const f32x16 s = tile_product<D>(y1, x1, c, hi);         // scores
        const f32x16 dp = tile_product<D>(y2, x2, c, hi);        // dO V^T
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = crow(r, hi);
            const int str = t0 + kk;
            const bool valid = valid_res && str < S;
            const float arg = KV ? fmaf(s[r], scale, ca) - sa[kk] : fmaf(s[r], scale, sa[kk]) - ca;
            const float p = valid ? expf(arg) : 0.f;
            float kp = 1.f;
            if (keep != nullptr) {
                const int64_t at = KV ? (nh * S + str) * S + res : (nh * S + res) * S + str;
                kp = (valid && keep[at] != 0) ? inv_keep : 0.f;
            }
            pd[r] = p;                                           // undropped probability
            kpv[r] = kp;
            dpf[r] = dp[r] * kp;                                 // gradient w.r.t. it, rounded (this file is built with contraction off)
        }
    };
    auto stage = [&](int t0) {
        __syncthreads();
        stage_tile<D>(y1p, ld1, t0, S, y1);
        stage_tile<D>(y2p, ld2, t0, S, y2);
        if (threadIdx.x < kTile) {
            const int row = t0 + threadIdx.x;
            const bool ok = row < S;
            if (KV) {
                sa[threadIdx.x] = ok ? lse[nh * S + row] : 0.f;
                sb[threadIdx.x] = ok ? delta[nh * S + row] : 0.f;
            } else {
                sa[threadIdx.x] = ok ? bias[row0 + row] : 0.f;
            }
        }
        __syncthreads();
    };

    if constexpr (!KV) {                                         // first sweep: delta = sum_k P dP
        float part = 0.f;
        for (int t0 = 0; t0 < S; t0 += kTile) {
            stage(t0);
            if (r0 >= S) continue;
            f32x16 p, dpf, kpv;
            tile_terms(t0, p, dpf, kpv);
#pragma unroll
            for (int r = 0; r < 16; ++r) part += p[r] * dpf[r];
        }
        cb = part + __shfl_xor(part, 32);
        if (valid_res && hi == 0) delta[nh * S + res] = cb;
    }
    f32x16 acc1[D / 32], acc2[KV ? D / 32 : 1];
#pragma unroll
    for (int b = 0; b < D / 32; ++b) acc1[b] = f32x16{0};
    if constexpr (KV) {
#pragma unroll
        for (int b = 0; b < D / 32; ++b) acc2[b] = f32x16{0};
    }

    for (int t0 = 0; t0 < S; t0 += kTile) {
        stage(t0);
        if (r0 >= S) continue;
        f32x16 p, dpf, kpv, ds;
        tile_terms(t0, p, dpf, kpv);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float dl = KV ? sb[crow(r, hi)] : cb;
            ds[r] = p[r] * (dpf[r] - dl) * scale;
        }
        tile_accumulate<D>(y1, ds, c, hi, acc1);                 // dQ^T += K^T dS | dK^T += Q^T dS
        if constexpr (KV) {
            const f32x16 pd = p * kpv;                           // the dropped probabilities: P * keep / (1 - p_drop)
            tile_accumulate<D>(y2, pd, c, hi, acc2);             // dV^T += dO^T P
        }
    }
    if (!valid_res) return;
    if constexpr (KV) {
        store_resident<D>(dk + (row0 + res) * lddk + h * D, hi, acc1, 1.f);
        store_resident<D>(dv + (row0 + res) * lddv + h * D, hi, acc2, 1.f);
    } else {
        store_resident<D>(dq + (row0 + res) * lddq + h * D, hi, acc1, 1.f);
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks both entry points share; nothing here touches the device
int check_common(const char *fn, int nseq, int S, int H, int d, const void *keep, float p_drop)
{
    if (d != 32 && d != 64 && d != 96 && d != 128)
        return set_error(LOCOV_ERR_UNSUPPORTED, "%s: head dim d must be 32, 64, 96 or 128 (got %d)", fn, d);
    if (S < 1 || S > LOCOV_MHA_MAX_S)
        return set_error(LOCOV_ERR_UNSUPPORTED, "%s: sequence length S must be in [1, %d] (got %d)", fn, LOCOV_MHA_MAX_S, S);
    if (nseq < 1 || nseq > LOCOV_MHA_MAX_GRID || H < 1 || H > LOCOV_MHA_MAX_GRID)
        return set_error(LOCOV_ERR_UNSUPPORTED, "%s: Nseq and H must be in [1, %d] (got Nseq=%d H=%d)", fn, LOCOV_MHA_MAX_GRID, nseq, H);
    if (keep != nullptr && !(p_drop >= 0.f && p_drop < 1.f))
        return set_error(LOCOV_ERR_INVALID_ARG, "%s: p_drop must be in [0, 1) with a keep mask (got %g)", fn, (double)p_drop);
    return LOCOV_OK;
}

int check_rows(const char *fn, const char *name, const void *p, int64_t ld, int H, int d)
{
    if (p == nullptr) return set_error(LOCOV_ERR_INVALID_ARG, "%s: null pointer %s", fn, name);
    if (!aligned16(p)) return set_error(LOCOV_ERR_INVALID_ARG, "%s: %s is not 16-byte aligned", fn, name);
    if (ld % 4 != 0 || ld < (int64_t)H * d)
        return set_error(LOCOV_ERR_INVALID_ARG, "%s: pitch of %s must be a multiple of 4 floats and >= H*d = %lld (got %lld)", fn, name,
                         (long long)H * d, (long long)ld);
    return LOCOV_OK;
}

#define MHA_CHECK(expr)            \
    do {                           \
        const int rc_ = (expr);    \
        if (rc_ != LOCOV_OK) return rc_; \
    } while (0)

template <int D>
int launch_fwd(dim3 grid, hipStream_t st, const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv,
               const float *bias, const uint8_t *keep, float inv_keep, float scale, int S, int H, float *ctx, int64_t ldo, float *lse)
{
    hipLaunchKernelGGL(mha_fwd_kernel<D>, grid, dim3(kMhaThreads), 0, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, ctx,
                       ldo, lse);
    return check_launch("locov_mha_fwd");
}

template <int D>
int launch_bwd(dim3 grid, hipStream_t st, const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv,
               const float *bias, const uint8_t *keep, float inv_keep, float scale, int S, int H, const float *dctx,
               int64_t ldo, const float *lse, float *delta, float *dq, int64_t lddq, float *dk, int64_t lddk, float *dv, int64_t lddv)
{
    hipLaunchKernelGGL((mha_bwd_kernel<D, false>), grid, dim3(kMhaThreads), 0, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S,
                       H, dctx, ldo, lse, delta, dq, lddq, dk, lddk, dv, lddv);
    MHA_CHECK(check_launch("locov_mha_bwd (dQ)"));
    hipLaunchKernelGGL((mha_bwd_kernel<D, true>), grid, dim3(kMhaThreads), 0, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S,
                       H, dctx, ldo, lse, delta, dq, lddq, dk, lddk, dv, lddv);
    return check_launch("locov_mha_bwd (dK, dV)");
}

}  // namespace
}  // namespace locov

using namespace locov;

extern "C" int locov_mha_fwd(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv, const float *bias,
                             const uint8_t *keep, float p_drop, float scale, int nseq, int S, int H, int d, float *ctx, int64_t ldo,
                             float *lse, locov_stream_t stream)
{
    const char *fn = "locov_mha_fwd";
    MHA_CHECK(check_common(fn, nseq, S, H, d, keep, p_drop));
    MHA_CHECK(check_rows(fn, "q", q, ldq, H, d));
    MHA_CHECK(check_rows(fn, "k", k, ldk, H, d));
    MHA_CHECK(check_rows(fn, "v", v, ldv, H, d));
    MHA_CHECK(check_rows(fn, "ctx", ctx, ldo, H, d));
    LOCOV_REQUIRE(bias && lse, "locov_mha_fwd: null pointer bias / lse");
    const float inv_keep = keep ? 1.f / (1.f - p_drop) : 1.f;
    const dim3 grid((unsigned)ceil_div(S, kBlockRows), (unsigned)H, (unsigned)nseq);
    const hipStream_t st = as_stream(stream);
    switch (d) {
    case 32: return launch_fwd<32>(grid, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, ctx, ldo, lse);
    case 64: return launch_fwd<64>(grid, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, ctx, ldo, lse);
    case 96: return launch_fwd<96>(grid, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, ctx, ldo, lse);
    default: return launch_fwd<128>(grid, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, ctx, ldo, lse);
    }
}

extern "C" int locov_mha_bwd(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv, const float *bias,
                             const uint8_t *keep, float p_drop, float scale, int nseq, int S, int H, int d,
                             const float *dctx, int64_t ldo, const float *lse, float *delta, float *dq, int64_t lddq, float *dk,
                             int64_t lddk, float *dv, int64_t lddv, locov_stream_t stream)
{
    const char *fn = "locov_mha_bwd";
    MHA_CHECK(check_common(fn, nseq, S, H, d, keep, p_drop));
    MHA_CHECK(check_rows(fn, "q", q, ldq, H, d));
    MHA_CHECK(check_rows(fn, "k", k, ldk, H, d));
    MHA_CHECK(check_rows(fn, "v", v, ldv, H, d));
    MHA_CHECK(check_rows(fn, "dctx", dctx, ldo, H, d));
    MHA_CHECK(check_rows(fn, "dq", dq, lddq, H, d));
    MHA_CHECK(check_rows(fn, "dk", dk, lddk, H, d));
    MHA_CHECK(check_rows(fn, "dv", dv, lddv, H, d));
    LOCOV_REQUIRE(bias && lse && delta, "locov_mha_bwd: null pointer bias / lse / delta");
    const float inv_keep = keep ? 1.f / (1.f - p_drop) : 1.f;
    const dim3 grid((unsigned)ceil_div(S, kBlockRows), (unsigned)H, (unsigned)nseq);
    const hipStream_t st = as_stream(stream);
    switch (d) {
    case 32: return launch_bwd<32>(grid, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, dctx, ldo, lse, delta, dq,
                                   lddq, dk, lddk, dv, lddv);
    case 64: return launch_bwd<64>(grid, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, dctx, ldo, lse, delta, dq,
                                   lddq, dk, lddk, dv, lddv);
    case 96: return launch_bwd<96>(grid, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, dctx, ldo, lse, delta, dq,
                                   lddq, dk, lddk, dv, lddv);
    default: return launch_bwd<128>(grid, st, q, ldq, k, ldk, v, ldv, bias, keep, inv_keep, scale, S, H, dctx, ldo, lse, delta, dq,
                                    lddq, dk, lddk, dv, lddv);
    }
}
