// LSM grounding branches: assembly of the `input_image` / `input_boxes` region dictionaries.
//
// Replaces the host loops of ovr/modeling/meta_arch/distill_prop_mmss_gcnn.py:273-328 (whole-image grid: valid-extent mask,
// normalised cell centres, SPATIAL_DROPOUT random valid cells per image, one fancy-index per image, pad_sequence, three
// torch.tensor(numpy).cuda() copies) and :348-399 (sampled boxes: min(len) random rows per image, box centres over the image
// size, masks) with one selection launch and one gather launch per branch, and one scatter launch per branch backward.
//
//   regions_select_kernel   one workgroup per image.  The image's keys go to LDS (a candidate that is outside the valid extent
//                           gets +inf); every valid candidate counts the valid candidates with a smaller (key, index) pair --
//                           its rank, i.e. the slot a stable argsort of the keys gives it.  <= kMaxCandidates candidates per
//                           image (LOCOV_REGIONS_MAX_CANDIDATES = 4 096 keys = 32 KB of LDS as float64; the LSM grid has 1 050, a
//                           sampled image <= 512): more is an error of the entry point, never a truncation.  Writes slot ->
//                           candidate (`indices`, per image, -1 = padding; `src_row`, the same as a row of the source matrix),
//                           candidate -> output row (`inv`, -1 = not selected), the uint8 mask, the loc rows and the zero mvm_mask.
//   regions_gather_kernel   one wave per output row: 64 lanes x 16 bytes per pass over the C floats of a contiguous source row
//                           (channels-last grid, box features); lanes over channels with stride gh*gw when the grid tensor is
//                           NCHW-contiguous.  Padding rows are written as zeros by the same launch.
//   regions_scatter_*       backward: every row (ROWS) / element (NCHW) of the source-shaped gradient is written exactly once,
//                           the selected slot's gradient or zero, through `inv`: no memset, no atomic, reproducible bits.
//
// The quotients of region_loc are IEEE fp32 divisions (__fdiv_rn; hipcc's default keeps fp32 division correctly rounded and
// build.py passes no fast-math flag): they must equal what numpy / torch form on the host.
#include "common.h"

#include <cmath>

namespace locov {

constexpr int kRegThreads = 256;
constexpr int kMaxCandidates = LOCOV_REGIONS_MAX_CANDIDATES;

#ifdef LOCOV_REGIONS_DEBUG      // -DLOCOV_REGIONS_DEBUG: index asserts inside the kernels
#include <cassert>
#define REG_ASSERT(c) assert(c)
#else
#define REG_ASSERT(c)
#endif

// per-image launch arguments, by value (B <= LOCOV_REGIONS_MAX_B)
struct RegionImages {
    int count[LOCOV_REGIONS_MAX_B];        // candidates: gh*gw | Ri
    int offset[LOCOV_REGIONS_MAX_B];       // first candidate's row in keys / inv / the source matrix
    int ext_a[LOCOV_REGIONS_MAX_B];        // grid: valid rows gh_i   | boxes: image height
    int ext_b[LOCOV_REGIONS_MAX_B];        // grid: valid columns gw_i | boxes: image width
    const float *boxes[LOCOV_REGIONS_MAX_B];   // boxes: [Ri, 4] (x0, y0, x1, y1)
};

__device__ __forceinline__ bool grid_valid(int c, int gw, int vh, int vw) { return c / gw < vh && c % gw < vw; }

// :293-296 ((k + 0.5) / g_i of the cell) | :368-383 (box centre / image size)
__device__ __forceinline__ float2 region_loc(const RegionImages &im, int i, int c, int mode, int gw)
{
    if (mode == LOCOV_REGIONS_BOXES) {
        const float4 b = reinterpret_cast<const float4 *>(im.boxes[i])[c];
        return make_float2(__fdiv_rn((b.x + b.z) * 0.5f, (float)im.ext_b[i]), __fdiv_rn((b.y + b.w) * 0.5f, (float)im.ext_a[i]));
    }
    return make_float2(__fdiv_rn((float)(c % gw) + 0.5f, (float)im.ext_b[i]), __fdiv_rn((float)(c / gw) + 0.5f, (float)im.ext_a[i]));
}

__global__ __launch_bounds__(kRegThreads) void regions_select_kernel(
    const double *__restrict__ keys, int mode, RegionImages im, int gw, int n, int limit, int mask_w, int mvm_w,
    int64_t *__restrict__ indices, int *__restrict__ src_row, int *__restrict__ inv, uint8_t *__restrict__ mask,
    float *__restrict__ loc, float *__restrict__ mvm)
{
    __shared__ double skey[kMaxCandidates];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int count = im.count[i], off = im.offset[i];
    const int vh = im.ext_a[i], vw = im.ext_b[i];

    for (int r = tid; r < mvm_w; r += kRegThreads) mvm[(int64_t)i * mvm_w + r] = 0.f;

    if (mode == LOCOV_REGIONS_GRID_ALL) {
        // :302 not taken: every cell is a slot, mask = the valid extent, loc = 0 outside it
        for (int c = tid; c < count; c += kRegThreads) {
            const bool v = grid_valid(c, gw, vh, vw);
            const float2 l = v ? region_loc(im, i, c, mode, gw) : make_float2(0.f, 0.f);
            mask[(int64_t)i * mask_w + c] = v ? 1 : 0;
            reinterpret_cast<float2 *>(loc)[(int64_t)i * n + c] = l;
        }
        return;
    }

    int valid = 0;
    if (mode == LOCOV_REGIONS_BOXES) {
        valid = count;
        for (int c = tid; c < count; c += kRegThreads) skey[c] = keys[off + c];
    } else {
        valid = min(vh, count / gw) * min(vw, gw);
        for (int c = tid; c < count; c += kRegThreads) skey[c] = grid_valid(c, gw, vh, vw) ? keys[off + c] : INFINITY;
    }
    const int take = min(min(limit, n), valid);
    // padding slots and the mask row
    for (int r = tid; r < n; r += kRegThreads) {
        if (r >= take) {
            indices[(int64_t)i * n + r] = -1;
            src_row[(int64_t)i * n + r] = -1;
            reinterpret_cast<float2 *>(loc)[(int64_t)i * n + r] = make_float2(0.f, 0.f);
        }
    }
    for (int r = tid; r < mask_w; r += kRegThreads) mask[(int64_t)i * mask_w + r] = r < take ? 1 : 0;
    __syncthreads();

    for (int c = tid; c < count; c += kRegThreads) {
        const double k = skey[c];
        int slot = -1;
        if (mode == LOCOV_REGIONS_BOXES || grid_valid(c, gw, vh, vw)) {
            int rank = 0;
            for (int o = 0; o < count; o++) {            // (every lane reads the same LDS word: a broadcast)
                const double ko = skey[o];
                rank += (ko < k || (ko == k && o < c)) ? 1 : 0;
            }
            if (rank < take) slot = rank;
        }
        inv[off + c] = slot < 0 ? -1 : i * n + slot;
        if (slot >= 0) {
            REG_ASSERT(slot < n && c < count);
            indices[(int64_t)i * n + slot] = c;
            src_row[(int64_t)i * n + slot] = off + c;
            reinterpret_cast<float2 *>(loc)[(int64_t)i * n + slot] = region_loc(im, i, c, mode, gw);
        }
    }
}

// One wave per output row.  ROWS: source row s at src + s * ld (VEC = 4: 16-byte lanes, C % 4 == 0 and aligned; VEC = 1 otherwise).
template <int VEC>
__global__ __launch_bounds__(kRegThreads) void regions_gather_rows_kernel(const float *__restrict__ src, int64_t ld, int64_t rows, int C,
                                                                         const int *__restrict__ src_row, float *__restrict__ out)
{
    const int64_t row = (int64_t)blockIdx.x * (kRegThreads / kWave) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int s = src_row[row];
    float *o = out + row * C;
    if (VEC == 4) {
        const float4 *p = s >= 0 ? reinterpret_cast<const float4 *>(src + (int64_t)s * ld) : nullptr;
        for (int c = lane; c < C / 4; c += kWave)
            reinterpret_cast<float4 *>(o)[c] = p ? p[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const float *p = s >= 0 ? src + (int64_t)s * ld : nullptr;
        for (int c = lane; c < C; c += kWave) o[c] = p ? p[c] : 0.f;
    }
}

// NCHW-contiguous source [B, C, hw]: output row (i, r) reads src[i, :, cell] with stride hw between channels.
__global__ __launch_bounds__(kRegThreads) void regions_gather_nchw_kernel(const float *__restrict__ src, int64_t rows, int n, int C, int64_t hw,
                                                                         const int *__restrict__ src_row, float *__restrict__ out)
{
    const int64_t row = (int64_t)blockIdx.x * (kRegThreads / kWave) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int s = src_row[row];                        // i * hw + cell
    float *o = out + row * C;
    if (s < 0) {
        for (int c = lane; c < C; c += kWave) o[c] = 0.f;
        return;
    }
    const int64_t i = row / n;
    REG_ASSERT(s >= i * hw && s < (i + 1) * hw);
    const float *p = src + i * C * hw + ((int64_t)s - i * hw);
    for (int c = lane; c < C; c += kWave) o[c] = p[(int64_t)c * hw];
}

// backward, ROWS: one wave per source row; the selected slot's gradient row or zeros
template <int VEC>
__global__ __launch_bounds__(kRegThreads) void regions_scatter_rows_kernel(const float *__restrict__ g, int64_t ld, int64_t rows, int C,
                                                                          const int *__restrict__ inv, float *__restrict__ out)
{
    const int64_t row = (int64_t)blockIdx.x * (kRegThreads / kWave) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int s = inv[row];
    float *o = out + row * ld;
    if (VEC == 4) {
        const float4 *p = s >= 0 ? reinterpret_cast<const float4 *>(g + (int64_t)s * C) : nullptr;
        for (int c = lane; c < C / 4; c += kWave)
            reinterpret_cast<float4 *>(o)[c] = p ? p[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const float *p = s >= 0 ? g + (int64_t)s * C : nullptr;
        for (int c = lane; c < C; c += kWave) o[c] = p ? p[c] : 0.f;
    }
}

// backward, NCHW: one lane per element of [B, C, hw], consecutive lanes on consecutive cells (coalesced stores)
__global__ __launch_bounds__(kRegThreads) void regions_scatter_nchw_kernel(const float *__restrict__ g, int64_t total, int C, int64_t hw,
                                                                          const int *__restrict__ inv, float *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * kRegThreads;
    for (int64_t e = (int64_t)blockIdx.x * kRegThreads + threadIdx.x; e < total; e += stride) {
        const int64_t plane = e / hw, cell = e - plane * hw;      // plane = i * C + c
        const int64_t i = plane / C, c = plane - i * C;
        const int s = inv[i * hw + cell];
        out[e] = s >= 0 ? g[(int64_t)s * C + c] : 0.f;
    }
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace locov

using namespace locov;

extern "C" {

int locov_regions_select(const double *keys, int mode, int B, const int *count_host, const int *ext_a_host, const int *ext_b_host,
                         int grid_w, const float *const *boxes_host, int n, int limit, int mask_w, int mvm_w, int64_t *indices,
                         int *src_row, int *inv, uint8_t *mask, float *loc, float *mvm, locov_stream_t stream)
{
    LOCOV_REQUIRE(mode == LOCOV_REGIONS_GRID || mode == LOCOV_REGIONS_GRID_ALL || mode == LOCOV_REGIONS_BOXES,
                  "locov_regions_select: unknown mode %d", mode);
    LOCOV_REQUIRE(B >= 1 && B <= LOCOV_REGIONS_MAX_B, "locov_regions_select: 1 <= B <= %d, got %d", LOCOV_REGIONS_MAX_B, B);
    LOCOV_REQUIRE(count_host && ext_a_host && ext_b_host, "locov_regions_select: null pointer (per-image host arrays)");
    LOCOV_REQUIRE(n >= 0 && limit >= 0 && mask_w >= 0 && mvm_w >= 0, "locov_regions_select: negative count (n=%d limit=%d mask_w=%d mvm_w=%d)",
                  n, limit, mask_w, mvm_w);
    const bool boxes = mode == LOCOV_REGIONS_BOXES;
    LOCOV_REQUIRE(boxes || grid_w >= 1, "locov_regions_select: grid_w must be >= 1, got %d", grid_w);
    LOCOV_REQUIRE(!boxes || boxes_host, "locov_regions_select: null pointer (boxes)");
    RegionImages im;
    int64_t total = 0;
    for (int i = 0; i < B; i++) {
        const int c = count_host[i];
        LOCOV_REQUIRE(c >= 0, "locov_regions_select: negative count: image %d has %d candidates", i, c);
        LOCOV_REQUIRE(ext_a_host[i] >= 0 && ext_b_host[i] >= 0, "locov_regions_select: negative count: image %d extent (%d, %d)", i,
                      ext_a_host[i], ext_b_host[i]);
        if (mode != LOCOV_REGIONS_GRID_ALL && c > LOCOV_REGIONS_MAX_CANDIDATES)
            return set_error(LOCOV_ERR_UNSUPPORTED, "locov_regions_select: image %d has %d candidates, over the LDS budget of %d keys", i, c,
                             LOCOV_REGIONS_MAX_CANDIDATES);
        if (boxes) {
            LOCOV_REQUIRE(c == 0 || boxes_host[i], "locov_regions_select: null pointer (boxes of image %d)", i);
            LOCOV_REQUIRE(c == 0 || aligned16(boxes_host[i]), "locov_regions_select: misaligned boxes of image %d", i);
            LOCOV_REQUIRE(c == 0 || (ext_a_host[i] > 0 && ext_b_host[i] > 0), "locov_regions_select: image %d has an empty image size", i);
            LOCOV_REQUIRE(n <= c, "locov_regions_select: n = %d exceeds the %d boxes of image %d", n, c, i);
        } else {
            LOCOV_REQUIRE(c % grid_w == 0, "locov_regions_select: %d cells is not a multiple of grid_w %d", c, grid_w);
            LOCOV_REQUIRE(ext_a_host[i] <= c / grid_w && ext_b_host[i] <= grid_w, "locov_regions_select: image %d extent (%d, %d) exceeds the grid", i,
                          ext_a_host[i], ext_b_host[i]);
        }
        im.count[i] = c;
        im.offset[i] = (int)total;
        im.ext_a[i] = ext_a_host[i];
        im.ext_b[i] = ext_b_host[i];
        im.boxes[i] = boxes ? boxes_host[i] : nullptr;
        total += c;
        LOCOV_REQUIRE(total < (int64_t)1 << 31, "locov_regions_select: too many candidates");
    }
    for (int i = B; i < LOCOV_REGIONS_MAX_B; i++) {
        im.count[i] = im.offset[i] = im.ext_a[i] = im.ext_b[i] = 0;
        im.boxes[i] = nullptr;
    }
    LOCOV_REQUIRE((int64_t)B * n < (int64_t)1 << 31, "locov_regions_select: B * n too large");
    if (mode == LOCOV_REGIONS_GRID_ALL) {
        for (int i = 0; i < B; i++)
            LOCOV_REQUIRE(im.count[i] == n && mask_w == n, "locov_regions_select: GRID_ALL needs n == mask_w == cells per image");
        LOCOV_REQUIRE(n == 0 || (mask && loc), "locov_regions_select: null pointer (outputs)");
    } else {
        LOCOV_REQUIRE(total == 0 || (keys && inv), "locov_regions_select: null pointer (keys / inv)");
        LOCOV_REQUIRE(n == 0 || (indices && src_row && loc), "locov_regions_select: null pointer (outputs)");
        LOCOV_REQUIRE(mask_w == 0 || mask, "locov_regions_select: null pointer (mask)");
    }
    LOCOV_REQUIRE(mvm_w == 0 || mvm, "locov_regions_select: null pointer (mvm_mask)");
    LOCOV_REQUIRE(loc == nullptr || ((uintptr_t)loc & 7) == 0, "locov_regions_select: misaligned loc");
    hipLaunchKernelGGL(regions_select_kernel, dim3((unsigned)B), dim3(kRegThreads), 0, as_stream(stream), keys, mode, im, boxes ? 1 : grid_w, n,
                       limit, mask_w, mvm_w, indices, src_row, inv, mask, loc, mvm);
    return check_launch("locov_regions_select");
}

static int check_gather(const char *what, int layout, int64_t ld, int64_t rows, int C, int64_t hw)
{
    LOCOV_REQUIRE(layout == LOCOV_REGIONS_ROWS || layout == LOCOV_REGIONS_NCHW, "%s: unknown layout %d", what, layout);
    LOCOV_REQUIRE(rows >= 0 && C >= 0, "%s: negative count (rows=%lld C=%d)", what, (long long)rows, C);
    LOCOV_REQUIRE(rows < (int64_t)1 << 31, "%s: too many rows", what);
    if (layout == LOCOV_REGIONS_ROWS)
        LOCOV_REQUIRE(ld >= C, "%s: ld %lld < C %d", what, (long long)ld, C);
    else
        LOCOV_REQUIRE(hw >= 1, "%s: hw must be >= 1", what);
    return LOCOV_OK;
}

int locov_regions_gather_fwd(const float *src, int layout, int64_t ld, int B, int n, int C, int64_t hw, const int *src_row, float *out,
                             locov_stream_t stream)
{
    LOCOV_REQUIRE(B >= 0 && n >= 0, "locov_regions_gather_fwd: negative count (B=%d n=%d)", B, n);
    const int64_t rows = (int64_t)B * n;
    int rc = check_gather("locov_regions_gather_fwd", layout, ld, rows, C, hw);
    if (rc) return rc;
    if (rows == 0 || C == 0) return LOCOV_OK;
    LOCOV_REQUIRE(src && src_row && out, "locov_regions_gather_fwd: null pointer");
    const dim3 grid((unsigned)ceil_div(rows, kRegThreads / kWave)), block(kRegThreads);
    if (layout == LOCOV_REGIONS_NCHW)
        hipLaunchKernelGGL(regions_gather_nchw_kernel, grid, block, 0, as_stream(stream), src, rows, n, C, hw, src_row, out);
    else if (C % 4 == 0 && ld % 4 == 0 && aligned16(src) && aligned16(out))
        hipLaunchKernelGGL(regions_gather_rows_kernel<4>, grid, block, 0, as_stream(stream), src, ld, rows, C, src_row, out);
    else
        hipLaunchKernelGGL(regions_gather_rows_kernel<1>, grid, block, 0, as_stream(stream), src, ld, rows, C, src_row, out);
    return check_launch("locov_regions_gather_fwd");
}

int locov_regions_gather_bwd(const float *grad_out, int layout, int64_t ld, int64_t rows, int C, int64_t hw, const int *inv,
                             float *grad_src, locov_stream_t stream)
{
    int rc = check_gather("locov_regions_gather_bwd", layout, ld, rows, C, hw);
    if (rc) return rc;
    if (rows == 0 || C == 0) return LOCOV_OK;
    LOCOV_REQUIRE(inv && grad_src, "locov_regions_gather_bwd: null pointer");      // (grad_out may be null when nothing was selected)
    if (layout == LOCOV_REGIONS_NCHW) {
        LOCOV_REQUIRE(rows % hw == 0, "locov_regions_gather_bwd: rows %lld is not a multiple of hw %lld", (long long)rows, (long long)hw);
        const int64_t total = rows * C;
        const int64_t blocks = ceil_div(total, kRegThreads);
        hipLaunchKernelGGL(regions_scatter_nchw_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(kRegThreads), 0,
                           as_stream(stream), grad_out, total, C, hw, inv, grad_src);
    } else {
        const dim3 grid((unsigned)ceil_div(rows, kRegThreads / kWave)), block(kRegThreads);
        if (C % 4 == 0 && ld % 4 == 0 && aligned16(grad_out) && aligned16(grad_src))
            hipLaunchKernelGGL(regions_scatter_rows_kernel<4>, grid, block, 0, as_stream(stream), grad_out, ld, rows, C, inv, grad_src);
        else
            hipLaunchKernelGGL(regions_scatter_rows_kernel<1>, grid, block, 0, as_stream(stream), grad_out, ld, rows, C, inv, grad_src);
    }
    return check_launch("locov_regions_gather_bwd");
}

}  // extern "C"
