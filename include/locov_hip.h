/*
 * locov_hip.h -- C ABI of the MI355X (gfx950) LSM ROI-head library, liblocov_hip.so.
 *
 * This is the drop-in boundary for LocOV's Localized-Semantic-Matching ROI-head hot
 * path.  LocOV itself is 100 % Python and reaches its kernels
 * through Detectron2 / torchvision / torch; every entry point below names the
 * reference interface (file:line under the LocOV tree) whose device arithmetic it
 * replaces.  The Python classes in locov_amd/ (same names, config keys and checkpoint
 * keys as the reference's) are the only callers; they bind these symbols with ctypes
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / HIP types in signatures.
 *   - Every pointer is a DEVICE pointer unless the parameter name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *     Calls only enqueue work on that stream: no allocation, no synchronisation, no
 *     hidden global state -> safe to capture in a hipGraph.  Exceptions, two: (1) the opt-in
 *     measurement aid locov_gemm_timing_* at the end of this header: a process-global,
 *     mutex-guarded list of HIP events, OFF by default, recording nothing while the launch
 *     stream is being captured; locov_gemm_timing_read() synchronises on those events.
 *     (2) locov_augment_images uploads its per-image table with a hipMemcpyAsync from PAGEABLE
 *     host memory: the runtime may make the host wait until `stream` has drained, and a captured
 *     copy node would keep a pointer to host memory that is freed when the call returns, so the
 *     call MUST NOT be captured (see its workspace note).  tests/stream_cases.py lists both.
 *   - Outputs are caller-allocated.  Tensors are dense row-major in the stated shape.
 *   - Return value: 0 on success, <0 on error (LOCOV_ERR_*); locov_last_error() returns
 *     a thread-local message for the last failing call on this thread.
 *   - Threading: re-entrant; one call stream per thread as with any HIP stream.
 */
#ifndef LOCOV_HIP_H
#define LOCOV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8: locov_detect_postprocess; later, additively: locov_grounding_ce_dist_fwd / _bwd, locov_distill_loss_fwd / _bwd,
 *    locov_detect_postprocess_wide (+ _workspace_bytes), locov_regions_select / _gather_fwd / _gather_bwd,
 *    locov_detect_postprocess_cs / _wide_cs (+ _workspace_bytes), locov_grounding_align_fwd / _bwd,
 *    locov_grounding_triplet_fwd / _bwd, locov_mha_fwd / _bwd, locov_rpn_proposals (+ _workspace_bytes),
 *    locov_rpn_label_anchors (+ _workspace_bytes), locov_rpn_sample_anchors, locov_rpn_loss (+ _workspace_bytes),
 *    locov_resnet_stem_fwd, locov_resnet_stem_fwd_sel, locov_resnet_stem_wgrad (+ _workspace_bytes),
 *    locov_preprocess_images, locov_detector_rescale, locov_sgd_step (+ _workspace_bytes),
 *    locov_coco_match (+ _workspace_bytes), locov_coco_accumulate, locov_lvis_match,
 *    locov_resize_flip_images, locov_resize_supported, locov_map_proposals,
 *    locov_augment_images (+ _workspace_bytes), locov_augment_supported, locov_proposal_recall */
#define LOCOV_ABI_VERSION 8

#define LOCOV_OK 0
#define LOCOV_ERR_INVALID_ARG (-1)
#define LOCOV_ERR_LAUNCH (-2)
#define LOCOV_ERR_UNSUPPORTED (-3)

/* element types for the mixed-precision entry points */
#define LOCOV_F32 0
#define LOCOV_BF16 1

/* row-normalisation modes (locov_rownorm_fwd) */
#define LOCOV_NORM_NONE 0
#define LOCOV_NORM_L2 1          /* normalize_vec   : logged_module.py:55-65 */
#define LOCOV_NORM_STANDARDIZE 2 /* standardize_vec : logged_module.py:68-72 */

/* epilogue flags of the GEMM entry points */
#define LOCOV_EPI_RELU 1u
/* locov_gemm_nt_f32_split*: x is ALREADY in the split layout of locov_split_f16x2_pack (written so by its producer),
 * scaled by x_scale: it is then staged by LDS DMA like W, with no conversion in the kernel */
#define LOCOV_GEMM_A_SPLIT 0x1000u
/* locov_gemm_nt_f32_split{,_segmean}: y is WRITTEN in the split layout of locov_split_f16x2_pack scaled by x_scale (the pre-split
 * x of the GEMM that consumes it: Res5 block outputs feed the next block's conv1, roi_emb_heads.py:217-245) / the residual
 * is READ from that layout (the same block output is the next block's identity shortcut).  hi + lo reproduces the fp32 value
 * to 2^-22 relative (exactly what the consuming GEMM's own split would keep); a finished value outside fp16's range raises the
 * range-guard word.  N and ldc must be multiples of 8. */
#define LOCOV_EPI_OUT_SPLIT 0x2000u
#define LOCOV_EPI_RES_SPLIT 0x4000u
#define LOCOV_SEGMEAN_RES_ROI_MAJOR 0x400u   /* locov_gemm_nt_f32_split_segmean: the residual rows are ROI-major */
/* locov_winograd_conv3x3_f32{,_split}: write the output rows ROI-major (row = roi * 49 + position) instead of
 * position-major (row = position * R + roi) -- the order locov_gemm_nt_f32_split_segmean consumes */
#define LOCOV_WINO_OUT_ROI_MAJOR 0x100u
/* ... and READ the input rows in that order */
#define LOCOV_WINO_IN_ROI_MAJOR 0x200u

typedef void *locov_stream_t;

int locov_abi_version(void);
const char *locov_last_error(void);

/* Kernel launches this library has enqueued in this process so far (every entry point checks its launches through one helper,
 * which counts them; an entry point that enqueues several kernels behind one check counts once per check).  A monotonic host-side
 * counter for diagnostics: locov_amd/sharding.GradientExchangeTrace places DistributedDataParallel's bucket-ready points on the
 * Res5 backward by it (ovr/engine/trainer.py:61-66), independent of what else shares the GPU. */
int64_t locov_launch_count(void);

/* Number of compute units / XCDs of the current device (for grid sizing in callers/bench). */
int locov_device_info(int *cu_count, int *wave_size, int *lds_bytes_per_cu);

/* ---------------------------------------------------------------------------------------
 * a-2  proposal -> FPN level assignment.
 * Replaces [D2-upstream] detectron2.modeling.poolers.assign_boxes_to_levels, reached from
 * ovr/modeling/roi_heads/roi_emb_heads.py:244 (self.pooler(features, boxes)) when the
 * pooler has >1 level.  boxes [R,4] XYXY fp32 -> levels [R] int64 in [0, max-min].
 * Bit-exact integer output (north_star).
 * ------------------------------------------------------------------------------------- */
int locov_level_assign(const float *boxes, int64_t R, int min_level, int max_level,
                       int canonical_box_size, int canonical_level, int64_t *levels,
                       locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-1  ROIAlign forward / backward, NCHW fp32 -- the stand-alone pooler contract.
 * Replaces [D2-upstream] ROIPooler -> ROIAlign -> torchvision.ops.roi_align, call site
 * ovr/modeling/roi_heads/roi_emb_heads.py:243-245 (_shared_roi_transform), pooler built
 * at :182-187 (output_size=14, scales=(1/16,), sampling_ratio=0, "ROIAlignV2").
 *   feat [N,C,H,W]; rois [R,5] = (batch_idx, x0, y0, x1, y1); out [R,C,pooled_h,pooled_w].
 *   sampling_ratio <= 0 -> adaptive ceil(roi/pooled) grid.  aligned != 0 -> ROIAlignV2.
 * Backward accumulates into grad_feat [N,C,H,W] (caller zeroes it) with fp32 atomics.
 * ------------------------------------------------------------------------------------- */
int locov_roi_align_fwd(const float *feat, int N, int C, int H, int W, const float *rois,
                        int64_t R, int pooled_h, int pooled_w, float spatial_scale,
                        int sampling_ratio, int aligned, float *out, locov_stream_t stream);

int locov_roi_align_bwd(const float *grad_out, int N, int C, int H, int W, const float *rois,
                        int64_t R, int pooled_h, int pooled_w, float spatial_scale,
                        int sampling_ratio, int aligned, float *grad_feat,
                        locov_stream_t stream);

/* Multi-level pooler in ONE launch: ROI r samples level levels[r] (output of
 * locov_level_assign).  Host arrays describe up to LOCOV_MAX_LEVELS feature maps that
 * share N and C.  Replaces the per-level nonzero / index_put_ loop of ROIPooler.forward. */
#define LOCOV_MAX_LEVELS 8
int locov_roi_align_levels_fwd(const float *const *feats_host, const int *H_host,
                               const int *W_host, const float *scales_host, int num_levels,
                               int N, int C, const float *rois, const int64_t *levels,
                               int64_t R, int pooled_h, int pooled_w, int sampling_ratio,
                               int aligned, float *out, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * MI355X-native layout path: channels-last feature map, channels on the
 * lanes, coalesced 16-byte gathers.
 *   locov_nchw_to_nhwc : [N,C,H,W] f32 -> [N,H,W,C] (f32 or bf16)
 *   locov_roi_align_nhwc_fwd : feat [N,H,W,C] -> out [R, ceil(ph/bin_stride), ceil(pw/bin_stride), C]
 *     bin_stride = 1: every bin.  bin_stride = 2: only even bins (ph, pw even) -- exactly
 *     the positions the stride-2 1x1 convs of Res5 block 0 read (STRIDE_IN_1X1=True,
 *     roi_emb_heads.py:217-241), so downstream results are unchanged.
 * ------------------------------------------------------------------------------------- */
int locov_nchw_to_nhwc(const float *in, int N, int C, int H, int W, void *out, int out_dtype,
                       locov_stream_t stream);

/* The pooler contract at HBM speed: same result as locov_roi_align_fwd, bit for bit
 * (out [R,C,pooled_h,pooled_w] fp32), but gathering from a channels-last COPY of the map
 * (feat_nhwc [N,H,W,C] fp32 from locov_nchw_to_nhwc; 17 MB per 1333x800 image, written once per
 * call) and transposing in LDS, so that both the taps and the output are fully coalesced. */
int locov_roi_align_from_nhwc_fwd(const float *feat_nhwc, int N, int H, int W, int C,
                                  const float *rois, int64_t R, int pooled_h, int pooled_w,
                                  float spatial_scale, int sampling_ratio, int aligned, float *out,
                                  locov_stream_t stream);

/* The same with a choice of arithmetic (the pooler of roi_emb_heads.py:182-187,243-245):
 *   LOCOV_ROIALIGN_EXACT : the call above -- torchvision's per-sample order, un-fused: bit-identical to the CPU oracle.
 *   LOCOV_ROIALIGN_FAST  : within 1e-5 of it (SURVEY.md 8d's ROIAlign gate).  Separable form: per bin and axis the samples'
 *     bilinear weights are summed per PIXEL, so a bin costs (gh+1)(gw+1) taps instead of 4 gh gw; and the proposal's
 *     output bins are cut into regions whose pixel rectangle x 32 channels is staged in LDS once ("LDS-staged proposal
 *     tiles"; a small box is one region) so that every tap is an LDS read.  A plan kernel computes both per ROI into
 *     `workspace` (locov_roi_align_plan_bytes(R) bytes, 16-byte aligned; unused by the exact mode).  ROIs whose samples lie
 *     more than a pixel apart (a forced sampling_ratio on a large box), whose grid exceeds 5 samples per axis, or pooled
 *     sizes above 16 take the exact arithmetic inside the same launch. */
#define LOCOV_ROIALIGN_EXACT 0
#define LOCOV_ROIALIGN_FAST 1
int64_t locov_roi_align_plan_bytes(int64_t R);
int locov_roi_align_from_nhwc_fwd_ex(const float *feat_nhwc, int N, int H, int W, int C,
                                     const float *rois, int64_t R, int pooled_h, int pooled_w,
                                     float spatial_scale, int sampling_ratio, int aligned, int mode,
                                     void *workspace, int64_t workspace_bytes, float *out,
                                     locov_stream_t stream);

int locov_roi_align_nhwc_fwd(const void *feat, int feat_dtype, int N, int H, int W, int C,
                             const float *rois, int64_t R, int pooled_h, int pooled_w,
                             float spatial_scale, int sampling_ratio, int aligned,
                             int bin_stride, int pos_major, void *out, int out_dtype,
                             locov_stream_t stream);

/* Same, with out_ld elements between consecutive output pixel rows (>= C): lets the rows be a
 * column block of a wider matrix (Res5 block 0 reads [conv2 output | pooled input] as one
 * K-concatenated GEMM operand). */
int locov_roi_align_nhwc_ld_fwd(const void *feat, int feat_dtype, int N, int H, int W, int C,
                                const float *rois, int64_t R, int pooled_h, int pooled_w,
                                float spatial_scale, int sampling_ratio, int aligned,
                                int bin_stride, int pos_major, void *out, int64_t out_ld,
                                int out_dtype, locov_stream_t stream);

/* Same again, for pooling a map that already went through a 1x1 convolution.  ROIAlign is linear, so
 * W . ROIAlign(F) == ROIAlign(W . F): Res5 block 0's conv1 and projection shortcut (both 1x1, stride 2 ==
 * the even bins; roi_emb_heads.py:217-241) are applied to the res4 MAP -- once per pixel instead of once
 * per ROI bin, 12x fewer rows at 1000 proposals per image -- and pooled here.
 *   feat_ld : elements between consecutive pixels of feat (>= C; the C channels pooled by this call may be
 *             a column block of a wider per-pixel vector, e.g. [conv1 | shortcut] outputs)
 *   ch_scale, ch_shift [C] (either may be null), relu: per-channel affine (FrozenBN) + ReLU applied to the
 *             pooled value, i.e. AFTER the pooling, exactly where the reference applies them.  A proposal whose image
 *             index is outside [0, N) pools to zero and then gets the affine and the ReLU like any other row. */
int locov_roi_align_nhwc_affine_fwd(const void *feat, int feat_dtype, int N, int H, int W, int C,
                                    int64_t feat_ld, const float *rois, int64_t R, int pooled_h,
                                    int pooled_w, float spatial_scale, int sampling_ratio,
                                    int aligned, int bin_stride, int pos_major,
                                    const float *ch_scale, const float *ch_shift, int relu,
                                    void *out, int64_t out_ld, int out_dtype,
                                    locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-4  spatial mean.  Replaces box_features.mean(dim=[2,3])
 * (roi_emb_heads.py:262,344,356).  x [R,C,HW] -> out [R,C].
 * channels_last == 1: x is [R,HW,C] (ROI-major pixel rows); == 2: x is [HW,R,C] (position-major).
 * ------------------------------------------------------------------------------------- */
int locov_spatial_mean_fwd(const float *x, int64_t R, int C, int HW, int channels_last,
                           float *out, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-5 / a-6 / a-8  y[M,N] = epi(x[M,K] . W[N,K]^T), fp32 in / fp32 accumulate on the
 * f32 MFMA pipe (exact fp32 products, no TF32).  nn.Linear layout (weight [out,in]).
 * Replaces self.bbox_pred(x) (box_emb_head.py:196), self.emb_pred(x) (:206) and, in fp32
 * mode, self.cls_score(x) (:211).
 *   epi: v = acc * scale[n] (if scale) + shift[n] (if shift) + residual[m,n] (if residual);
 *        ReLU if (flags & LOCOV_EPI_RELU).     shift == bias for nn.Linear.
 *   lda / ldc: row strides (elements) of x and y (>= K / >= N); residual uses ldc.
 * ------------------------------------------------------------------------------------- */
int locov_gemm_nt_f32(const float *x, int64_t lda, const float *W, const float *scale,
                      const float *shift, const float *residual, float *y, int64_t ldc,
                      int64_t M, int N, int K, unsigned flags, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-3  Res5 stage building blocks on channels-last pixel matrices.
 * Replace [D2-upstream] BottleneckBlock's conv2d + FrozenBatchNorm2d + ReLU (+ residual add)
 * as built by roi_emb_heads.py:217-241 and applied at :245,:323.
 *   - 1x1 convolutions are locov_gemm_nt_f32 on x [R*H*W, Cin] (weight [N,Cin,1,1] == [N,Cin]).
 *   - locov_conv3x3_nhwc_f32: 3x3 / pad 1 / stride 1 as an implicit GEMM (K = 9*Cin) over R
 *     independent HxW tiles; w_packed [N, 9*Cin] comes from locov_pack_conv3x3_weight
 *     ([N,Cin,3,3] -> k = (ky*3+kx)*Cin + c).  Same epilogue as locov_gemm_nt_f32.
 *     Row order of x / y / residual: pos_major == 0 -> ROI-major  row = r*H*W + (y*W + x);
 *                                    pos_major != 0 -> POSITION-major row = (y*W + x)*R + r.
 *     Position-major is the fast layout: tap validity is then uniform per workgroup and the
 *     zero-padding taps are skipped instead of multiplied (18 % of a 7x7 tile's MACs).
 *   - locov_frozen_bn_fold: scale = weight*rsqrt(var+eps), shift = bias - mean*scale, the
 *     per-channel affine FrozenBatchNorm2d applies; feeds the GEMM epilogue's scale/shift.
 * ------------------------------------------------------------------------------------- */
int locov_conv3x3_nhwc_f32(const float *x, int64_t R, int H, int W, int Cin, int pos_major,
                           const float *w_packed, const float *scale, const float *shift,
                           const float *residual, float *y, int N, unsigned flags,
                           locov_stream_t stream);

int locov_pack_conv3x3_weight(const float *w, int N, int Cin, void *out, int out_dtype,
                              locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-3  The same 3x3 / pad 1 / stride 1 convolution (BottleneckBlock.conv2 + FrozenBN + ReLU,
 * roi_emb_heads.py:217-241 applied at :245,:323) on 7x7 POSITION-major tiles, evaluated in
 * the minimal-filtering (Winograd) domain: each row of 7 outputs is an F(4,3) | F(3,3) pair,
 * 121 products per (ROI, cin, cout) instead of 361 real taps -> 3x fewer MFMA FLOPs.
 *   U  = locov_winograd_pack_weight(w [N,Cin,3,3])  -> [121, N, Cin] fp32 (transform in fp64)
 *   y[(p*R + r), n] = relu?( conv(x)[..] * scale[n] + shift[n] ),  x rows [(p*R + r), Cin], p = y*7+x
 *   ldy: elements between consecutive rows of y (>= N; y may be a column block of a wider matrix)
 *   workspace: locov_winograd_workspace_bytes(R, Cin, N) bytes of device memory, 16-B aligned
 *   flags: 0 or LOCOV_EPI_RELU.  Cin % 32 == 0, N % 4 == 0.
 * fp32 throughout; differs from the direct form by rounding only (~5e-6 of the activation
 * range over the whole stage; the 1e-4 logits gate holds, tests/test_gpu_winograd.py).
 * locov_gemm_nt_batched_f32 is the batched NT GEMM it runs on: problem b uses
 * x + b*stride_x, W + b*stride_w ([N,K] rows of K), y + b*stride_y (elements).
 * ------------------------------------------------------------------------------------- */
int64_t locov_winograd_workspace_bytes(int64_t R, int Cin, int N);

int locov_winograd_pack_weight(const float *w, int N, int Cin, float *U, locov_stream_t stream);

int locov_winograd_conv3x3_f32(const float *x, int64_t R, int Cin, const float *U,
                               const float *scale, const float *shift, float *y, int64_t ldy,
                               int N, unsigned flags, void *workspace, int64_t workspace_bytes,
                               locov_stream_t stream);

/* The same convolution with the 121 transform-domain GEMMs in split-operand arithmetic (see
 * locov_gemm_nt_f32_split below): U_split = locov_split_f16x2_pack of the [121*N, Cin] matrix U with
 * w_scale = u_scale; the transformed input is scaled by v_scale before its split. */
int locov_winograd_conv3x3_f32_split(const float *x, int64_t R, int Cin, const void *U_split,
                                     float u_scale, float v_scale, const float *scale,
                                     const float *shift, float *y, int64_t ldy, int N, unsigned flags,
                                     void *workspace, int64_t workspace_bytes, unsigned *overflow,
                                     locov_stream_t stream);

int locov_gemm_nt_batched_f32(const float *x, int64_t lda, int64_t stride_x, const float *W,
                              int64_t stride_w, float *y, int64_t ldc, int64_t stride_y,
                              int64_t M, int N, int K, int batch, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * f-4  Multi-token class scoring of the grounding predictor.  Replaces the part of
 * GroundingModule.forward after its token_score Linear (box_emb_grounding_head.py:163-225:
 * per-class padding, masked softmax / hardmax over the tokens, attention-weighted distance).
 *   sim [R, Ttot]      raw token similarities = emb . token_bank^T (locov_gemm_nt_f32)
 *   tok_off [K1]       first column of class k in sim;  num_tok [K1] its real token count
 *                      (0 = no tokens: attention 0, score -0, like the reference's bg row)
 *   gmin [1]           device scalar: minimum of the reference's padded similarity tensor
 *   scores [R, K1] = -sum_t att_t * dist_t;   att [R, K1, Tmax] (may be null)
 *   cosine: dist = (1 - sim)/T with NaN similarities zeroed; else dist = -sim/T.  Tmax <= 32.
 * ------------------------------------------------------------------------------------- */
int locov_token_attention_fwd(const float *sim, int64_t R, int Ttot, const int *tok_off,
                              const int *num_tok, int K1, int Tmax, float temperature,
                              int cosine, int hardmax, const float *gmin, float *scores,
                              float *att, locov_stream_t stream);

/* The way back through the same lines under autograd (box_emb_grounding_head.py:152-183 with DETACH_CLASS_PREDICTOR off:
 * loss_cls reaches emb_pred's input through the masked softmax / hardmax and the attention-weighted distance).  The attention
 * is recomputed from sim and gmin; nothing else is saved by the forward.
 *   grad_scores [R, K1]       upstream gradient of scores
 *   grad_att [R, K1, Tmax]    upstream gradient of att, or null (the predictor drops the attention)
 *   grad_sim [R, Ttot]        written completely: class k owns the columns [tok_off[k], tok_off[k] + max(num_tok[k], 1)) and
 *                             the classes' ranges must partition [0, Ttot), so every element has exactly one writer (no atomics,
 *                             no zeroed buffer, the same bits on every run).  A token-less class's column, and under cosine a
 *                             NaN similarity (zeroed by the forward), get 0; gmin gets no gradient (detached in the reference);
 *                             under hardmax the one-hot attention is a constant and grad_att contributes nothing. */
int locov_token_attention_bwd(const float *sim, int64_t R, int Ttot, const int *tok_off,
                              const int *num_tok, int K1, int Tmax, float temperature,
                              int cosine, int hardmax, const float *gmin, const float *grad_scores,
                              const float *grad_att, float *grad_sim, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Opt-in reduced-precision form of the Res5 GEMMs (MODEL.ROI_BOX_HEAD.RES5_DTYPE: "bf16"; the default
 * and the parity path are fp32): bf16 operands on the bf16 MFMA pipe, fp32 accumulate, fp32 epilogue
 * (scale / shift / residual / ReLU as in locov_gemm_nt_f32) and fp32 output.  x / W / w_packed hold
 * bf16 bit patterns (locov_f32_to_bf16, locov_pack_conv3x3_weight(out_dtype = LOCOV_BF16)).
 * K % 8 == 0 (GEMM), Cin % 64 == 0 (conv).
 * ------------------------------------------------------------------------------------- */
int locov_gemm_nt_bf16(const uint16_t *x, int64_t lda, const uint16_t *W, const float *scale,
                       const float *shift, const float *residual, float *y, int64_t ldc,
                       int64_t M, int N, int K, unsigned flags, locov_stream_t stream);

int locov_conv3x3_nhwc_bf16(const uint16_t *x, int64_t R, int H, int W, int Cin, int pos_major,
                            const uint16_t *w_packed, const float *scale, const float *shift,
                            const float *residual, float *y, int N, unsigned flags,
                            locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Opt-in split-operand form of the fp32 Res5 GEMMs (MODEL.ROI_BOX_HEAD.RES5_DTYPE: "f16x2"; replaces the
 * same reference convolutions as locov_gemm_nt_f32, roi_emb_heads.py:217-245).  Every fp32 operand value v,
 * scaled by a power of two s that places the data in fp16's range, is represented as hi + lo with
 * hi = fp16(s v), lo = fp16(s v - hi) (22 significant bits; absolute floor 2^-25 / s), and x . W^T is formed
 * on the f16 matrix pipe as (hi.hi + hi.lo + lo.hi) / (s_x s_w) with fp32 accumulation: fp32 in, fp32 out,
 * a result within about two fp32 roundings per operand of the fp32-MFMA GEMM.  |s_x x| and |s_w w| must stay
 * below 65504 (x_scale = 16 covers |x| < 4094; choose w_scale from max |w|).  x is split on the fly; W is
 * split once by locov_split_f16x2_pack into `out`, a buffer of the SAME size as the fp32 matrix
 * (rows * K * 4 bytes; per row and group of 8 columns: 8 hi halves, then 8 lo halves).
 * K % 32 == 0; N, lda, ldc % 4 == 0; 16-byte aligned pointers.  Epilogue as locov_gemm_nt_f32.
 * RANGE GUARD: `overflow` (device pointer to one 32-bit word, or null) -- a launch in which any x value had
 * |x_scale * x| >= 65504 ORs 1 into it; the outputs such a value feeds are inf / NaN.  The word is only
 * ever set, never cleared: the caller zeroes it, enqueues any number of split launches and reads it once afterwards
 * (locov_amd's heads then repeat that call on the f32 MFMA).  Costs two v_max3_f32 per staged 16-byte chunk.
 * locov_split_f16x2_pack raises the same word when |w_scale * w| >= 65504, so that a caller may keep a weight's scale from
 * one optimizer step to the next (no host read of max |w| per step) and still learn when it stopped covering the data.
 * ------------------------------------------------------------------------------------- */
int locov_split_f16x2_pack(const float *w, int64_t rows, int K, int64_t ld, float w_scale, void *out,
                           unsigned *overflow, locov_stream_t stream);

int locov_gemm_nt_f32_split(const float *x, int64_t lda, const void *W_split, const float *scale,
                            const float *shift, const float *residual, float *y, int64_t ldc,
                            int64_t M, int N, int K, unsigned flags, float x_scale, float w_scale,
                            unsigned *overflow, locov_stream_t stream);

/* The last 1x1 convolution of Res5 fused with the spatial mean behind it (roi_emb_heads.py:245 -> :262,:344,:356):
 *   out[q, n] = mean over p < seg of relu?( scale[n] * (x[q*seg + p, :] . W[n, :]) + shift[n] + residual[p*R + q, n] )
 * with R = M / seg ROIs: x rows are ROI-major (LOCOV_WINO_OUT_ROI_MAJOR), the residual is the POSITION-major [M, N]
 * tensor of the previous block -- or, with LOCOV_SEGMEAN_RES_ROI_MAJOR in `flags`, a ROI-major one (row q*seg + p) --
 * and the [M, N] result is never written.  Per M-tile and ROI the kernel leaves column
 * sums in `workspace` (locov_gemm_segmean_workspace_bytes), a second small kernel adds the one or two partials of
 * each ROI in a fixed order (deterministic).  43 <= seg <= 128 (a 128-row tile holds at most four ROIs; Res5's 7x7
 * positions give 49), M % seg == 0, otherwise as locov_gemm_nt_f32_split.  M * N * 4 may pass 2^32 where the launch
 * takes the 256 x 256 tile (pre-split x, ROI-major residual, >= 1 024 tiles: the Res5 call of thousands of proposals); the
 * 128 x 128 form needs M * N * 4 < 2^32.  locov_gemm_segmean_supported says (1 / 0) whether a shape can be launched at
 * all -- the caller of roi_emb_heads.py:262,344,356 falls back to the unfused convolution + locov_spatial_mean_fwd. */
int locov_gemm_segmean_supported(int64_t lda, int64_t M, int N, int K, int seg, unsigned flags);
int64_t locov_gemm_segmean_workspace_bytes(int64_t M, int N);
int locov_gemm_nt_f32_split_segmean(const float *x, int64_t lda, const void *W_split, const float *scale,
                                    const float *shift, const float *residual, float *out, int64_t M,
                                    int N, int K, int seg, unsigned flags, float x_scale, float w_scale,
                                    void *workspace, int64_t workspace_bytes, unsigned *overflow,
                                    locov_stream_t stream);

/* `batch` independent problems (strides in fp32 elements; W_split problem b starts stride_w * 4 bytes * b in) */
int locov_gemm_nt_batched_f32_split(const float *x, int64_t lda, int64_t stride_x, const void *W_split,
                                    int64_t stride_w, float *y, int64_t ldc, int64_t stride_y,
                                    int64_t M, int N, int K, int batch, float x_scale, float w_scale,
                                    unsigned *overflow, locov_stream_t stream);

/* Measurement aid (bench.py's roofline block) -- process-global state, off by default (see Conventions): while
 * enabled, every GEMM-kernel launch made by this library (from any thread) is bracketed by HIP events on its launch
 * stream; launches on a stream that is being captured into a hipGraph are not recorded.  read() waits for them and
 * returns, for one kernel class, the number of launches, the sum of their durations (ms) and
 * the FLOPs they executed.  cls: 0 = gemm_nt_kernel<128x128, plain / batched> (1x1 convs, FCs,
 * Winograd-domain GEMMs), 1 = the position-major direct 3x3 conv, 2 = the other tile shapes,
 * 3 / 4 = classes 0 / 1 launched with bf16 operands, 5 = the split-operand GEMM on its 128x128 tile (gemm_split_kernel, every
 * form), 6 / 7 = the TN (weight-gradient) GEMM on the f32 MFMA / in split arithmetic; the split-operand GEMM on its 256x256 tile
 * (gemm_split_big_kernel) by launch kind: 8 = with the Winograd input transform in the epilogue
 * (locov_conv1x1_winograd_conv3x3_f32_split), 9 = one problem (the 1x1 convolutions), 10 = batched (the Winograd-domain GEMMs),
 * 11 = mean-fused (locov_gemm_nt_f32_split_segmean).
 * read_ex() also returns the ALGORITHMIC HBM bytes of those launches (every operand read once, every result written once;
 * stated for classes 5 and 8-11, 0 elsewhere); bytes may be null.
 * enable(on) clears what was recorded. */
int locov_gemm_timing_enable(int on);
int locov_gemm_timing_read(int cls, int64_t *launches, double *ms, double *flops);
int locov_gemm_timing_read_ex(int cls, int64_t *launches, double *ms, double *flops, double *bytes);

int locov_frozen_bn_fold(const float *weight, const float *bias, const float *running_mean,
                         const float *running_var, float eps, int C, float *scale, float *shift,
                         locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-7  row normalisation of [R,D] fp32: L2 (x / max(||x||, eps)) or standardise
 * ((x - mean) / (std_unbiased + eps)).  Replaces normalize_vec / standardize_vec
 * (logged_module.py:55-72) applied at box_emb_head.py:207-210 and to the bank at :223-232.
 * In-place allowed (y == x).
 * ------------------------------------------------------------------------------------- */
int locov_rownorm_fwd(const float *x, int64_t R, int D, int mode, float eps, float *y,
                      locov_stream_t stream);

/* Backward of locov_rownorm_fwd (training with a non-detached class predictor, box_emb_head.py:197-210):
 * grad_x from the forward INPUT x and grad_y.  L2 with |x| <= eps: the clamp is active, grad_x = grad_y / eps. */
int locov_rownorm_bwd(const float *x, const float *grad_y, int64_t R, int D, int mode, float eps,
                      float *grad_x, locov_stream_t stream);

/* fp32 -> bf16 (round-to-nearest-even, NaN preserved) for packing the text bank / embeddings */
int locov_f32_to_bf16(const float *x, int64_t n, uint16_t *y, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-8  region x text similarity GEMM, bf16 operands / fp32 accumulate on the bf16 MFMA pipe:
 *   logits[R,K1] = emb[R,D] . bank[K1,D]^T          (bias is identically zero,
 *   box_emb_head.py:234).  emb, bank are bf16 (uint16 storage).  Config 3 of BASELINE.json.
 * ------------------------------------------------------------------------------------- */
int locov_sim_gemm_bf16(const uint16_t *emb, const uint16_t *bank, int64_t R, int D, int K1,
                        float *logits, int64_t ldc, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-11  proposal labelling of a whole batch in one launch: the device half of SampleAllROIHeads.label_and_sample_proposals
 * (ovr/modeling/roi_heads/roi_emb_heads.py:25-118) -- [D2-upstream] pairwise_iou of every proposal with ITS image's ground truth,
 * Matcher (intervals [thr_lo[k], thr_hi[k]) -> thr_label[k] in {-1, 0, 1}; the first maximum wins, as torch.max), the class
 * labels of ROIHeads._sample_proposals (matched class / num_classes for background / -1 for ignored), the sort keys of the
 * sampler (rnd [2, total] uniform doubles: key = rnd + 2 [not in the population] + 4 image -- image-major, population first,
 * uniformly random inside it) and, per image, rows[i] = {foreground count, background count, entries of the quality matrix that
 * fail `>= 0` (the Matcher's assert), foreground boxes without positive width and height (Box2BoxTransform's assert)}.
 *   boxes [total, 4] / gt_boxes [sum M, 4] XYXY fp32 and gt_classes [sum M] int64 on the device, concatenated over the images;
 *   prop_offsets / gt_offsets: n_images + 1 HOST ints (rows of image i: [off[i], off[i+1])); rows [n_images, 4] int64, ZEROED by
 *   the caller; gt_index [total] int64 = matched row of the CONCATENATED ground truth (0 for an image without any);
 *   labels [total] int64; key_pos / key_neg [total] double.  At most LOCOV_LABEL_MAX_IMAGES images, LOCOV_LABEL_MAX_THRESHOLDS
 *   intervals.  Bit-identical to the torch-op form (tests/test_gpu_roi_heads.py).
 * ------------------------------------------------------------------------------------- */
#define LOCOV_LABEL_MAX_IMAGES 64
#define LOCOV_LABEL_MAX_THRESHOLDS 6
int locov_label_proposals(const float *boxes, const int *prop_offsets, const float *gt_boxes, const int64_t *gt_classes,
                          const int *gt_offsets, int n_images, const float *thr_lo, const float *thr_hi, const int *thr_label,
                          int n_thresholds, int64_t num_classes, const double *rnd, int64_t *gt_index, int64_t *labels,
                          double *key_pos, double *key_neg, int64_t *rows, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-11  the sampler behind that labelling, for a batch in which every image fills its budget: the rest of
 * SampleAllROIHeads.label_and_sample_proposals (ovr/modeling/roi_heads/roi_emb_heads.py:79-106: [D2-upstream]
 * ROIHeads._sample_proposals -> subsample_labels, then `proposals_per_image[sampled_idxs]`, gt_classes, the matched target's
 * fields, fg_proposal) in ONE launch, without a host read.  Image i takes num_pos = min(rows[i][0], max_pos) foreground proposals
 * in ascending key_pos, then budget - num_pos background proposals in ascending key_neg (the heads of the image's segments of
 * the two global argsorts the torch form takes), into slots [i * budget, (i + 1) * budget) of every output:
 *   picked (row of the concatenated proposals), out_boxes [.,4], out_classes (= labels[picked]), out_gt_boxes [.,4] (the matched
 *   ground-truth box; zeros for an image without ground truth), out_fg (class != num_classes), rois [.,5] = (image, box) -- the
 *   pooler's input format, convert_boxes_to_pooler_format of the sampled boxes -- and, when `field` is given, field_out =
 *   field[picked] (one more fp32 per-proposal field: objectness_logits).
 * All inputs are locov_label_proposals' outputs / inputs of the same batch, on the same stream.  A batch in which an image has
 * fewer candidates than its budget gets in-range but meaningless rows there: the caller learns it from `rows` (its one host read)
 * and samples that batch the host-driven way.  1..4096 proposals per image, ties between equal keys broken by row number.
 * ------------------------------------------------------------------------------------- */
int locov_sample_proposals(const double *key_pos, const double *key_neg, const int64_t *labels, const int64_t *gt_index,
                           const int64_t *rows, const float *boxes, const float *gt_boxes, const float *field,
                           const int *prop_offsets, const int *gt_offsets, int n_images, int budget, int max_pos,
                           int64_t num_classes, int64_t *picked, float *out_boxes, int64_t *out_classes, float *out_gt_boxes,
                           int64_t *out_fg, float *rois, float *field_out, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-11  the box-regression loss of the training heads in ONE launch.  Replaces the torch-op chain of [D2-upstream]
 * FastRCNNOutputLayers.box_reg_loss as the reference configures it (ovr/modeling/roi_heads/box_emb_grounding_head.py:278-279,
 * 370-374: "smooth_l1", SMOOTH_L1_BETA; Box2BoxTransform weights :368) -- get_deltas(proposal, matched ground truth) of the
 * foreground rows (0 <= gt_classes < num_classes), smooth-L1 (plain L1 below beta 1e-5) against the predicted deltas, summed in a
 * fixed order and divided by max(R, 1) -- and d loss / d pred_deltas from the same launch.
 *   proposal_boxes / gt_boxes [R, 4] XYXY fp32 (16-byte aligned), pred_deltas [R, ld] with ld = 4 (class-agnostic) or
 *   4 * num_classes, gt_classes [R] int64; loss [1]; dpred [R, ld] or NULL: written completely when ld == 4, otherwise only the four
 *   columns of a foreground row's class (the caller zeroes it).  Foreground boxes must have positive width and height (the
 *   labelling's validity bit, locov_label_proposals' rows[:, 3]).
 * ------------------------------------------------------------------------------------- */
int locov_box_reg_loss(const float *proposal_boxes, const float *gt_boxes, const float *pred_deltas, int64_t ld,
                       const int64_t *gt_classes, int64_t R, int64_t num_classes, float wx, float wy, float ww, float wh,
                       float smooth_l1_beta, float *loss, float *dpred, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-11  the IoU forms of that loss -- BBOX_REG_LOSS_TYPE "giou", "diou", "ciou" -- in ONE launch.  Replaces the torch-op chain of
 * [D2-upstream] FastRCNNOutputLayers.box_reg_loss for a loss type other than "smooth_l1" (the reference imports fvcore's giou_loss and
 * documents the key as `One of: "smooth_l1", "giou"`: ovr/modeling/roi_heads/box_emb_head.py:5,102,165 and
 * box_emb_grounding_head.py:5,305,374; [D2-upstream] _dense_box_regression_loss also takes "diou" and "ciou"): for the foreground
 * rows (0 <= gt_classes < num_classes) Box2BoxTransform.apply_deltas of the row's four predicted deltas (per-class predictions: the
 * four columns of the row's class) onto its proposal -- d / weight, dw and dh clamped to at most scale_clamp, centre = dx * W + cx,
 * size = exp(dw) * W -- then, against the matched ground-truth box with eps = 1e-7 ([fvcore, unverified]):
 *   inter = (min x2 - max x1) * (min y2 - max y1) where both factors are > 0 (strictly), else 0;  union = area_p + area_g - inter;
 *   iou = inter / (union + eps);  (cw, ch) and area_c: the smallest enclosing box
 *     LOCOV_BOX_IOU_GIOU  1 - (iou - (area_c - union) / (area_c + eps))
 *     LOCOV_BOX_IOU_DIOU  1 - iou + dist / (cw^2 + ch^2 + eps), dist = the squared distance of the centres ((x1 + x2) / 2, (y1 + y2) / 2)
 *     LOCOV_BOX_IOU_CIOU  diou + alpha * v, v = 4 / pi^2 (atan(wg / hg) - atan(w / h))^2, alpha = v / (1 - iou + v + eps) held constant
 *                         in the gradient (fvcore forms it under no_grad)
 * summed over the foreground rows in a fixed order and divided by max(R, 1) -- the smooth-L1 form's normalisation -- and
 * d loss / d pred_deltas from the same launch: a delta above the clamp gets exactly zero (torch.clamp: equality passes the gradient),
 * equal arguments of a max / min share the gradient half and half (torch.max / torch.min of two tensors), nothing flows through an
 * intersection that is masked out.  The row's arithmetic is fp64 from the fp32 inputs; the loss and each gradient entry are rounded
 * to fp32 once.  One workgroup, no atomics: the same inputs give the same bits.  No allocation, no synchronisation.
 *   Arguments as locov_box_reg_loss: proposal_boxes / gt_boxes [R, 4] XYXY fp32 (16-byte aligned), pred_deltas [R, ld] with ld = 4 or
 *   4 * num_classes, gt_classes [R] int64; loss [1]; dpred [R, ld] or NULL: written completely when ld == 4 (zeros in background /
 *   ignored rows), otherwise only the four columns of a foreground row's class (the caller zeroes it).  scale_clamp is a double
 *   (Box2BoxTransform's log(1000 / 16) is no fp32 number).  Background and ignored rows' predictions are never read: an inf or NaN
 *   there reaches neither the value nor the gradient.  Foreground proposals must have positive width and height.  R == 0: loss = 0.
 * ------------------------------------------------------------------------------------- */
#define LOCOV_BOX_IOU_GIOU 0
#define LOCOV_BOX_IOU_DIOU 1
#define LOCOV_BOX_IOU_CIOU 2
int locov_box_iou_loss(const float *proposal_boxes, const float *gt_boxes, const float *pred_deltas, int64_t ld,
                       const int64_t *gt_classes, int64_t R, int64_t num_classes, float wx, float wy, float ww, float wh,
                       double scale_clamp, int kind, float *loss, float *dpred, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-11  the classification loss of the training heads and its training statistics from ONE pass over the logits.  Replaces the
 * torch-op chain of [D2-upstream] FastRCNNOutputLayers.losses' `cross_entropy(scores, gt_classes, reduction="mean")`, which the
 * reference's predictors inherit (ovr/modeling/roi_heads/box_emb_head.py:60 and box_emb_grounding_head.py:259: both subclass
 * FastRCNNOutputLayers and define no losses of their own; roi_emb_heads.py:266,347 call it), and gathers the counts of [D2-upstream,
 * unverified] _log_classification_stats, which upstream's losses() calls first.
 *   scores [R, ld] fp32 with ld >= C columns per row (a column block of a wider matrix is fine; no alignment is required -- 16-byte
 *   loads are used when base, ld and C allow them, with the same bits either way), gt_classes [R] int64, ignore_index: torch's -100.
 *   loss [1]: mean over the rows that count (label in [0, C) and not ignore_index) of logsumexp(row) - row[label], max-subtracted;
 *   NaN when no row counts, as torch's.
 *   dscores [R, C] contiguous or NULL: d loss / d scores = (softmax - onehot) / n_valid, exact zeros in the rows that do not count.
 *   NULL (the scores need no gradient): nothing of that size is written.
 *   stats [6] int64 or NULL: num_instances (= R), num_fg, num_accurate, fg_num_accurate, num_false_negative, num_invalid with
 *   pred = argmax(row) (lowest index among equal maxima), bg = C - 1, foreground = 0 <= label < bg; num_accurate: pred == label;
 *   fg_num_accurate: the same over the foreground rows; num_false_negative: foreground rows with pred == bg; num_invalid: labels
 *   that are neither in [0, C) nor ignore_index (torch asserts on the device for these; here the row is treated as ignored).
 *   workspace: locov_cls_loss_workspace_bytes(R) bytes, 8-byte aligned: one partial per block, added in block order by a second
 *   small launch -- no atomics, the same inputs give the same bits.  No host read.
 * ------------------------------------------------------------------------------------- */
int64_t locov_cls_loss_workspace_bytes(int64_t R);

int locov_cls_loss(const float *scores, int64_t ld, const int64_t *gt_classes, int64_t R, int C, int64_t ignore_index,
                   void *workspace, int64_t workspace_bytes, float *loss, float *dscores, int64_t *stats, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-11  the federated class set of LVIS-style training, formed on the device in ONE launch without a host read.  Restates
 * [D2-upstream, unverified] FastRCNNOutputLayers.get_fed_loss_classes (MODEL.ROI_BOX_HEAD.USE_FED_LOSS; public Detectron2, not part of
 * the reference): `torch.unique(gt_classes)`, whose length is a device-to-host read, and `torch.multinomial(prob, num_fed - len(unique),
 * replacement=False)`, whose data-dependent sample count is another.
 *   gt_classes [R] int64 (any R >= 0), weights [K] fp32: the per-class sampling weights (upstream: image count to the power
 *   FED_LOSS_FREQ_WEIGHT_POWER), rnd [K] fp32: strictly positive Exp(1) draws made by the caller, num_fed >= 0: the size the set is
 *   filled up to (FED_LOSS_NUM_CLASSES), 1 <= K <= LOCOV_FED_LOSS_MAX_CLASSES.
 *   A class c in [0, K] is present when some label equals it; the background label K counts towards the number present, as it does in
 *   upstream's unique, but has no mask entry; labels outside [0, K] are skipped.  n_sample = max(0, num_fed - n_present).  Among the
 *   classes in [0, K) that are not present and whose weight is finite and > 0, the n_sample largest keys weights[c] / rnd[c] -- a
 *   correctly rounded fp32 division, so a torch restatement gives the same bits -- are sampled, equal keys going to the lower class
 *   index.  Dividing by Exp(1) draws and taking the top n is a weighted sample without replacement: the distribution is
 *   torch.multinomial's, the random stream is not.  With fewer such classes than n_sample all of them are taken (upstream's multinomial
 *   raises there).
 *   mask [K] bytes: present[c] || sampled[c];  counts [2] int32: {labels present, classes sampled}.  Both stay on the device.
 *   One block: a presence bitmap in LDS, then a radix select over the keys and a scan for the equal keys at the cut.
 * ------------------------------------------------------------------------------------- */
#define LOCOV_FED_LOSS_MAX_CLASSES 32767
int locov_fed_loss_classes(const int64_t *gt_classes, int64_t R, const float *weights, const float *rnd, int K, int num_fed,
                           unsigned char *mask, int *counts, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-11  the per-class sigmoid classification loss of LVIS-style training, its gradient and the training statistics from ONE pass
 * over the logits.  Replaces the torch-op chain of [D2-upstream, unverified] FastRCNNOutputLayers.sigmoid_cross_entropy_loss
 * (MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE; public Detectron2, not part of the reference): an [R, K + 1] zeros target, an index-put, a slice,
 * binary_cross_entropy_with_logits, the class-mask broadcast and a sum; the counts are those of _log_classification_stats, which
 * upstream logs whatever the loss type.
 *   scores [R, ld] fp32 with C = K + 1 columns per row and ld >= C (a column block of a wider matrix is fine; no alignment is required
 *   -- 16-byte loads are used when base, ld and C allow them, with the same bits either way), gt_classes [R] int64, class_mask [K]
 *   bytes (locov_fed_loss_classes' mask) or NULL for every class.
 *   loss [1]: sum over rows r and classes c < K of mask[c] * bce(x_rc, t_rc) / R with t_rc = 1 exactly when gt_classes[r] == c and
 *   bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|)).  The background column never enters the loss; a background label (K) makes its row
 *   all-negative.
 *   dscores [R, C] contiguous or NULL: d loss / d scores = mask[c] * (sigmoid(x) - t) / R for c < K, exactly 0 in the background column
 *   and in masked-out classes.  NULL (the scores need no gradient): nothing of that size is written.
 *   stats [6] int64 or NULL: locov_cls_loss' six counters in its order, from the argmax over all C columns (lowest index among equal
 *   maxima).  A label outside [0, K] counts in num_invalid (upstream's index-put fails for it) and its row contributes nothing: no loss
 *   terms and an exactly zero gradient; the divisor stays R.
 *   workspace: locov_sigmoid_cls_loss_workspace_bytes(R) bytes, 8-byte aligned: one partial per block, added in block order by a
 *   second small launch -- no atomics, the same inputs give the same bits.  No host read.
 * ------------------------------------------------------------------------------------- */
int64_t locov_sigmoid_cls_loss_workspace_bytes(int64_t R);

int locov_sigmoid_cls_loss(const float *scores, int64_t ld, const int64_t *gt_classes, const unsigned char *class_mask, int64_t R, int C,
                           void *workspace, int64_t workspace_bytes, float *loss, float *dscores, int64_t *stats, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-10  greedy NMS on the device.  Replaces [D2-upstream] torchvision.ops.nms as reached from
 * box_predictor.inference -> fast_rcnn_inference -> batched_nms
 * (ovr/modeling/roi_heads/roi_emb_heads.py:280,357).
 *   boxes_sorted [K,4] XYXY fp32, ALREADY in descending score order (class-aware NMS: the caller
 *   adds the per-class coordinate offsets first, exactly as torchvision's batched_nms does)
 *   keep [K] bytes (1 = kept), num_keep [1] int32 -- both on the device; no host sync.
 *   workspace: locov_nms_workspace_bytes(K) bytes of device memory.
 * ------------------------------------------------------------------------------------- */
int64_t locov_nms_workspace_bytes(int64_t K);

int locov_nms_sorted(const float *boxes_sorted, int64_t K, float iou_threshold, void *workspace,
                     unsigned char *keep, int *num_keep, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-10  the detection post-processing of the evaluation call, on the device, without a host read.  Replaces the torch-op chain
 * of [D2-upstream] FastRCNNOutputLayers.inference as the reference reaches it (ovr/modeling/roi_heads/roi_emb_heads.py:280,357;
 * evaluation runs it once per image: configs/coco_stt.yaml:50 TEST.IMS_PER_BATCH 1): Box2BoxTransform.apply_deltas with
 * class-agnostic deltas (ovr/modeling/roi_heads/box_emb_head.py:160-161 CLS_AGNOSTIC_BBOX_REG), Boxes.clip, `probs[:, :K] >
 * score_thresh`, class-wise NMS (batched_nms's coordinate shift, greedy in descending score order, IoU > nms_thresh dropped) and the
 * top `topk` detections per image in descending score order, ties in candidate (row, class) order.
 *   probs [R, ld_probs] fp32 = softmax of the logits (K foreground columns + background), deltas / proposal_boxes [R, 4] fp32
 *   (16-byte aligned), rows of image i = [row_offsets[i], row_offsets[i + 1]) (n_images + 1 HOST ints), image_hw: n_images HOST
 *   (height, width) pairs; wx..wh: Box2BoxTransform weights, scale_clamp its clamp of dw / dh.
 *   out_boxes [n_images, topk, 4], out_scores / out_classes / out_rows [n_images, topk] (rows: proposal index inside its image);
 *   every slot of a call is written: the slots at or beyond an image's count are empty (box 0, score 0, class -1, row -1), also
 *   for an image without candidates, an image over the candidate limit and a call without a single proposal;
 *   counts_and_flags [n_images + 1] int32: detections per image, then LOCOV_DETECT_FLAG_* bits -- when one is set the outputs are
 *   not to be used (the caller runs the torch chain): NONFINITE = a decoded box or a probability is inf / NaN (the reference drops
 *   such proposals with a warning), OVERFLOW = an image has more than LOCOV_DETECT_MAX_CANDIDATES candidates.
 *   workspace: locov_detect_postprocess_workspace_bytes(R, n_images) bytes.  At most LOCOV_LABEL_MAX_IMAGES images, 16 383
 *   proposals per image, 32 767 classes.  Bit-identical to the torch chain (tests/test_gpu_postprocess.py).
 * ------------------------------------------------------------------------------------- */
#define LOCOV_DETECT_MAX_CANDIDATES 8192
#define LOCOV_DETECT_FLAG_NONFINITE 1
#define LOCOV_DETECT_FLAG_OVERFLOW 2
int64_t locov_detect_postprocess_workspace_bytes(int64_t R, int n_images);

int locov_detect_postprocess(const float *probs, int64_t ld_probs, int num_classes, const float *deltas, const float *proposal_boxes,
                             const int *row_offsets, const float *image_hw, int n_images, float wx, float wy, float ww, float wh,
                             float scale_clamp, float score_thresh, float nms_thresh, int topk, void *workspace, int64_t workspace_bytes,
                             float *out_boxes, float *out_scores, int64_t *out_classes, int64_t *out_rows, int *counts_and_flags,
                             locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-10b the same post-processing for any candidate count (LVIS-style thresholds: SCORE_THRESH_TEST 1e-4, 1 203 classes -> up to
 * 1.2e6 candidates per image), bit-identical to the torch chain for every count.  Arguments as locov_detect_postprocess, plus
 * per_class_above: an image with n >= per_class_above candidates runs one NMS per class on the unshifted boxes, one below it
 * a single NMS on the class-shifted boxes (batched_nms's two branches; the decision is per image, on the device).
 *   counts_and_flags: as locov_detect_postprocess; only LOCOV_DETECT_FLAG_NONFINITE is ever set (the caller then runs the chain).
 *   Limits: at most LOCOV_LABEL_MAX_IMAGES images, 16 383 proposals per image, 32 767 classes, 1 <= topk <= 8 192, and
 *   R x K < 2^31 (R = all rows of the call, K = num_classes).
 *   workspace: locov_detect_postprocess_wide_workspace_bytes(row_offsets, n_images, num_classes, per_class_above) bytes, from host
 *   data only.  With R_i the rows of image i, W_i = ceil(R_i / 64), cap_i = clamp(per_class_above - 1, 0, R_i x K), n = n_images:
 *       16 R + 16 n K + 180 352 n + 8 (sum_i R_i W_i + sum_i cap_i W_i + R K)
 *   (decoded boxes; per (image, class) counts, survivors, offsets, cursors; per image 128 B of state, 6 x 2 048 histogram bins
 *   and 16 384 select slots; the row overlap matrices; the shifted branch's overlap words; the candidate keys).  0 for empty
 *   input (n_images == 0 or R == 0); < 0 on an argument error.
 * ------------------------------------------------------------------------------------- */
int64_t locov_detect_postprocess_wide_workspace_bytes(const int *row_offsets, int n_images, int num_classes, int per_class_above);

int locov_detect_postprocess_wide(const float *probs, int64_t ld_probs, int num_classes, const float *deltas, const float *proposal_boxes,
                                  const int *row_offsets, const float *image_hw, int n_images, float wx, float wy, float ww, float wh,
                                  float scale_clamp, float score_thresh, float nms_thresh, int topk, int per_class_above, void *workspace,
                                  int64_t workspace_bytes, float *out_boxes, float *out_scores, int64_t *out_classes, int64_t *out_rows,
                                  int *counts_and_flags, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-10c the two post-processing pipelines with CLASS-SPECIFIC box regression ([D2-upstream] MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG
 * False, Detectron2's default; the plain FastRCNNOutputLayers that build_box_predictor accepts, ovr/modeling/roi_heads/
 * box_emb_head.py:239-249).  Replaces the same call site: ovr/modeling/roi_heads/roi_emb_heads.py:280,357 -> fast_rcnn_inference on
 * boxes [R, 4K].  Arguments as locov_detect_postprocess / locov_detect_postprocess_wide, plus
 *   deltas [R, ld_deltas] fp32, 16-byte aligned, ld_deltas a multiple of 4 and >= 4 x box_classes;
 *   box_classes: 1 = class-agnostic (bit for bit the result of the entry point without _cs) or num_classes: candidate (r, c) has the
 *   box apply_deltas(deltas[r, 4c : 4c + 4], proposal r) clipped to its image.  Any other value: LOCOV_ERR_INVALID_ARG.
 * With box_classes = num_classes: batched_nms's shift unit is the maximum coordinate over the candidates' OWN boxes + 1; the shifted
 * branch takes the IoU on each candidate's own shifted box, the per-class branch on the candidates' own unshifted boxes (a wave per
 * (image, class) segment tests the pairs inside its greedy sweep: no row x row matrix); out_boxes holds the candidate's own box;
 * NONFINITE is raised when ANY of the R x K decoded boxes is inf / NaN before clipping, a candidate's or not (the chain tests the
 * whole [R, 4K] tensor), or any of the K + 1 probabilities of a row.  Orders, outputs, OVERFLOW and the limits are unchanged;
 * R x K < 2^31 holds for both pipelines.
 *   workspaces, from host data only; 0 for empty input, < 0 on an argument error.  With B = box_classes:
 *     locov_detect_postprocess_cs_workspace_bytes(R, n_images, num_classes, ld_deltas, box_classes)
 *         = align16(R (16 B + 8) + 4 ceil4(n_images)) + 4 522 000 n_images + 64
 *       (decoded boxes [R, B], row counts and offsets, candidates per image; per image the 8 192-slot lists and overlap bit sets);
 *     locov_detect_postprocess_wide_cs_workspace_bytes(row_offsets, n_images, num_classes, per_class_above, ld_deltas, box_classes)
 *         = 16 R B + 16 n K + 180 352 n + 8 (M + sum_i cap_i W_i + R K),   M = sum_i R_i W_i for B = 1, 0 for B = K > 1
 *       (W_i, cap_i, n as for locov_detect_postprocess_wide_workspace_bytes).
 * ------------------------------------------------------------------------------------- */
int64_t locov_detect_postprocess_cs_workspace_bytes(int64_t R, int n_images, int num_classes, int64_t ld_deltas, int box_classes);

int locov_detect_postprocess_cs(const float *probs, int64_t ld_probs, int num_classes, const float *deltas, int64_t ld_deltas, int box_classes,
                                const float *proposal_boxes, const int *row_offsets, const float *image_hw, int n_images, float wx, float wy,
                                float ww, float wh, float scale_clamp, float score_thresh, float nms_thresh, int topk, void *workspace,
                                int64_t workspace_bytes, float *out_boxes, float *out_scores, int64_t *out_classes, int64_t *out_rows,
                                int *counts_and_flags, locov_stream_t stream);

int64_t locov_detect_postprocess_wide_cs_workspace_bytes(const int *row_offsets, int n_images, int num_classes, int per_class_above,
                                                         int64_t ld_deltas, int box_classes);

int locov_detect_postprocess_wide_cs(const float *probs, int64_t ld_probs, int num_classes, const float *deltas, int64_t ld_deltas,
                                     int box_classes, const float *proposal_boxes, const int *row_offsets, const float *image_hw, int n_images,
                                     float wx, float wy, float ww, float wh, float scale_clamp, float score_thresh, float nms_thresh, int topk,
                                     int per_class_above, void *workspace, int64_t workspace_bytes, float *out_boxes, float *out_scores,
                                     int64_t *out_classes, int64_t *out_rows, int *counts_and_flags, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-10d the RPN's proposal generation of one feature level, on the device, without a host read.  Replaces the torch-op chain of
 * [D2-upstream] RPN.predict_proposals -> find_top_rpn_proposals (top-k, gather, Box2BoxTransform.apply_deltas, the finite test,
 * Boxes.clip, nonempty, torchvision's batched_nms, slice) as the reference reaches it: the evaluation call OvrRCNN.inference
 * (ovr/modeling/meta_arch/ovr_rcnn.py:76-124, backbone -> proposal_generator -> roi_heads) and the STT fine-tune's proposals
 * (ovr/modeling/meta_arch/distill_prop_mmss_gcnn.py:243-246,508-509).  The reference tree has no RPN source of its own; the
 * operation is restated from public sources.  Per image n:
 *   candidates: all hwa anchors, flat index i = (y W + x) A + a (the order of an NHWC head output);
 *   selection: descending logit, then ascending i (-0.0 and +0.0 compare equal; outputs carry the original bits); the first
 *     P = min(hwa, pre_nms_topk) -- the stable descending sort, where torch.topk leaves the order of ties open;
 *   box = apply_deltas(deltas[n, i], anchors[i]) with weights (wx, wy, ww, wh) and scale_clamp; a selected logit or a component of a
 *     selected decoded box that is inf / NaN (before clipping) raises LOCOV_RPN_FLAG_NONFINITE -- it is raised for ANY non-finite
 *     logit of the image, selected or not; the outputs are then not to be used (the caller runs the torch chain);
 *   clip to the image's (h, w); boxes whose width or height is not > min_box_size are dropped (they suppress nothing);
 *   greedy NMS in selection order: a box is dropped when IoU(kept, box) > nms_thresh for an earlier kept box;
 *   the first post_nms_topk survivors, in order.
 *   logits [n_images, hwa], deltas [n_images, hwa, 4] (16-byte aligned), anchors [hwa, 4] (16-byte aligned) fp32; image_hw:
 *   n_images HOST (height, width) pairs.
 *   out_boxes [n_images, post_nms_topk, 4] (16-byte aligned), out_logits [n_images, post_nms_topk] fp32, out_index
 *   [n_images, post_nms_topk] int64 (the flat i); rows at or beyond an image's count are zero (boxes 0, logits 0, index -1);
 *   counts_and_flags [n_images + 1] int32: survivors written per image, then the flag word.
 *   Limits, checked before any HIP call: 1 <= post_nms_topk <= pre_nms_topk <= 16 384, hwa < 2^22, at most LOCOV_LABEL_MAX_IMAGES
 *   images; n_images == 0 or hwa == 0 is a no-op success.
 *   workspace: locov_rpn_proposals_workspace_bytes(n_images, hwa, pre_nms_topk) bytes, from host data only.  With
 *   W = ceil(min(hwa, pre_nms_topk) / 64):
 *       n_images (512 W^2 + 1 544 W)
 *   (per image 64 W selection slots of a box, a logit and an index, W words of size-filter bits, and the 64 W x W words of the
 *   overlap bit matrix: 18 MB at 12 000 boxes).  0 for empty input; < 0 on an argument error.
 * ------------------------------------------------------------------------------------- */
#define LOCOV_RPN_FLAG_NONFINITE 1
#define LOCOV_RPN_MAX_PRE_NMS_TOPK 16384
int64_t locov_rpn_proposals_workspace_bytes(int n_images, int64_t hwa, int pre_nms_topk);

int locov_rpn_proposals(const float *logits, const float *deltas, const float *anchors, int64_t hwa, const float *image_hw, int n_images,
                        float wx, float wy, float ww, float wh, float scale_clamp, int pre_nms_topk, int post_nms_topk, float min_box_size,
                        float nms_thresh, void *workspace, int64_t workspace_bytes, float *out_boxes, float *out_logits, int64_t *out_index,
                        int *counts_and_flags, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-10e the RPN's training half of one feature level on the device, without a host read: anchor labelling, the sample draw and the
 * two losses with their gradients.  Replaces the torch-op chains of [D2-upstream] RPN.label_and_sample_anchors (pairwise_iou, Matcher
 * with allow_low_quality_matches, Boxes.inside_box, subsample_labels) and RPN.losses (binary_cross_entropy_with_logits over the
 * sampled anchors, Box2BoxTransform.get_deltas + smooth_l1_loss over the sampled positives), which the reference runs in every
 * detection step (ovr/modeling/meta_arch/ovr_rcnn.py:54-73, distill_prop_mmss_gcnn.py:243-267,595-616).  The reference tree has no
 * RPN source of its own; the operation is restated from public sources.  The anchors [hwa, 4] (flat index i = (y W + x) A + a) are
 * shared by the images of the batch.  Limits of all three, checked before any HIP call: at most LOCOV_LABEL_MAX_IMAGES images,
 * hwa < 2^22; n_images == 0 or hwa == 0 is a no-op success.
 *
 * locov_rpn_label_anchors -- per image n and anchor i:
 *   iou = pairwise_iou(gt box, anchor) in torch's operation order, every step rounded on its own; the matched box is the FIRST
 *   maximum over the image's boxes; the label is the Matcher's: 1, overwritten by lab[k] of every interval lo[k] <= max < hi[k]
 *   that holds; with allow_low_quality every anchor whose iou with some box of the image EQUALS that box's maximum over all anchors
 *   becomes 1 (it keeps its first-maximum box; a box that overlaps no anchor has the maximum 0 and promotes every anchor that does
 *   not touch it, as upstream); an image without ground truth: every label 0, matched boxes 0; boundary_thresh >= 0: anchors not
 *   inside [-t, w + t) x [-t, h + t) get -1 (Boxes.inside_box; after the promotion).
 *   anchors [hwa, 4], gt_boxes [sum M, 4] fp32 (16-byte aligned); gt_offsets_host: n_images + 1 HOST row offsets starting at 0;
 *   image_hw_host: n_images HOST (height, width) pairs; thr_*_host: the Matcher's n_thresholds <= LOCOV_LABEL_MAX_THRESHOLDS intervals.
 *   labels [n_images, hwa] int8 in {-1, 0, 1} (before the draw); matched_boxes [n_images, hwa, 4] fp32 (16-byte aligned);
 *   counts [n_images, 4] int32: (anchors labelled 1, anchors labelled 0, -, -) -- the entry point zeroes all four.
 *   workspace: locov_rpn_label_anchors_workspace_bytes(n_images, hwa, n_gt) = 16 ceil(n_gt / 4) bytes (one maximum per ground-truth
 *   box; zeroed by the entry point), n_gt = sum M; 0 for empty input; < 0 on an argument error.
 *
 * locov_rpn_sample_anchors -- subsample_labels with background label 0, the randomness passed in: rnd [2, n_images, hwa] float64
 *   uniforms in [0, 1).  num_pos = min(#label 1, max_pos) anchors of label 1 with the smallest rnd[0] stay 1, then
 *   num_neg = min(#label 0, budget - num_pos) anchors of label 0 with the smallest rnd[1] stay 0; equal keys are taken in ascending
 *   anchor index; every other anchor becomes -1.  labels / counts: locov_rpn_label_anchors' outputs; out_labels [n_images, hwa] int8
 *   (must not alias labels); counts[n, 2] = num_pos, counts[n, 3] = num_neg are written.  Requires 0 <= max_pos <= budget.
 *
 * locov_rpn_loss -- one pass over logits [n_images, hwa], deltas [n_images, hwa, 4], labels (after the draw), anchors and
 *   matched_boxes:
 *     loss[0] = cls_scale * sum over labels >= 0 of max(x, 0) - x y + log1p(exp(-|x|)),  y = [label == 1]
 *     loss[1] = loc_scale * sum over labels == 1 of smooth_l1(deltas - get_deltas(anchor, matched box); beta)  (beta < 1e-5: L1)
 *     dlogits = cls_scale (sigmoid(x) - y) where label >= 0, else 0;  ddeltas = loc_scale d smooth_l1 where label == 1, else 0
 *   (the caller folds the normaliser and the loss weights into the two scales).  Both gradients are written completely.  The sums
 *   are fp64 per-block partials added in block order: the same inputs give the same bits.  flags[0] (zeroed by the entry point)
 *   receives LOCOV_RPN_LOSS_FLAG_DEGENERATE when an anchor of label 1 has no positive width and height (Box2BoxTransform's assert).
 *   deltas, anchors, matched_boxes, ddeltas 16-byte aligned.
 *   workspace: locov_rpn_loss_workspace_bytes(n_images, hwa) = 16 n_images ceil(hwa / 256) bytes; < 0 on an argument error.
 * ------------------------------------------------------------------------------------- */
#define LOCOV_RPN_LOSS_FLAG_DEGENERATE 1
int64_t locov_rpn_label_anchors_workspace_bytes(int n_images, int64_t hwa, int64_t n_gt);

int locov_rpn_label_anchors(const float *anchors, int64_t hwa, const float *gt_boxes, const int *gt_offsets_host, const float *image_hw_host,
                            int n_images, const float *thr_lo_host, const float *thr_hi_host, const int *thr_label_host, int n_thresholds,
                            int allow_low_quality, float boundary_thresh, void *workspace, int64_t workspace_bytes, int8_t *labels,
                            float *matched_boxes, int *counts, locov_stream_t stream);

int locov_rpn_sample_anchors(const int8_t *labels, const double *rnd, int64_t hwa, int n_images, int budget, int max_pos, int *counts,
                             int8_t *out_labels, locov_stream_t stream);

int64_t locov_rpn_loss_workspace_bytes(int n_images, int64_t hwa);

int locov_rpn_loss(const float *logits, const float *deltas, const int8_t *labels, const float *anchors, const float *matched_boxes,
                   int64_t hwa, int n_images, float wx, float wy, float ww, float wh, float smooth_l1_beta, float cls_scale, float loc_scale,
                   void *workspace, int64_t workspace_bytes, float *loss, float *dlogits, float *ddeltas, int *flags, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-12  LSM grounding: word<->region alignment -> [caption, image] cost matrices.
 * Replaces the B^2-replicated chain of GroundingHead.forward
 * (ovr/modeling/mmss_heads/grounding_head.py:116-243) for LOCAL_METRIC "dot", ALIGNMENT
 * "softmax", GLOBAL_METRIC "aligned_local" (configs/coco_lsm.yaml); ALIGNMENT "hardmax" and a
 * single direction: locov_grounding_align_fwd / _bwd below.
 *   S [B*T, B*NR] = caption token embeddings [B*T, L] . region embeddings [B*NR, L]^T
 *     (one locov_gemm_nt_f32 call; the region embeddings are v2l_projection(region_features),
 *     grounding_head.py:111, itself a locov_gemm_nt_f32 call)
 *   caption_mask [B,T] = attention_mask * (1 - special_tokens_mask) as fp32, region_mask [B,NR] fp32
 *   cost_w2r / cost_r2w [B,B] (row = caption, column = image): global_dist_w2r / _r2w of :219-228,
 *     before the all-empty fix-up of :232-243 (a [B,B] select the host applies).
 * The backward returns dS given the gradients of the two cost matrices.
 * ------------------------------------------------------------------------------------- */
int locov_grounding_fwd(const float *S, int B, int T, int NR, const float *caption_mask,
                        const float *region_mask, float temperature, float *cost_w2r,
                        float *cost_r2w, locov_stream_t stream);

int locov_grounding_bwd(const float *S, int B, int T, int NR, const float *caption_mask,
                        const float *region_mask, float temperature, const float *grad_w2r,
                        const float *grad_r2w, float *grad_S, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-12  the same launch with the alignment rule chosen and either direction optional (grounding_head.py:161-174 and
 * ALIGN_WORDS_TO_REGIONS / ALIGN_REGIONS_TO_WORDS).  Added under ABI version 8.  Same kernel, same LDS tile, same limits; with
 * LOCOV_GROUNDING_ALIGN_SOFTMAX and both directions given the results are bit-identical to locov_grounding_fwd / _bwd.
 *   alignment HARDMAX: every word aligns to its valid region of largest S[t, r] (the lowest index on ties, torch's argmax rule;
 *     region 0 with its unmasked distance when the image has no valid region -- every entry then equals the reference's fill), and
 *     cost_w2r[c, i] = sum_t cm[t] * (-S[t, r*(t)] / temperature) / max(num_words, 1); regions to words symmetrically over the valid
 *     words of each valid region (word 0 when the caption has none).  The one-hot is a constant: the backward adds
 *     -g_w2r[c, i] * cm[t] / (temperature * max(num_words, 1)) to dS[t, r*(t)], the region direction likewise, summed where both meet.
 *   cost_w2r / cost_r2w (forward), grad_w2r / grad_r2w (backward): NULL turns that direction off -- it is neither computed nor
 *     read; both NULL is LOCOV_ERR_INVALID_ARG.  grad_S is always written in full (zeros where nothing flows).
 * ------------------------------------------------------------------------------------- */
#define LOCOV_GROUNDING_ALIGN_SOFTMAX 0
#define LOCOV_GROUNDING_ALIGN_HARDMAX 1
int locov_grounding_align_fwd(const float *S, int B, int T, int NR, const float *caption_mask, const float *region_mask,
                              float temperature, int alignment, float *cost_w2r, float *cost_r2w, locov_stream_t stream);
int locov_grounding_align_bwd(const float *S, int B, int T, int NR, const float *caption_mask, const float *region_mask,
                              float temperature, int alignment, const float *grad_w2r, const float *grad_r2w, float *grad_S,
                              locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-12  the cross-entropy tail of GroundingHead.forward on the [B, B] caption x image costs of locov_grounding_fwd, in ONE launch
 * (ovr/modeling/mmss_heads/grounding_head.py:239-251: pairs with neither words nor regions get max(cost) + 100; :273-290
 * diag(-log_softmax(-cost, dim 0 | 1)).mean(); :357-377 (cost.argmin(dim 0 | 1) == arange).mean()).
 *   cost_w2r / cost_r2w [B, B] (either may be NULL: ALIGN_WORDS_TO_REGIONS / ALIGN_REGIONS_TO_WORDS off), caption_mask [B, T],
 *   region_mask [B, NR] fp32; out8 = {CE choose caption, CE choose image, accuracy choose caption, accuracy choose image} for w2r,
 *   then for r2w.  _bwd: g_* = device scalars d L / d (each of the four CE values) or NULL (= 0); dcost_* [B, B].
 *   B <= LOCOV_GROUNDING_CE_MAX_B.
 * ------------------------------------------------------------------------------------- */
#define LOCOV_GROUNDING_CE_MAX_B 64
int locov_grounding_ce_fwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask, int B,
                           int T, int NR, float *out8, locov_stream_t stream);
int locov_grounding_ce_bwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask, int B,
                           int T, int NR, const float *g_w2r_caption, const float *g_w2r_image, const float *g_r2w_caption,
                           const float *g_r2w_image, float *dcost_w2r, float *dcost_r2w, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-12  the same cross-entropy tail when GroundingHead also returns its distributions (MMSS_HEAD.DISTILLATION_LOSS, grounding_head.py:
 * 380-382 hands {"w2r", "r2w"} to the distillation losses, distill_prop_mmss_gcnn.py:424-442).  Added under ABI version 8.
 *   _fwd: what locov_grounding_ce_fwd does, and also writes the filled costs pw_w2r / pw_r2w [B, B] (:239-251: the cost where the
 *     caption has words or the image has regions, else max(cost) + 100 in fp32 -- bit-identical to torch.where(ok, cost,
 *     cost.max() + 100)).  pw_* is required where cost_* is given.
 *   _bwd: as locov_grounding_ce_bwd, plus the upstream gradients g_pw_w2r / g_pw_r2w [B, B] of the returned distributions (NULL = 0),
 *     added to dcost on the ok pairs only: the fill is a detached constant.
 * ------------------------------------------------------------------------------------- */
int locov_grounding_ce_dist_fwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask, int B,
                                int T, int NR, float *out8, float *pw_w2r, float *pw_r2w, locov_stream_t stream);
int locov_grounding_ce_dist_bwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask, int B,
                                int T, int NR, const float *g_w2r_caption, const float *g_w2r_image, const float *g_r2w_caption,
                                const float *g_r2w_image, const float *g_pw_w2r, const float *g_pw_r2w, float *dcost_w2r, float *dcost_r2w,
                                locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-12  the triplet tail of GroundingHead.forward (LOSS "triplet", grounding_head.py:279-343) on the same [B, B] costs, ONE launch
 * each way.  Added under ABI version 8.  B <= LOCOV_GROUNDING_CE_MAX_B; cost_w2r / cost_r2w: either may be NULL.
 *   Pairs with neither words nor regions get max(cost) + 100 first (:239-251, a detached constant, bit-identical to
 *   torch.where(ok, cost, cost.max() + 100)).  positive = the diagonal.  The negative of column j ("choose caption") is, over the
 *   rows i != j, the minimum (LOCOV_TRIPLET_HARDEST) or maximum (LOCOV_TRIPLET_EASIEST) of cost[i, j], or (LOCOV_TRIPLET_GIVEN) the
 *   entry at reduced index k = neg_idx[...][j]: row k if k < j, else row k + 1 -- what gather on the matrix without its diagonal
 *   picks (NEGATIVE_MINING "random", the draw made by the caller).  Rows ("choose image") likewise.
 *   loss = mean(relu(positive - negative + margin)) in that fp32 order; B < 2: negative = positive + margin, zero gradient.
 *   neg_idx: int64 [2 directions (w2r, r2w)][2 choices (caption, image)][B], required for GIVEN (values in [0, B - 1); the caller
 *     vouches for them, the device clamps rather than follow one out of the matrix), ignored otherwise.
 *   out8: the layout of locov_grounding_ce_fwd with the two losses in the CE slots; the accuracies are the same argmin means.
 *   pw_w2r / pw_r2w: the filled costs, NULL where not wanted.
 *   _bwd: g_* = device scalars d L / d (each of the four losses) or NULL (= 0), g_pw_* [B, B] the upstream gradients of the returned
 *     distributions (NULL = 0).  The gradient reaches the diagonal entry and the selected negative of each active hinge; the filled
 *     pairs are constants.
 * ------------------------------------------------------------------------------------- */
#define LOCOV_TRIPLET_HARDEST 0
#define LOCOV_TRIPLET_EASIEST 1
#define LOCOV_TRIPLET_GIVEN 2
int locov_grounding_triplet_fwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask, int B,
                                int T, int NR, int mining, float margin, const int64_t *neg_idx, float *out8, float *pw_w2r,
                                float *pw_r2w, locov_stream_t stream);
int locov_grounding_triplet_bwd(const float *cost_w2r, const float *cost_r2w, const float *caption_mask, const float *region_mask, int B,
                                int T, int NR, int mining, float margin, const int64_t *neg_idx, const float *g_w2r_caption,
                                const float *g_w2r_image, const float *g_r2w_caption, const float *g_r2w_image, const float *g_pw_w2r,
                                const float *g_pw_r2w, float *dcost_w2r, float *dcost_r2w, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The distillation losses of the LSM meta-architecture over the [B, B] caption x image costs, ONE launch each way (SURVEY 8f-3;
 * ovr/modeling/meta_arch/distill_mmss_gcnn.py:211-433, called three times per step at distill_prop_mmss_gcnn.py:424-442).
 * Added under ABI version 8.
 *   trans [B, B] = the transformer's costs, w2r / r2w [B, B] = GroundingHead's distributions (rows = captions, columns = images).
 *   A cost matrix is read per image over the captions ("cap": softmax of -cost / temperature over dim 0) and per caption over the
 *   images ("img": over dim 1).  kind:
 *     LOCOV_DISTILL_KD   MultiDistillLoss (:211-290): temperature^2 * KL(teacher || student), "batchmean" (sum / B), over
 *                        {cap, img} x {w2r, r2w}; transformer_teacher != 0: trans teaches w2r and r2w, else w2r and r2w teach trans.
 *     LOCOV_DISTILL_JS   MultiDistillLossJS (:293-376): 1/2 KL(P || M) + 1/2 KL(Q || M), M = the mixture of the "cap" views; as in
 *                        the reference (:357-366) the "img" terms are measured against the "cap" mixture too.
 *     LOCOV_DISTILL_MSE  MultiDistillLossL2 (:379-433): mse(trans, S) + mse(trans^T, S^T) for S = w2r, r2w (temperature unused).
 *   The result is multiplied by loss_weight.  _fwd writes the scalar *loss.  _bwd takes the device scalar grad_loss = d L / d loss and
 *   writes grad_trans / grad_w2r / grad_r2w [B, B]; any of them may be NULL (a detached teacher, an input without grad).
 *   0 * log 0 := 0 as torch.nn.functional.kl_div defines it.  The one intended difference from torch: where a teacher probability
 *   underflows to exactly 0, torch's teacher gradient there is NaN (d/dp of p log p at 0); the kernel returns the finite limit (0 for
 *   that element's softmax term).
 *   1 <= B <= LOCOV_DISTILL_MAX_B, temperature > 0.
 * ------------------------------------------------------------------------------------- */
#define LOCOV_DISTILL_KD 0   /* MultiDistillLoss,   distill_mmss_gcnn.py:211-290 */
#define LOCOV_DISTILL_JS 1   /* MultiDistillLossJS, distill_mmss_gcnn.py:293-376 */
#define LOCOV_DISTILL_MSE 2  /* MultiDistillLossL2, distill_mmss_gcnn.py:379-433 */
#define LOCOV_DISTILL_MAX_B 64 /* B = IMS_PER_BATCH per GPU (configs/coco_lsm.yaml: 32 over 8 GPUs = 4) */
int locov_distill_loss_fwd(const float *trans, const float *w2r, const float *r2w, int B, int kind, int transformer_teacher,
                           float temperature, float loss_weight, float *loss, locov_stream_t stream);
int locov_distill_loss_bwd(const float *trans, const float *w2r, const float *r2w, int B, int kind, int transformer_teacher,
                           float temperature, float loss_weight, const float *grad_loss, float *grad_trans, float *grad_w2r,
                           float *grad_r2w, locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Backward of the predictor's dense layers under autograd (locov_pool_fc_bwd, locov_sim_gemm_bwd; the
 * forward arithmetic they differentiate is box_emb_head.py:196 bbox_pred, :206 emb_pred, :211 cls_score).
 *
 * locov_pool_fc_bwd: x [R,C5] (the pooled features; the [R,C5,7,7] form composes with locov_spatial_mean_bwd),
 *   emb_w [D,C5], bbox_w [4,C5], grad_emb [R,D] and / or grad_deltas [R,4] (either may be null: a detached class
 *   predictor, roi_heads DETACH_CLASS_PREDICTOR, sends no grad_emb).  Outputs, each optional (null = not wanted):
 *   grad_x [R,C5] = grad_emb . emb_w + grad_deltas . bbox_w;  grad_emb_w [D,C5] = grad_emb^T x, grad_emb_b [D] = column
 *   sums; grad_bbox_w [4,C5], grad_bbox_b [4] likewise.  Deterministic (no atomics).  C5 % 4 == 0, D % 4 == 0.
 * locov_sim_gemm_bwd: grad_logits [R,K1], emb [R,D], bank [K1,D] -> grad_emb [R,D] = grad_logits . bank (any K1) and /
 *   or grad_bank [K1,D] = grad_logits^T emb (K1 % 4 == 0 only: the reference freezes the bank, box_emb_head.py:234-235,
 *   so no caller on the path asks for it).  fp32 (the bf16 similarity GEMM is an inference-only option).
 * workspace: device memory of at least *_workspace_bytes(...) bytes, 256-byte aligned (transposed weight copies and the
 * TN GEMM's partial tiles); R == 0 writes zero weight gradients and returns.
 * ------------------------------------------------------------------------------------- */
int64_t locov_pool_fc_bwd_workspace_bytes(int64_t R, int C5, int D);
int locov_pool_fc_bwd(const float *x, int64_t R, int C5, const float *emb_w, int D, const float *bbox_w,
                      const float *grad_emb, const float *grad_deltas, float *grad_x, float *grad_emb_w,
                      float *grad_emb_b, float *grad_bbox_w, float *grad_bbox_b, void *workspace,
                      int64_t workspace_bytes, locov_stream_t stream);
int64_t locov_sim_gemm_bwd_workspace_bytes(int64_t R, int D, int K1);
int locov_sim_gemm_bwd(const float *grad_logits, const float *emb, const float *bank, int64_t R, int D, int K1,
                       float *grad_emb, float *grad_bank, void *workspace, int64_t workspace_bytes,
                       locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-4...a-8 in one call: EmbeddingFastRCNNOutputLayers.forward (box_emb_head.py:179-212)
 * preceded by the spatial mean of its caller (roi_emb_heads.py:262,344,356).
 *   x        [R,C5,HW] fp32 (HW may be 1)            pooled  [R,C5]  (out; == x when HW==1 is allowed)
 *   emb_w    [D,C5], emb_b [D]                        emb     [R,D]   (out, after optional norm)
 *   bbox_w   [4,C5], bbox_b [4]                       deltas  [R,4]   (out)
 *   bank     [K1,D] fp32 (already normalised by set_class_embeddings if enabled)
 *   bank_bf16 optional packed copy; used when sim_dtype == LOCOV_BF16 (emb_bf16 [R,D] scratch)
 *   logits   [R,K1] (out)
 * Weights are read at call time (the reference re-assigns emb_pred.weight/bias to the
 * grounding head's parameters, distill_prop_mmss_gcnn.py:121-125).
 * ------------------------------------------------------------------------------------- */
int locov_box_head_fwd(const float *x, int64_t R, int C5, int HW, int channels_last,
                       const float *emb_w, const float *emb_b, const float *bbox_w,
                       const float *bbox_b, const float *bank, const uint16_t *bank_bf16,
                       int D, int K1, int norm_mode, int sim_dtype, float *pooled,
                       float *deltas, float *emb, uint16_t *emb_bf16, float *logits,
                       locov_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a-3 under autograd: the backward pass of the Res5 stage (the LSM head TRAINS the Res5 convolution weights --
 * configs/coco_lsm.yaml:8 FREEZE_AT 0, FrozenBN only freezes the statistics -- through
 * roi_emb_heads.py:323 (whole grid) and :343-347 (sampled proposals); the reference gets these gradients from
 * cuDNN via torch autograd).  All tensors are channels-last pixel-row matrices as in the forward entry points.
 *
 * locov_gemm_nt_f32_ex       : locov_gemm_nt_f32 with an explicit row pitch of W (ldb) and an optional `mask`
 *                              [M, ldc]: the finished value is kept where mask > 0 and zeroed elsewhere -- the ReLU
 *                              backward of a saved activation fused into the data-gradient GEMM  dx = g . (s*W)
 *                              (W given transposed, locov_weight_transpose_scale).
 * locov_conv3x3_nhwc_f32_ex  : locov_conv3x3_nhwc_f32 with the same mask (3x3 data gradient = convolution with the
 *                              flipped, transposed filter, locov_conv3x3_weight_flip).
 * locov_winograd_conv3x3_f32_ex : the same for 7x7 tiles in the Winograd domain.
 * locov_gemm_tn_f32          : out[b][N,K] = row_scale[n] * sum_m a_b[m,n] * b_b[m,k] -- the weight gradient
 *                              dW = s * g^T x of a 1x1 convolution (contraction over the pixel rows; split over M,
 *                              partial tiles reduced in a fixed order: deterministic).  batch problems with strides
 *                              (elements); workspace: locov_gemm_tn_workspace_bytes(M, N, K, batch).
 * locov_winograd_wgrad_f32   : dw [N,Cin,3,3] of a 3x3 convolution over R 7x7 tiles, in the Winograd domain:
 *                              dU_f = ((A (x) A) g)_f^T ((BT (x) BT) x)_f (121 TN GEMMs), dw = row_scale * (G (x) G)^T dU.
 *                              flags: 0 (position-major rows) or LOCOV_WINO_IN_ROI_MAJOR (both x and g).
 * locov_im2col3x3_nhwc / locov_conv3x3_wgrad_unpack : the general-grid form of the same gradient
 *                              (dw_packed [N, 9*Cin] = g^T . im2col(x) through locov_gemm_tn_f32).
 * amax_out (locov_relu_mask, locov_spatial_mean_bwd, locov_gemm_nt_f32_split_ex, locov_winograd_conv3x3_f32_split_ex): optional
 *                              16-byte operand-scale slot, ZEROED by the caller; the launch folds max |the tensor it writes| into
 *                              word 2 (an atomic max on the bit pattern), and a later split GEMM that takes the slot as its
 *                              x_scale_dev / a_scale_dev derives the tensor's power-of-two scale from that word (words 0-1 stay
 *                              zero: "not reduced by locov_split_scale_from_amax") -- the gradient is not read a second time
 *                              just to find its range.
 * locov_relu_mask, locov_spatial_mean_bwd, locov_rows_stride2, locov_roi_align_nhwc_bwd : element-wise pieces --
 *                              ReLU backward, the mean's broadcast (roi_emb_heads.py:344) fused with it, block 0's
 *                              stride-2 pixel selection on the whole grid and its adjoint, and the adjoint of
 *                              locov_roi_align_nhwc_fwd (fp32 atomics into a zeroed channels-last map gradient).
 * ------------------------------------------------------------------------------------- */
int locov_gemm_nt_f32_ex(const float *x, int64_t lda, const float *W, int64_t ldb, const float *scale,
                         const float *shift, const float *residual, const float *mask, float *y, int64_t ldc,
                         int64_t M, int N, int K, unsigned flags, locov_stream_t stream);

int locov_conv3x3_nhwc_f32_ex(const float *x, int64_t R, int H, int W, int Cin, int pos_major,
                              const float *w_packed, const float *scale, const float *shift,
                              const float *residual, const float *mask, float *y, int N, unsigned flags,
                              locov_stream_t stream);

int locov_winograd_conv3x3_f32_ex(const float *x, int64_t R, int Cin, const float *U, const float *scale,
                                  const float *shift, const float *mask, float *y, int64_t ldy, int N,
                                  unsigned flags, void *workspace, int64_t workspace_bytes,
                                  locov_stream_t stream);

int64_t locov_gemm_tn_workspace_bytes(int64_t M, int N, int K, int batch);
int locov_gemm_tn_f32(const float *a, int64_t lda, int64_t stride_a, const float *b, int64_t ldb,
                      int64_t stride_b, float *out, int64_t ldo, int64_t stride_o, int64_t M, int N, int K,
                      int batch, const float *row_scale, void *workspace, int64_t workspace_bytes,
                      locov_stream_t stream);

/* The same gradients in the split-operand arithmetic of the forward (3 f16 MFMAs per fp32 product block instead of 16 f32
 * ones).  A gradient tensor has no a-priori range, so its operand scale is chosen ON THE DEVICE:
 *   locov_split_scale_from_amax : scale_out[0] = s = the power of two with max |s x| in [2^(target_log2-1), 2^target_log2), scale_out[1] = 1/s,
 *                                 scale_out[2..3] = scratch (max bits, arrival tickets; zero again afterwards); a 16-byte memset and
 *                                 ONE kernel (the workgroup drawing the last ticket writes the scale), no host read.  scale_out: 16 bytes.
 *   locov_split_scale_from_amax_zeroed : the same without the memset, for 16 bytes whose words 2..3 are ALREADY zero (fresh from a
 *                                 zeroed pool, or last used by one of these two calls).
 *   locov_gemm_nt_f32_split_ex  : locov_gemm_nt_f32_split with the epilogue `mask` of locov_gemm_nt_f32_ex and, when
 *                                 x_scale_dev is non-null, the operand scale of x read from it (x_scale is then ignored).
 *   locov_gemm_tn_f32_split     : locov_gemm_tn_f32 with split operands: a (the gradient) scaled by a_scale_dev[0], b (the
 *                                 activation) by b_scale; both are converted on their way into LDS.  Same workspace,
 *                                 same fixed-order chunk reduction, same range-guard word.
 *   locov_winograd_wgrad_f32_split : locov_winograd_wgrad_f32 with its 121 TN GEMMs in that arithmetic (the transformed
 *                                 gradient's scale is chosen on the device, the transformed activation is scaled by 0.25). */
int locov_split_scale_from_amax(const float *x, int64_t n, float target_log2, float *scale_out,
                                locov_stream_t stream);
/* An upper bound of max |.| of a tensor that is about to be derived from SMALL ones, without a pass over the large tensor:
 * folds  max_i (muls[i] * max |xs[i]|)  (count <= LOCOV_AMAX_BOUND_MAX device tensors of ns[i] elements, ns[i] % 4 == 0; host
 * arrays) into word 2 of `slot`, a ZEROED 16-byte operand-scale slot as for amax_out.  The training step's head of the
 * backward chain: the masked broadcast of the pooled gradient (locov_spatial_mean_bwd: g = grad / 49 where the activation is
 * positive) and the masked whole-grid gradient (locov_relu_mask) are bounded by their small inputs (roi_emb_heads.py:344,:323). */
#define LOCOV_AMAX_BOUND_MAX 4
int locov_amax_bound(const float *const *xs, const int64_t *ns, const float *muls, int count, float *slot,
                     locov_stream_t stream);
int locov_split_scale_from_amax_zeroed(const float *x, int64_t n, float target_log2, float *scale_out,
                                       locov_stream_t stream);
int locov_gemm_nt_f32_split_ex(const float *x, int64_t lda, const void *W_split, const float *scale,
                               const float *shift, const float *residual, const float *mask, float *y,
                               int64_t ldc, int64_t M, int N, int K, unsigned flags, float x_scale,
                               const float *x_scale_dev, float w_scale, unsigned *overflow,
                               float *amax_out, locov_stream_t stream);
int locov_gemm_tn_f32_split(const float *a, int64_t lda, int64_t stride_a, const float *b, int64_t ldb,
                            int64_t stride_b, float *out, int64_t ldo, int64_t stride_o, int64_t M, int N,
                            int K, int batch, const float *row_scale, const float *a_scale_dev,
                            float b_scale, unsigned *overflow, void *workspace, int64_t workspace_bytes,
                            locov_stream_t stream);
/* locov_winograd_conv3x3_f32_split with the output `mask` of locov_winograd_conv3x3_f32_ex and, with v_scale_auto != 0, the
 * scale of the transformed input chosen on the device (the input is a gradient: the data gradient of a 3x3 convolution).
 * y_split_scale > 0: y is written in the split layout of locov_split_f16x2_pack scaled by y_split_scale (N % 32 == 0, ldy == N,
 * no mask) -- the pre-split A operand (LOCOV_GEMM_A_SPLIT) of the 1x1 convolution that follows; out-of-range values raise
 * *overflow here.  (With a fixed v_scale the transformed input is handed to the batched GEMM in that layout as well.)
 * y_split_scale < 0 (no mask): y stays fp32 and is RANGE-CHECKED for the split GEMM that will read it at operand scale
 * -y_split_scale (|scale * y| >= 65504 raises *overflow here, one launch before that GEMM's own check: a caller that waits for
 * the guard word -- roi_emb_heads.py:343-347 under autograd -- can record its event in front of the stage's last launches). */
int locov_winograd_conv3x3_f32_split_ex(const float *x, int64_t R, int Cin, const void *U_split, float u_scale,
                                        float v_scale, int v_scale_auto, const float *scale, const float *shift,
                                        const float *mask, float *y, int64_t ldy, int N, unsigned flags,
                                        float y_split_scale, void *workspace, int64_t workspace_bytes,
                                        unsigned *overflow, float *amax_out, locov_stream_t stream);
int locov_winograd_wgrad_f32_split(const float *x, const float *g, int64_t R, int Cin, int N, unsigned flags,
                                   const float *row_scale, float *dw, unsigned *overflow, void *workspace,
                                   int64_t workspace_bytes, locov_stream_t stream);
/* ... with the transformed activation the FORWARD already made: v_split = the first 121 * R * Cin floats of the workspace that
 * locov_winograd_conv3x3_f32_split[_ex] was given for the same x (split layout x 0.25, one pass: R proposals) -- a training step
 * that keeps that workspace per bottleneck (roi_emb_heads.py:343-347 under autograd) saves the second input transform, and the TN
 * GEMMs stage the operand as it is (locov_gemm_tn_f32_split_b).  Cin % 8 == 0.  The same bits as locov_winograd_wgrad_f32_split.
 *   locov_gemm_tn_f32_split_b : locov_gemm_tn_f32_split whose b is ALREADY in the split layout of locov_split_f16x2_pack at scale
 *   b_scale (K, ldb, stride_b multiples of 8): transposed on its way into LDS, not converted; the same bits. */
int locov_winograd_wgrad_f32_split_v(const float *v_split, const float *g, int64_t R, int Cin, int N, unsigned flags,
                                     const float *row_scale, float *dw, unsigned *overflow, void *workspace,
                                     int64_t workspace_bytes, locov_stream_t stream);
int locov_gemm_tn_f32_split_b(const float *a, int64_t lda, int64_t stride_a, const float *b_split, int64_t ldb,
                              int64_t stride_b, float *out, int64_t ldo, int64_t stride_o, int64_t M, int N,
                              int K, int batch, const float *row_scale, const float *a_scale_dev,
                              float b_scale, unsigned *overflow, void *workspace, int64_t workspace_bytes,
                              locov_stream_t stream);
/* A bottleneck's first two convolutions in ONE call (roi_emb_heads.py:217-245: conv1 1x1 + FrozenBN + ReLU, then conv2 3x3 + FrozenBN
 * + ReLU?) in split arithmetic:  y = locov_winograd_conv3x3_f32_split_ex(relu(x . W1^T * scale1 + shift1), ...)  -- the same bits as
 * locov_gemm_nt_f32_split (LOCOV_GEMM_A_SPLIT | LOCOV_EPI_RELU) followed by that call, which is what it falls back to.  Where the shapes
 * fill the chip with 256x256 tiles (both operands pre-split, C % 256 == 0, >= 1 024 tiles) the 1x1 convolution's epilogue applies the
 * Winograd INPUT transform itself: the [49 R, C] pixel tensor between the two convolutions is never written or re-read.
 *   x_split [49 R, K] (row pitch ldx): split layout x x_scale, ROI-major rows (r*49 + position); W1_split [C, K] x w1_scale;
 *   U_split [121, N, C] x u_scale; v_scale: operand scale of the transformed pixels; flags: LOCOV_WINO_IN_ROI_MAJOR (required)
 *   | LOCOV_WINO_OUT_ROI_MAJOR | LOCOV_EPI_RELU (of the 3x3); y, ldy, y_split_scale as in locov_winograd_conv3x3_f32_split_ex.
 *   workspace: locov_conv1x1_winograd_workspace_bytes_for(R, K, C, N, ldx) bytes -- the transform-domain workspace, plus the
 *   [49 R, C] pixel scratch only when these shapes take the two-launch fallback; locov_conv1x1_winograd_workspace_bytes(R, C, N)
 *   is the upper bound over both forms (always sufficient). */
int64_t locov_conv1x1_winograd_workspace_bytes(int64_t R, int C, int N);
int64_t locov_conv1x1_winograd_workspace_bytes_for(int64_t R, int K, int C, int N, int64_t ldx);
/* The same for block 0, whose 1x1 convolution ran on the feature MAP (ROIAlign is linear): the pooler + FrozenBN + ReLU + conv2 in one
 * call -- locov_roi_align_nhwc_affine_fwd(bin_stride 2, ROI-major, relu) followed by locov_winograd_conv3x3_f32_split_ex, and those
 * bits.  With C % 64 == 0 the ROIAlign workgroup (one ROI x 64 channels) keeps its 49 pooled rows in LDS and writes their Winograd
 * input transform itself; otherwise the two launches.  feat_nhwc: fp32 [Nimg, H, W, C] with pixel pitch feat_ld; pooled: 14 (the
 * even bins form the 7 x 7 tile); workspace: locov_roi_align_winograd_workspace_bytes(R, C, N) (the pixel scratch only for the
 * two-launch fallback; locov_conv1x1_winograd_workspace_bytes is the upper bound); the other arguments as above. */
int64_t locov_roi_align_winograd_workspace_bytes(int64_t R, int C, int N);
int locov_roi_align_winograd_conv3x3_f32_split(const float *feat_nhwc, int Nimg, int H, int W, int C, int64_t feat_ld,
                                               const float *rois, int64_t R, int pooled, float spatial_scale,
                                               int sampling_ratio, int aligned, const float *scale1, const float *shift1,
                                               const void *U_split, float u_scale, float v_scale, const float *scale2,
                                               const float *shift2, float *y, int64_t ldy, int N, unsigned flags,
                                               float y_split_scale, void *workspace, int64_t workspace_bytes,
                                               unsigned *overflow, locov_stream_t stream);
int locov_conv1x1_winograd_conv3x3_f32_split(const float *x_split, int64_t ldx, int K, float x_scale, const void *W1_split,
                                             float w1_scale, const float *scale1, const float *shift1, int64_t R, int C,
                                             const void *U_split, float u_scale, float v_scale, const float *scale2,
                                             const float *shift2, float *y, int64_t ldy, int N, unsigned flags,
                                             float y_split_scale, void *workspace, int64_t workspace_bytes,
                                             unsigned *overflow, locov_stream_t stream);

int64_t locov_winograd_wgrad_workspace_bytes(int64_t R, int Cin, int N);
int locov_winograd_wgrad_f32(const float *x, const float *g, int64_t R, int Cin, int N, unsigned flags,
                             const float *row_scale, float *dw, void *workspace, int64_t workspace_bytes,
                             locov_stream_t stream);

/* Every split-operand form of the Res5 convolution weights a training step needs, in ONE launch (csrc/weight_prep.hip).
 * The LSM configuration trains the Res5 convolutions (configs/coco_lsm.yaml:8), so each step re-derives, per 1x1 convolution,
 * W [N,K] (forward, roi_emb_heads.py:323,343) and (s W)^T [K,N] (data gradient); per 3x3 convolution the Winograd-domain
 * filter of the proposals' 7x7 tiles, the im2col filter of the whole-grid call, and both forms of the flipped filter
 * flip(s w) -- each in the (hi, lo) f16 split layout of locov_split_f16x2_pack, scaled by `scale` (a power of two).  One job =
 * one operand; results are bit-identical to locov_weight_transpose_scale / locov_conv3x3_weight_flip /
 * locov_winograd_pack_weight / locov_pack_conv3x3_weight followed by locov_split_f16x2_pack.  `overflow` as there. */
#define LOCOV_WEIGHT_PREP_MAX_JOBS 32
enum {
    LOCOV_PREP_PLAIN = 0,       /* w [N,K]                -> [N,K]                        (K % 32 == 0)   */
    LOCOV_PREP_TRANSPOSE = 1,   /* w [N,K], s[N]          -> [K,N] = (s w)^T              (N % 32 == 0)   */
    LOCOV_PREP_IM2COL = 2,      /* w [N,Cin,3,3]          -> [N, 9 Cin], column = tap * Cin + c   (Cin % 32 == 0) */
    LOCOV_PREP_IM2COL_FLIP = 3, /* w [N,Cin,3,3], s[N]    -> [Cin, 9 N] of flip(s w)      (N % 32 == 0)   */
    LOCOV_PREP_WINO = 4,        /* w [N,Cin,3,3]          -> U [121, N, Cin]              (Cin % 32 == 0) */
    LOCOV_PREP_WINO_FLIP = 5    /* w [N,Cin,3,3], s[N]    -> U [121, Cin, N] of flip(s w) (N % 32 == 0)   */
};
typedef struct locov_weight_prep_job {
    const float *w;             /* the convolution weight as stored (device) */
    const float *row_scale;     /* FrozenBN scale s[n] (device) or NULL */
    void *out;                  /* destination, same byte size as the fp32 operand would have (device) */
    float scale;                /* power-of-two operand scale */
    int kind, N, K;             /* K = Cin for the 3x3 kinds */
} locov_weight_prep_job;
int locov_res5_weight_prep(const locov_weight_prep_job *jobs, int n_jobs, unsigned *overflow, locov_stream_t stream);

int locov_weight_transpose_scale(const float *w, int N, int K, const float *row_scale, float *out,
                                 locov_stream_t stream);
int locov_conv3x3_weight_flip(const float *w, int N, int Cin, const float *row_scale, float *out,
                              locov_stream_t stream);
int locov_im2col3x3_nhwc(const float *x, int64_t R, int H, int W, int C, float *col, locov_stream_t stream);
int locov_conv3x3_wgrad_unpack(const float *dw_packed, int N, int Cin, const float *row_scale, float *dw,
                               locov_stream_t stream);
int locov_relu_mask(const float *g, const float *act, int64_t n, float *out, float *amax_out, locov_stream_t stream);
/* locov_zero_if_raised : the GradScaler-style skip of a backward pass in split arithmetic, decided ON THE DEVICE.  `flag` is the
 *                          pass's range-guard word (Res5RowsFn.backward -- the gradients of roi_emb_heads.py:323,343-347's Res5
 *                          calls, which the reference's cuDNN autograd computes in fp32 and cannot overflow): when it is non-zero
 *                          each of the n_tensors (<= LOCOV_ZERO_LIST_MAX) fp32 gradient tensors (`tensors[i]`, `counts[i]` elements;
 *                          host arrays of device pointers / counts) is zero-filled, so that no inf / NaN produced beyond fp16's range
 *                          reaches an optimizer step or DDP's all-reduce; when it is zero nothing is read or written.  One launch,
 *                          no host read -- the caller learns of the skip from the word whenever it next reads it. */
#define LOCOV_ZERO_LIST_MAX 24
int locov_zero_if_raised(float *const *tensors, const int64_t *counts, int n_tensors, const unsigned *flag,
                         locov_stream_t stream);

int locov_spatial_mean_bwd(const float *g, const float *act, int64_t R, int C, int HW, float *out,
                           float *amax_out, locov_stream_t stream);
int locov_rows_stride2(const float *src, int N, int H, int W, int C, int forward, float *dst,
                       locov_stream_t stream);
int locov_roi_align_nhwc_bwd(const float *grad_rows, int64_t grad_ld, int N, int H, int W, int C,
                             const float *rois, int64_t R, int pooled_h, int pooled_w, float spatial_scale,
                             int sampling_ratio, int aligned, int bin_stride, int pos_major, float *grad_feat,
                             locov_stream_t stream);

/* The grounding branches' region dictionaries (csrc/regions.hip): what ovr/modeling/meta_arch/distill_prop_mmss_gcnn.py:273-328
 * (`input_image`: the whole-image grid) and :348-399 (`input_boxes`: the sampled boxes) assemble on the host with numpy loops, one
 * fancy-index per image, pad_sequence and blocking torch.tensor(numpy).cuda() copies -- here one selection launch and one gather
 * launch per branch, one scatter launch per branch backward, no host wait.
 *
 * locov_regions_select : per image i (one workgroup; B <= LOCOV_REGIONS_MAX_B, everything per-image is a HOST array passed on as
 *     launch arguments), slot r receives the valid candidate with the r-th smallest (key, candidate index) pair -- the first
 *     slots of a stable argsort of the keys over the valid candidates, which stands in for np.random.shuffle (:308, :358).
 *       mode LOCOV_REGIONS_GRID     :302-320.  count_host[i] = gh * gw cells (row-major, grid_w = gw); a cell (y, x) is valid when
 *                                   y < ext_a_host[i] and x < ext_b_host[i] (the extents of :281-284, formed by the caller);
 *                                   image i fills min(limit, valid_i) slots (limit = SPATIAL_DROPOUT); loc = ((x + 0.5) /
 *                                   ext_b, (y + 0.5) / ext_a) (:293-296).
 *       mode LOCOV_REGIONS_GRID_ALL :285-300 without the subsampling of :302: n = mask_w = gh * gw, slot = cell, mask = the valid
 *                                   extent, loc = 0 outside it; keys / indices / src_row / inv are not touched (may be NULL).
 *       mode LOCOV_REGIONS_BOXES    :349-391.  count_host[i] = boxes of image i (all valid), boxes_host[i] = its [count, 4]
 *                                   fp32 XYXY boxes (a HOST array of device pointers), ext_a_host / ext_b_host = image height /
 *                                   width; n <= every count; loc = ((x0 + x1) / 2 / width, (y0 + y1) / 2 / height) (:368-383).
 *     keys [sum count] float64 (finite), image after image.  Outputs: indices [B, n] int64 (candidate of each slot within its
 *     image, -1 = padding), src_row [B, n] int32 (the same as a row of the concatenated candidates), inv [sum count] int32
 *     (candidate -> output row i * n + slot, -1 = not selected; what the backward reads), mask [B, mask_w] uint8 (1 for the filled
 *     slots: `new_mask` :305 has width SPATIAL_DROPOUT, which may exceed n), loc [B, n, 2] fp32 (0 for padding, as pad_sequence
 *     writes), mvm [B, mvm_w] fp32 zeros (`mvm_mask`, :326 / :397).  The quotients are IEEE fp32 divisions.
 *     More than LOCOV_REGIONS_MAX_CANDIDATES candidates in one image (the keys' LDS budget) -> LOCOV_ERR_UNSUPPORTED.
 * locov_regions_gather_fwd : out [B * n, C] = the source row src_row names, zeros where it is -1 (pad_sequence, :314 / :385).
 *     layout LOCOV_REGIONS_ROWS: source row s at src + s * ld (channels-last grid features, box features; 16-byte lanes when
 *     C % 4 == 0 and everything is 16-byte aligned); LOCOV_REGIONS_NCHW: src is [B, C, hw] contiguous and s = i * hw + cell.
 * locov_regions_gather_bwd : the gradient of that w.r.t. the source, in the source's layout: grad_src ([rows, C] with row pitch ld |
 *     [rows / hw, C, hw]) is written EVERYWHERE exactly once -- row inv[s] of grad_out [B * n, C], or zero -- no memset, no atomic. */
#define LOCOV_REGIONS_MAX_B 64
#define LOCOV_REGIONS_MAX_CANDIDATES 4096
#define LOCOV_REGIONS_GRID 0
#define LOCOV_REGIONS_GRID_ALL 1
#define LOCOV_REGIONS_BOXES 2
#define LOCOV_REGIONS_ROWS 0
#define LOCOV_REGIONS_NCHW 1
int locov_regions_select(const double *keys, int mode, int B, const int *count_host, const int *ext_a_host,
                         const int *ext_b_host, int grid_w, const float *const *boxes_host, int n, int limit, int mask_w,
                         int mvm_w, int64_t *indices, int *src_row, int *inv, uint8_t *mask, float *loc, float *mvm,
                         locov_stream_t stream);
int locov_regions_gather_fwd(const float *src, int layout, int64_t ld, int B, int n, int C, int64_t hw, const int *src_row,
                             float *out, locov_stream_t stream);
int locov_regions_gather_bwd(const float *grad_out, int layout, int64_t ld, int64_t rows, int C, int64_t hw, const int *inv,
                             float *grad_src, locov_stream_t stream);

/* ---- fused multi-head self-attention core (csrc/mha.hip): TransformerHead's BERT layers ------------------------------------
 * (ovr/modeling/mmss_heads/transformer_head.py:170-176 -> BertSelfAttention).  Added under ABI version 8.
 *
 *   ctx = dropout(softmax(Q K^T * scale + bias[n, key])) V      for every (sequence n < Nseq, head h < H)
 *
 *   q, k, v, ctx : fp32 [Nseq * S, H * d], row pitches ldq / ldk / ldv / ldo in floats (the operands may be column blocks of one
 *                  [Nseq * S, 3 H d] matrix, or separate tensors); head h is columns [h * d, (h + 1) * d).
 *   bias         : fp32 [Nseq, S], finite; added per key, broadcast over heads and queries (the reference passes its 0 / 1
 *                  attention mask here, so padded keys are down-weighted, not excluded).
 *   keep, p_drop : optional dropout: uint8 [Nseq, H, S, S] keep mask ([n][h][query][key]) drawn by the caller; kept
 *                  probabilities are multiplied by 1 / (1 - p_drop).  keep == NULL: no dropout (p_drop is not read).
 *   lse          : out, fp32 [Nseq, H, S]: log-sum-exp of the biased, scaled scores of each query (what the backward reads).
 *   Products on v_mfma_f32_32x32x2_f32, softmax in fp32 with the running maximum subtracted; no S x S tensor is written.
 *
 * locov_mha_bwd: dq, dk, dv (pitches lddq / lddk / lddv) from dctx (pitch ldo) -- the probabilities are recomputed from q, k,
 *   bias and lse with the same keep mask; ctx is not needed.  delta: fp32 [Nseq, H, S] scratch (sum_k P dP of each query row,
 *   written by the first of the two launches, read by the second).  No atomics: each output row is summed by one wave in a fixed
 *   order, so the result is bitwise reproducible.  No gradient for bias.
 *
 * Supported: 1 <= S <= LOCOV_MHA_MAX_S, d in {32, 64, 96, 128}, Nseq, H <= LOCOV_MHA_MAX_GRID; anything else is
 *   LOCOV_ERR_UNSUPPORTED.  Pointers 16-byte aligned, pitches multiples of 4 floats and >= H * d, else LOCOV_ERR_INVALID_ARG.
 *   Every check happens before the first launch; no host wait. */
#define LOCOV_MHA_MAX_S 4096
#define LOCOV_MHA_MAX_GRID 65535
int locov_mha_fwd(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv, const float *bias,
                  const uint8_t *keep, float p_drop, float scale, int nseq, int S, int H, int d, float *ctx, int64_t ldo,
                  float *lse, locov_stream_t stream);
int locov_mha_bwd(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv, const float *bias,
                  const uint8_t *keep, float p_drop, float scale, int nseq, int S, int H, int d, const float *dctx,
                  int64_t ldo, const float *lse, float *delta, float *dq, int64_t lddq, float *dk, int64_t lddk, float *dv,
                  int64_t lddv, locov_stream_t stream);

/* ---- the ResNet stem in one launch (csrc/resnet_stem.hip): the front of the C4 backbone -----------------------------------
 * ([D2-upstream] detectron2.modeling.backbone.resnet.BasicStem; the reference tree has no source for it).  Added under ABI
 * version 8.
 *
 *   CH = (H + 1) / 2, CW = (W + 1) / 2, PH = (CH + 1) / 2, PW = (CW + 1) / 2
 *   c[n, k, i, j] = sum_{c, u, v} x[n, c, 2 i - 3 + u, 2 j - 3 + v] w[k, c, u, v]        (zero outside the image)
 *   a             = relu(c * scale[k] + shift[k])                                        (the FrozenBN fold)
 *   y[n, p, q, k] = max a[n, k, i, j] over i in {2p - 1, 2p, 2p + 1} within [0, CH), j likewise within [0, CW)
 *
 *   x     : fp32 [N, 3, H, W], NCHW, contiguous.
 *   w     : fp32 [Cout, 3, 7, 7] as conv1.weight stores it (16-byte aligned); scale, shift: fp32 [Cout].
 *   y     : out, fp32 [N, PH, PW, Cout] channels-last (16-byte aligned): the pixel rows the GEMM kernels take.
 *   A conv row CH or column CW (an odd CH / CW puts one next to the last window) does not exist: it is left out of the maximum,
 *   not computed from zero padding.  Exact fp32 products, fp32 accumulation; the conv intermediate stays on chip.  No atomics;
 *   an image's result does not depend on N or on the other images of the launch.
 * Supported: Cout == 64.  Cout != 64, N < 0, H or W <= 0, a null or misaligned pointer, sizes whose element offsets leave int64 or
 *   whose tiles leave the launch grid: LOCOV_ERR_INVALID_ARG before any launch.  N == 0: LOCOV_OK, nothing is read or written. */
int locov_resnet_stem_fwd(const float *x, int N, int H, int W, const float *w, const float *scale, const float *shift, int Cout,
                          float *y, locov_stream_t stream);

/* ---- the stem under autograd (csrc/resnet_stem.hip): its only trainable tensor is conv1.weight -------------------------------
 * Added under ABI version 8.
 *
 * locov_resnet_stem_fwd_sel: the training forward.  The same kernel as locov_resnet_stem_fwd -- y is bit-identical -- that also
 * writes, per pooled element, which conv position its gradient goes to:
 *   sel   : out, uint8 [N, PH, PW, Cout].  3 di + dj (0 .. 8): the conv position (2p - 1 + di, 2q - 1 + dj) that FIRST attains the
 *           window maximum in row-major scan (torch's max-pool rule) when that maximum is > 0; 9 when the pooled value is 0
 *           (nothing passes the ReLU).  Only positions that exist (0 <= row < CH, 0 <= column < CW) compete.
 *   Everything else, and every error, as locov_resnet_stem_fwd (sel must not be null).
 *
 * locov_resnet_stem_wgrad: the weight gradient.
 *   gconv[n, i, j, o] = sum of g[n, p, q, o] over the (up to four) windows (p, q) whose sel names conv position (i, j)
 *   dw[o, c, u, v]    = scale[o] * sum_{n, i, j} gconv[n, i, j, o] x[n, c, 2 i - 3 + u, 2 j - 3 + v]      (zero outside the image)
 *   x     : fp32 [N, 3, H, W], NCHW, contiguous (the forward's).
 *   g     : fp32 [N, PH, PW, Cout]: the gradient of the pooled map y, channels-last.
 *   sel   : uint8 [N, PH, PW, Cout] of locov_resnet_stem_fwd_sel (an element with code 9 passes nothing, whatever its g).
 *   scale : fp32 [Cout], the FrozenBN fold's scale.
 *   dw    : out, fp32 [Cout, 3, 7, 7] (overwritten, not accumulated into).
 *   workspace: at least locov_resnet_stem_wgrad_workspace_bytes(N, H, W) bytes, 4-byte aligned (per-workgroup partials; at most
 *           512 x 147 x 64 floats whatever N is).
 *   fp32 products and accumulation.  Per-wave partial sums are reduced in a fixed order (in the workgroup through LDS, across
 *   workgroups by a second small launch): no atomics, two calls give the same bits, nothing is read by the host.
 * Supported: Cout == 64.  Cout != 64, N < 0, H or W <= 0, a null or misaligned pointer, sizes whose element offsets leave int64,
 *   a workspace that is too small: LOCOV_ERR_INVALID_ARG before any launch.  N == 0: LOCOV_OK, nothing is read or written.
 * locov_resnet_stem_wgrad_workspace_bytes: 0 for N <= 0 or H, W <= 0. */
int locov_resnet_stem_fwd_sel(const float *x, int N, int H, int W, const float *w, const float *scale, const float *shift, int Cout,
                              float *y, uint8_t *sel, locov_stream_t stream);
int64_t locov_resnet_stem_wgrad_workspace_bytes(int N, int H, int W);
int locov_resnet_stem_wgrad(const float *x, int N, int H, int W, const float *g, const uint8_t *sel, const float *scale, int Cout,
                            float *dw, void *workspace, int64_t workspace_bytes, locov_stream_t stream);

/* ---- the two ends of the detector call, one launch each for the whole batch (csrc/image_batch.hip) ---------------------------
 * Added under ABI version 8.  What the meta-architecture does around backbone -> RPN -> ROI heads (ovr/modeling/meta_arch/
 * ovr_rcnn.py:45,101,122; [D2-upstream] GeneralizedRCNN.preprocess_image / _postprocess, detector_postprocess).
 *
 * locov_preprocess_images: out[n, c, y, x] = (float(image_n[c, y, x]) - mean[c]) / std[c] inside image n, pad_value outside it.
 *   images_host : host array of n_images DEVICE pointers; image n is [channels, heights_host[n], widths_host[n]], contiguous, of
 *                 element type `dtype` (LOCOV_IMAGE_U8 or LOCOV_IMAGE_F32, one type per call), aligned to its element size only.
 *   mean_host, std_host : host arrays of `channels` (1 .. LOCOV_IMAGE_MAX_CHANNELS) floats.
 *   out         : fp32 [n_images, channels, Hb, Wb], 16-byte aligned.  EVERY element is written (the padding too): the caller
 *                 need not clear it.  Hb * Wb < 2^31.
 *   The subtraction and the division are two separately rounded fp32 operations, the division IEEE-correct: the bits of the CPU
 *   torch expression (x - pixel_mean) / pixel_std followed by ImageList.from_tensors' padding (applied AFTER the normalisation).
 *   Every table travels as a kernel argument: one launch, no copy, no workspace, nothing read by the host.
 *   n_images == 0: LOCOV_OK, nothing is written.  More than LOCOV_LABEL_MAX_IMAGES images, a null pointer, an unknown dtype,
 *   channels outside 1 .. 4, an image larger than Hb x Wb, a misaligned out: LOCOV_ERR_INVALID_ARG before any HIP call.
 *
 * locov_detector_rescale: detector_postprocess' box part for the results of a batch: Boxes.scale, Boxes.clip, Boxes.nonempty.
 *   boxes       : fp32 [T, 4] XYXY, the images' results concatenated; image i owns rows [roff_host[i], roff_host[i + 1]).
 *   scale_x_host, scale_y_host : per image, the fp32 factors (output size / image size, formed by the caller).
 *   out_h_host, out_w_host     : per image, the output size the boxes are clipped to.
 *   out_boxes   : fp32 [T, 4] (not `boxes`).  Per row x * scale_x, y * scale_y (one fp32 product each), clamped to [0, out_w] /
 *                 [0, out_h] as torch.clamp does (NaN stays NaN); a row is kept iff (x2 - x1 > 0) & (y2 - y1 > 0).  The kept rows
 *                 of image i stand at the front of its segment, in their original order; the rest of the segment is zero.
 *   src         : int64 [T]: for a kept row, the row WITHIN its image it came from; -1 behind the image's count.
 *   counts      : int32 [n_images], device: the number of kept rows per image (the caller's one host read).
 *   One launch, one workgroup per image, any number of rows per image; vector stores only.  Two calls give the same bits.
 *   n_images == 0: LOCOV_OK.  More than LOCOV_LABEL_MAX_IMAGES images, a null pointer, a decreasing roff, misaligned boxes:
 *   LOCOV_ERR_INVALID_ARG before any HIP call.  (With T == 0 only `counts` is touched; boxes / out_boxes / src may be null.) */
#define LOCOV_IMAGE_U8 0
#define LOCOV_IMAGE_F32 1
#define LOCOV_IMAGE_MAX_CHANNELS 4
int locov_preprocess_images(const void *const *images_host, const int *heights_host, const int *widths_host, int n_images, int dtype,
                            int channels, const float *mean_host, const float *std_host, float pad_value, float *out, int Hb, int Wb,
                            locov_stream_t stream);
int locov_detector_rescale(const float *boxes, const int *roff_host, const float *scale_x_host, const float *scale_y_host,
                           const int *out_h_host, const int *out_w_host, int n_images, float *out_boxes, int64_t *src, int *counts,
                           locov_stream_t stream);

/* ---- the image side of the dataset mapper in one launch for the whole batch (csrc/image_resize.hip) ---------------------------
 * Added under ABI version 8.  What BasicTextImageDatasetMapper.__call__ (ovr/data/mappers/basic_mappers.py:116-124) does to the
 * decoded image under every shipped config: [D2-upstream] ResizeShortestEdge -> ResizeTransform.apply_image (Pillow's
 * Image.resize(..., BILINEAR) on uint8), RandomFlip -> HFlipTransform / VFlipTransform, then image.transpose(2, 0, 1).
 *
 * locov_resize_flip_images: out_n[c, y', x'] = resized_n[y, x, c], with (y', x') = (y, x), (y, ow - 1 - x) or (oh - 1 - y, x).
 *   images_host : host array of n_images DEVICE pointers; image n is uint8 [heights_host[n], widths_host[n], channels],
 *                 contiguous, aligned to one byte only.  One channel count (1 .. LOCOV_IMAGE_MAX_CHANNELS) per call.
 *   outs_host   : host array of n_images DEVICE pointers; output n is uint8 [channels, out_heights_host[n], out_widths_host[n]],
 *                 contiguous, aligned to one byte only, not overlapping any input.  EVERY byte of it is written, nothing else.
 *   flips_host  : per image LOCOV_FLIP_NONE, LOCOV_FLIP_HORIZONTAL or LOCOV_FLIP_VERTICAL, applied AFTER the resize.
 *   `resized` is Pillow's ImagingResample for 8-bit channels with the bilinear filter, bit for bit.  Per axis, in fp64 with every
 *   operation rounded on its own (scale = in / out, fs = max(scale, 1), support = fs):
 *     center = (xx + 0.5) * scale;  xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), in) - xmin
 *     w[x] = f((x + xmin - center + 0.5) * (1 / fs)), f(t) = 1 - |t| below 1 and 0 from there;  w[x] /= sum of the w[x] (if != 0)
 *     k[x] = (int)(w[x] * 2^22 + 0.5)   (- 0.5 for a negative weight; the conversion truncates)
 *   and each pass is clamp((2^21 + sum k[x] * pixel[xmin + x]) >> 22, 0, 255) in int32.  The horizontal pass comes first and its
 *   ROUNDED bytes are what the vertical pass reads; a pass between equal sizes is the identity by these formulas.
 *   The taps are formed on the device from the sizes: no coefficient upload, no workspace, nothing read by the host.  One launch:
 *   a workgroup owns 16 x 64 output pixels of one image and keeps the horizontal pass of the source rows its band needs in LDS.
 *   No atomics; vector stores only; two calls give the same bits.
 *   Supported: every upscale, and every downscale of at most LOCOV_RESIZE_MAX_TAPS taps per axis, i.e. ceil(in / out) <= 8 (a
 *   factor of 8 per axis); locov_resize_supported answers for one image without a launch (1 / 0).
 *   n_images == 0: LOCOV_OK, nothing is touched.  More than LOCOV_LABEL_MAX_IMAGES images, a null pointer, a size < 1, channels
 *   outside 1 .. 4, an unknown flip, more taps than the limit, h * w * channels or oh * ow * channels above 2^31 - 1 (the kernel's
 *   offsets within an image are int32 quantities): LOCOV_ERR_INVALID_ARG before any HIP call. */
#define LOCOV_RESIZE_MAX_TAPS 17
#define LOCOV_FLIP_NONE 0
#define LOCOV_FLIP_HORIZONTAL 1
#define LOCOV_FLIP_VERTICAL 2
int locov_resize_supported(int in_h, int in_w, int out_h, int out_w, int channels);
int locov_resize_flip_images(const void *const *images_host, const int *heights_host, const int *widths_host, void *const *outs_host,
                             const int *out_heights_host, const int *out_widths_host, const int *flips_host, int n_images, int channels,
                             locov_stream_t stream);

/* ---- the strong augmentation of the dataset mapper for the whole batch (csrc/image_augment.hip) -------------------------------
 * Added under ABI version 8.  What BasicTextImageDatasetMapper.__call__ (ovr/data/mappers/basic_mappers.py:171-180) does with the
 * Compose of build_complete_augmentation (ovr/data/detection_utils.py:60-100) AFTER the resize and flip: torchvision's ColorJitter,
 * RandomGrayscale, the reference's GaussianBlur (Pillow's ImageFilter.GaussianBlur) and three RandomErasing between ToTensor and
 * ToPILImage.  The draws are made by the caller; the bytes are Pillow's and torch's, bit for bit.
 *
 * locov_augment_images:
 *   images_host : host array of n_images DEVICE pointers; image n is uint8 [3, height, width] PLANAR (what
 *                 locov_resize_flip_images writes), contiguous, aligned to one byte only.  Plane 0 plays R.
 *   outs_host   : host array of n_images DEVICE pointers to outputs of the same shape, each distinct from every input (the blur
 *                 reads a pixel's neighbours).  EVERY byte of an output is written, nothing else.
 *   descs_host  : host array of n_images locov_augment_desc, one image's draws each:
 *     height, width : the image's size.
 *     n_ops, ops  : the colour jitter, 0 .. 4 DISTINCT operations LOCOV_AUG_OP_* in the order they run (n_ops == 0: no jitter).
 *     brightness, contrast, saturation : ImageEnhance's factors, i.e. Image.blend(degenerate, image, f): in fp32
 *                   t = d + f * (x - d), the product rounded before the sum; for 0 <= f <= 1 the byte is (int)t, otherwise 0 for
 *                   t <= 0, 255 for t >= 255, else (int)t.  d is 0 (brightness), the pixel's L (saturation) and
 *                   (int)(sum(L) / (height * width) + 0.5), the division in fp64, over the WHOLE image as it stands when contrast
 *                   runs.  L = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16.
 *     hue_shift   : 0 .. 255, added modulo 256 to H between Pillow's convert("HSV") and convert("RGB"), which run even for 0.
 *                   RGB -> HSV: v = max; max == min gives h = s = 0; else in fp32 cr = max - min, s = cr / max, rc = (max - r) / cr
 *                   (gc, bc alike), h = bc - gc | 2 + rc - bc | 4 + gc - rc for r, g or b the maximum (tested in that order), summed
 *                   in fp64 from the fp32 terms and rounded to fp32, h = fmod(h / 6 + 1, 1) in fp64 rounded to fp32, and the bytes
 *                   are (int)((double)h * 255), (int)((double)s * 255).  HSV -> RGB in fp64: s == 0 gives grey v; else fs = s / 255,
 *                   i = floor(h * 6 / 255), f = h * 6 / 255 - i, p = floor(v * (1 - fs) + 0.5), q = floor(v * (1 - fs * f) + 0.5),
 *                   t = floor(v * (1 - fs * (1 - f)) + 0.5), and i % 6 selects (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q).
 *     gray        : non-zero writes L to all three planes, after the jitter.
 *     sigma       : 0 for no blur, else ImageFilter.GaussianBlur(radius = sigma): with s2 = sigma * sigma / 3 (fp32),
 *                   L = (float)sqrt(12.0 * s2 + 1.0), l = (float)floor((L - 1.0) / 2.0), a = (2l + 1)(l(l + 1) - 3 s2) / (6 (s2 -
 *                   (l + 1)^2)) in fp32, the box radius is fr = l + a.  Three horizontal box passes, then three vertical, each
 *                   writing rounded bytes the next one reads: radius = (int)fr, ww = (uint32)(2^24 / (fr * 2 + 1)) (fp32 division),
 *                   fw = (2^24 - (2 radius + 1) ww) / 2, out[x] = (ww * sum(in[x - radius .. x + radius]) + fw * (in[x - radius - 1]
 *                   + in[x + radius + 1]) + 2^23) >> 24 in uint32, indices clamped to the line.
 *     n_erase, erase : 0 .. LOCOV_AUG_MAX_ERASERS rectangles (i, j, eh, ew) inside the image (an empty one is allowed), applied in
 *                   order, so a later one wins.  Eraser e takes its [3, eh, ew] fp32 values, plane-major, from `noise` at
 *                   noise_offset + 3 * (the areas of the erasers before it), and writes (int)(v * 255.0f) & 255.
 *     noise_offset : the image's first element in `noise`.
 *   noise       : device, fp32 [n_noise], aligned to 4 bytes; may be NULL when no eraser reads it.
 *   workspace   : device, aligned to 16 bytes, locov_augment_images_workspace_bytes(descs_host, n_images) bytes: the derived
 *                 per-image table (copied there from the host on `stream`) and the contrast partials.
 *   The table's copy is a hipMemcpyAsync from PAGEABLE host memory: the library's buffer is free once the call returns, but the
 *   runtime may make the host wait until `stream` has drained before it stages the bytes, so the call is ordered on `stream`
 *   without being asynchronous to the host (no pinned staging buffer is kept).
 *   At most two launches and one host-to-device copy on `stream`, nothing read by the host: (1), only when some image's chain has
 *   contrast, a workgroup redoes the operations before contrast on 4 096 pixels and writes their INTEGER sum of L to the workspace;
 *   (2) a workgroup owns 32 x 64 output pixels, sums its image's partials, loads the tile with a halo of 3 * ((int)fr + 1) pixels
 *   per side, runs jitter and grayscale in registers, the six box passes in LDS and substitutes the erasers' bytes at the store.
 *   No atomics; no floating-point reduction; vector stores only; two calls give the same bits.
 *   Supported sigma: (int)fr + 1 <= 2, which holds for 0 < sigma up to about 2.449 and so for the reference's [0.1, 2.0];
 *   locov_augment_supported answers without a launch (1 / 0).
 *   n_images == 0: LOCOV_OK, nothing is touched.  More than LOCOV_LABEL_MAX_IMAGES images, a null pointer, an output that is its
 *   input, a size < 1, height * width * 3 above 2^31 - 1, an unknown or repeated operation, a factor that is not finite, hue_shift
 *   outside 0 .. 255, a sigma that is neither 0 nor supported, more erasers than the maximum, a rectangle outside the image, noise
 *   read before 0 or past n_noise, a misaligned or too small workspace: LOCOV_ERR_INVALID_ARG before any HIP call. */
#define LOCOV_AUG_OP_BRIGHTNESS 1
#define LOCOV_AUG_OP_CONTRAST 2
#define LOCOV_AUG_OP_SATURATION 3
#define LOCOV_AUG_OP_HUE 4
#define LOCOV_AUG_MAX_ERASERS 3
typedef struct locov_augment_desc {
    int32_t height, width;
    int32_t n_ops, ops[4];
    float brightness, contrast, saturation;
    int32_t hue_shift, gray;
    float sigma;
    int32_t n_erase, erase[LOCOV_AUG_MAX_ERASERS][4];
    int64_t noise_offset;
} locov_augment_desc;
int locov_augment_supported(float sigma);
int64_t locov_augment_images_workspace_bytes(const locov_augment_desc *descs_host, int n_images);
int locov_augment_images(const void *const *images_host, void *const *outs_host, const locov_augment_desc *descs_host, int n_images,
                         const float *noise, int64_t n_noise, void *workspace, int64_t workspace_bytes, locov_stream_t stream);

/* ---- the proposal side of the dataset mapper in one launch for the whole batch (csrc/proposal_map.hip) ------------------------
 * Added under ABI version 8.  What the mapper does with an image's precomputed proposals under MODEL.LOAD_OBJ_PROPOSALS
 * (ovr/data/mappers/basic_mappers.py:130-133: [D2-upstream] transform_proposals; coco_mappers.py:82-106: change_proposals_as_gt).
 *
 * locov_map_proposals:
 *   rows        : the STORE, device, [n_store_rows, 5] row-major, XYXY + objectness logit, fp32 (LOCOV_PROPOSAL_F32) or fp64
 *                 (LOCOV_PROPOSAL_F64), aligned to its element size.  Image i of the call owns the store rows
 *                 [row_start_host[i], row_start_host[i] + n_rows_host[i]); row_start_host (int64) may be in any order, with gaps.
 *   fx_host, fy_host : per image, the DOUBLE factors new_w * 1.0 / w and new_h * 1.0 / h (1.0 for no resize).  The kernel rounds
 *                 them once to the rows' dtype, as numpy does with a Python scalar beside an array.
 *   flips_host  : per image LOCOV_FLIP_NONE, LOCOV_FLIP_HORIZONTAL or LOCOV_FLIP_VERTICAL.
 *   new_h_host, new_w_host : per image, the size the boxes are flipped in and clipped to.
 *   Per row and axis, in the rows' dtype with every operation rounded on its own: both ends times the factor, their min / max
 *   (a NaN end makes both NaN, as ndarray.min does); on the flipped axis size - lo and size - hi and their min / max again; then
 *   ONE rounding to fp32, clamped to [0, size] as torch.clamp does (NaN stays NaN).  A row is kept iff (x2 - x1 > 0) & (y2 - y1 > 0)
 *   in fp32.  The proposal list of an image is its first `topk` kept rows in their original order; its pseudo-GT list is the subset
 *   of THAT list with (float)logit > thr.
 *   Outputs over T = sum of n_rows_host, image i's segment starting at the sum of the counts before it:
 *     prop_boxes fp32 [T, 4], prop_logits fp32 [T], prop_src int64 [T]; gt_boxes fp32 [T, 4], gt_logits fp32 [T], gt_classes
 *     int64 [T] (ones), gt_src int64 [T]; counts int32 [n_images, 2], device: (proposals, pseudo-GT) per image, the caller's one
 *     host read.  The lists stand at the front of the segment; behind the count the segment holds zeros, src is -1 and gt_classes
 *     is 0.  src is the row WITHIN the image.  EVERY output element is written.
 *   One launch, one workgroup per image, any number of rows per image; no atomics, vector stores only.  Two calls give the same bits.
 *   n_images == 0: LOCOV_OK, nothing is touched.  More than LOCOV_LABEL_MAX_IMAGES images, a null pointer, a negative count, size
 *   or topk, an unknown dtype or flip, rows outside the store, misaligned pointers (boxes 16 bytes, int64 outputs 8, the rest their
 *   element size), T above 2^31 - 1: LOCOV_ERR_INVALID_ARG before any HIP call.  (With T == 0 only `counts` is touched.) */
#define LOCOV_PROPOSAL_F32 0
#define LOCOV_PROPOSAL_F64 1
int locov_map_proposals(const void *rows, int64_t n_store_rows, int dtype, const int64_t *row_start_host, const int *n_rows_host,
                        const double *fx_host, const double *fy_host, const int *flips_host, const int *new_h_host,
                        const int *new_w_host, int n_images, int topk, float thr, float *prop_boxes, float *prop_logits,
                        int64_t *prop_src, float *gt_boxes, float *gt_logits, int64_t *gt_classes, int64_t *gt_src, int *counts,
                        locov_stream_t stream);

/* ---- the caption path of the LSM step in one launch (csrc/caption.hip): BertEmbedding after the tokenizer --------------------
 * (ovr/modeling/language/transf_models.py:105-154).  Added under ABI version 8.
 *
 * locov_caption_embed_fwd, for N = B * T tokens (flat position n = i * T + j):
 *   packed  : int32 [4, N]: input_ids, token_type_ids, attention_mask, special_tokens_mask as the tokenizer produced them.  The
 *             CALLER has validated 0 <= id < V and 0 <= type < type_vocab on the host (they are host integers before the upload).
 *   draws   : float64 [2, N], or NULL when masked language modelling is inactive (neither training nor ..._VALIDATION).
 *   The rule of :114-137, every comparison in double.  eligible = draws && !special && attention.  Eligible, u = draws[0][n]:
 *     u < p: mlm_mask = 1 and q = u / p; q < p_mask: id = mask_id, special = 1; else q < p_mask_noise (the HOST's double sum
 *     p_mask + p_noise): id = min((int)(draws[1][n] * len_tok), len_tok - 1); else the id stays.  u >= p, or not eligible: nothing
 *     changes and mlm_mask = 0.  target_ids is the id before the rule.
 *   ints    : out, int64 [int_rows, N]: input_ids, token_type_ids, attention_mask, special_tokens_mask and, with int_rows == 6,
 *             target_ids and mlm_mask.  int_rows is 4 (MASKED_LANGUAGE_MODELING off; draws must be NULL) or 6.
 *   W       : fp32 [V, H], the word table.  input_emb: out, fp32 [N, H] = W[input_ids] (the ids AFTER the rule), bit copies.
 *   P       : fp32 [max_pos, H] or NULL.  NULL (ADD_POSITION_EMBEDDING off): encoded_tokens has the values of input_emb and
 *             nothing else is read or written.  Otherwise, with Tt fp32 [type_vocab, H], gamma / beta fp32 [H] and eps:
 *               x = (W[id] + Tt[type]) + P[j];  mean = sum x / H;  rstd = 1 / sqrt(sum (x - mean)^2 / H + eps)
 *               encoded [N, H] = ((x - mean) * rstd * gamma + beta) * (keep ? keep[n, c] / (1 - p_drop) : 1)
 *             in fp32, the row in registers, both sums by wave shuffles; mean / rstd: out, fp32 [N] (what the backward reads).
 *   keep    : optional uint8 [N, H] keep mask drawn by the caller (the convention of locov_mha_fwd); NULL: no dropout.
 *   One launch, one wave per token; 16-byte lanes when H % 4 == 0 and every pointer is 16-byte aligned (keep: 4-byte), scalar
 *   lanes otherwise.  The kernel never reads outside the tables given valid ids: mask_id < V and len_tok <= V are checked here.
 *   N > LOCOV_CAPTION_MAX_TOKENS or H > LOCOV_CAPTION_MAX_HIDDEN: LOCOV_ERR_UNSUPPORTED, never a truncation.  A null pointer,
 *   N % T != 0, T > max_pos, mask_id >= V, len_tok > V, p outside (0, 1], p_drop outside [0, 1): LOCOV_ERR_INVALID_ARG.  Every
 *   check happens before any HIP call.  N == 0: LOCOV_OK, nothing is read or written.
 *
 * locov_caption_embed_bwd: dW [V, H], the gradient of the word table (the only trainable tensor, :156-164).
 *   ints    : the forward's output (rows 0 and 1 are read: the ids after the rule, the token types).
 *   g_in    : fp32 [N, H], gradient of input_emb (may be NULL on the LayerNorm path); g_enc: fp32 [N, H], gradient of encoded
 *             (LayerNorm path only; without it the caller passes the sum of its gradients as g_in).
 *   P, Tt, gamma, mean, rstd, keep, p_drop: as in the forward (P == NULL: the gather-only path).
 *   Three launches at most: the tokens are ranked by (id, flat position) by one workgroup (ids in LDS); on the LayerNorm path one
 *   wave per token forms dx = LN-backward(g_enc * keep / (1 - p_drop)) + g_in into the workspace; then one wave per vocabulary
 *   row binary-searches its run of tokens and writes 0.0f + their gradient rows, added in ascending flat position -- zeros for
 *   an id no token has.  No atomics, a fixed summation order, every element of dW written by the launch (no memset): two calls
 *   give the same bits.  workspace: locov_caption_embed_bwd_workspace_bytes(N, H, P != NULL) bytes, 16-byte aligned.
 *   Limits and errors as in the forward.  V == 0 or H == 0: LOCOV_OK.  N == 0: dW is written as zeros. */
#define LOCOV_CAPTION_MAX_TOKENS 8192
#define LOCOV_CAPTION_MAX_HIDDEN 4096
int locov_caption_embed_fwd(const int *packed, const double *draws, int N, int T, int H, int V, const float *W, const float *P,
                            int max_pos, const float *Tt, int type_vocab, const float *gamma, const float *beta, float eps,
                            const uint8_t *keep, float p_drop, double p, double p_mask, double p_mask_noise, int mask_id, int len_tok,
                            int int_rows, int64_t *ints, float *input_emb, float *encoded, float *mean, float *rstd,
                            locov_stream_t stream);
int64_t locov_caption_embed_bwd_workspace_bytes(int N, int H, int layer_norm);
int locov_caption_embed_bwd(const int64_t *ints, int N, int T, int H, int V, const float *W, const float *P, const float *Tt,
                            const float *gamma, const float *mean, const float *rstd, const uint8_t *keep, float p_drop,
                            const float *g_enc, const float *g_in, float *dW, void *workspace, int64_t workspace_bytes,
                            locov_stream_t stream);

/* ---- the optimiser step over a list of tensors (csrc/sgd.hip): torch.optim.SGD with Detectron2's per-parameter clipping --------
 * (ovr/engine/solver.py:27; [D2-upstream] maybe_add_gradient_clipping).  Added under ABI version 8.
 *
 * locov_sgd_step, per tensor of the table, in fp32 and in the order of torch.optim.SGD's single-tensor path:
 *     g'   = g                                              (LOCOV_SGD_CLIP_NONE)
 *          = clamp(g, -clip_value, clip_value)              (LOCOV_SGD_CLIP_VALUE; NaN stays NaN)
 *          = g * min(1, clip_value / (||g||_2 + 1e-6))      (LOCOV_SGD_CLIP_NORM; the norm of THIS tensor)
 *     d    = g' + wd * p                                    (skipped when wd == 0)
 *     buf' = d  if the record's FIRST flag is set, else  momentum * buf + (1 - dampening) * d        (skipped when momentum == 0)
 *     dd   = d + momentum * buf' (nesterov) | buf' (momentum) | d (momentum == 0)
 *     p'   = p - lr * dd
 *   g is never written.  Each a * b + c above is one fused multiply-add.  dampening is a double: 1 - dampening is formed in double
 *   and rounded to fp32 once, as torch forms its alpha.
 *   table       : DEVICE memory the caller owns, 16-byte aligned: n_tensors records of LOCOV_SGD_RECORD_BYTES bytes
 *                   { float *p; const float *g; float *buf; int64 n; int64 chunk0; int32 cls; int32 first; }
 *                 followed by int32 chunk_tensor[total_chunks].  A tensor of n >= 1 elements owns ceil(n / LOCOV_SGD_CHUNK)
 *                 consecutive chunks from chunk0 (record 0 at 0, no gaps), and chunk_tensor names each chunk's record.  p, g,
 *                 buf: fp32, contiguous, 4-byte aligned (16-byte aligned tensors move as 16-byte lanes, others as scalar lanes);
 *                 buf may be null when momentum == 0 and is not read when `first` is set.  0 <= cls < n_classes.  The entry
 *                 cannot read the table: its contents are the caller's responsibility.
 *   lr_host, wd_host : host arrays of n_classes (1 .. LOCOV_SGD_MAX_CLASSES) floats; they travel as kernel arguments.
 *   workspace   : LOCOV_SGD_CLIP_NORM only: locov_sgd_workspace_bytes(n_tensors, total_chunks) bytes, 8-byte aligned.
 *   Launches: one (clip none / value), three (norm: a fp64 sum of squares per chunk, the coefficient per tensor rounded once to
 *   fp32, the update).  No atomics, fixed summation order: two calls give the same bits.  Nothing is read by the host.
 *   n_tensors == 0 or total_chunks == 0: LOCOV_OK, nothing is launched.  A null table, a negative count or size, more than
 *   LOCOV_SGD_MAX_CLASSES classes, an unknown clip type, clip_value <= 0 with clipping on, nesterov with momentum == 0 or
 *   dampening != 0: LOCOV_ERR_INVALID_ARG before any HIP call. */
#define LOCOV_SGD_MAX_CLASSES 8
#define LOCOV_SGD_CHUNK 4096
#define LOCOV_SGD_RECORD_BYTES 48
#define LOCOV_SGD_CLIP_NONE 0
#define LOCOV_SGD_CLIP_VALUE 1
#define LOCOV_SGD_CLIP_NORM 2
int64_t locov_sgd_workspace_bytes(int n_tensors, int64_t total_chunks);
int locov_sgd_step(const void *table, int n_tensors, int64_t total_chunks, const float *lr_host, const float *wd_host, int n_classes,
                   float momentum, double dampening, int nesterov, int clip_type, float clip_value, void *workspace,
                   int64_t workspace_bytes, locov_stream_t stream);

/* ---- COCO-protocol box evaluation (csrc/coco_eval.hip): the public COCOeval, iouType "bbox", useCats 1 --------------------------
 * (what ovr/evaluation/custom_coco_eval.py:29 sits on).  Added under ABI version 8.  fp64 and integers only, each step rounded on
 * its own: the outputs equal the numpy definition in locov_amd/evaluation.py bit for bit, and two calls give the same bits.
 *
 * A CELL is one (image, category) pair; cells are numbered category-major (cell = category * n_images + image rank), so a
 * category's cells and dets are contiguous.  Both entry points only enqueue work; nothing is read by the host.
 *
 * locov_coco_match: greedy matching of every cell's dets to its gts, for every area range and IoU threshold.
 *   det_offsets, gt_offsets : int32 [n_cells + 1], CSR.  The entry cannot read them: the kernel clamps every offset into
 *                 [0, n_det] / [0, n_gt] and takes a descending pair as an empty cell, so no content can send it out of bounds.
 *   det_boxes   : fp32 [n_det, 4] XYXY in cell order, a cell's dets in descending score (ties in input order).  Only the first
 *                 max_det dets of a cell take part; the bits of the others are written as 0 (the accumulation never counts them:
 *                 their in-cell rank is above every cap).  XYWH is formed in fp32 (w = x2 - x1), then widened; area = w * h.
 *   gt_boxes    : fp64 [n_gt, 4] XYWH, gt_area fp64 [n_gt] (the annotation's own field), gt_crowd uint8 [n_gt], in cell order.
 *   area_ranges_host : n_areas (1 .. LOCOV_COCO_MAX_AREAS) pairs lo, hi;  iou_thresholds_host : n_thresholds (1 ..
 *                 LOCOV_COCO_MAX_THRESHOLDS) doubles.  They travel as kernel arguments.
 *   IoU (double): w = min(dx + dw, gx + gw) - max(dx, gx), h likewise; 0 if w <= 0 or h <= 0; else i = w * h,
 *                 u = crowd ? dw * dh : dw * dh + gw * gh - i;  IoU = i / u.
 *   Per (range a, threshold t), the dets in order: best = min(t, 1 - 1e-10); over the gts not ignored in a (ignored = crowd or
 *                 area outside [lo, hi]) and not yet matched at (a, t), in order, a gt with IoU >= best is taken and raises best
 *                 (equal IoU moves to the later gt); if none was taken, the same over the ignored gts, where a matched crowd gt can
 *                 be taken again.  The det takes the gt's ignore flag; an unmatched det with its area outside [lo, hi] is ignored.
 *   det_bits    : out uint8 [n_det, n_areas * n_thresholds]: bit 0 matched, bit 1 ignored.
 *   gt_ignore   : out uint8 [n_areas, n_gt].
 *   workspace   : locov_coco_match_workspace_bytes(n_gt, max_det) bytes, 8-byte aligned (needed when n_det > 0 and n_gt > 0): a
 *                 cell whose IoU matrix and matched flags exceed its 8 KiB of LDS keeps them there, at a slot given by its gt offset.
 *   max_det > LOCOV_COCO_MAX_DET or n_cells > 4 * LOCOV_COCO_MAX_BLOCKS: LOCOV_ERR_UNSUPPORTED.  n_cells == 0 or no det and no gt:
 *   LOCOV_OK, nothing launched.  A null pointer, a negative count, max_det < 1, a range with lo > hi, list lengths outside their
 *   limits, a small workspace: LOCOV_ERR_INVALID_ARG before any HIP call.
 *
 * locov_coco_accumulate: precision / recall / scores per (threshold, category, range, cap).
 *   cat_offsets : int32 [n_categories + 1] into the three acc_* arrays (clamped like the offsets above).
 *   acc_index, acc_rank, acc_score : per det, in (category, descending score, image rank, in-cell rank) order: its row of det_bits,
 *                 its in-cell rank, its score (fp64).  A det counts under cap m when acc_rank < max_dets_host[m].
 *   npig        : int32 [n_categories, n_areas]: the category's gts not ignored in the range.
 *   max_dets_host : 1 .. LOCOV_COCO_MAX_CAPS positive ascending caps;  recall_thresholds_host : 1 ..
 *                 LOCOV_COCO_MAX_RECALL_THRESHOLDS ascending doubles.
 *   Over the counted dets: tp / fp = running counts of the not-ignored matched / unmatched dets; rc = tp / npig;
 *                 pr = tp / (fp + tp + 2^-52), made non-increasing from the right; for recall threshold r the first det with
 *                 rc >= r gives precision and score, 0 once none does.  recall = the last rc, 0 with no det.
 *   precision, scores : out fp64 [T, R, K, A, M] (scores may be null);  recall : out fp64 [T, K, A, M].  Every element is written;
 *                 -1 where npig == 0.
 *   One workgroup per (category, range, cap, threshold) walks the category's dets in chunks with integer carries and a running
 *   maximum: no atomics.  More than LOCOV_COCO_MAX_BLOCKS workgroups: LOCOV_ERR_UNSUPPORTED.  n_categories == 0: LOCOV_OK.
 *   A null pointer, a negative count, more than LOCOV_COCO_MAX_CAPS caps, caps or recall thresholds not ascending:
 *   LOCOV_ERR_INVALID_ARG before any HIP call. */
#define LOCOV_COCO_MAX_AREAS 4
#define LOCOV_COCO_MAX_THRESHOLDS 16
#define LOCOV_COCO_MAX_CAPS 3
#define LOCOV_COCO_MAX_RECALL_THRESHOLDS 256
#define LOCOV_COCO_MAX_DET 4096
#define LOCOV_COCO_MAX_BLOCKS 8388608
int64_t locov_coco_match_workspace_bytes(int n_gt, int max_det);
int locov_coco_match(const int *det_offsets, const int *gt_offsets, int64_t n_cells, int n_det, int n_gt, int max_det,
                     const float *det_boxes, const double *gt_boxes, const double *gt_area, const uint8_t *gt_crowd,
                     const double *area_ranges_host, int n_areas, const double *iou_thresholds_host, int n_thresholds,
                     uint8_t *det_bits, uint8_t *gt_ignore, void *workspace, int64_t workspace_bytes, locov_stream_t stream);
int locov_coco_accumulate(const int *cat_offsets, int n_categories, const int *acc_index, const int *acc_rank,
                          const double *acc_score, int n_det, const uint8_t *det_bits, const int *npig, int n_areas,
                          int n_thresholds, const int *max_dets_host, int n_max_dets, const double *recall_thresholds_host,
                          int n_recall_thresholds, double *precision, double *recall, double *scores, locov_stream_t stream);

/* ---- LVIS-protocol box evaluation (csrc/coco_eval.hip): the public LVISEval, which Detectron2's LVISEvaluator sits on ------------
 * (what ovr/evaluation/evaluator.py:39-50 returns for every dataset whose name contains "lvis").  Added under ABI version 8.
 *
 * locov_lvis_match: locov_coco_match's kernel under the federated protocol; every argument it shares with locov_coco_match means
 * the same, its frame, limits, workspace (locov_coco_match_workspace_bytes) and error codes are the same.  The differences:
 *   gt_ignore_in : uint8 [n_gt], the annotation's own `ignore` field.  It stands where gt_crowd stood in the ignore test (a gt is
 *                 ignored in range a if gt_ignore_in or its area is outside [lo, hi]) and nowhere else: the IoU is always
 *                 i / (dw * dh + gw * gh - i), and a gt matched at (a, t) is never taken again, ignored or not.
 *   cell_flags  : uint8 [n_cells], bits LOCOV_LVIS_CELL_*: the image's neg_category_ids / not_exhaustive_category_ids.
 *                 An unmatched det is ignored if its area is outside [lo, hi] OR its cell is NOT_EXHAUSTIVE.
 *                 A cell with no gt and no NEG bit is UNLISTED: its dets are neither true nor false positives.  The first max_det
 *                 of them get bits 2 (unmatched, ignored) in every column; locov_coco_accumulate repeats its running counts
 *                 over such a det, so precision and recall are those of the dets without them (the `scores` output is not:
 *                 pass scores = NULL to locov_coco_accumulate).
 *   max_det     : the caller's cap; LVIS caps per image over all categories, which the caller applies before the cell order, so
 *                 no cell holds more.  The precision / recall arrays come from locov_coco_accumulate with the one cap max_det.
 *   A null cell_flags (with cells and a det or gt) or gt_ignore_in (with n_gt > 0): LOCOV_ERR_INVALID_ARG before any HIP call. */
#define LOCOV_LVIS_CELL_NEG 1            /* the category is in the image's neg_category_ids */
#define LOCOV_LVIS_CELL_NOT_EXHAUSTIVE 2 /* ... in its not_exhaustive_category_ids */
int locov_lvis_match(const int *det_offsets, const int *gt_offsets, const uint8_t *cell_flags, int64_t n_cells, int n_det, int n_gt,
                     int max_det, const float *det_boxes, const double *gt_boxes, const double *gt_area, const uint8_t *gt_ignore_in,
                     const double *area_ranges_host, int n_areas, const double *iou_thresholds_host, int n_thresholds,
                     uint8_t *det_bits, uint8_t *gt_ignore, void *workspace, int64_t workspace_bytes, locov_stream_t stream);

/* ---- Class-agnostic proposal recall (csrc/proposal_recall.hip): Detectron2's _evaluate_box_proposals ----------------------------
 * (what its COCOEvaluator / LVISEvaluator, which ovr/evaluation/evaluator.py:47-50 builds, report as "box_proposals": AR, ARs, ARm,
 * ARl at 100 and at 1000 proposals per image).  Added under ABI version 8.  fp32, each step rounded on its own, and integers: the
 * outputs equal proposal_recall_host in locov_amd/evaluation.py bit for bit, and two calls give the same bits.
 *
 * locov_proposal_recall: the greedy one-to-one matching of every image's proposals to its gts, for every area range and limit.
 *   prop_offsets, gt_offsets : int32 [n_images + 1], CSR by image.  The entry cannot read them: the kernel clamps every offset into
 *                 [0, n_prop] / [0, n_gt] and takes a descending pair as an empty image, so no content can send it out of bounds.
 *   prop_boxes  : fp32 [n_prop, 4] XYXY, an image's proposals in descending objectness (ties in input order); under limit l only
 *                 the first limits_host[l] of an image take part.  gt_boxes : fp32 [n_gt, 4] XYXY;  gt_area : fp32 [n_gt] (the
 *                 annotation's own field).  Both box arrays 16-byte aligned.  The boxes are finite.
 *   gt_skip     : uint8 [n_gt] or NULL: a gt with a nonzero byte is left out before anything else (COCO: iscrowd; LVIS: NULL).
 *   max_gt_per_image : the caller's statement of the largest gt count of one image; a longer segment is cut to it.
 *   area_ranges_host : n_areas (1 .. LOCOV_COCO_MAX_AREAS) pairs lo, hi;  limits_host : n_limits (1 ..
 *                 LOCOV_PROPOSAL_RECALL_MAX_LIMITS) positive ascending ints;  iou_thresholds_host : n_thresholds (1 ..
 *                 LOCOV_COCO_MAX_THRESHOLDS) floats.  They travel as kernel arguments.
 *   Per (image, range a, limit l): an image with no gt left after gt_skip, or with no proposal, is SKIPPED: all its counts are 0.
 *                 Otherwise num_pos = its gts with lo <= area <= hi (fp32), and min(P, num_pos) times: over the unused proposals x
 *                 unused gts in the range, the largest IoU (select_common.h's box_pairwise_iou), ties to the lowest gt, then to
 *                 the lowest proposal; the IoU is that step's overlap and both are used from then on.
 *   gt_overlaps : out fp32 [n_areas * n_limits, n_gt]: row a * n_limits + l holds, in each image's gt segment, the steps' overlaps
 *                 in match order, then zeros (the maxima never rise: the walk ends at the first 0).  Every element of a segment is
 *                 written.
 *   counts      : out int32 [n_images, n_areas * n_limits, n_thresholds + 1]: per threshold t the overlaps >= it (fp32 compare),
 *                 then num_pos.  Every element is written.  The totals are the integer sum over the images, the caller's.
 *   One workgroup per (image, range, limit); no atomics on global memory, no host read.  limits_host[last] >
 *   LOCOV_PROPOSAL_RECALL_MAX_LIMIT, max_gt_per_image > LOCOV_PROPOSAL_RECALL_MAX_GT or n_images * n_areas * n_limits >
 *   LOCOV_COCO_MAX_BLOCKS: LOCOV_ERR_UNSUPPORTED before any launch.  n_images == 0, or no proposal and no gt: LOCOV_OK, nothing
 *   launched.  A null pointer, a negative count, limits not ascending, a range with lo > hi, list lengths outside their limits, a
 *   misaligned pointer: LOCOV_ERR_INVALID_ARG before any HIP call. */
#define LOCOV_PROPOSAL_RECALL_MAX_LIMIT 2048 /* proposals per image: 16 B each in LDS */
#define LOCOV_PROPOSAL_RECALL_MAX_GT 1024    /* gts per image (COCO: below 100; LVIS: a few hundred) */
#define LOCOV_PROPOSAL_RECALL_MAX_LIMITS 4
int locov_proposal_recall(const int *prop_offsets, const int *gt_offsets, int n_images, int n_prop, int n_gt, int max_gt_per_image,
                          const float *prop_boxes, const float *gt_boxes, const float *gt_area, const uint8_t *gt_skip,
                          const float *area_ranges_host, int n_areas, const int *limits_host, int n_limits,
                          const float *iou_thresholds_host, int n_thresholds, float *gt_overlaps, int *counts, locov_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LOCOV_HIP_H */
