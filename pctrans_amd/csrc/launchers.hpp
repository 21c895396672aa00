// The host side of the library in one place: the single declaration of every launcher, device-preparation and kernel-choice
// function that crosses a translation unit, and the status and kernel-id names they speak in.  Every file that defines or
// calls one of them includes this header, so a definition that drifts from its declaration fails to compile in its own file.
//
// Status convention.  A launcher returns 0 on success, a positive hipError_t from the launch, or a negative status.  A negative
// status is one of the PCT_ERR_* names of include/pctrans_hip.h, with one exception that never crosses the C ABI:
// PCT_NOT_COVERED, "this kernel does not cover the call, try the next one", which the routers consume and c_abi.hip
// translates (abi_status) where a launcher without a fallback hands it up.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pctrans_hip.h"

namespace pct {

constexpr int PCT_NOT_COVERED = -100;

// MSDeformAttn kernel ids: what pct_msda_set_kernel_choice / pct_msda_set_bwd_kernel_choice take (AUTO = follow the routing)
// and pct_msda_last_kernel / pct_msda_last_bwd_kernel report.  The numbers are part of the ABI's diagnostics.
enum MsdaFwdKernel { MSDA_FWD_AUTO = 0, MSDA_FWD_WIN = 1, MSDA_FWD_GENERIC = 2, MSDA_FWD_QUAD = 3, MSDA_FWD_COL = 4 };
enum MsdaBwdKernel { MSDA_BWD_AUTO = 0, MSDA_BWD_WIN = 1, MSDA_BWD_GENERIC = 2, MSDA_BWD_COL = 3 };

// ---- MSDeformAttn: one call = one struct.  Every launch_msda_* takes it by const reference; what only one launcher needs
// (`planes`, `forced`) comes as an extra argument.  value / out are of the launcher's storage type, loc / attn of its
// accumulator type (float, or double for the fp64 kernels).
// ref != nullptr: fused front-end (loc = raw offsets, attn = raw logits, ref = reference points, images ref_batch_stride
// floats apart) -----------------------------------------------------------------------------------------------------------
struct MsdaFwdCall {
  const void *value;
  const int64_t *shapes, *starts;
  const void *loc, *attn;
  int N, S, M, D, L, Lq, P;
  void *out;
  hipStream_t stream;
  const float *ref;
  long long ref_batch_stride;

  // the same call for images b0 .. b0 + n - 1 (elem / loc_elem: bytes per element of value and out / of loc and attn)
  MsdaFwdCall images(long long b0, int n, size_t elem, size_t loc_elem) const
  {
    MsdaFwdCall c = *this;
    const long long rec0 = b0 * Lq * M;                                        // first (query, head) record of image b0
    c.value = static_cast<const char *>(value) + b0 * S * M * D * (long long)elem;
    c.loc = static_cast<const char *>(loc) + rec0 * L * P * 2 * (long long)loc_elem;
    c.attn = static_cast<const char *>(attn) + rec0 * L * P * (long long)loc_elem;
    c.out = static_cast<char *>(out) + rec0 * D * (long long)elem;
    if (ref) c.ref = ref + b0 * ref_batch_stride;
    c.N = n;
    return c;
  }
};
struct MsdaBwdCall {
  const void *value;
  const int64_t *shapes, *starts;
  const void *loc, *attn, *grad_out;
  int N, S, M, D, L, Lq, P;
  void *grad_value, *grad_loc, *grad_attn;
  hipStream_t stream;
};

// The geometry and arithmetic headroom the two fp32 pyramid-column kernels (msda_forward_col.hip, msda_backward_col.hip)
// share; each launcher adds its own alignment checks.  (planes_forward_supported in MultiScaleDeformableAttention.py mirrors it.)
template <typename Call>   // MsdaFwdCall or MsdaBwdCall
inline bool msda_col_covers(const Call &c)
{
  const int N = c.N, S = c.S, M = c.M, D = c.D, L = c.L, Lq = c.Lq, P = c.P;
  if (D != 16 || P != 4 || L < 3 || L > 5 || Lq != S || M < 1) return false;
  if ((long long)N * ((long long)S + 4096) * M >= 0x7fffffffLL) return false;   // item / record arithmetic headroom
  if ((long long)S * M * L * P * 8 >= 0x7fffffffLL) return false;               // 32-bit byte offsets inside an image, all tensors
  if ((long long)S * M * D * 4 >= 0x7fffffffLL) return false;                   // (0x80000000 is the out-of-range sentinel)
  return S < (1 << 24) && M < (1 << 16);                                        // 24-bit multiplies in the record index
}

// ---- MSDeformAttn forward.  launch_msda_forward is the route the plain entry points take (msda_route.hip: a specialised
// kernel, else the generic one), launch_msda_forward_special the specialised kernels alone and launch_msda_forward_planes
// the piece-plane operands' one.  The others launch one kernel each (msda_forward*.hip); the specialised ones return
// PCT_NOT_COVERED for a call they do not cover ----------------------------------------------------------------------------
template <typename T> int launch_msda_forward(const MsdaFwdCall &c);
template <typename T> int launch_msda_forward_special(const MsdaFwdCall &c);
int launch_msda_forward_planes(const MsdaFwdCall &c);
template <typename T> int launch_msda_forward_generic(const MsdaFwdCall &c);
template <typename T> int launch_msda_forward_win(const MsdaFwdCall &c);
template <typename T> int launch_msda_forward_dpp(const MsdaFwdCall &c);
int launch_msda_forward_col(const MsdaFwdCall &c, bool planes);
template <typename T> int launch_msda_forward_col16(const MsdaFwdCall &c);
void set_msda_kernel_choice(int v);     // a MsdaFwdKernel; anything else: follow PCT_MSDA_KERNEL
int msda_last_kernel();

// ---- MSDeformAttn backward.  launch_msda_backward is the route (msda_route.hip): it zeroes the gradients, then column ->
// windowed -> generic.  The others launch one kernel each (msda_backward*.hip) into gradients already zeroed --------------
template <typename A> int launch_msda_backward(const MsdaBwdCall &c);
template <typename A> int launch_msda_backward_generic(const MsdaBwdCall &c);
int launch_msda_backward_win(const MsdaBwdCall &c);
int launch_msda_backward_col(const MsdaBwdCall &c, bool forced);
// the generic backward kernel reduces a record's three channel sums by wave shuffles and stores grad_loc / grad_attn plainly
// (as the specialised kernels do) when its D / VEC lanes form a power-of-two group inside a wave; otherwise it adds into them
inline bool msda_backward_shuffles(int D, size_t elem)
{
  const int vecw = 16 / (int)elem, cv = D / vecw;
  return D % vecw == 0 && cv <= 64 && (cv & (cv - 1)) == 0;
}
hipError_t zero_fill(void *ptr, size_t bytes, hipStream_t stream);   // msda_backward.hip: by a kernel, not hipMemsetAsync
void set_msda_bwd_kernel_choice(int c);  // a MsdaBwdKernel; anything else: follow PCT_MSDA_BWD_KERNEL
int msda_bwd_last_kernel();

// ---- backward of the fused front-end (msda_fused_backward.hip; include/pctrans_hip_msda_train.h): the two kernels around
// launch_msda_backward<float>.  R = N * Lq * M records.  expand: offsets, logits, reference points -> locations [R][L * P][2]
// and softmax weights [R][L * P]; fold, in place on the routed backward's grad_loc / grad_attn: -> grad_offsets, grad_logits.
// Every tensor but ref 16-byte aligned.  PCT_NOT_COVERED: L * P above 64 or no multiple of 4, an odd P, 2^37 records or more ----
int launch_msda_fused_expand(const float *logits, const float *offsets, const float *ref, long long ref_batch_stride,
                             const int64_t *shapes, long long R, int M, int Lq, int L, int P, float *loc, float *w,
                             hipStream_t stream);
int launch_msda_fused_fold(const float *w, const int64_t *shapes, long long R, int L, int P, float *grad_offsets,
                           float *grad_logits, hipStream_t stream);

// ---- once per device, outside any stream capture (pct_prepare_device) ---------------------------------------------------
unsigned *win_queue_slot(hipStream_t stream);      // msda_win_common.hpp: a launch's set of per-XCD work-item counters
int prepare_win_queue_device();
int prepare_msda_backward_col_device();
int prepare_ffn_device();

// ---- dynamic mask head (dyn_mask_head*.hip).  out_dtype: 0 = f32, 2 = bf16 -------------------------------------------
int launch_dyn_mask_head(const float *feat, const float *ref, const float *params, int N, int C, int Q, int H, int W, int stride,
                         int rel_coord, int th, int tw, int out_dtype, void *up, unsigned char *amask, hipStream_t stream);
int launch_dyn_mask_head_mfma(const float *feat, const float *ref, const float *params, int N, int C, int Q, int H, int W,
                              int stride, int rel_coord, int th, int tw, void *scratch, void *up, unsigned char *amask,
                              hipStream_t stream);
int launch_dyn_mask_head_fused(const float *feat, const float *ref, const float *params, int N, int C, int Q, int H, int W,
                               int stride, int rel_coord, int th, int tw, void *workspace, void *up, unsigned char *amask,
                               hipStream_t stream);
// backward of the fp32 forward (dyn_mask_head_bwd.hip): two or three launches, deterministic, partial sums in `workspace`
int launch_dyn_mask_head_bwd(const float *feat, const float *ref, const float *params, const float *grad_up, int N, int C, int Q,
                             int H, int W, int stride, int rel_coord, void *workspace, float *grad_feat, float *grad_ref,
                             float *grad_params, hipStream_t stream);

// ---- the encoder's GEMMs and norms.  epi: 0 = bias, 1 = bias + ReLU, 2 = residual + LayerNorm -------------------------
int launch_linear_k128(const float *x, long long ldx, const float *x2, long long ldx2, long long x2_period, const float *w,
                       const float *bias, long long rows, int n, int epi, float *y, long long ldy, const float *residual,
                       long long ldr, const float *gamma, const float *beta, float eps, hipStream_t stream);
// The two split-bf16 launchers return PCT_NOT_COVERED when an operand is not 16-byte aligned for the dwordx4 epilogue:
// launch_linear_k128 then falls back to its fp32-MFMA kernel, pct_linear_k128_multi_f32 (no fallback) reports PCT_ERR_ALIGNMENT
int launch_linear_k128_split(const float *x, long long ldx, const float *x2, long long ldx2, long long x2_period, const float *w,
                             const float *bias, long long rows, int n, int epi, float *y, long long ldy, const float *residual,
                             long long ldr, const float *gamma, const float *beta, float eps, hipStream_t stream);
int launch_linear_k128_split_multi(const float *x, long long ldx, const float *x2, long long ldx2, long long x2_period, int nseg,
                                   const float *const *w, const float *const *bias, const int *n, const int *use_add,
                                   float *const *y, const long long *ldy, long long rows, hipStream_t stream);
int launch_linear_ln_split(const float *x, long long ldx, const float *w, unsigned short *w_pieces, int K, const float *bias,
                           const float *residual, long long ldr, const float *gamma, const float *beta, float eps, long long rows,
                           float *out, long long ldo, hipStream_t stream);
int launch_ffn_fused_split(const float *x, long long ldx, const float *w1, const float *b1, const float *w2, const float *b2,
                           const float *gamma, const float *beta, float eps, int F, long long rows, void *img_ws, float *out,
                           long long ldo, hipStream_t stream);
int launch_conv1x1_nchw_split(const float *x, const float *w, const float *bias, unsigned short *w_split_ws, int N, int K, int HW,
                              float *y, hipStream_t stream);
int launch_conv1x1_groupnorm_tokens(const float *x, const float *w, const float *bias, unsigned short *w_split_ws,
                                    const float *gamma, const float *beta, float eps, int N, int K, int HW, float *partial_ws,
                                    float *stats, float *out, long long out_batch_stride, hipStream_t stream);
int launch_add_layernorm(const float *x, const float *y, const float *gamma, const float *beta, float eps, long long rows,
                         int cols, float *out, hipStream_t stream);
int launch_groupnorm_flatten(const float *x, const float *gamma, const float *beta, int N, int C, int HW, int groups, float eps,
                             float *stats, float *out, long long out_batch_stride, long long out_offset, hipStream_t stream);

// ---- the decoder's semantic head in eval mode (conv3x3_bn_relu.hip; include/pctrans_hip_seg.h): bf16 maps of 128 channels, NCHW or
// channels-last (nhwc).  PCT_NOT_COVERED for any other channel count or an image of 2^24 pixels or more.
// bnp / bn_a / bn_b: {mean, var, gamma, beta} ----
int launch_conv3x3_bn_relu(const void *x, int nhwc, const float *w, const float *const *bnp, float eps, void *w_ws, int N, int C, int H,
                           int W, void *out, hipStream_t stream);
int launch_seg_head(const void *x, int nhwc, const float *w_a, const float *const *bn_a, float eps_a, const float *w_b,
                    const float *const *bn_b, float eps_b, const float *w_logits, const float *b_logits, void *w_ws, void *mid,
                    int N, int C, int H, int W, void *out, hipStream_t stream);

// ---- one FPN level of the pixel decoder in eval mode (fpn_stage.hip; include/pctrans_hip_fpn.h): fp32, split-bf16 products.
// norm1 / norm3: {mean, var, gamma, beta}, a null mean = no norm.  PCT_NOT_COVERED: in_channels % 16 != 0 or an image of 2^24
// pixels or more ----
int launch_fpn_stage(const float *x, const float *enc, long long enc_batch_stride, int enc_nhwc, const float *w1, const float *b1,
                     const float *const *norm1, float eps1, const float *w3, const float *b3, const float *const *norm3, float eps3,
                     void *w_ws, float *y_ws, int N, int K, int H, int W, float *out, hipStream_t stream);

// ---- the decoder's attention and the matcher ------------------------------------------------------------------------
int launch_masked_attention(const void *q, const void *k, const void *vT, const unsigned char *mask, int N, int heads, int Q,
                            int S, int head_dim, int v_head_dim, float scale, int out_dtype, void *out, hipStream_t stream);
int launch_cross_attention(const void *q_c, const void *q_s, const void *k_c, const void *k_p, const void *v,
                           const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S, float scale,
                           void *out, hipStream_t stream);
// the same for any S >= 1 with mask rows mask_pitch bytes apart (cross_attention.hip; include/pctrans_hip_xattn.h).
// PCT_NOT_COVERED: heads % 4 != 0 or an operand of 2^31 elements or more
int launch_cross_attention_ragged(const void *q_c, const void *q_s, const void *k_c, const void *k_p, const void *v,
                                  const unsigned char *mask, int mask_pitch, const unsigned char *row_open, int N, int heads,
                                  int Q, int S, float scale, void *out, hipStream_t stream);
// the same with the keys of every workgroup of that grid divided over `splits` workgroups, and a combine launch
// (cross_attention.hip; include/pctrans_hip_xattn_split.h).  splits == 1: launch_cross_attention_ragged.  After that launcher's
// PCT_NOT_COVERED and empty-call answers: PCT_ERR_BAD_ARG for splits outside 1 .. min(16, ceil(S / 64)) or, with splits >= 2, a
// null or too small workspace; PCT_ERR_ALIGNMENT for a workspace off 16 bytes
int launch_cross_attention_split_keys(const void *q_c, const void *q_s, const void *k_c, const void *k_p, const void *v,
                                      const unsigned char *mask, int mask_pitch, const unsigned char *row_open, int N, int heads,
                                      int Q, int S, float scale, int splits, void *workspace, long long workspace_bytes, void *out,
                                      hipStream_t stream);
// bytes of that workspace: splits * N * heads * Q records of 16 + 1 + 1 floats (0 for splits == 1)
long long cross_attention_split_keys_workspace(int N, int heads, int Q, int splits);
// differentiable fp32 cross-attention (cross_attention_train.hip; include/pctrans_hip_attn_train.h).  PCT_NOT_COVERED: heads
// outside {4, 8} or a tensor of 2^31 elements or more.  workspace: N * heads * Q floats
int launch_cross_attention_fwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                   const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S,
                                   float scale, float *out, float *lse, hipStream_t stream);
int launch_cross_attention_bwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                   const unsigned char *mask, const unsigned char *row_open, const float *out, const float *lse,
                                   const float *grad_out, int N, int heads, int Q, int S, float scale, float *workspace,
                                   float *grad_q_c, float *grad_q_s, float *grad_k_c, float *grad_k_p, float *grad_v,
                                   hipStream_t stream);
// the same with the keys of every query-side workgroup divided over min(splits, ceil(S / 64)) workgroups and combine launches
// (cross_attention_train_split.hip; include/pctrans_hip_attn_train_split.h).  After that launcher's PCT_NOT_COVERED:
// PCT_ERR_BAD_ARG for splits outside 1 .. 16, a null workspace or workspace_bytes below the need; PCT_ERR_ALIGNMENT for a
// workspace off 16 bytes -- all before any launch.  Forward 2 launches, backward 4
int launch_cross_attention_split_fwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                         const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S,
                                         float scale, int splits, void *workspace, long long workspace_bytes, float *out,
                                         float *lse, hipStream_t stream);
int launch_cross_attention_split_bwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                         const unsigned char *mask, const unsigned char *row_open, const float *lse,
                                         const float *grad_out, int N, int heads, int Q, int S, float scale, int splits,
                                         void *workspace, long long workspace_bytes, float *grad_q_c, float *grad_q_s,
                                         float *grad_k_c, float *grad_k_p, float *grad_v, hipStream_t stream);
// bytes of that workspace, enough for either direction: with R = N * heads * Q, 136 * splits * R + 4 * R rounded up to 16
long long cross_attention_split_train_workspace(int N, int heads, int Q, int splits);
// differentiable fp32 self-attention (self_attention_train.hip; include/pctrans_hip_self_attn_train.h).  PCT_NOT_COVERED: heads
// outside {4, 8}, more than 512 queries or an operand of 2^31 elements or more.  workspace: N * heads * Q floats
int launch_self_attention_fwd_f32(const float *q_c, const float *q_p, const float *k_c, const float *k_p, const float *v, int N,
                                  int heads, int Q, float scale, float *out, float *lse, hipStream_t stream);
int launch_self_attention_bwd_f32(const float *q_c, const float *q_p, const float *k_c, const float *k_p, const float *v,
                                  const float *lse, const float *grad_out, int N, int heads, int Q, float scale, float *workspace,
                                  float *grad_q, float *grad_k, float *grad_v, hipStream_t stream);
// the same two forwards for evaluation: no lse, any query count, loads one step ahead (attention_eval.hip;
// include/pctrans_hip_attn_eval.h).  PCT_NOT_COVERED: heads outside {4, 8} or an operand of 2^31 elements or more
int launch_cross_attention_eval_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                    const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S,
                                    float scale, float *out, hipStream_t stream);
int launch_self_attention_eval_f32(const float *q_c, const float *q_p, const float *k_c, const float *k_p, const float *v, int N,
                                   int heads, int Q, float scale, float *out, hipStream_t stream);
int launch_lsap(const float *cost, int batch, int num_query, int ld_target, const int *num_target, int *row_for_target,
                int *status, hipStream_t stream);

// ---- how the loss, target and metric kernels split an image's pixels: workgroups ("chunks", at most max_chunks per image: that
// bounds a workspace) that each walk `passes` consecutive passes of per_pass pixels.  The Python workspace formulas mirror it
// (pctrans_amd/_lib.py: chunk_plan) ----------------------------------------------------------------------------------------
struct ChunkPlan {
  int passes, chunks;
};
inline ChunkPlan chunk_plan(const long long pixels, const int per_pass, const int max_chunks)
{
  ChunkPlan m;
  const long long subs = (pixels + per_pass - 1) / per_pass;
  m.passes = (int)((subs + max_chunks - 1) / max_chunks);
  m.chunks = (int)((subs + m.passes - 1) / m.passes);
  return m;
}

// ---- point-sampled mask losses (point_loss.hip; include/pctrans_hip_train.h).  An index array may be nullptr (identity);
// PCT_ERR_UNSUPPORTED before any launch for a geometry the kernels do not cover -----------------------------------------
int launch_point_sample(const float *planes, const int *plane_index, const float *coords, int num_planes, int H, int W, int K,
                        int P, int per_row, float *out, hipStream_t stream);
int launch_point_loss_backward(const float *x, const float *t, const float *coords, const float *alpha, const float *beta,
                               const float *gamma, int K, int P, int H, int W, float *grad_planes, hipStream_t stream);
int launch_point_match_cost(const float *pred, int B, int Q, int H, int W, const float *tgt, int num_tgt, int Ht, int Wt,
                            const int *tgt_start, const int *tgt_count, int Gmax, const float *coords, int P, float cost_mask,
                            float cost_dice, void *workspace, float *cost, hipStream_t stream);
// the selection, the loss forward and the cost pass of 0 < num_heads <= PCT_POINT_MAX_HEADS predictions in one launch: `preds`
// a host array of device pointers, copied into a by-value kernel argument; every per-head array carries a leading [num_heads]
// dimension.  The single-head selection and loss forward call these with one head
int launch_point_select_many(const float *const *preds, int num_heads, const int *src_index, int num_pred, int H, int W,
                             const float *cand_coords, int K, int S, int num_keep, float *out_coords, int out_row_points,
                             int *out_index, hipStream_t stream);
int launch_point_loss_forward_many(const float *const *preds, int num_heads, const int *src_index, int num_pred, int H, int W,
                                   const float *tgt, const int *tgt_index, int num_tgt, int Ht, int Wt, const float *coords, int K,
                                   int P, float *x, float *t, float *sums, hipStream_t stream);
int launch_point_match_cost_many(const float *const *preds, int num_heads, int B, int Q, int H, int W, const float *tgt, int num_tgt,
                                 int Ht, int Wt, const int *tgt_start, const int *tgt_count, int Gmax, const float *coords, int P,
                                 float cost_mask, float cost_dice, void *workspace, float *cost, hipStream_t stream);

// ---- pixel-embedding loss (embedding_loss.hip; include/pctrans_hip_train.h).  PCT_ERR_UNSUPPORTED before any launch for a
// geometry the kernels do not cover ---------------------------------------------------------------------------------------
int launch_instance_label_map(const float *planes, int num_planes, int Ht, int Wt, const int *start, const int *count, int B, int h,
                              int w, int *labels, hipStream_t stream);
int launch_emb_loss_forward(const float *emb, const int *labels, int B, int E, int h, int w, int L, float delta_v, float delta_d,
                            float alpha, float beta, float gama, void *workspace, float *table, float *loss, int *status,
                            hipStream_t stream);
int launch_emb_loss_backward(const float *emb, const int *labels, const float *table, const float *grad_out, int B, int E, int h,
                             int w, int L, float delta_v, float *grad_emb, hipStream_t stream);

// ---- mask side of the query-contrast loss (reid_dice.hip; include/pctrans_hip_reid.h): rows of the pairwise sigmoid dice and
// their backward.  PCT_ERR_UNSUPPORTED before any launch for a geometry the kernels do not cover ----------------------------
int launch_reid_dice_forward(const float *logits, const int *image_start, const int *key, int N, int Q, int h, int w, int I,
                             void *workspace, float *sums, float *dice, int *status, hipStream_t stream);
int launch_reid_dice_backward(const float *logits, const int *image_start, const int *key, const float *dice, const float *sums,
                              const float *grad_dice, int N, int Q, int h, int w, int I, void *workspace, float *grad_logits,
                              hipStream_t stream);

// ---- query side of the query-contrast loss and the per-item reduction of both sides (reid_query.hip;
// include/pctrans_hip_reid_query.h).  PCT_ERR_UNSUPPORTED before any launch for a geometry the kernels do not cover ---------------
int launch_reid_nearest_positive(const float *query, const int *pos, int Q, int N, int C, int max_pos, int *nearest,
                                 hipStream_t stream);
int launch_reid_query_rows_forward(const float *query, const int *image_start, const int *key, int Q, int N, int C, int I,
                                   float *norm, float *dots, float *cosines, hipStream_t stream);
int launch_reid_query_rows_backward(const float *query, const int *image_start, const int *key, const float *norm,
                                    const float *cosines, const float *grad_dots, const float *grad_cosines, int Q, int N, int C,
                                    int I, void *workspace, float *grad_query, hipStream_t stream);
int launch_contrast_loss_rows(const float *rows, const int *image_of, const int *key, const int *owner, int I, int Q, int N,
                              float inv_temperature, float *loss, float *coef, hipStream_t stream);

// ---- the criterion's reference-point L1 loss of all heads and its strided semantic focal loss (aux_losses.hip;
// include/pctrans_hip_aux_loss.h).  fg_dtype: 0 one byte, 4 float32.  PCT_ERR_BAD_ARG / PCT_ERR_UNSUPPORTED before any launch for a
// geometry that is wrong or not covered ----------------------------------------------------------------------------------------
int launch_refpoint_l1_forward(const float *points, const float *target_points, const int *src, const int *tgt, int heads,
                               long long rows, int dims, int num_targets, int pairs, float num_masks, float *loss, int *status,
                               hipStream_t stream);
int launch_refpoint_l1_backward(const float *points, const float *target_points, const int *src, const int *tgt,
                                const float *grad_loss, int heads, long long rows, int dims, int num_targets, int pairs,
                                float num_masks, float *grad_points, hipStream_t stream);
int launch_sigmoid_focal_strided_forward(const float *logits, const void *fg, int fg_dtype, int batch, int out_h, int out_w,
                                         int height, int width, int stride, float alpha, void *workspace, float *loss,
                                         float *num_pos, hipStream_t stream);
int launch_sigmoid_focal_strided_backward(const float *logits, const void *fg, int fg_dtype, const float *num_pos,
                                          const float *grad_loss, int batch, int out_h, int out_w, int height, int width,
                                          int stride, float alpha, float *grad_logits, hipStream_t stream);

// ---- instance targets from label maps (instance_targets.hip; include/pctrans_hip_targets.h).  dtype: 0 uint8, 1 int16, 2 int32,
// 3 int64, 4 float32.  PCT_ERR_UNSUPPORTED before any launch for a geometry the kernels do not cover -------------------------
int instance_targets_geometry_status(int dtype, int N, int H, int W);     // PCT_OK or PCT_ERR_UNSUPPORTED
int launch_instance_targets_census(const void *labels, int dtype, int N, int H, int W, int ignore_label, void *workspace, int *ids,
                                   int *pixels, float *centres, int *num, int *status, hipStream_t stream);
int launch_instance_targets_planes(const void *labels, int dtype, int N, int H, int W, const void *workspace, const int *counts,
                                   long long total_planes, int max_count, int *starts, uint8_t *masks, float *planes, uint8_t *fg,
                                   hipStream_t stream);

// ---- validation metrics from label maps (label_metrics.hip; include/pctrans_hip_metrics.h).  dtype codes as the instance targets'.
// PCT_ERR_UNSUPPORTED before any launch for a geometry the kernels do not cover ----------------------------------------------------
int label_metrics_geometry_status(int pred_dtype, int gt_dtype, int N, int H, int W);     // PCT_OK or PCT_ERR_UNSUPPORTED
int launch_label_overlap(const void *pred, int pred_dtype, const void *gt, int gt_dtype, const uint8_t *fg, int N, int H, int W,
                         void *workspace, int *values, int *areas, int *num, int *range, int *table, int *status,
                         hipStream_t stream);
int launch_label_metrics(const int *values, const int *areas, const int *num, const int *range, const int *table, int N,
                         double *metrics, int *counts, hipStream_t stream);

// ---- small-object merging of label maps (label_merge.hip; include/pctrans_hip_merge.h).  dtype codes as the instance targets';
// `passes` [num_passes, 2] (threshold, window) in host memory.  PCT_ERR_BAD_ARG for wrong passes, PCT_ERR_UNSUPPORTED for a
// geometry the kernels do not cover, both before any launch ----------------------------------------------------------------
int label_merge_status(int dtype, int N, int H, int W, const int *passes, int num_passes);
int launch_label_merge_small(const void *labels, int dtype, const uint8_t *fg, int N, int H, int W, const int *passes,
                             int num_passes, void *workspace, void *out, int *values, int *final_, int *areas_before,
                             int *areas_after, int *num, int *merges, int *status, hipStream_t stream);

// ---- instance post-processing (instance_post.hip; include/pctrans_hip_post.h).  dataset: 0 = CVPPP, 1 = BBBC -----------------
int instance_geometry_status(int N, int Q, int H, int W);     // PCT_OK or PCT_ERR_UNSUPPORTED
int launch_instance_masks(const void *logits, int bf16, int N, int Q, int h, int w, int H, int W, int dataset, unsigned *bits,
                          int *areas, hipStream_t stream);
int launch_instance_labels_from_bits(const unsigned *bits, const int *areas, int N, int Q, int H, int W, int dataset,
                                     void *workspace, short *labels, hipStream_t stream);
int launch_instance_labels(const void *logits, int bf16, int N, int Q, int h, int w, int H, int W, int dataset, void *workspace,
                           short *labels, hipStream_t stream);

}  // namespace pct
