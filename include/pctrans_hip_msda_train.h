/* Backward of MSDeformAttn with the module front-end fused in: entry point of libpctrans_hip.so.  Included by pctrans_hip.h (status
 * codes, PCT_API, conventions: there); include that header, not this one.  The caller (pctrans_amd/msda_train.py, reached with
 * MSDeformAttn.train_front = "hip") takes it only for fp32 device operands outside autocast when a gradient is required and the
 * reference points need none; everything else keeps the torch chain (pixel_decoder/ops/modules/ms_deform_attn.py). */
#ifndef PCTRANS_HIP_MSDA_TRAIN_H
#define PCTRANS_HIP_MSDA_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- replaces, per MSDeformAttn of a training step, the backward of
 *          w   = softmax(attn_logits over num_levels * num_point)
 *          loc = ref_points[:, :, None, :, None, :] + offsets / (W_l, H_l)      IEEE division and addition, as torch forms them
 *          out = ms_deform_attn(value, loc, w)
 *      that is: torch's softmax, division and broadcast-add backward passes and pct_ms_deform_attn_backward_f32 between them,
 *      with the [batch, num_query, heads, levels, points, 2] locations, the softmax output and their two gradients as autograd
 *      tensors.  The forward of the pair is pct_ms_deform_attn_fused_forward_f32, which this entry leaves as it is.
 *   value, spatial_shapes, level_start, ref_points, ref_batch_stride, offsets, attn_logits
 *                   as pct_ms_deform_attn_fused_forward_f32 takes them (ref_points [batch or 1, num_query, num_levels, 2],
 *                   ref_batch_stride 0 for one table shared by the batch); offsets and attn_logits 16-byte aligned
 *   grad_output     [batch, num_query, num_heads * channels] fp32
 *   workspace       device scratch, 16-byte aligned, 12 * batch * num_query * num_heads * num_levels * num_point bytes: the
 *                   recomputed locations (8 bytes per sample) followed by the recomputed weights (4 bytes per sample)
 *   grad_value      as value;  grad_offsets  as offsets;  grad_logits  as attn_logits (the last two 16-byte aligned).  All three
 *                   are fully defined on return
 * With (gv, gloc, gw) what pct_ms_deform_attn_backward_f32 returns at (loc, w):
 *          grad_value = gv,   grad_offsets = gloc / (W_l, H_l),   grad_logits = w * (gw - sum_k w_k gw_k)
 * Launches on `stream`: expand (offsets, logits -> loc, w in the workspace; expf and true division, not the forward kernel's
 * exp2 / rcp), the routed backward exactly as pct_ms_deform_attn_backward_f32 runs it -- pyramid-column, windowed or generic
 * kernel, pct_msda_set_bwd_kernel_choice and pct_msda_last_bwd_kernel apply -- writing its location and weight gradients
 * into grad_offsets / grad_logits, and fold, which rewrites those two in place (csrc/msda_fused_backward.hip).  No second pair
 * of gradient tensors exists.  No allocation, no host synchronisation; may be recorded into a HIP graph under the conditions
 * of pct_ms_deform_attn_backward_f32.  A sample the sampling kernel gates out has exactly zero grad_offsets.
 * Status: PCT_ERR_UNSUPPORTED for num_levels * num_point > 64 or not a multiple of 4, an odd num_point, and wherever
 * pct_ms_deform_attn_backward_f32 refuses; PCT_ERR_IM2COL_STEP as there; PCT_ERR_ALIGNMENT for a tensor not aligned as stated.
 * batch == 0 or num_query == 0: PCT_OK, nothing launched (and nothing written: an empty query set leaves grad_value to the
 * caller, whose gradient is then zero). */
PCT_API int pct_ms_deform_attn_fused_backward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                                  const float *ref_points, long long ref_batch_stride, const float *offsets,
                                                  const float *attn_logits, const float *grad_output, int batch,
                                                  int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                                  int num_point, int im2col_step, void *workspace, float *grad_value,
                                                  float *grad_offsets, float *grad_logits, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_MSDA_TRAIN_H */
