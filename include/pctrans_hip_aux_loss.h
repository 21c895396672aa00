/* The criterion's reference-point and semantic losses in training: entry points of libpctrans_hip.so.  Included by pctrans_hip.h
 * (status codes, PCT_API, conventions: there; PCT_POINT_MAX_HEADS: pctrans_hip_train.h); include that header, not this one.  The
 * caller (pctrans_amd/aux_loss.py: refpoint_l1_losses, sem_focal_loss) takes them for
 * contiguous fp32 device tensors outside autocast; the torch chains they restate are loss/maskformer_criterion.py:
 * loss_refpoints, loss_sem.  Kernels: csrc/aux_losses.hip.
 *
 * Common to the four entries: every pointer is a device pointer, 4-byte aligned (fg: 1 byte for the byte type; workspace: 16);
 * everything runs on `stream`, nothing is allocated, the host is never synchronised, and no floating-point atomic is used -- every
 * sum has one order that depends on the shapes alone, so two calls on the same operands give the same bits.  A negative count, a
 * non-positive size or a missing pointer returns PCT_ERR_BAD_ARG, a misaligned pointer PCT_ERR_ALIGNMENT, a geometry outside what
 * is covered PCT_ERR_UNSUPPORTED (callers keep their torch formulation): all before any launch. */
#ifndef PCTRANS_HIP_AUX_LOSS_H
#define PCTRANS_HIP_AUX_LOSS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- replaces, for all supervised heads of a step at once (SetCriterion.loss_refpoints, once per head),
 *          src_points = reference_points[batch_idx, src_idx]; target_points = cat(center_points[tgt_idx]).flatten(1)
 *          loss = F.l1_loss(src_points, target_points, reduction="none").sum() / num_masks
 *      -------------------------------------------------------------------------------------------------------------------------
 *   points         [heads, rows, dims] fp32, dense: rows = batch * num_query, dims = 2 * points_num (the decoder's stacked
 *                  outputs_coords)
 *   target_points  [num_targets, dims] fp32
 *   src, tgt       [heads, pairs] int32: pair k of head h matches row src[h, k] = b * num_query + q of points[h] with row
 *                  tgt[h, k] of target_points.  Rows may repeat
 *   num_masks      the criterion's normaliser
 *   loss           [heads] fp32 out: loss[h] = (sum_k sum_d |points[h, src[h, k], d] - target_points[tgt[h, k], d]|) / num_masks.
 *                  Order of the sum: thread t of 256 adds the terms of pairs t, t + 256, ... in ascending pair order, each pair's
 *                  coordinates in ascending d; the lanes of a wave by the 6-step butterfly (csrc/wave_reduce.hpp), the four waves in
 *                  ascending order: a term passes through at most ceil(pairs / 256) * dims + 9 additions
 *   status         one int32 out: the number of pairs (over all heads) with src outside [0, rows) or tgt outside [0, num_targets).
 *                  Such a pair reads nothing and contributes nothing, forward and backward (the convention of
 *                  pct_reid_dice_rows_forward_f32)
 * Covered: heads <= PCT_POINT_MAX_HEADS, dims <= 8, rows < 2^31 - 1; anything else PCT_ERR_UNSUPPORTED.  pairs == 0 or heads == 0:
 * PCT_OK, `loss` written with zeros (and `status` with 0) where heads > 0; src / tgt / target_points may then be NULL.  One
 * launch. */
PCT_API int pct_refpoint_l1_forward_f32(const float *points, const float *target_points, const int32_t *src, const int32_t *tgt,
                                        int heads, long long rows, int dims, int num_targets, int pairs, float num_masks,
                                        float *loss, int32_t *status, void *stream);

/* Backward of the above.  Operands as given to the forward;
 *   grad_loss      [heads] fp32: dL/dloss[h]
 *   grad_points    [heads, rows, dims] fp32 out, every element written by the one launch (no fill pass): a row that pair k lists
 *                  gets sgn(points - target) * (grad_loss[h] / num_masks), sgn(0) = 0 (torch's l1_loss backward); a row several
 *                  pairs of one head list gets the sum of their terms in ascending pair order; any other row exact zeros
 * Status rules and geometry as the forward; heads == 0 or rows == 0: PCT_OK, nothing launched. */
PCT_API int pct_refpoint_l1_backward_f32(const float *points, const float *target_points, const int32_t *src, const int32_t *tgt,
                                         const float *grad_loss, int heads, long long rows, int dims, int num_targets, int pairs,
                                         float num_masks, float *grad_points, void *stream);

/* ---- replaces (SetCriterion.loss_sem with out_stride = stride; sigmoid_focal_loss of loss/maskformer_criterion.py, gamma = 2)
 *          one_hot = fg[:, None, stride // 2::stride, stride // 2::stride].float()
 *          num_pos = (one_hot > 0).sum().float().clamp(min=1.0)
 *          loss = sigmoid_focal_loss(logits, one_hot, alpha=alpha, gamma=2.0, reduction="sum") / num_pos
 *      -------------------------------------------------------------------------------------------------------------------------
 *   logits         [batch, out_h, out_w] fp32, dense
 *   fg             [batch, height, width], dense: fg_dtype 0 = one byte per pixel (bool / uint8), 4 = fp32 (the dtype codes of
 *                  pct_instance_targets_census); any other code PCT_ERR_UNSUPPORTED.  The target of output pixel (i, j) is
 *                  t = (float) fg[n, stride / 2 + i * stride, stride / 2 + j * stride]
 *   stride, alpha  stride >= 1; alpha < 0: no class weight
 *   workspace      device scratch, 16-byte aligned, PCT_FOCAL_WORKSPACE_BYTES bytes: per workgroup (at most 256, each a run of
 *                  consecutive outputs) the loss sum and the count of positive targets, added in ascending order by the
 *                  finalising launch
 *   loss           one fp32 out: (sum l) / max(num_pos, 1), per element in fp32
 *                      p = sigmoid(x), ce = max(x, 0) - x t + log1p(exp(-|x|)), m = 1 - (p t + (1 - p)(1 - t)),
 *                      l = ce m^2, times alpha t + (1 - alpha)(1 - t) when alpha >= 0
 *                  (exp(-|x|) cannot overflow).  A workgroup's sum: thread t of 256 adds outputs t, t + 256, ... of its run in
 *                  ascending order, lanes by the butterfly, waves in ascending order
 *   num_pos        one fp32 out: #{t > 0}, unclamped (an integer count, converted once); the backward reads it
 * Geometry: out_h == ceil((height - stride / 2) / stride) > 0 and the same for the width, else PCT_ERR_BAD_ARG;
 * batch * out_h * out_w < 2^31 - 1, else PCT_ERR_UNSUPPORTED.  Two launches. */
#define PCT_FOCAL_WORKSPACE_BYTES 2048
PCT_API int pct_sigmoid_focal_strided_forward_f32(const float *logits, const void *fg, int fg_dtype, int batch, int out_h,
                                                  int out_w, int height, int width, int stride, float alpha, void *workspace,
                                                  float *loss, float *num_pos, void *stream);

/* Backward of the above.  logits, fg, geometry, stride and alpha as given to the forward, num_pos as it wrote it;
 *   grad_loss      one fp32: dL/dloss
 *   grad_logits    [batch, out_h, out_w] fp32 out, every element written:
 *                      grad_loss * w * ((p - t) m^2 - 2 ce m (2 t - 1) p (1 - p)) / max(num_pos, 1),
 *                  w = alpha t + (1 - alpha)(1 - t) or 1; p, ce and m recomputed from the logit
 * One launch. */
PCT_API int pct_sigmoid_focal_strided_backward_f32(const float *logits, const void *fg, int fg_dtype, const float *num_pos,
                                                   const float *grad_loss, int batch, int out_h, int out_w, int height, int width,
                                                   int stride, float alpha, float *grad_logits, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_AUX_LOSS_H */
