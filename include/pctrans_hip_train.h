/* Opt-in training entry points of libpctrans_hip.so.  Included by pctrans_hip.h (status codes, PCT_API, conventions: there);
 * include that header, not this one.  What is declared here is reached only when a caller switches it on -- the default head and
 * the default training step never call it -- so pctrans_hip.h keeps exactly the entry points that have a default call site. */
#ifndef PCTRANS_HIP_TRAIN_H
#define PCTRANS_HIP_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dynamic mask head, backward of the fp32 forward (the training path) ------------------------------------------
 * What autograd computes for the reference's dynamic_mask_with_coords + mask_heads_forward
 * (transformer_decoder/mask2former_transformer_decoder.py:647-719) from the gradient of the x2-upsampled logits; the
 * attention mask is detached there and carries no gradient.  Inputs as pct_dynamic_mask_head_forward with out_dtype = 0
 * took them (nothing is saved by the forward: the MLP is recomputed with the forward kernel's operation order, so the
 * ReLU gates are the forward's; the derivative of ReLU at 0 is 0, as torch's), plus
 *   grad_up     [batch, num_query, 2*height, 2*width] fp32, 8-byte aligned
 * Outputs, fully overwritten:
 *   grad_feat   [batch, channels, height, width] fp32     (summed over the queries)
 *   grad_ref    [batch, num_query, 2] fp32                (rel_coord = 0: may be NULL, else written as zero)
 *   grad_params [batch, num_query, G] fp32, in the order of `params`
 * `workspace`: caller-owned, 16-byte aligned, nothing is allocated inside the call,
 *   4 * batch * (ceil(height*width / 128) * num_query * G  +  8 * channels * height*width)  bytes
 * (per-tile partial sums of grad_params, per-query-group partial sums of grad_feat).  A call is two or three launches on
 * `stream` and no host synchronisation; it may be recorded into a HIP graph and replayed.  No atomic operation touches an
 * output or the workspace and every sum runs in a fixed order: results are bit-identical from call to call.  The sums over
 * pixels run on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation).  Geometry: channels == 16 (three layers of 8),
 * any height, width, num_query, rel_coord 0 / 1; anything else returns PCT_ERR_UNSUPPORTED and callers keep their
 * differentiable dense formulation. */
PCT_API int pct_dynamic_mask_head_backward_f32(const float *mask_feat, const float *ref_points, const float *params,
                                               const float *grad_up, int batch, int channels, int num_query, int height,
                                               int width, int stride, int rel_coord, void *workspace, float *grad_feat,
                                               float *grad_ref, float *grad_params, void *stream);

/* ---- point-sampled mask losses (the matcher's and the criterion's point_sample + BCE + dice) --------------------------
 * What the reference computes with detectron2's point_sample and its sigmoid_ce_loss / dice_loss
 * (loss/matcher.py:70-222, loss/maskformer_criterion.py:23-116 and its loss_masks).  Sampling is
 * F.grid_sample(input, 2c - 1, mode="bilinear", padding_mode="zeros", align_corners=False) on fp32 planes in fp32:
 * x = c_x * width - 0.5, y = c_y * height - 0.5, taps at floor and floor + 1, a tap outside the plane contributes zero; a
 * coordinate of any value (outside [0, 1], NaN) reads nothing outside its plane.  Planes are contiguous [n, height, width];
 * coordinates are (x, y) pairs, 8-byte aligned; every other pointer is 4-byte aligned.  An index array is int32 on the device
 * and may be NULL (identity: entry k is plane k); an index outside its planes gives NaN for that row and reads nothing.
 * Each call is one launch on `stream`, no workspace, no host synchronisation, no floating-point atomic; every sum runs in a
 * fixed order: results are bit-identical from call to call.  Calls may be recorded into a HIP graph.
 * Status: a negative count, non-positive size or missing pointer PCT_ERR_BAD_ARG; misaligned pointer PCT_ERR_ALIGNMENT;
 * geometry outside what is covered PCT_ERR_UNSUPPORTED (callers keep their torch formulation); num_out / num_pairs == 0 or
 * num_points == 0: PCT_OK, nothing is launched and nothing is written.
 *
 * Gather.  out[k, p] = sample of plane plane_index[k] of planes [num_planes, height, width] at
 * coords[k / planes_per_coord_row, p, :];  coords [coord_rows, num_points, 2], out [num_out, num_points].
 * planes_per_coord_row >= 1: the matcher passes its query (target) count, one coordinate row serving a whole image; the
 * criterion passes 1.  Covered: height * width < 2^31 - 1 and num_out * ceil(num_points / 256) < 2^31 - 1. */
PCT_API int pct_point_sample_f32(const float *planes, const int32_t *plane_index, const float *coords, int num_planes, int height,
                                 int width, int num_out, int num_points, int coord_rows, int planes_per_coord_row, float *out,
                                 void *stream);

/* Loss forward.  For pair k: x[k, p] = sample of plane src_index[k] of pred [num_pred_planes, height, width] and
 * t[k, p] = sample of plane tgt_index[k] of tgt [num_tgt_planes, tgt_height, tgt_width], both at coords[k, p, :]
 * (coords [num_pairs, num_points, 2]; x, t [num_pairs, num_points], kept by the caller for the backward), and
 *   sums[k, 0..3] = sum_p bce(x, t),  sum_p sigma(x) t,  sum_p sigma(x),  sum_p t
 * with bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|)), torch's binary_cross_entropy_with_logits.  One workgroup per pair:
 * each thread sums its points in ascending order, the threads are summed by a fixed tree.
 * Covered: what the backward covers for (height, width), and tgt_height * tgt_width < 2^31 - 1.
 * It is the one-head case of pct_point_mask_loss_forward_many_f32 (below): that entry's checks, that entry's launch. */
PCT_API int pct_point_mask_loss_forward_f32(const float *pred, const int32_t *src_index, int num_pred_planes, int height,
                                            int width, const float *tgt, const int32_t *tgt_index, int num_tgt_planes,
                                            int tgt_height, int tgt_width, const float *coords, int num_pairs, int num_points,
                                            float *x, float *t, float *sums, void *stream);

/* Loss backward.  From x, t, coords of the forward and three per-pair coefficient vectors on the device, alpha, beta,
 * gamma [num_pairs] (for loss_mask = sum_k sums[k,0] / P / M and loss_dice = sum_k (1 - N_k / D_k) / M with
 * N_k = 2 sums[k,1] + 1, D_k = sums[k,2] + sums[k,3] + 1 and incoming gradients g_m, g_d:  alpha = g_m / (P M),
 * beta_k = g_d N_k / (D_k^2 M), gamma_k = 2 g_d / (D_k M)):
 *   grad_x[k, p] = alpha_k (sigma(x) - t) + sigma(x) (1 - sigma(x)) (beta_k - gamma_k t)
 * scattered to the four taps of point p with its bilinear weights into grad_planes [num_pairs, height, width]: compact (plane
 * k belongs to pair k), fully overwritten, so no zero-fill is needed before the call.
 * Fixed point instead of floating-point atomics: one workgroup per (pair, band of 32 rows) holds a signed 64-bit accumulator
 * per band pixel in LDS, adds round(w * grad_x * s) with workgroup-scope integer adds -- independent of their order -- and
 * stores float(sum) / s.  The scale is a power of two taken per pair on the device from
 *   bound_k = |alpha_k| + (|beta_k| + |gamma_k|) / 4  >=  |grad_x[k, p]|     (labels in [0, 1])
 *   bound_k = m 2^e, m in [0.5, 1):  s = 2^(30 - e), the exponent clamped to [-126, 126]
 * so that one contribution is below 2^30 (1 + 2^-20) in magnitude and the at most 2^31 - 1 contributions one pixel can receive
 * cannot overflow 63 bits.  Quantisation: a contribution moves by at most half a quantum, 1 / (2 s) <= bound_k 2^-30 (or 2^-127
 * where the clamp holds); a pixel that receives n contributions differs from the exact sum of its fp32 products by at most
 * n bound_k 2^-30, plus the one rounding of the conversion back to fp32.  Non-finite coefficients give a NaN plane.
 * Covered: width <= 256 (32 rows of 64-bit accumulators in 64 KiB of LDS), height * width < 2^31 - 1,
 * num_pairs * ceil(height / 32) < 2^31 - 1. */
PCT_API int pct_point_mask_loss_backward_f32(const float *x, const float *t, const float *coords, const float *alpha,
                                             const float *beta, const float *gamma, int num_pairs, int num_points, int height,
                                             int width, float *grad_planes, void *stream);

/* Uncertain-point selection (the criterion's get_uncertain_point_coords_with_randomness without its gather, topk, gather and
 * cat).  For pair k and candidate s, x = sample of plane src_index[k] of pred [num_pred_planes, height, width] at
 * cand_coords[k, s, :] (cand_coords [num_pairs, num_cand, 2]), computed by the gather's code: bit-identical to what
 * pct_point_sample_f32 returns for that plane and coordinate.  It is never written to memory.  The uncertainty is -|x|
 * (calculate_uncertainty); the key of a candidate is the bit pattern of |x| as an unsigned 32-bit integer (+0 and -0 tie), and
 * 0 for a NaN x (torch.topk ranks a NaN above every number: NaN counts as most uncertain).
 * The num_keep candidates with the smallest keys are selected; among the candidates whose key equals the num_keep-th smallest
 * the ones with the lowest candidate numbers are taken.  The selected candidates are written in ascending candidate number:
 * their coordinates, copied bit for bit, to out_coords[k, 0 .. num_keep), row k starting at out_coords + k * out_row_points * 2
 * (out_row_points >= num_keep; the points num_keep .. out_row_points of a row are not touched: the caller's fresh uniform
 * points live there), and their numbers to out_index [num_pairs, num_keep] unless it is NULL.  A row whose src_index is outside
 * the planes gets NaN coordinates and numbers -1.  cand_coords and out_coords are 8-byte aligned.
 * One workgroup of 1024 threads per pair: the keys stay in registers, a radix select (four 8-bit passes over LDS histograms,
 * integer adds) finds the num_keep-th smallest key and how many of its equals are admitted, one scan in candidate order
 * places the selected ones.  No sort, no workspace; everything is a function of the inputs alone.
 * Status, beyond the common rules: num_keep > num_cand or out_row_points < num_keep PCT_ERR_BAD_ARG; num_pairs == 0 or
 * num_keep == 0 PCT_OK with nothing launched.
 * Covered: num_cand <= 65536 (64 keys per thread) and height * width < 2^31 - 1.
 * It is the one-head case of pct_point_select_uncertain_many_f32 (below): that entry's checks, that entry's launch. */
PCT_API int pct_point_select_uncertain_f32(const float *pred, const int32_t *src_index, int num_pred_planes, int height,
                                           int width, const float *cand_coords, int num_pairs, int num_cand, int num_keep,
                                           float *out_coords, int out_row_points, int32_t *out_index, void *stream);

/* Matcher cost matrices (Point_HungarianMatcher._batched_costs without its two gathers and its chain of elementwise, einsum
 * and reduce launches).  pred [batch * num_query, height, width] and tgt [num_tgt_planes, tgt_height, tgt_width] are fp32 planes,
 * the targets of the images concatenated: image b owns the planes tgt_start[b] .. tgt_start[b] + tgt_count[b] (int32 arrays
 * [batch] on the device).  coords [batch, num_points, 2]: one row of points per image, serving all its planes.  With
 * x = sample of pred[b, q] and t = sample of target g of image b at the image's P = num_points points -- computed by the gather's
 * code: the bits pct_point_sample_f32 returns, never written to memory --
 *   ce[q, g]   = ( sum_p softplus(-x) t  +  sum_p softplus(x) (1 - t) ) / P
 *   dice[q, g] = 1 - (2 sum_p sigma(x) t + 1) / (sum_p sigma(x) + sum_p t + 1)
 *   cost[b, q, g] = cost_mask ce + cost_dice dice                      cost [batch, num_query, max_targets] fp32
 * softplus(-x) = max(-x, 0) + log1p(e), softplus(x) = max(x, 0) + log1p(e), sigma(x) from the same e = exp(-|x|): torch's
 * binary_cross_entropy_with_logits against ones and zeros.  The cross-entropy is the sum of two products of non-negative
 * factors, as the reference forms it: nothing cancels where a confident prediction meets its target.  The products over the
 * points run on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation).
 * cost is fully overwritten; columns g >= tgt_count[b] are written as exactly 0 (a negative count is 0, a count above
 * max_targets is max_targets).  A target plane outside 0 .. num_tgt_planes gives NaN in its column and reads nothing.
 * Two launches on `stream`: workgroups (chunk of the points, 128 queries x 64 targets, image) write partial sums to the
 * workspace, a second kernel adds the chunks in ascending order and forms the cost.  No floating-point atomic, no host
 * synchronisation, nothing allocated; every sum runs in a fixed order: results are bit-identical from call to call.  The call
 * may be recorded into a HIP graph.
 * `workspace`: caller-owned, 16-byte aligned, at least
 *   4 * batch * chunks * (2 Qp Gp + Qp + Gp) bytes,   Qp = 128 ceil(num_query / 128),  Gp = 64 ceil(max_targets / 64),
 *   chunks = max(1, min(32, ceil(num_points / 128), ceil(512 / (batch * (Qp / 128) * (Gp / 64)))))
 * Status: the common rules; batch, num_query, max_targets or num_points == 0: PCT_OK, nothing is launched and nothing is written
 * (for num_points == 0 the reference's 0 / 0 is left to the caller).  Covered: both planes below 2^31 - 1 pixels, batch <= 65535,
 * num_points <= 2^30, (Qp / 128) * (Gp / 64) <= 65535 -- the assignment's limits (1024 queries, 512 targets) included. */
PCT_API int pct_point_match_cost_f32(const float *pred, int batch, int num_query, int height, int width, const float *tgt,
                                     int num_tgt_planes, int tgt_height, int tgt_width, const int32_t *tgt_start,
                                     const int32_t *tgt_count, int max_targets, const float *coords, int num_points,
                                     float cost_mask, float cost_dice, void *workspace, float *cost, void *stream);

/* ---- the same three stages for several prediction heads in one launch -------------------------------------------------------
 * A training step supervises the decoder's last layer and its auxiliary heads against the same targets; their predictions are
 * separate tensors of one geometry.  The three entries below give the selection, the loss forward and the matcher costs a head
 * dimension: one launch (two for the costs) covers every (head, pair) or (head, image), the workgroup taking its head from a grid
 * dimension.  `preds` is a HOST array of num_heads device pointers, each to fp32 planes [num_pred_planes, height, width] (the
 * costs: [batch * num_query, height, width]) of the one common geometry.  The call copies the pointers into a structure that is
 * passed to the kernel by value: nothing is uploaded, allocated or synchronised, and the array may be reused at once.
 * Every per-head array is the single-head array with a leading [num_heads] dimension; the target planes, tgt_start and
 * tgt_count are shared by all heads.
 * Bit identity.  A workgroup works on its head's pointer and its head's slices alone, and no sum's order depends on num_heads:
 * for every head the entry writes exactly the bits the single-head entry -- for the selection and the loss forward the same
 * kernels launched with one head, for the costs kernels of its own around the same device functions -- writes
 * when called with preds[h] and the slices [h] of the arrays, the NaN rows of an index outside the planes and the zero columns
 * past an image's target count included.
 * Status: num_heads < 0 or > PCT_POINT_MAX_HEADS, preds == NULL with num_heads > 0, or a NULL entry PCT_ERR_BAD_ARG; num_heads == 0
 * PCT_OK with nothing launched; otherwise the rules of the single-head entry, the alignment of every entry included.
 *
 * Selection: pct_point_select_uncertain_f32 per head.  src_index [num_heads, num_pairs] or NULL (the identity in every head),
 * cand_coords [num_heads, num_pairs, num_cand, 2], out_coords [num_heads, num_pairs, out_row_points, 2], out_index
 * [num_heads, num_pairs, num_keep] or NULL.  The same three kernel classes by num_cand (16, 40 or 64 keys per thread).
 *
 * Loss forward: pct_point_mask_loss_forward_f32 per head.  src_index, tgt_index [num_heads, num_pairs] (each may be NULL: the
 * identity in every head), coords [num_heads, num_pairs, num_points, 2], x, t [num_heads, num_pairs, num_points], sums
 * [num_heads, num_pairs, 4].
 * The loss backward needs no entry of its own: pct_point_mask_loss_backward_f32 never reads the prediction, so called with
 * num_pairs = num_heads * num_pairs on the stacked x, t, coords and alpha, beta, gamma [num_heads * num_pairs] it IS the backward
 * of all heads in one launch, grad_planes [num_heads * num_pairs, height, width] compact.
 *
 * Matcher costs: pct_point_match_cost_f32 per head.  coords [num_heads, batch, num_points, 2], cost
 * [num_heads, batch, num_query, max_targets].  The points are chunked as the single-head call chunks them for `batch` images
 * (not for num_heads * batch), so every sum runs in the single call's order.  `workspace`: caller-owned, 16-byte aligned, at least
 *   num_heads * (4 * batch * chunks * (2 Qp Gp + Qp + Gp)) bytes, with Qp, Gp and chunks of pct_point_match_cost_f32 for `batch`;
 * head h owns the h-th part.  Covered: what the single-head entry covers, and num_heads * batch <= 65535. */
#define PCT_POINT_MAX_HEADS 16
PCT_API int pct_point_select_uncertain_many_f32(const float *const *preds, int num_heads, const int32_t *src_index,
                                                int num_pred_planes, int height, int width, const float *cand_coords,
                                                int num_pairs, int num_cand, int num_keep, float *out_coords, int out_row_points,
                                                int32_t *out_index, void *stream);
PCT_API int pct_point_mask_loss_forward_many_f32(const float *const *preds, int num_heads, const int32_t *src_index,
                                                 int num_pred_planes, int height, int width, const float *tgt,
                                                 const int32_t *tgt_index, int num_tgt_planes, int tgt_height, int tgt_width,
                                                 const float *coords, int num_pairs, int num_points, float *x, float *t,
                                                 float *sums, void *stream);
PCT_API int pct_point_match_cost_many_f32(const float *const *preds, int num_heads, int batch, int num_query, int height, int width,
                                          const float *tgt, int num_tgt_planes, int tgt_height, int tgt_width,
                                          const int32_t *tgt_start, const int32_t *tgt_count, int max_targets, const float *coords,
                                          int num_points, float cost_mask, float cost_dice, void *workspace, float *cost,
                                          void *stream);

/* ---- pixel-embedding loss (SetCriterion.loss_embedding: the label map and the reference's discriminative_loss,
 * loss/loss.py:297-355) -----------------------------------------------------------------------------------------------------
 * Label map.  planes [num_planes, plane_height, plane_width] fp32 are the images' target masks concatenated, image b owning the
 * planes plane_start[b] .. plane_start[b] + plane_count[b] (int32 [batch] on the device).  labels [batch, height, width] int32,
 * fully overwritten:
 *   labels[b, y, x] = 1 + the lowest g with plane g of image b > 0 at (sy, sx), else 0
 *   sy = min((int)floorf(y * (float)plane_height / height), plane_height - 1), sx likewise: torch's "nearest" source index
 * which is argmax over the zero-prepended stack of F.interpolate(masks, (height, width), "nearest") > 0 (ties go to the first
 * index; a NaN is not positive).  Only the sampled elements are read; a plane outside 0 .. num_planes is skipped and not read.
 * One launch.  Covered: both sizes below 2^31 - 1 pixels, batch <= 65535. */
PCT_API int pct_instance_label_map_f32(const float *planes, int num_planes, int plane_height, int plane_width,
                                       const int32_t *plane_start, const int32_t *plane_count, int batch, int height, int width,
                                       int32_t *labels, void *stream);

/* Loss forward.  embedding [batch, channels, height, width] fp32 contiguous, labels [batch, height, width] int32 in
 * 0 .. num_labels (0 is background).  With P_g the pixels of label g of one image, n_g their number, mu_g their mean,
 * r_p = |e_p - mu_g| and the image's present labels (n_g > 0, g >= 1), num_id of them:
 *   var  = (1 / num_id) sum_g (1 / n_g) sum_p (r_p - delta_v)^2                                  (no hinge: the reference has none)
 *   dist = sum_{i != j} relu(delta_d - |mu_i - mu_j|)^2 / (num_id (num_id - 1)) / 2              (only when num_id > 1)
 *   reg  = (1 / num_id) sum_g |mu_g|
 *   loss = (alpha sum_b var + beta sum_b dist + gama sum_b reg) / batch,   an image without instances adding 0
 * `loss`: one float on the device.  `status`: one int32 on the device, the number of labels outside 0 .. num_labels; such pixels
 * contribute nothing (they count as background) and nothing synchronises.
 * `table` [batch, num_labels + 1, 4 + 2 nch] fp32 with nch = 32, 64 or 128 channel slots for channels <= 32, <= 64, <= 128 (68 floats
 * up to 32 channels), fully overwritten, is what the backward needs, per label: [0] n_g, [1] the coefficient
 * c_g = alpha / (batch num_id n_g), [2] sum_p (r_p - delta_v)^2, [3] 0, [4 .. 4 + nch) mu_g, [4 + nch .. 4 + 2 nch) the vector
 *   T_g = -c_g S_g / n_g + (beta d dist / d mu_g + gama d reg / d mu_g) / (batch n_g),   S_g = sum_p 2 (r_p - delta_v)(e_p - mu_g) / r_p
 * (everything that reaches a pixel through its centroid; terms with r_p = 0, coinciding centroids and a zero centroid have
 * gradient 0, as torch's norm backward makes them).  Channels past `channels`, absent labels and row 0 are zero.
 * Six launches: per-label sums over (chunk of pixels, tile of 32 labels, image) on v_mfma_f32_32x32x2_f32 with the one-hot
 * operand formed in registers from the labels -- a 0 / 1 operand makes every product exact: a label's sum is the fp32 sum of its
 * pixels in ascending order inside a chunk -- the chunks added in ascending order; the same again for S_g with mu_g known; 32
 * labels per workgroup against all for the pairwise term; workgroups and images added in ascending order.  No floating-point
 * atomic, nothing allocated, no host synchronisation: results are bit-identical from call to call and the call may be recorded
 * into a HIP graph.
 * `workspace`: caller-owned, 16-byte aligned, at least
 *   4 * batch * (chunks * ((nch + 2) * 32 * (num_labels / 32 + 1) + 1) + 4 * ceil(num_labels / 32)) bytes   (nch + 2 = 34 up to 32 channels),
 *   subs = ceil(height * width / 256), passes = ceil(subs / 64), chunks = ceil(subs / passes)
 * Status: a non-positive size or count or a missing pointer PCT_ERR_BAD_ARG; misaligned pointer PCT_ERR_ALIGNMENT.
 * Covered: channels <= 128 (in tiles of 32 channels: one workgroup of the sums per channel tile), num_labels <= 1024, height * width < 2^31 - 1, batch <= 65535; anything else PCT_ERR_UNSUPPORTED and
 * callers keep their torch formulation. */
PCT_API int pct_discriminative_loss_forward_f32(const float *embedding, const int32_t *labels, int batch, int channels, int height,
                                                int width, int num_labels, float delta_v, float delta_d, float alpha, float beta,
                                                float gama, void *workspace, float *table, float *loss, int32_t *status,
                                                void *stream);

/* Loss backward, per pixel, no scatter: with g the pixel's label and grad_out one float on the device,
 *   grad_embedding[b, :, p] = grad_out (c_g 2 (1 - delta_v / r_p)(e_p - mu_g) + T_g)
 * and 0 for background and labels outside 0 .. num_labels; the first term is 0 where r_p = 0.  r_p is recomputed by the forward's
 * code.  grad_embedding [batch, channels, height, width] is fully overwritten.  One launch.  Covered: as the forward. */
PCT_API int pct_discriminative_loss_backward_f32(const float *embedding, const int32_t *labels, const float *table,
                                                 const float *grad_out, int batch, int channels, int height, int width,
                                                 int num_labels, float delta_v, float *grad_embedding, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_TRAIN_H */
