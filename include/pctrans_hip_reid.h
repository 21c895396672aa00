/* Mask side of the query-contrast ("re-id") loss in training: entry points of libpctrans_hip.so.  Included by pctrans_hip.h
 * (status codes, PCT_API, conventions: there); include that header, not this one.  The caller (pctrans_amd/reid_dice.py, reached
 * with MultiScaleMaskedTransformerDecoder.reid_dice = "hip") takes them for contiguous fp32 device logits; everything else keeps
 * the torch chain (transformer_decoder/query_contrast.py: select_pos_neg_mask). */
#ifndef PCTRANS_HIP_REID_H
#define PCTRANS_HIP_REID_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- replaces the rows that select_pos_neg_mask keeps of, per image (dice_for,
 *      transformer_decoder/mask2former_transformer_decoder.py: dec.py:917-927, gathered at dec.py:880-901),
 *          x = sigmoid(inputs.flatten(1)); numerator = x @ x.T; s = x.sum(-1)
 *          dice = (2 * numerator + 1) / (s[:, None] + s[None, :] + 1)                          [Q, Q], of which row k_i is kept
 *      without the [batch, num_query, height * width] sigmoid tensor and the [batch, num_query, num_query] matrix
 *      (csrc/reid_dice.hip) -------------------------------------------------------------------------------------------------------
 *   logits        [batch, num_query, height, width] fp32, dense
 *   image_start   [batch + 1] int32: image n owns rows image_start[n] .. image_start[n + 1] - 1 (rows are grouped by image; an
 *                 image may own none).  Values are clamped to [0, num_rows] before use
 *   key           [num_rows] int32: the query k_i of row i.  Keys may repeat and need not be sorted
 *   workspace     device scratch, 16-byte aligned, 4 * chunks * (num_rows + batch) * num_query bytes with
 *                     subs = ceil(height * width / 64), passes = ceil(subs / 128), chunks = ceil(subs / passes)
 *                 (per-chunk partial sums, added in ascending chunk order by the finalize kernels)
 *   sums          [batch, num_query] fp32 out: s[n, q] = sum_p sigmoid(logits[n, q, p])
 *   dice          [num_rows, num_query] fp32 out: D[i, q] = (2 num[i, q] + 1) / (s[n_i, k_i] + s[n_i, q] + 1),
 *                 num[i, q] = sum_p x[n_i, k_i, p] x[n_i, q, p]; the diagonal entry q = k_i included
 *   status        one int32 out: the number of rows whose key is outside [0, num_query) or that lie past the num_query-th row
 *                 of their image.  Such a row reads nothing, its row of `dice` is 0 and it adds nothing to any gradient (the
 *                 convention of pct_discriminative_loss_forward_f32)
 * fp32 operands, fp32 accumulation on v_mfma_f32_32x32x2_f32: a sum is an fmaf chain over at most passes * 64 pixels, then
 * `chunks` additions.  No floating-point atomic: two calls on the same operands give the same bits.
 * Geometry: num_query <= 1024, at most num_query rows per image (num_rows <= batch * num_query is what the host can check),
 * height * width < 2^31 - 1, batch <= 65535; anything else returns PCT_ERR_UNSUPPORTED before any launch.  num_rows == 0:
 * PCT_OK, nothing launched, nothing written.  Three launches on `stream`, no allocation, no host synchronisation. */
PCT_API int pct_reid_dice_rows_forward_f32(const float *logits, const int32_t *image_start, const int32_t *key, int batch,
                                           int num_query, int height, int width, int num_rows, void *workspace, float *sums,
                                           float *dice, int32_t *status, void *stream);

/* Backward of the above (what autograd runs for dec.py:917-927 and the gather of dec.py:880-901: two batched GEMMs over
 * [num_query, height * width] operands, the sigmoid backward and an add).  logits, image_start, key as given to the forward;
 * dice and sums as it wrote them;
 *   grad_dice     [num_rows, num_query] fp32: G = dL/dD
 *   workspace     device scratch, 16-byte aligned, 4 * (3 * num_rows * num_query + num_rows + batch * num_query) bytes
 *                 (a = 2 G / den and its transpose, b = -G D / den, the rows' sums of b, the per-query constant)
 *   grad_logits   [batch, num_query, height, width] fp32 out, every element written; exact zeros for an image without rows
 *       dL/dx[n, q, p] = sum_{i of n} a[i, q] x[n, k_i, p] + sum_{i: k_i = q} sum_q' a[i, q'] x[n, q', p]
 *                      + sum_{i of n} b[i, q] + sum_{i: k_i = q} sum_q' b[i, q'],      dL/dz = dL/dx x (1 - x)
 * The sigmoid is recomputed; nothing of size [batch, num_query, height * width] but grad_logits is written.  Every sum has a
 * fixed order (rows ascending, queries ascending): two calls on the same operands give the same bits.
 * Non-finite values: the second sum reaches query k_i through a product with a 0 / 1 factor shared by a tile of 32 queries, so a
 * non-finite inner sum of row i (an overflowed a x; only with overflowed incoming gradients) makes 0 * inf = NaN for the 32
 * queries of k_i's tile at that pixel, where the torch chain confines it to query k_i.  Finite inputs are not affected.
 * Status rules and geometry as the forward; num_rows == 0 writes zeros.  Three launches on `stream` (one when num_rows == 0). */
PCT_API int pct_reid_dice_rows_backward_f32(const float *logits, const int32_t *image_start, const int32_t *key, const float *dice,
                                            const float *sums, const float *grad_dice, int batch, int num_query, int height,
                                            int width, int num_rows, void *workspace, float *grad_logits, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_REID_H */
