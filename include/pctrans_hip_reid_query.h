/* Query side of the query-contrast ("re-id") loss in training, and the per-item reduction of both of its sides: entry points of
 * libpctrans_hip.so.  Included by pctrans_hip.h (status codes, PCT_API, conventions: there); include that header, not this one.
 * The caller (pctrans_amd/reid_query.py, reached with MultiScaleMaskedTransformerDecoder.reid_query = "hip" and
 * SetCriterion.contrast_loss = "hip") takes them for a dense fp32 device query tensor; everything else keeps the torch chain
 * (transformer_decoder/query_contrast.py, loss/maskformer_criterion.py: _contrast_softplus).
 *
 * Common to the three query entries:
 *   query         [num_query, batch, channels] fp32, dense, 16-byte aligned: the decoder's output as it stands; row (q, n) starts
 *                 at (q * batch + n) * channels.  Nothing is transposed or copied
 * Geometry: num_query <= 1024, channels <= 512 with channels % 4 == 0, batch <= 65535, at most num_query rows per image
 * (num_rows <= batch * num_query is what the host can check); anything else returns PCT_ERR_UNSUPPORTED before any launch.
 * No allocation, no host synchronisation, no floating-point atomic: two calls on the same operands give the same bits.
 *
 * Arithmetic (csrc/reid_query.hip): fp32 on the VALU.  A row is held by one wave, 16-byte coalesced loads, lane l holding the
 * float4s l and l + 64; a dot product <x, y> is per lane an fmaf chain over its channels in ascending order (at most 8), then a
 * 6-step xor butterfly over the wave.  Its fp32 summation chain has length L = 14 (8 + 6) whatever `channels` is.  Equal rows
 * give equal bits: every norm and every dot product of these entries is that one expression. */
#ifndef PCTRANS_HIP_REID_QUERY_H
#define PCTRANS_HIP_REID_QUERY_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- replaces, of query_contrast_items / _plan (dec.py:618-622, :800-830): the [batch, num_query, num_query] table
 *          emb_dist = F.cosine_similarity(q.unsqueeze(2), q.unsqueeze(1), dim=-1)
 *      (a [batch, num_query, num_query, channels] broadcast), its gather at the matched columns, masked_fill and argmax ------------
 *   pos           [batch, max_pos] int32: the matched queries of each image in matcher order, padded with -1 (any value outside
 *                 [0, num_query) is padding and is skipped; positions keep counting)
 *   nearest       [batch, num_query] int32 out: for every query r the position p in its image's list that maximises
 *                     cos(x_r, x_pos[p]) = <x_r, x_pos[p]> / (max(|x_r|, 1e-8) * max(|x_pos[p]|, 1e-8)),
 *                 the first maximum winning (two equal rows among the positives give equal cosines bit for bit); -1 for an image
 *                 without positives.  Matched queries get a value too; the caller ignores it
 * 1 <= max_pos <= num_query, else PCT_ERR_UNSUPPORTED.  One launch on `stream`. */
PCT_API int pct_reid_nearest_positive_f32(const float *query, const int32_t *pos, int num_query, int batch, int channels,
                                          int max_pos, int32_t *nearest, void *stream);

/* ---- replaces, of select_pos_neg_query (dec.py:832-878): the gather query[img, order] into [num_rows, num_query - 1, channels],
 *      its contraction with the keys, F.normalize of all queries and the auxiliary cosine products -----------------------------------
 *   image_start   [batch + 1] int32: image n owns rows image_start[n] .. image_start[n + 1] - 1 (rows are grouped by image; an
 *                 image may own none).  Values are clamped to [0, num_rows] before use
 *   key           [num_rows] int32: the query k_i of row i.  Keys may repeat and need not be sorted.  A key outside [0, num_query)
 *                 reads nothing: its rows of `dots` and `cosines` are 0 and it adds nothing to any gradient
 *   norm          [batch, num_query] fp32 out: m[n, q] = max(|x[n, q]|, 1e-12) (F.normalize's denominator)
 *   dots          [num_rows, num_query] fp32 out: S[i, q] = <x[n_i, q], x[n_i, k_i]>
 *   cosines       [num_rows, num_query] fp32 out: Cs[i, q] = S[i, q] / (m[n_i, q] * m[n_i, k_i])
 * The diagonal q = k_i is included in both.  A row outside every image's (clamped) range is not written.
 * num_rows == 0: PCT_OK, nothing launched, nothing written.  One launch on `stream`; no workspace. */
PCT_API int pct_reid_query_rows_forward_f32(const float *query, const int32_t *image_start, const int32_t *key, int num_query,
                                            int batch, int channels, int num_rows, float *norm, float *dots, float *cosines,
                                            void *stream);

/* Backward of the above (what autograd runs for the gathers, the einsum and F.normalize: an index_put_ with accumulate over
 * [num_rows, num_query - 1, channels]).  query, image_start, key as given to the forward; norm and cosines as it wrote them;
 *   grad_dots     [num_rows, num_query] fp32: gS = dL/dS
 *   grad_cosines  [num_rows, num_query] fp32: gC = dL/dCs
 *   workspace     device scratch, 16-byte aligned, 4 * num_rows * (channels + 2 * num_query + 1) bytes
 *                 (y [num_rows, channels], then a and b [num_rows, num_query], then the rows' sums of b)
 *   grad_query    [num_query, batch, channels] fp32 out, every element written; exact zeros for an image without rows
 * With a[i, q] = gS[i, q] + gC[i, q] / (m_q m_k) and b[i, q] = -gC[i, q] Cs[i, q]:
 *       dL/dx[n, q] = sum_{i of n} a[i, q] x[n, k_i]  +  sum_{i: k_i = q} y[i]
 *                   + ((sum_{i of n} b[i, q]) + (sum_{i: k_i = q} sum_q' b[i, q'])) / m_q^2 * x[n, q],
 *       y[i] = sum_q' a[i, q'] x[n, q']
 * Where m[n, q] was clamped (m <= 1e-12) it is a constant and the last line is dropped for that row.  Summation order: items
 * ascending; inside y the queries in 4 (channels <= 256) or 2 contiguous ranges of ceil(num_query / ranges),
 * ascending inside a range, the ranges added in ascending order; a row's sum of b per thread ascending (stride 256), butterfly,
 * four partials in order.  An element passes through at most rows_of_image + num_query + 8 additions.
 * num_rows == 0 writes zeros.  Three launches on `stream` (one when num_rows == 0). */
PCT_API int pct_reid_query_rows_backward_f32(const float *query, const int32_t *image_start, const int32_t *key, const float *norm,
                                             const float *cosines, const float *grad_dots, const float *grad_cosines, int num_query,
                                             int batch, int channels, int num_rows, void *workspace, float *grad_query,
                                             void *stream);

/* ---- replaces _contrast_softplus of SetCriterion.loss_reid_query / loss_reid_mask (crit.py:318-377: label building, two
 *      masked_fill + logsumexp, softplus) and its backward -----------------------------------------------------------------------
 *   rows          [num_rows, num_query] fp32: the scores of item i against every query of its image (S of the entry above, or D of
 *                 pct_reid_dice_rows_forward_f32)
 *   image_of      [num_rows] int32: the image n_i of item i (outside [0, batch): the item's loss and coefficients are 0)
 *   key           [num_rows] int32: the item's own query k_i, which takes no part
 *   owner         [batch, num_query] int32: the item whose cluster holds query q, or -1 for a matched query
 *   loss          [num_rows] fp32 out;  coef [num_rows, num_query] fp32 out: d loss_i / d rows[i, q]
 * With z = rows * inv_temperature, P = {q : owner[n_i, q] = i}, Ng = {q != k_i, q not in P}:
 *       A = lse_Ng(z), B = lse_P(-z), loss = softplus(A + B), s = sigmoid(A + B),
 *       coef = s softmax_Ng(z) inv_temperature on Ng, -s softmax_P(-z) inv_temperature on P, 0 at the key.
 * An item without negatives (or without positives) gives exactly 0 loss and 0 coefficients.  Max-subtracted sums with expf /
 * logf / log1pf (no fast-math): a sum runs per thread ascending (stride 256), butterfly, four partials in order.
 * num_query <= 1024, batch <= 65535, else PCT_ERR_UNSUPPORTED.  num_rows == 0: PCT_OK, nothing launched.  One launch. */
PCT_API int pct_contrast_loss_rows_f32(const float *rows, const int32_t *image_of, const int32_t *key, const int32_t *owner,
                                       int num_rows, int num_query, int batch, float inv_temperature, float *loss, float *coef,
                                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_REID_QUERY_H */
