/* Differentiable fp32 cross-attention of the decoder: entry points of libpctrans_hip.so.  Included by pctrans_hip.h (status
 * codes, PCT_API, conventions: there); include that header, not this one.  The caller (pctrans_amd/attention_train.py, reached
 * with CrossAttentionLayer.attn_train = "hip") takes them only for fp32 device operands outside autocast when a gradient is
 * required; everything else keeps the torch chain (transformer_decoder/attention.py: attention_core). */
#ifndef PCTRANS_HIP_ATTN_TRAIN_H
#define PCTRANS_HIP_ATTN_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- replaces, per cross-attention layer of a training step (mask2former_transformer_decoder.py: CrossAttentionLayer),
 *          q = cat([q_content, q_pos] per head); k = cat([k_content, k_pos] per head)          two concatenation passes
 *          out = softmax(masked_fill(q * scale . k^T, mask & ~row_open, -inf)) . v              attention_core
 *      and the reverse of all of it in the backward (csrc/cross_attention_train.hip) ---------------------------------------------
 *   q_content, q_pos          [num_query, batch, heads * 16] fp32, dense, 16-byte aligned
 *   k_content, k_pos, v       [num_key, batch, heads * 16] fp32, dense, 16-byte aligned
 *   mask                      [batch, num_query, num_key] bytes, nonzero = may not attend; NULL = no mask
 *   row_open                  [batch, num_query] bytes, nonzero = this query ignores its row of `mask`; NULL = none does
 *                             (ignored without a mask)
 *   scale                     the factor on the scores: (2 * 16)^-0.5 for the decoder's [content 16 | position 16] heads
 *   out                       [num_query, batch, heads * 16] fp32, 16-byte aligned
 *   lse                       [2][batch, heads, num_query] fp32, 16-byte aligned.  Plane 0: row maximum + log of the row sum of
 *                             the scaled scores; plane 1: what fp32 left of that sum (formed in fp64), which the backward
 *                             subtracts as well -- one fp32 word of lse is a relative error of up to ulp(lse) / 2 on every
 *                             recomputed probability of the row
 * fp32 operands; the scores are accumulated in fp64 (v_mfma_f64_16x16x4_f64 on the widened operands) and the exponent is rounded to
 * fp32 once, every other product is fp32 with fp32 accumulation (v_mfma_f32_16x16x4_f32); the [batch, heads, num_query, num_key]
 * probabilities are never written.
 * A query with nothing attendable (every key masked, row_open not set): out = 0, lse = 0 in both planes (a sentinel that no
 * live position reads), and every gradient of and through that row is 0 -- where torch's masked softmax gives NaN.  The decoder never makes
 * such a row (its row_open is mask.all(-1)).
 * Geometry: heads in {4, 8}, any num_query >= 1 and num_key >= 1 with batch <= 65535 and each operand below 2^31 elements;
 * anything else returns PCT_ERR_UNSUPPORTED and the caller keeps the torch chain.  Speed rule, applied by the caller and not by
 * this entry (pctrans_amd/attention_train.py: supported, MAX_KEYS): forward + backward were measured faster than the torch chain on
 * the device up to 1 024 keys and slower at 3 136 and 4 096 (profiles/attn_train.json), so CrossAttentionLayer sends calls of
 * more than 1 024 keys to the torch chain.  batch, num_query or num_key == 0: PCT_OK,
 * nothing launched.  One launch on `stream`, no allocation, no host synchronisation. */
PCT_API int pct_cross_attention_forward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                            const float *v, const unsigned char *mask, const unsigned char *row_open, int batch,
                                            int heads, int num_query, int num_key, float scale, float *out, float *lse,
                                            void *stream);

/* Backward of the above.  The five operands, mask, row_open and scale as given to the forward; lse as it wrote it;
 *   out                       the forward's output.  Not read (D is formed from P and dP, see workspace); may be NULL.  Kept so
 *                             that the entry takes what a backward of this operation is handed
 *   grad_out                  [num_query, batch, heads * 16] fp32, dense, 16-byte aligned
 *   workspace                 device scratch, 16-byte aligned: batch * heads * num_query floats (D = rowsum(grad_out * out), formed
 *                             once per call as the equal sum over the keys of P dP, the form torch's softmax backward evaluates)
 *   grad_q_content, grad_q_pos, grad_k_content, grad_k_pos, grad_v   in the operands' layouts, 16-byte aligned, fully overwritten
 * P = exp(scale * s - lse) is recomputed per 16 x 16 tile; masked positions contribute exactly 0.  No floating-point atomic: a
 * key's rows are summed by the one wave that owns them over the queries in ascending order, a query's rows by four waves over
 * interleaved key tiles and then in wave order -- two calls on the same operands give the same bits.
 * Status rules and geometry as the forward.  Three launches on `stream`, no allocation, no host synchronisation. */
PCT_API int pct_cross_attention_backward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                             const float *v, const unsigned char *mask, const unsigned char *row_open,
                                             const float *out, const float *lse, const float *grad_out, int batch, int heads,
                                             int num_query, int num_key, float scale, float *workspace, float *grad_q_content,
                                             float *grad_q_pos, float *grad_k_content, float *grad_k_pos, float *grad_v,
                                             void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_ATTN_TRAIN_H */
