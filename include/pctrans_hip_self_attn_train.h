/* Differentiable fp32 self-attention of the decoder: entry points of libpctrans_hip.so.  Included by pctrans_hip.h (status
 * codes, PCT_API, conventions: there); include that header, not this one.  The caller (pctrans_amd/self_attention_train.py,
 * reached with SelfAttentionLayer.self_attn_train = "hip") takes them only for fp32 device operands outside autocast when a
 * gradient is required and the layer has no mask; everything else keeps the torch chain (transformer_decoder/attention.py:
 * attention_core). */
#ifndef PCTRANS_HIP_SELF_ATTN_TRAIN_H
#define PCTRANS_HIP_SELF_ATTN_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- replaces, per self-attention layer of a training step (mask2former_transformer_decoder.py: SelfAttentionLayer),
 *          q = q_content + q_pos; k = k_content + k_pos                                         two adds
 *          out = softmax((q * scale) . k^T) . v  per head, with its permutes                    attention_core
 *      and the reverse of all of it in the backward (csrc/self_attention_train.hip) -------------------------------------------
 *   q_content, q_pos, k_content, k_pos, v   [num_query, batch, heads * 16] fp32, dense, 16-byte aligned: what the layer's five
 *                             projections write.  Keys are the queries: there is one count
 *   scale                     the factor on the scores: 16^-0.5 for the decoder's heads of 16 dims
 *   out                       [num_query, batch, heads * 16] fp32, 16-byte aligned
 *   lse                       [2][batch, heads, num_query] fp32, 16-byte aligned.  Plane 0: row maximum + log of the row sum of
 *                             the scaled scores; plane 1: what fp32 left of that sum (formed in fp64), which the backward
 *                             subtracts as well -- one fp32 word of lse is a relative error of up to ulp(lse) / 2 on every
 *                             recomputed probability of the row
 * Per head q = fl32(q_content + q_pos) and k = fl32(k_content + k_pos): one fp32 rounding each, as torch's add; the sums are
 * not written.  The scores are accumulated in fp64 (v_mfma_f64_16x16x4_f64 on the widened operands) and the exponent is rounded
 * to fp32 once, every other product is fp32 with fp32 accumulation (v_mfma_f32_16x16x4_f32); the [batch, heads, num_query,
 * num_query] probabilities are never written.
 * There is no mask and no padding mask (the decoder gives its self-attention none), so every row has an attendable key; a call
 * with a mask keeps the torch chain.
 * Geometry: heads in {4, 8}, 1 <= num_query <= 512 (the backward keeps the keys and values of one (image, head) in LDS: 64 KiB
 * at 512), batch <= 65535 and each operand below 2^31 elements; anything else returns PCT_ERR_UNSUPPORTED and the caller keeps
 * the torch chain.  No speed rule beyond that: forward + backward were measured faster than the torch chain at 100, 300 and
 * 512 queries (profiles/self_attn_train.json).  batch or num_query == 0: PCT_OK, nothing launched.
 * One launch on `stream`, no allocation, no host synchronisation. */
PCT_API int pct_self_attention_forward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                           const float *v, int batch, int heads, int num_query, float scale, float *out,
                                           float *lse, void *stream);

/* Backward of the above.  The five operands and scale as given to the forward; lse as it wrote it;
 *   out                       the forward's output.  Not read (D is formed from P and dP, see workspace); may be NULL.  Kept so
 *                             that the entry takes what a backward of this operation is handed
 *   grad_out                  [num_query, batch, heads * 16] fp32, dense, 16-byte aligned
 *   workspace                 device scratch, 16-byte aligned: batch * heads * num_query floats (D = rowsum(grad_out * out), formed
 *                             once per call as the equal sum over the keys of P dP, the form torch's softmax backward evaluates)
 *   grad_q, grad_k, grad_v    in the operands' layout, 16-byte aligned, fully overwritten.  grad_q is the gradient of q_content
 *                             and of q_pos, grad_k that of k_content and of k_pos (the add's backward is the identity)
 * P = exp(scale * s - lse) is recomputed per 16 x 16 tile.  No floating-point atomic: a key's rows are summed by the one wave
 * that owns them over the queries in ascending order, a query's row and its D by four waves over interleaved key tiles and
 * then in wave order -- two calls on the same operands give the same bits.
 * Status rules and geometry as the forward.  Two launches on `stream` (query side with D, then key side), no allocation, no
 * host synchronisation. */
PCT_API int pct_self_attention_backward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                            const float *v, const float *out, const float *lse, const float *grad_out, int batch,
                                            int heads, int num_query, float scale, float *workspace, float *grad_q, float *grad_k,
                                            float *grad_v, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_SELF_ATTN_TRAIN_H */
