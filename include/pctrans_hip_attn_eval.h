/* The decoder's cross- and self-attention in fp32 evaluation: entry points of libpctrans_hip.so.  Included by pctrans_hip.h
 * (status codes, PCT_API, conventions: there); include that header, not this one.  The caller (pctrans_amd/attention_eval.py,
 * reached with CrossAttentionLayer.attn_eval / SelfAttentionLayer.attn_eval = "hip") takes them only for fp32 device operands
 * outside autocast when no gradient is required; everything else keeps the branch it had (the bf16 kernels, the training
 * kernels, or the torch chain of transformer_decoder/attention.py: attention_core). */
#ifndef PCTRANS_HIP_ATTN_EVAL_H
#define PCTRANS_HIP_ATTN_EVAL_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- replaces, per cross-attention layer of an fp32 evaluation forward (mask2former_transformer_decoder.py: CrossAttentionLayer),
 *          q = cat([q_content, q_pos] per head); k = cat([k_content, k_pos] per head)          two concatenation passes
 *          out = softmax(masked_fill(q * scale . k^T, mask & ~row_open, -inf)) . v              attention_core
 *      (csrc/attention_eval.hip) --------------------------------------------------------------------------------------------
 * Operands, layouts, alignment, the mask and row_open conventions and the arithmetic are those of
 * pct_cross_attention_forward_f32 (pctrans_hip_attn_train.h), and `out` has the same bits as that entry's on the same
 * operands.  What differs: no lse is written (there is no backward), and a wave loads its next 16 keys while it works on the
 * current ones -- the key counts here are those of whole images (4 096 - 5 655 on the finest level).
 *   q_content, q_pos          [num_query, batch, heads * 16] fp32, dense, 16-byte aligned
 *   k_content, k_pos, v       [num_key, batch, heads * 16] fp32, dense, 16-byte aligned
 *   mask                      [batch, num_query, num_key] bytes, nonzero = may not attend; NULL = no mask
 *   row_open                  [batch, num_query] bytes, nonzero = this query ignores its row of `mask`; NULL = none does
 *                             (ignored without a mask)
 *   scale                     the factor on the scores: (2 * 16)^-0.5 for the decoder's [content 16 | position 16] heads
 *   out                       [num_query, batch, heads * 16] fp32, 16-byte aligned
 * A query with nothing attendable (every key masked, row_open not set): out = 0, where torch's masked softmax gives NaN.
 * Geometry: heads in {4, 8}, any num_query >= 1 and num_key >= 1 with batch <= 65535 and each operand below 2^31 elements;
 * anything else returns PCT_ERR_UNSUPPORTED and the caller keeps the torch chain.  batch, num_query or num_key == 0: PCT_OK,
 * nothing launched.  Speed rule, applied by the caller and not by this entry (pctrans_amd/attention_eval.py: supported): as
 * replays of a HIP graph the kernel took 0.25 - 0.61 x the torch chain's time at every shape timed (100 queries at 256 / 1 024 /
 * 4 096 keys, 300 queries at 374 / 1 452 / 5 655 keys, 1 / 8 / 32 images, 8 heads; profiles/attention_eval.json) except 100
 * queries of one image on 4 096 keys (56 workgroups of 64 key steps: 1.005 x, a tie).  The layers send calls of up to 5 655
 * keys, 600 queries and 32 images, and above 1 452 keys only grids of at least 152 workgroups (ceil(num_query / 16) * heads *
 * batch; the smallest that was timed faster there); everything else keeps the torch chain.
 * One launch on `stream`, no allocation, no host synchronisation. */
PCT_API int pct_cross_attention_eval_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                         const float *v, const unsigned char *mask, const unsigned char *row_open, int batch,
                                         int heads, int num_query, int num_key, float scale, float *out, void *stream);

/* ---- replaces, per self-attention layer of an fp32 evaluation forward (SelfAttentionLayer),
 *          q = q_content + q_pos; k = k_content + k_pos                                         two adds
 *          out = softmax((q * scale) . k^T) . v  per head, with its permutes                    attention_core
 * The five operands [num_query, batch, heads * 16] fp32, dense, 16-byte aligned, and the arithmetic as
 * pct_self_attention_forward_f32 (pctrans_hip_self_attn_train.h), with the same bits in `out`; no lse, and no limit on
 * num_query (the 512 of that header is its backward's).  No mask.
 * Geometry: heads in {4, 8}, num_query >= 1, batch <= 65535, each operand below 2^31 elements; anything else returns
 * PCT_ERR_UNSUPPORTED.  batch or num_query == 0: PCT_OK, nothing launched.  Speed rule of the caller: faster than the torch chain
 * at all of 100 / 300 / 600 queries and 1 / 8 / 32 images (0.28 - 0.50 x); it sends calls of up to 600 queries and 32 images.
 * One launch on `stream`, no allocation, no host synchronisation. */
PCT_API int pct_self_attention_eval_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                        const float *v, int batch, int heads, int num_query, float scale, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_ATTN_EVAL_H */
