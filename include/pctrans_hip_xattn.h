/* The decoder's split-operand cross-attention for any key count: entry point of libpctrans_hip.so.  Included by pctrans_hip.h
 * (status codes, PCT_API, conventions: there); include that header, not this one.  The caller
 * (pctrans_amd/ragged_attention.py: cross_attention, reached with CrossAttentionLayer.ragged_keys = "hip") takes it for bf16
 * device tensors with gradients disabled.  Kernel: csrc/cross_attention.hip, the RAGGED instantiations. */
#ifndef PCTRANS_HIP_XATTN_H
#define PCTRANS_HIP_XATTN_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- pct_cross_attention_bf16 (pctrans_hip.h) without its num_key % 64 == 0 condition ---------------------------------------
 * The same operands, layouts and arithmetic; the same result, bit for bit, as pct_masked_attention_bf16 on the per-head
 * concatenated operands with head_dim 32, for every num_key >= 1, and as pct_cross_attention_bf16 where that covers the call.
 *   q_content, q_pos [Q, N, heads*16]   k_content, k_pos, v [S, N, heads*16]   bfloat16, 16-byte aligned
 *   mask        [N, Q, mask_pitch] bytes, 16-byte aligned, or NULL (mask_pitch is then ignored): byte s < S of a row nonzero =
 *               that query may not attend to key s.  mask_pitch % 16 == 0 and mask_pitch >= S; the bytes of a row at positions
 *               >= S are never trusted (they may be uninitialised), and no byte at or past mask_pitch is read
 *   row_open    [N, Q] bytes or NULL: nonzero = ignore this query's mask row.  An opened row attends to every key < S and to
 *               nothing else
 *   out         [Q, N, heads*16] bfloat16, 8-byte aligned
 * Nothing past key S - 1 of k_content, k_pos or v is read.  A fully masked row that is not opened yields NaN, as there.
 * Status, in this order: PCT_ERR_BAD_ARG for batch < 0, heads <= 0, num_query < 0, num_key < 1, and with a mask for
 * mask_pitch < num_key or mask_pitch % 16 != 0; PCT_OK without a launch for batch == 0 or num_query == 0; PCT_ERR_BAD_ARG for
 * a null operand; PCT_ERR_ALIGNMENT; PCT_ERR_UNSUPPORTED for heads % 4 != 0 or an operand of 2^31 - 1 elements or more.  One
 * launch on `stream`. */
PCT_API int pct_cross_attention_ragged_bf16(const void *q_content, const void *q_pos, const void *k_content, const void *k_pos,
                                            const void *v, const unsigned char *mask, int mask_pitch,
                                            const unsigned char *row_open, int batch, int heads, int num_query, int num_key,
                                            float scale, void *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_XATTN_H */
