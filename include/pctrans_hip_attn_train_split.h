/* Differentiable fp32 cross-attention of the decoder with the keys divided over several workgroups: entry points of
 * libpctrans_hip.so.  Included by pctrans_hip.h (status codes, PCT_API, conventions: there); include that header, not this one.
 * The caller (pctrans_amd/split_key_attention_train.py, reached with CrossAttentionLayer.attn_train_split = "hip") takes them for
 * what pctrans_hip_attn_train.h's entries cover, at key counts that caller's plan routes.  Kernels:
 * csrc/cross_attention_train_split.hip on csrc/attn_train_common.hpp. */
#ifndef PCTRANS_HIP_ATTN_TRAIN_SPLIT_H
#define PCTRANS_HIP_ATTN_TRAIN_SPLIT_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- bytes of workspace the two entries below need for these arguments (one figure, enough for either direction) ---------------
 * With R = batch * heads * num_query rows: 136 * splits * R + 4 * R, each part rounded up to 16 bytes -- the backward's fp64
 * partial D per (split, row), D per row, and the unscaled partial grad_q (2 * 16 floats) per (split, row).  The forward uses the
 * first 76 * splits * R bytes: per (split, row) the maximum as fp64, the row sum and 16 unnormalised sums as fp32.  At 2 images, 8
 * heads, 300 queries and 16 splits: 10.0 MiB.  Negative: the status the compute entries give for these arguments --
 * PCT_ERR_BAD_ARG for batch < 0, heads <= 0, num_query < 0, splits < 1 or splits > 16; PCT_ERR_UNSUPPORTED for heads outside
 * {4, 8}. */
PCT_API long long pct_cross_attention_split_train_workspace(int batch, int heads, int num_query, int splits);

/* ---- pct_cross_attention_forward_f32 (pctrans_hip_attn_train.h) with the keys of every 16-query workgroup divided over
 * min(splits, ceil(num_key / 64)) workgroups ------------------------------------------------------------------------------------
 * The operands of that entry with its layouts, alignment and meaning; then
 *   splits      1 .. 16.  The call's C = ceil(num_key / 64) chunks of 64 keys are divided in order: split j of s = min(splits, C)
 *               walks the chunks floor(j * C / s) .. floor((j + 1) * C / s) - 1 and leaves, per image, head and query, the
 *               maximum m_j of its scores (fp64; -inf where the query has no live key there), its row sum l_j and its 16
 *               unnormalised sums acc_j relative to m_j (fp32), formed exactly as the unsplit kernel forms them over those keys
 *   workspace   pct_cross_attention_split_train_workspace(batch, heads, num_query, splits) bytes, 16-byte aligned.  Every word
 *               that is read is written by this call first: the contents before the call do not matter
 * A second launch combines in ascending j, in fp64: M = max m_j, l = sum l_j exp(m_j - M), acc = sum acc_j exp(m_j - M); l and
 * acc are rounded once to fp32, out = acc / l in fp32, lse = M + log(l) from the fp64 sum, in the two planes of the unsplit entry.
 * A query with nothing attendable: out = 0, lse = 0 in both planes, as there.
 * splits == 1 (or num_key <= 64) gives the bits of pct_cross_attention_forward_f32 in out and lse; with any splits so does a query
 * whose live keys all lie in one split's chunks.  The same arguments give the same bits in every call.
 * Status, in this order: that of pct_cross_attention_forward_f32 for its arguments, with `workspace` among the pointers that may
 * be neither NULL (PCT_ERR_BAD_ARG) nor off 16 bytes (PCT_ERR_ALIGNMENT) -- PCT_OK without a launch for batch, num_query or
 * num_key == 0 included; PCT_ERR_UNSUPPORTED for a geometry outside that entry's; PCT_ERR_BAD_ARG for splits < 1, splits > 16 or
 * workspace_bytes below the need.  Nothing is launched unless the status is PCT_OK.  Two launches on `stream`, no allocation, no
 * host synchronisation, no floating-point atomic. */
PCT_API int pct_cross_attention_split_forward_f32(const float *q_content, const float *q_pos, const float *k_content,
                                                  const float *k_pos, const float *v, const unsigned char *mask,
                                                  const unsigned char *row_open, int batch, int heads, int num_query, int num_key,
                                                  float scale, int splits, void *workspace, long long workspace_bytes, float *out,
                                                  float *lse, void *stream);

/* Backward of the above: pct_cross_attention_backward_f32 with the two sweeps of its query pass divided the same way.  The
 * arguments of that entry (`out` is not read and may be NULL) with `splits`, `workspace` and `workspace_bytes` as above in place
 * of its float workspace; lse as either forward wrote it.  Four launches on `stream`, in this order:
 *   1  per split, sum_k P dP over its keys: the four waves' fp64 sums added in wave order, kept as fp64 per (split, row)
 *   2  D of a row = those partial sums added in ascending j, rounded once to fp32 (written for launch 3); then per split
 *      dq += k^T dS^T over its keys, the four waves' sums added in wave order, unscaled, to the workspace
 *   3  the key pass of the unsplit entry, unchanged: grad_k_content, grad_k_pos, grad_v
 *   4  grad_q_content, grad_q_pos = (0 + the splits' dq in ascending j) * scale
 * splits == 1 (or num_key <= 64) gives the bits of pct_cross_attention_backward_f32 in all five gradients; with any splits a
 * query whose live keys all lie in one split's chunks has that entry's D and grad_q rows, and if every query of the call is such
 * a row all five gradients have its bits.  No floating-point atomic and no counter: two calls on the same arguments give the same
 * bits.  Status rules as the forward.  No allocation, no host synchronisation. */
PCT_API int pct_cross_attention_split_backward_f32(const float *q_content, const float *q_pos, const float *k_content,
                                                   const float *k_pos, const float *v, const unsigned char *mask,
                                                   const unsigned char *row_open, const float *out, const float *lse,
                                                   const float *grad_out, int batch, int heads, int num_query, int num_key,
                                                   float scale, int splits, void *workspace, long long workspace_bytes,
                                                   float *grad_q_content, float *grad_q_pos, float *grad_k_content,
                                                   float *grad_k_pos, float *grad_v, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_ATTN_TRAIN_SPLIT_H */
