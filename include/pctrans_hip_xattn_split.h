/* The decoder's split-operand cross-attention with the keys divided over several workgroups: entry points of libpctrans_hip.so.
 * Included by pctrans_hip.h (status codes, PCT_API, conventions: there); include that header, not this one.  The caller
 * (pctrans_amd/split_key_attention.py: cross_attention, reached with CrossAttentionLayer.split_keys = "hip") takes it for bf16
 * device tensors with gradients disabled, on grids too small to fill the device.  Kernels: csrc/cross_attention.hip, the PARTIAL
 * instantiations and cross_attention_combine_kernel. */
#ifndef PCTRANS_HIP_XATTN_SPLIT_H
#define PCTRANS_HIP_XATTN_SPLIT_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- bytes of workspace pct_cross_attention_split_keys_bf16 needs for these arguments ------------------------------------------
 * splits * batch * heads * num_query records of 16 + 1 + 1 floats (unnormalised output, running maximum, running sum); 0 for
 * splits == 1, batch == 0 or num_query == 0.  Negative: the status the compute entry gives for these arguments -- PCT_ERR_BAD_ARG
 * for batch < 0, heads <= 0, num_query < 0, splits < 1 or splits > 16; PCT_ERR_UNSUPPORTED for heads % 4 != 0. */
PCT_API long long pct_cross_attention_split_keys_workspace(int batch, int heads, int num_query, int splits);

/* ---- pct_cross_attention_ragged_bf16 (pctrans_hip_xattn.h) with the keys of every (image, 4 heads, 4 query tiles) divided over
 * `splits` workgroups ----------------------------------------------------------------------------------------------------------
 * The operands of that entry, in its order, with its layouts, alignment and meaning; then
 *   splits      1 .. min(16, ceil(num_key / 64)).  The call's ceil(num_key / 64) chunks of 64 keys are divided in order: split j
 *               walks the chunks floor(j * nch / splits) .. floor((j + 1) * nch / splits) - 1 and leaves, per query and head, its
 *               unnormalised output o_j (16 floats, relative to its running maximum m_j), m_j and its sum l_j in the workspace
 *   workspace   pct_cross_attention_split_keys_workspace(...) bytes, 16-byte aligned; may be NULL for splits == 1.  Every word
 *               the combine reads is written by this call first: the contents before the call do not matter
 * A second launch combines in ascending j: M = max m_j, w_j = exp(m_j - M) (0 where m_j = -inf), L = sum w_j l_j,
 * out = bf16(sum w_j o_j * (1 / L)).  A row without a live key in any split yields NaN, as there.  The same arguments give the
 * same bits in every call.  splits == 1 is pct_cross_attention_ragged_bf16 itself: one launch, its bits.
 * Nothing past key num_key - 1, past mask_pitch or past workspace_bytes is touched; no allocation, no host synchronisation.
 * Status, in this order: that of pct_cross_attention_ragged_bf16 for its arguments (PCT_OK without a launch for batch == 0 or
 * num_query == 0 included); PCT_ERR_BAD_ARG for splits < 1, splits > min(16, ceil(num_key / 64)), or with splits >= 2 a NULL
 * workspace or workspace_bytes below the need; PCT_ERR_ALIGNMENT for a workspace off 16 bytes.  splits >= 2: two launches on
 * `stream`. */
PCT_API int pct_cross_attention_split_keys_bf16(const void *q_content, const void *q_pos, const void *k_content, const void *k_pos,
                                                const void *v, const unsigned char *mask, int mask_pitch,
                                                const unsigned char *row_open, int batch, int heads, int num_query, int num_key,
                                                float scale, int splits, void *workspace, long long workspace_bytes, void *out,
                                                void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_XATTN_SPLIT_H */
