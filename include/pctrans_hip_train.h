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

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_TRAIN_H */
