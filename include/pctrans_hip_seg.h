/* The decoder's semantic head in eval mode: entry points of libpctrans_hip.so on bf16 maps.  Included by pctrans_hip.h (status
 * codes, PCT_API, conventions: there); include that header, not this one.  The caller
 * (pctrans_amd/fused_ops.py: seg_head_forward) takes them only for bf16 maps under autocast with gradients disabled and
 * BatchNorm in eval mode; training, GroupNorm variants and other channel counts keep the torch expression.
 *
 * Common to both entries (csrc/conv3x3_bn_relu.hip):
 *   x, mid        bf16 as raw bit patterns, dense: channels_last == 0 [batch, 128, height, width] (2-byte aligned),
 *                 channels_last != 0 [batch, height, width, 128] (16-byte aligned) -- the layout the pixel decoder's mask
 *                 features have as a view of the encoder's token rows
 *   w             [128, 128, 3, 3] fp32 (the module's parameter; rounded to bf16 per call, as autocast does), no convolution bias
 *   mean, var, gamma, beta   [128] fp32: the BatchNorm's running statistics and affine parameters, read on every call
 *   w_ws          device workspace, 16-byte aligned, refilled on every call: 128 * 128 * 9 * 2 bytes per 3x3 convolution
 * The 3x3 convolution has stride 1, padding 1, dilation 1.  Rounding points are the torch chain's: the convolution's fp32
 * accumulator is rounded to bf16, (z - mean) * rsqrt(var + eps) * gamma + beta is evaluated in fp32 and rounded to bf16, then
 * max(., 0).  channels != 128 or height * width >= 2^24: PCT_ERR_UNSUPPORTED.  batch == 0 returns 0 and launches nothing. */
#ifndef PCTRANS_HIP_SEG_H
#define PCTRANS_HIP_SEG_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one block: replaces Sequential(Conv2d(128, 128, 3, padding=1, bias=False), BatchNorm2d(128).eval(), ReLU) of
 * transformer_decoder/conv_with_kaiming_uniform.py:125-169 as the decoder builds it for `seg_head` ------------------------------
 *   out: 128 channels, in the layout of x.  Two launches on `stream`. */
PCT_API int pct_conv3x3_bn_relu_bf16(const void *x, const float *w, const float *mean, const float *var, const float *gamma,
                                     const float *beta, float eps, void *w_ws, int batch, int channels, int height, int width,
                                     int channels_last, void *out, void *stream);

/* ---- the whole head: replaces `self.logits(self.seg_head(mask_features))` (mask2former_transformer_decoder.py:533-534): two
 * blocks as above and Conv2d(128, 1, 1) -----------------------------------------------------------------------------------------
 *   w_logits [128] fp32 (rounded to bf16 per call), b_logits [1] fp32 or NULL; the sum over the channels is accumulated in fp32,
 *   the bias added in fp32, the result rounded to bf16
 *   w_ws: twice the size above; mid: the first block's output in the layout of x, caller-owned scratch of x's size
 *   out [batch, 1, height, width] bf16, 2-byte aligned.  The second block's 128-channel map is never written.  Three launches on `stream`. */
PCT_API int pct_seg_head_bf16(const void *x, const float *w_a, const float *mean_a, const float *var_a, const float *gamma_a,
                              const float *beta_a, float eps_a, const float *w_b, const float *mean_b, const float *var_b,
                              const float *gamma_b, const float *beta_b, float eps_b, const float *w_logits,
                              const float *b_logits, void *w_ws, void *mid, int batch, int channels, int height, int width,
                              int channels_last, void *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_SEG_H */
