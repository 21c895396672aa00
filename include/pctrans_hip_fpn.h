/* One FPN level of the pixel decoder in eval mode: entry point of libpctrans_hip.so on fp32 maps.  Included by pctrans_hip.h
 * (status codes, PCT_API, conventions: there); include that header, not this one.  The caller (pctrans_amd/fused_ops.py:
 * fpn_stage, reached with MSDeformAttnPixelDecoder.fpn = "hip") takes it only for fp32 device maps outside autocast with no
 * gradient required and norms with fixed statistics; GroupNorm, LayerNorm, training mode and resize ratios other than 2 keep
 * the torch statements. */
#ifndef PCTRANS_HIP_FPN_H
#define PCTRANS_HIP_FPN_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- replaces, per FPN level (pixel_decoder/msdeformattn.py:302-305),
 *          cur_fpn = lateral_conv(x)                                      1x1 convolution (+ bias) + norm
 *          y = enc + F.interpolate(cur_fpn, size=enc.shape[-2:], mode="bilinear", align_corners=False)
 *          out = output_conv(y)                                           3x3 convolution (+ bias) + norm + ReLU
 *      for x twice as high and wide as enc, where the resize is the 2 x 2 mean (csrc/fpn_stage.hip) -----------------------------
 *   x            [batch, in_channels, 2 * height, 2 * width] fp32, dense NCHW, 16-byte aligned; in_channels % 16 == 0
 *   enc          [batch, 128, height, width] fp32, read where it lies, images enc_batch_stride floats apart
 *                (>= 128 * height * width): enc_channels_last == 0 dense NCHW per image (4-byte aligned);
 *                enc_channels_last != 0 [height, width, 128] per image, as a view of the encoder's token rows (16-byte
 *                aligned, enc_batch_stride % 4 == 0)
 *   w_lateral    [128, in_channels] fp32; w_output [128, 128, 3, 3] fp32 (stride 1, zero padding 1); b_* [128] fp32 or NULL
 *   mean_*, var_*, gamma_*, beta_*, eps_*   the norm behind each convolution as its fixed statistics and affine, [128] fp32:
 *                (v - mean) / sqrt(var + eps) * gamma + beta.  mean == NULL and var == NULL: no norm (gamma, beta ignored);
 *                one of the four missing otherwise: PCT_ERR_BAD_ARG
 *   w_ws         device workspace, 16-byte aligned, refilled on every call: (in_channels / 16 + 72) * 12288 bytes
 *   y_ws         device scratch, 16-byte aligned: batch * 128 * height * width floats (enc + resized lateral, in a layout of the
 *                kernels' own)
 *   out          [batch, 128, height, width] fp32, dense NCHW
 * Every product is evaluated in split bf16 (three bf16 pieces per fp32 operand, six partial products, fp32 accumulation): as
 * accurate as the fp32 convolutions it replaces (tests/test_fpn_stage_gpu.py, against float64).  Any height, width >= 1.
 * channels != 128, in_channels % 16 != 0 or height * width >= 2^24: PCT_ERR_UNSUPPORTED.  batch == 0 returns 0 and launches
 * nothing.  Three launches on `stream`, no host synchronisation, no allocation. */
PCT_API int pct_fpn_stage_f32(const float *x, const float *enc, long long enc_batch_stride, int enc_channels_last,
                              const float *w_lateral, const float *b_lateral, const float *mean_lateral, const float *var_lateral,
                              const float *gamma_lateral, const float *beta_lateral, float eps_lateral, const float *w_output,
                              const float *b_output, const float *mean_output, const float *var_output, const float *gamma_output,
                              const float *beta_output, float eps_output, void *w_ws, float *y_ws, int batch, int in_channels,
                              int channels, int height, int width, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCTRANS_HIP_FPN_H */
