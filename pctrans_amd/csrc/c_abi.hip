// extern "C" surface of libpctrans_hip.so -- see include/pctrans_hip.h for the contract and the reference
// interfaces (file:line) each entry point replaces.  Argument validation mirrors the reference host wrappers
// (ops/src/cuda/ms_deform_attn_cuda.cu:33-57, 98-122); device/contiguity checks need tensor metadata and live in
// the Python shim (pctrans_amd/MultiScaleDeformableAttention.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "launchers.hpp"
#include "msda_common.hpp"

namespace {

int check_common(const void *value, const int64_t *shapes, const int64_t *starts, const void *loc,
                 const void *attn, int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                 size_t elem, size_t loc_elem)
{
  if (N < 0 || S < 0 || Lq < 0 || M <= 0 || D <= 0 || L <= 0 || P <= 0 || im2col_step <= 0) return PCT_ERR_BAD_ARG;
  if (N == 0) return PCT_OK;
  const int step = N < im2col_step ? N : im2col_step;
  if (N % step != 0) return PCT_ERR_IM2COL_STEP;  // cu:57
  if (Lq == 0) return PCT_OK;                     // nothing to sample: empty loc / attn may be null
  if (!value || !shapes || !starts || !loc || !attn) return PCT_ERR_BAD_ARG;
  // per-image offsets are 32-bit in the kernels (as in the reference, cuh:260-283)
  if ((long long)S * M * D >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  if ((uintptr_t)value % elem || (uintptr_t)loc % loc_elem || (uintptr_t)attn % loc_elem ||
      (uintptr_t)shapes % 8 || (uintptr_t)starts % 8)
    return PCT_ERR_ALIGNMENT;
  return PCT_OK;
}

// A launcher's status as the ABI reports it.  PCT_NOT_COVERED never crosses the ABI: from a launcher that has no other kernel to
// fall back on it is PCT_ERR_UNSUPPORTED (`not_covered`: where a launcher uses it for something else); every other status is
// a PCT_ERR_* or a hipError_t already.
int abi_status(int rc, int not_covered = PCT_ERR_UNSUPPORTED) { return rc == pct::PCT_NOT_COVERED ? not_covered : rc; }

// launch(sub-call) for the batch in chunks of images whose value tensor stays below 2 GiB (at least one image): the specialised
// kernels address one launch's value tensor with 32-bit byte offsets, as the reference chunks with im2col_step (cu:66-80) --
// same results.  elem / loc_elem: bytes per element of value and out / of loc and attn.  Stops at the first status that is
// not 0 and returns it.
template <typename Launch>
int for_image_chunks(const pct::MsdaFwdCall &c, size_t elem, size_t loc_elem, Launch launch)
{
  const long long image_bytes = (long long)c.S * c.M * c.D * (long long)elem;
  int chunk = c.N;
  while (chunk > 1 && (long long)chunk * image_bytes >= 0x7fffffffLL) chunk = (chunk + 1) / 2;
  for (int b0 = 0; b0 < c.N; b0 += chunk) {
    const int rc = launch(c.images(b0, c.N - b0 < chunk ? c.N - b0 : chunk, elem, loc_elem));
    if (rc != 0) return rc;
  }
  return PCT_OK;
}

template <typename T, typename LT>
int forward_impl(const void *value, const int64_t *shapes, const int64_t *starts, const LT *loc, const LT *attn,
                 int N, int S, int M, int D, int L, int Lq, int P, int im2col_step, void *out, void *stream)
{
  const int rc = check_common(value, shapes, starts, loc, attn, N, S, M, D, L, Lq, P, im2col_step,
                              sizeof(typename pct::Traits<T>::store_t), sizeof(LT));
  if (rc != PCT_OK) return rc;
  if (N == 0 || Lq == 0) return PCT_OK;
  if (!out) return PCT_ERR_BAD_ARG;
  if ((uintptr_t)out % sizeof(typename pct::Traits<T>::store_t)) return PCT_ERR_ALIGNMENT;
  const pct::MsdaFwdCall call{value, shapes, starts, loc, attn, N, S, M, D, L, Lq, P, out, static_cast<hipStream_t>(stream), nullptr, 0};
  return for_image_chunks(call, sizeof(typename pct::Traits<T>::store_t), sizeof(LT), pct::launch_msda_forward<T>);
}

template <typename A>
int backward_impl(const A *value, const int64_t *shapes, const int64_t *starts, const A *loc, const A *attn,
                  const A *grad_out, int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                  A *grad_value, A *grad_loc, A *grad_attn, void *stream)
{
  const int rc = check_common(value, shapes, starts, loc, attn, N, S, M, D, L, Lq, P, im2col_step, sizeof(A),
                              sizeof(A));
  if (rc != PCT_OK) return rc;
  if (N == 0) return PCT_OK;
  if (!grad_value || !grad_loc || !grad_attn || (Lq > 0 && !grad_out)) return PCT_ERR_BAD_ARG;
  if ((uintptr_t)grad_out % sizeof(A) || (uintptr_t)grad_value % sizeof(A) || (uintptr_t)grad_loc % sizeof(A) ||
      (uintptr_t)grad_attn % sizeof(A))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_msda_backward<A>(
      {value, shapes, starts, loc, attn, grad_out, N, S, M, D, L, Lq, P, grad_value, grad_loc, grad_attn, static_cast<hipStream_t>(stream)});
}

// The arguments the three dynamic-mask-head entry points share.  They differ in the workspace (`has_ws`: required, aligned to
// ws_mask + 1) and in the alignment of up_logits (up_mask + 1).  PCT_OK also for an empty call: the caller returns then.
int check_dyn_mask_head(const float *mask_feat, const float *ref_points, const float *params, int batch, int channels,
                        int num_query, int height, int width, int stride, int rel_coord, int target_h, int target_w,
                        const void *up_logits, unsigned up_mask, bool has_ws, const void *ws, unsigned ws_mask,
                        const unsigned char *attn_mask)
{
  if (batch < 0 || num_query < 0 || channels <= 0 || height <= 0 || width <= 0 || stride <= 0 || target_h <= 0 ||
      target_w <= 0)
    return PCT_ERR_BAD_ARG;
  if (batch == 0 || num_query == 0) return PCT_OK;
  if (!mask_feat || !params || !up_logits || !attn_mask || (has_ws && !ws) || (rel_coord && !ref_points)) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)mask_feat | (uintptr_t)params | (uintptr_t)ref_points) & 3u) return PCT_ERR_ALIGNMENT;
  if (((uintptr_t)up_logits & up_mask) || (has_ws && ((uintptr_t)ws & ws_mask))) return PCT_ERR_ALIGNMENT;
  if ((long long)height * width >= 0x7fffffffLL / 64) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

// the second operand of the K = 128 entry points (x_add == NULL: none)
int check_x_add(const float *x_add, long long ld_add, long long add_period)
{
  if (!x_add) return PCT_OK;
  if (ld_add < 128 || (ld_add & 3) || ((uintptr_t)x_add & 15u)) return PCT_ERR_ALIGNMENT;
  if (add_period < 32 || add_period * ld_add * 4 > 0x7fffffffLL) return PCT_ERR_BAD_ARG;
  return PCT_OK;
}

// The arguments the instance post-processing entries share.  PCT_OK also for an empty call (batch == 0): the caller returns then.
int check_instance_post(int batch, int num_query, int h, int w, int height, int width, int dataset)
{
  if (batch < 0 || num_query < 0 || h <= 0 || w <= 0 || height <= 0 || width <= 0 || (dataset != 0 && dataset != 1))
    return PCT_ERR_BAD_ARG;
  if ((long long)h * w >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  return pct::instance_geometry_status(batch, num_query, height, width);
}

int instance_masks_impl(const void *logits, int bf16, int batch, int num_query, int h, int w, int height, int width, int dataset,
                        uint32_t *bits, int32_t *areas, void *stream)
{
  const int rc = check_instance_post(batch, num_query, h, w, height, width, dataset);
  if (rc != PCT_OK || batch == 0 || num_query == 0) return rc;
  if (!logits || !bits || !areas) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)logits & (bf16 ? 1u : 3u)) || ((uintptr_t)bits & 15u) || ((uintptr_t)areas & 3u)) return PCT_ERR_ALIGNMENT;
  return pct::launch_instance_masks(logits, bf16, batch, num_query, h, w, height, width, dataset, bits, areas,
                                    static_cast<hipStream_t>(stream));
}

// no query: every label is background
int instance_labels_empty(int batch, int height, int width, int16_t *labels, void *stream)
{
  if (!labels) return PCT_ERR_BAD_ARG;
  return (int)hipMemsetAsync(labels, 0, (size_t)batch * height * width * sizeof(int16_t), static_cast<hipStream_t>(stream));
}

int instance_labels_impl(const void *logits, int bf16, int batch, int num_query, int h, int w, int height, int width, int dataset,
                         void *workspace, int16_t *labels, void *stream)
{
  const int rc = check_instance_post(batch, num_query, h, w, height, width, dataset);
  if (rc != PCT_OK || batch == 0) return rc;
  if (num_query == 0) return instance_labels_empty(batch, height, width, labels, stream);
  if (!logits || !workspace || !labels) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)logits & (bf16 ? 1u : 3u)) || ((uintptr_t)workspace & 15u) || ((uintptr_t)labels & 1u)) return PCT_ERR_ALIGNMENT;
  return pct::launch_instance_labels(logits, bf16, batch, num_query, h, w, height, width, dataset, workspace, labels,
                                     static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int pct_instance_masks_f32(const float *logits, int batch, int num_query, int h, int w, int height, int width, int dataset,
                           uint32_t *bits, int32_t *areas, void *stream)
{
  return instance_masks_impl(logits, 0, batch, num_query, h, w, height, width, dataset, bits, areas, stream);
}

int pct_instance_masks_bf16(const void *logits, int batch, int num_query, int h, int w, int height, int width, int dataset,
                            uint32_t *bits, int32_t *areas, void *stream)
{
  return instance_masks_impl(logits, 1, batch, num_query, h, w, height, width, dataset, bits, areas, stream);
}

int pct_instance_labels_from_bits(const uint32_t *bits, const int32_t *areas, int batch, int num_query, int height, int width,
                                  int dataset, void *workspace, int16_t *labels, void *stream)
{
  const int rc = check_instance_post(batch, num_query, 1, 1, height, width, dataset);
  if (rc != PCT_OK || batch == 0) return rc;
  if (num_query == 0) return instance_labels_empty(batch, height, width, labels, stream);
  if (!bits || !areas || !workspace || !labels) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)bits & 15u) || ((uintptr_t)areas & 3u) || ((uintptr_t)workspace & 15u) || ((uintptr_t)labels & 1u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_instance_labels_from_bits(bits, areas, batch, num_query, height, width, dataset, workspace, labels,
                                               static_cast<hipStream_t>(stream));
}

int pct_instance_labels_f32(const float *logits, int batch, int num_query, int h, int w, int height, int width, int dataset,
                            void *workspace, int16_t *labels, void *stream)
{
  return instance_labels_impl(logits, 0, batch, num_query, h, w, height, width, dataset, workspace, labels, stream);
}

int pct_instance_labels_bf16(const void *logits, int batch, int num_query, int h, int w, int height, int width, int dataset,
                             void *workspace, int16_t *labels, void *stream)
{
  return instance_labels_impl(logits, 1, batch, num_query, h, w, height, width, dataset, workspace, labels, stream);
}

int pct_conv3x3_bn_relu_bf16(const void *x, const float *w, const float *mean, const float *var, const float *gamma,
                             const float *beta, float eps, void *w_ws, int batch, int channels, int height, int width,
                             int channels_last, void *out, void *stream)
{
  if (batch < 0 || channels <= 0 || height <= 0 || width <= 0) return PCT_ERR_BAD_ARG;
  if (batch == 0) return PCT_OK;
  if (!x || !w || !mean || !var || !gamma || !beta || !w_ws || !out) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)x | (uintptr_t)out) & (channels_last ? 15u : 1u)) ||
      (((uintptr_t)w | (uintptr_t)mean | (uintptr_t)var | (uintptr_t)gamma | (uintptr_t)beta) & 3u) || ((uintptr_t)w_ws & 15u))
    return PCT_ERR_ALIGNMENT;
  const float *const bnp[4] = {mean, var, gamma, beta};
  return abi_status(pct::launch_conv3x3_bn_relu(x, channels_last, w, bnp, eps, w_ws, batch, channels, height, width, out,
                                                static_cast<hipStream_t>(stream)));
}

int pct_seg_head_bf16(const void *x, const float *w_a, const float *mean_a, const float *var_a, const float *gamma_a,
                      const float *beta_a, float eps_a, const float *w_b, const float *mean_b, const float *var_b,
                      const float *gamma_b, const float *beta_b, float eps_b, const float *w_logits, const float *b_logits, void *w_ws,
                      void *mid, int batch, int channels, int height, int width, int channels_last, void *out, void *stream)
{
  if (batch < 0 || channels <= 0 || height <= 0 || width <= 0) return PCT_ERR_BAD_ARG;
  if (batch == 0) return PCT_OK;
  const float *const bn_a[4] = {mean_a, var_a, gamma_a, beta_a}, *const bn_b[4] = {mean_b, var_b, gamma_b, beta_b};
  uintptr_t f32_bits = (uintptr_t)w_a | (uintptr_t)w_b | (uintptr_t)w_logits | (uintptr_t)b_logits;
  for (int i = 0; i < 4; ++i) {
    if (!bn_a[i] || !bn_b[i]) return PCT_ERR_BAD_ARG;
    f32_bits |= (uintptr_t)bn_a[i] | (uintptr_t)bn_b[i];
  }
  if (!x || !w_a || !w_b || !w_logits || !w_ws || !mid || !out) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)x | (uintptr_t)mid) & (channels_last ? 15u : 1u)) || ((uintptr_t)out & 1u) || (f32_bits & 3u) || ((uintptr_t)w_ws & 15u)) return PCT_ERR_ALIGNMENT;
  return abi_status(pct::launch_seg_head(x, channels_last, w_a, bn_a, eps_a, w_b, bn_b, eps_b, w_logits, b_logits, w_ws, mid, batch, channels,
                                         height, width, out, static_cast<hipStream_t>(stream)));
}

int pct_fpn_stage_f32(const float *x, const float *enc, long long enc_batch_stride, int enc_channels_last, const float *w_lateral,
                      const float *b_lateral, const float *mean_lateral, const float *var_lateral, const float *gamma_lateral,
                      const float *beta_lateral, float eps_lateral, const float *w_output, const float *b_output,
                      const float *mean_output, const float *var_output, const float *gamma_output, const float *beta_output,
                      float eps_output, void *w_ws, float *y_ws, int batch, int in_channels, int channels, int height, int width,
                      float *out, void *stream)
{
  if (batch < 0 || in_channels <= 0 || channels <= 0 || height <= 0 || width <= 0) return PCT_ERR_BAD_ARG;
  if (enc_batch_stride < (long long)channels * height * width) return PCT_ERR_BAD_ARG;
  if (batch == 0) return PCT_OK;
  if (!x || !enc || !w_lateral || !w_output || !w_ws || !y_ws || !out) return PCT_ERR_BAD_ARG;
  const float *const n1[4] = {mean_lateral, var_lateral, gamma_lateral, beta_lateral};
  const float *const n3[4] = {mean_output, var_output, gamma_output, beta_output};
  uintptr_t f32_bits = (uintptr_t)w_lateral | (uintptr_t)b_lateral | (uintptr_t)w_output | (uintptr_t)b_output | (uintptr_t)out;
  for (int i = 0; i < 4; ++i) {                                    /* a norm is given whole or not at all */
    if ((n1[0] && !n1[i]) || (n3[0] && !n3[i]) || (!n1[0] && n1[1]) || (!n3[0] && n3[1])) return PCT_ERR_BAD_ARG;
    if (n1[0]) f32_bits |= (uintptr_t)n1[i];
    if (n3[0]) f32_bits |= (uintptr_t)n3[i];
  }
  if (channels != 128 || in_channels % 16 || (long long)height * width >= (1LL << 24)) return PCT_ERR_UNSUPPORTED;
  if ((((uintptr_t)x | (uintptr_t)w_ws | (uintptr_t)y_ws) & 15u) || (f32_bits & 3u) ||
      ((uintptr_t)enc & (enc_channels_last ? 15u : 3u)) || (enc_channels_last && (enc_batch_stride & 3)))
    return PCT_ERR_ALIGNMENT;
  return abi_status(pct::launch_fpn_stage(x, enc, enc_batch_stride, enc_channels_last, w_lateral, b_lateral, n1, eps_lateral, w_output,
                                          b_output, n3, eps_output, w_ws, y_ws, batch, in_channels, height, width, out,
                                          static_cast<hipStream_t>(stream)));
}

int pct_abi_version(void) { return PCT_ABI_VERSION; }

const char *pct_error_string(int code)
{
  switch (code) {
    case PCT_OK: return "ok";
    case PCT_ERR_BAD_ARG: return "bad argument (null pointer or non-positive size)";
    case PCT_ERR_IM2COL_STEP: return "batch must be divisible by min(batch, im2col_step)";
    case PCT_ERR_ALIGNMENT: return "pointer not aligned to its element size";
    case PCT_ERR_UNSUPPORTED: return "shape not supported by the gfx950 kernels";
    default: break;
  }
  if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
  return "unknown error";
}

int pct_ms_deform_attn_forward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                   const float *sampling_loc, const float *attn_weight, int batch,
                                   int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                   int num_point, int im2col_step, float *output, void *stream)
{
  return forward_impl<float, float>(value, spatial_shapes, level_start, sampling_loc, attn_weight, batch,
                                    spatial_size, num_heads, channels, num_levels, num_query, num_point,
                                    im2col_step, output, stream);
}

int pct_ms_deform_attn_forward_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                   const double *sampling_loc, const double *attn_weight, int batch,
                                   int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                   int num_point, int im2col_step, double *output, void *stream)
{
  return forward_impl<double, double>(value, spatial_shapes, level_start, sampling_loc, attn_weight, batch,
                                      spatial_size, num_heads, channels, num_levels, num_query, num_point,
                                      im2col_step, output, stream);
}

int pct_ms_deform_attn_forward_f16(const void *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                   const float *sampling_loc, const float *attn_weight, int batch,
                                   int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                   int num_point, int im2col_step, void *output, void *stream)
{
  return forward_impl<pct::half_bits, float>(value, spatial_shapes, level_start, sampling_loc, attn_weight, batch,
                                             spatial_size, num_heads, channels, num_levels, num_query, num_point,
                                             im2col_step, output, stream);
}

int pct_ms_deform_attn_forward_bf16(const void *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                    const float *sampling_loc, const float *attn_weight, int batch,
                                    int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                    int num_point, int im2col_step, void *output, void *stream)
{
  return forward_impl<pct::bf16_bits, float>(value, spatial_shapes, level_start, sampling_loc, attn_weight, batch,
                                             spatial_size, num_heads, channels, num_levels, num_query, num_point,
                                             im2col_step, output, stream);
}

int pct_ms_deform_attn_fused_forward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                         const float *ref_points, long long ref_batch_stride, const float *offsets,
                                         const float *attn_logits, int batch, int spatial_size, int num_heads,
                                         int channels, int num_levels, int num_query, int num_point, float *output,
                                         void *stream)
{
  const int rc = check_common(value, spatial_shapes, level_start, offsets, attn_logits, batch, spatial_size, num_heads,
                              channels, num_levels, num_query, num_point, 1, sizeof(float), sizeof(float));
  if (rc != PCT_OK) return rc;
  if (batch == 0 || num_query == 0) return PCT_OK;
  if (!output || !ref_points || ref_batch_stride < 0) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)output | (uintptr_t)ref_points) & 3u) return PCT_ERR_ALIGNMENT;
  const pct::MsdaFwdCall call{value, spatial_shapes, level_start, offsets, attn_logits, batch, spatial_size, num_heads, channels,
                              num_levels, num_query, num_point, output, static_cast<hipStream_t>(stream), ref_points, ref_batch_stride};
  return abi_status(for_image_chunks(call, sizeof(float), sizeof(float), pct::launch_msda_forward_special<float>));
}

int pct_ms_deform_attn_forward_planes_f32(const float *value_planes, const int64_t *spatial_shapes, const int64_t *level_start,
                                          const float *loc_planes, const float *attn_planes, const float *ref_points,
                                          long long ref_batch_stride, int batch, int spatial_size, int num_heads, int channels,
                                          int num_levels, int num_query, int num_point, float *output, void *stream)
{
  const int rc = check_common(value_planes, spatial_shapes, level_start, loc_planes, attn_planes, batch, spatial_size, num_heads,
                              channels, num_levels, num_query, num_point, 1, sizeof(float), sizeof(float));
  if (rc != PCT_OK) return rc;
  if (batch == 0 || num_query == 0) return PCT_OK;
  if (!output || ref_batch_stride < 0) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)output | (uintptr_t)ref_points) & 3u) return PCT_ERR_ALIGNMENT;
  if (num_query != spatial_size || channels != 16 || num_point != 4) return PCT_ERR_UNSUPPORTED;
  const pct::MsdaFwdCall call{value_planes, spatial_shapes, level_start, loc_planes, attn_planes, batch, spatial_size, num_heads,
                              channels, num_levels, num_query, num_point, output, static_cast<hipStream_t>(stream), ref_points,
                              ref_batch_stride};
  return abi_status(for_image_chunks(call, sizeof(float), sizeof(float), pct::launch_msda_forward_planes));
}

int pct_ms_deform_attn_backward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                    const float *sampling_loc, const float *attn_weight, const float *grad_output,
                                    int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                    int num_query, int num_point, int im2col_step, float *grad_value,
                                    float *grad_sampling_loc, float *grad_attn_weight, void *stream)
{
  return backward_impl<float>(value, spatial_shapes, level_start, sampling_loc, attn_weight, grad_output, batch,
                              spatial_size, num_heads, channels, num_levels, num_query, num_point, im2col_step,
                              grad_value, grad_sampling_loc, grad_attn_weight, stream);
}

int pct_ms_deform_attn_backward_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                    const double *sampling_loc, const double *attn_weight,
                                    const double *grad_output, int batch, int spatial_size, int num_heads,
                                    int channels, int num_levels, int num_query, int num_point, int im2col_step,
                                    double *grad_value, double *grad_sampling_loc, double *grad_attn_weight,
                                    void *stream)
{
  return backward_impl<double>(value, spatial_shapes, level_start, sampling_loc, attn_weight, grad_output, batch,
                               spatial_size, num_heads, channels, num_levels, num_query, num_point, im2col_step,
                               grad_value, grad_sampling_loc, grad_attn_weight, stream);
}

int pct_ms_deform_attn_fused_backward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                          const float *ref_points, long long ref_batch_stride, const float *offsets,
                                          const float *attn_logits, const float *grad_output, int batch, int spatial_size,
                                          int num_heads, int channels, int num_levels, int num_query, int num_point,
                                          int im2col_step, void *workspace, float *grad_value, float *grad_offsets,
                                          float *grad_logits, void *stream)
{
  const int rc = check_common(value, spatial_shapes, level_start, offsets, attn_logits, batch, spatial_size, num_heads, channels,
                              num_levels, num_query, num_point, im2col_step, sizeof(float), sizeof(float));
  if (rc != PCT_OK) return rc;
  if (batch == 0 || num_query == 0) return PCT_OK;
  if (!ref_points || ref_batch_stride < 0 || !grad_output || !workspace || !grad_value || !grad_offsets || !grad_logits)
    return PCT_ERR_BAD_ARG;
  const long long LP = (long long)num_levels * num_point;
  if (LP > 64 || LP % 4 || num_point % 2) return PCT_ERR_UNSUPPORTED;
  if ((((uintptr_t)ref_points | (uintptr_t)grad_output | (uintptr_t)grad_value) & 3u) ||
      (((uintptr_t)offsets | (uintptr_t)attn_logits | (uintptr_t)workspace | (uintptr_t)grad_offsets | (uintptr_t)grad_logits) & 15u))
    return PCT_ERR_ALIGNMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long records = (long long)batch * num_query * num_heads;
  float *loc = static_cast<float *>(workspace), *w = loc + records * LP * 2;     // LP % 4 == 0: w is 16-byte aligned too
  int st = pct::launch_msda_fused_expand(attn_logits, offsets, ref_points, ref_batch_stride, spatial_shapes, records, num_heads,
                                         num_query, num_levels, num_point, loc, w, s);
  if (st != 0) return abi_status(st);
  st = pct::launch_msda_backward<float>({value, spatial_shapes, level_start, loc, w, grad_output, batch, spatial_size, num_heads,
                                         channels, num_levels, num_query, num_point, grad_value, grad_offsets, grad_logits, s});
  if (st != 0) return st;
  return abi_status(pct::launch_msda_fused_fold(w, spatial_shapes, records, num_levels, num_point, grad_offsets, grad_logits, s));
}

int pct_dynamic_mask_head_forward(const float *mask_feat, const float *ref_points, const float *params, int batch,
                                  int channels, int num_query, int height, int width, int stride, int rel_coord,
                                  int target_h, int target_w, int out_dtype, void *up_logits,
                                  unsigned char *attn_mask, void *stream)
{
  const int rc = check_dyn_mask_head(mask_feat, ref_points, params, batch, channels, num_query, height, width, stride, rel_coord,
                                     target_h, target_w, up_logits, 15u, false, nullptr, 0u, attn_mask);
  if (rc != PCT_OK || batch == 0 || num_query == 0) return rc;
  return pct::launch_dyn_mask_head(mask_feat, ref_points, params, batch, channels, num_query, height, width, stride,
                                   rel_coord, target_h, target_w, out_dtype, up_logits, attn_mask,
                                   static_cast<hipStream_t>(stream));
}

int pct_dynamic_mask_head_forward_mfma(const float *mask_feat, const float *ref_points, const float *params, int batch,
                                       int channels, int num_query, int height, int width, int stride, int rel_coord,
                                       int target_h, int target_w, void *scratch, void *up_logits,
                                       unsigned char *attn_mask, void *stream)
{
  const int rc = check_dyn_mask_head(mask_feat, ref_points, params, batch, channels, num_query, height, width, stride, rel_coord,
                                     target_h, target_w, up_logits, 7u, true, scratch, 1u, attn_mask);
  if (rc != PCT_OK || batch == 0 || num_query == 0) return rc;
  return pct::launch_dyn_mask_head_mfma(mask_feat, ref_points, params, batch, channels, num_query, height, width,
                                        stride, rel_coord, target_h, target_w, scratch, up_logits, attn_mask,
                                        static_cast<hipStream_t>(stream));
}

int pct_dynamic_mask_head_forward_fused_bf16(const float *mask_feat, const float *ref_points, const float *params, int batch,
                                             int channels, int num_query, int height, int width, int stride,
                                             int rel_coord, int target_h, int target_w, void *workspace,
                                             void *up_logits, unsigned char *attn_mask, void *stream)
{
  const int rc = check_dyn_mask_head(mask_feat, ref_points, params, batch, channels, num_query, height, width, stride, rel_coord,
                                     target_h, target_w, up_logits, 15u, true, workspace, 15u, attn_mask);
  if (rc != PCT_OK || batch == 0 || num_query == 0) return rc;
  return abi_status(pct::launch_dyn_mask_head_fused(mask_feat, ref_points, params, batch, channels, num_query, height, width,
                                                    stride, rel_coord, target_h, target_w, workspace, up_logits, attn_mask,
                                                    static_cast<hipStream_t>(stream)));
}

int pct_dynamic_mask_head_backward_f32(const float *mask_feat, const float *ref_points, const float *params,
                                       const float *grad_up, int batch, int channels, int num_query, int height, int width,
                                       int stride, int rel_coord, void *workspace, float *grad_feat, float *grad_ref,
                                       float *grad_params, void *stream)
{
  if (batch < 0 || num_query < 0 || channels <= 0 || height <= 0 || width <= 0 || stride <= 0) return PCT_ERR_BAD_ARG;
  if (!grad_feat && batch > 0) return PCT_ERR_BAD_ARG;
  if (channels != 16) return PCT_ERR_UNSUPPORTED;
  if (batch > 65535 || (long long)height * width >= 0x7fffffffLL / 64) return PCT_ERR_UNSUPPORTED;
  if (batch == 0) return PCT_OK;
  if (num_query == 0)        // no query: the feature gradient is zero, the other outputs are empty
    return pct::launch_dyn_mask_head_bwd(mask_feat, ref_points, params, grad_up, batch, channels, 0, height, width, stride,
                                         rel_coord, workspace, grad_feat, grad_ref, grad_params,
                                         static_cast<hipStream_t>(stream));
  if (!mask_feat || !params || !grad_up || !workspace || !grad_params || (rel_coord && (!ref_points || !grad_ref)))
    return PCT_ERR_BAD_ARG;
  if (((uintptr_t)mask_feat | (uintptr_t)params | (uintptr_t)ref_points | (uintptr_t)grad_feat | (uintptr_t)grad_ref |
       (uintptr_t)grad_params) & 3u)
    return PCT_ERR_ALIGNMENT;
  if (((uintptr_t)grad_up & 7u) || ((uintptr_t)workspace & 15u)) return PCT_ERR_ALIGNMENT;     // grad_up: 8-byte loads
  return pct::launch_dyn_mask_head_bwd(mask_feat, ref_points, params, grad_up, batch, channels, num_query, height, width, stride,
                                       rel_coord, workspace, grad_feat, grad_ref, grad_params,
                                       static_cast<hipStream_t>(stream));
}

int pct_point_sample_f32(const float *planes, const int32_t *plane_index, const float *coords, int num_planes, int height,
                         int width, int num_out, int num_points, int coord_rows, int planes_per_coord_row, float *out,
                         void *stream)
{
  if (num_planes < 0 || height <= 0 || width <= 0 || num_out < 0 || num_points < 0 || coord_rows < 0 || planes_per_coord_row < 1)
    return PCT_ERR_BAD_ARG;
  if (num_out == 0 || num_points == 0) return PCT_OK;
  if (!planes || !coords || !out || num_planes == 0 || (num_out - 1) / planes_per_coord_row >= coord_rows) return PCT_ERR_BAD_ARG;
  if (!plane_index && num_out > num_planes) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)planes | (uintptr_t)plane_index | (uintptr_t)out) & 3u) || ((uintptr_t)coords & 7u)) return PCT_ERR_ALIGNMENT;
  return pct::launch_point_sample(planes, plane_index, coords, num_planes, height, width, num_out, num_points,
                                  planes_per_coord_row, out, static_cast<hipStream_t>(stream));
}

int pct_point_mask_loss_forward_f32(const float *pred, const int32_t *src_index, int num_pred_planes, int height, int width,
                                    const float *tgt, const int32_t *tgt_index, int num_tgt_planes, int tgt_height,
                                    int tgt_width, const float *coords, int num_pairs, int num_points, float *x, float *t,
                                    float *sums, void *stream)
{
  // The one-head case of the _many entry (so is the selection below): its checks in its order, its launch.
  // A NULL `pred` is the table's missing entry, PCT_ERR_BAD_ARG, and is seen before any alignment, pred's own included.
  const float *const one[1] = {pred};
  return pct_point_mask_loss_forward_many_f32(one, 1, src_index, num_pred_planes, height, width, tgt, tgt_index, num_tgt_planes,
                                              tgt_height, tgt_width, coords, num_pairs, num_points, x, t, sums, stream);
}

int pct_point_mask_loss_backward_f32(const float *x, const float *t, const float *coords, const float *alpha, const float *beta,
                                     const float *gamma, int num_pairs, int num_points, int height, int width,
                                     float *grad_planes, void *stream)
{
  if (num_pairs < 0 || num_points < 0 || height <= 0 || width <= 0) return PCT_ERR_BAD_ARG;
  if (num_pairs == 0 || num_points == 0) return PCT_OK;
  if (!x || !t || !coords || !alpha || !beta || !gamma || !grad_planes) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)x | (uintptr_t)t | (uintptr_t)alpha | (uintptr_t)beta | (uintptr_t)gamma | (uintptr_t)grad_planes) & 3u) ||
      ((uintptr_t)coords & 7u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_point_loss_backward(x, t, coords, alpha, beta, gamma, num_pairs, num_points, height, width, grad_planes,
                                         static_cast<hipStream_t>(stream));
}

int pct_point_select_uncertain_f32(const float *pred, const int32_t *src_index, int num_pred_planes, int height, int width,
                                   const float *cand_coords, int num_pairs, int num_cand, int num_keep, float *out_coords,
                                   int out_row_points, int32_t *out_index, void *stream)
{
  const float *const one[1] = {pred};
  return pct_point_select_uncertain_many_f32(one, 1, src_index, num_pred_planes, height, width, cand_coords, num_pairs, num_cand,
                                             num_keep, out_coords, out_row_points, out_index, stream);
}

int pct_point_match_cost_f32(const float *pred, int batch, int num_query, int height, int width, const float *tgt,
                             int num_tgt_planes, int tgt_height, int tgt_width, const int32_t *tgt_start, const int32_t *tgt_count,
                             int max_targets, const float *coords, int num_points, float cost_mask, float cost_dice,
                             void *workspace, float *cost, void *stream)
{
  if (batch < 0 || num_query < 0 || height <= 0 || width <= 0 || num_tgt_planes < 0 || tgt_height <= 0 || tgt_width <= 0 ||
      max_targets < 0 || num_points < 0)
    return PCT_ERR_BAD_ARG;
  if (batch == 0 || num_query == 0 || max_targets == 0 || num_points == 0) return PCT_OK;
  if (!pred || (!tgt && num_tgt_planes > 0) || !tgt_start || !tgt_count || !coords || !workspace || !cost) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)pred | (uintptr_t)tgt | (uintptr_t)tgt_start | (uintptr_t)tgt_count | (uintptr_t)cost) & 3u) ||
      ((uintptr_t)coords & 7u) || ((uintptr_t)workspace & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_point_match_cost(pred, batch, num_query, height, width, tgt, num_tgt_planes, tgt_height, tgt_width, tgt_start,
                                      tgt_count, max_targets, coords, num_points, cost_mask, cost_dice, workspace, cost,
                                      static_cast<hipStream_t>(stream));
}

// The head table of the *_many entries: PCT_OK when 0 < num_heads <= PCT_POINT_MAX_HEADS entries are all present and 4-byte
// aligned.  num_heads == 0 is the callers' own early return.
static int point_heads_status(const float *const *preds, int num_heads)
{
  if (num_heads < 0 || num_heads > PCT_POINT_MAX_HEADS || !preds) return PCT_ERR_BAD_ARG;
  uintptr_t bits = 0;
  for (int h = 0; h < num_heads; ++h) {
    if (!preds[h]) return PCT_ERR_BAD_ARG;
    bits |= (uintptr_t)preds[h];
  }
  return (bits & 3u) ? PCT_ERR_ALIGNMENT : PCT_OK;
}

int pct_point_select_uncertain_many_f32(const float *const *preds, int num_heads, const int32_t *src_index, int num_pred_planes,
                                        int height, int width, const float *cand_coords, int num_pairs, int num_cand, int num_keep,
                                        float *out_coords, int out_row_points, int32_t *out_index, void *stream)
{
  if (num_heads < 0 || num_heads > PCT_POINT_MAX_HEADS || num_pred_planes < 0 || height <= 0 || width <= 0 || num_pairs < 0 ||
      num_cand < 0 || num_keep < 0 || num_keep > num_cand || out_row_points < num_keep)
    return PCT_ERR_BAD_ARG;
  if (num_heads == 0 || num_pairs == 0 || num_keep == 0) return PCT_OK;
  if (!preds || !cand_coords || !out_coords || num_pred_planes == 0) return PCT_ERR_BAD_ARG;
  if (!src_index && num_pairs > num_pred_planes) return PCT_ERR_BAD_ARG;
  if (const int rc = point_heads_status(preds, num_heads); rc != PCT_OK) return rc;
  if ((((uintptr_t)src_index | (uintptr_t)out_index) & 3u) || (((uintptr_t)cand_coords | (uintptr_t)out_coords) & 7u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_point_select_many(preds, num_heads, src_index, num_pred_planes, height, width, cand_coords, num_pairs, num_cand,
                                       num_keep, out_coords, out_row_points, out_index, static_cast<hipStream_t>(stream));
}

int pct_point_mask_loss_forward_many_f32(const float *const *preds, int num_heads, const int32_t *src_index, int num_pred_planes,
                                         int height, int width, const float *tgt, const int32_t *tgt_index, int num_tgt_planes,
                                         int tgt_height, int tgt_width, const float *coords, int num_pairs, int num_points, float *x,
                                         float *t, float *sums, void *stream)
{
  if (num_heads < 0 || num_heads > PCT_POINT_MAX_HEADS || num_pred_planes < 0 || num_tgt_planes < 0 || height <= 0 || width <= 0 ||
      tgt_height <= 0 || tgt_width <= 0 || num_pairs < 0 || num_points < 0)
    return PCT_ERR_BAD_ARG;
  if (num_heads == 0 || num_pairs == 0 || num_points == 0) return PCT_OK;
  if (!preds || !tgt || !coords || !x || !t || !sums || num_pred_planes == 0 || num_tgt_planes == 0) return PCT_ERR_BAD_ARG;
  if ((!src_index && num_pairs > num_pred_planes) || (!tgt_index && num_pairs > num_tgt_planes)) return PCT_ERR_BAD_ARG;
  if (const int rc = point_heads_status(preds, num_heads); rc != PCT_OK) return rc;
  if ((((uintptr_t)src_index | (uintptr_t)tgt | (uintptr_t)tgt_index | (uintptr_t)x | (uintptr_t)t | (uintptr_t)sums) & 3u) ||
      ((uintptr_t)coords & 7u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_point_loss_forward_many(preds, num_heads, src_index, num_pred_planes, height, width, tgt, tgt_index,
                                             num_tgt_planes, tgt_height, tgt_width, coords, num_pairs, num_points, x, t, sums,
                                             static_cast<hipStream_t>(stream));
}

int pct_point_match_cost_many_f32(const float *const *preds, int num_heads, int batch, int num_query, int height, int width,
                                  const float *tgt, int num_tgt_planes, int tgt_height, int tgt_width, const int32_t *tgt_start,
                                  const int32_t *tgt_count, int max_targets, const float *coords, int num_points, float cost_mask,
                                  float cost_dice, void *workspace, float *cost, void *stream)
{
  if (num_heads < 0 || num_heads > PCT_POINT_MAX_HEADS || batch < 0 || num_query < 0 || height <= 0 || width <= 0 ||
      num_tgt_planes < 0 || tgt_height <= 0 || tgt_width <= 0 || max_targets < 0 || num_points < 0)
    return PCT_ERR_BAD_ARG;
  if (num_heads == 0 || batch == 0 || num_query == 0 || max_targets == 0 || num_points == 0) return PCT_OK;
  if (!preds || (!tgt && num_tgt_planes > 0) || !tgt_start || !tgt_count || !coords || !workspace || !cost) return PCT_ERR_BAD_ARG;
  if (const int rc = point_heads_status(preds, num_heads); rc != PCT_OK) return rc;
  if ((((uintptr_t)tgt | (uintptr_t)tgt_start | (uintptr_t)tgt_count | (uintptr_t)cost) & 3u) || ((uintptr_t)coords & 7u) ||
      ((uintptr_t)workspace & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_point_match_cost_many(preds, num_heads, batch, num_query, height, width, tgt, num_tgt_planes, tgt_height,
                                           tgt_width, tgt_start, tgt_count, max_targets, coords, num_points, cost_mask, cost_dice,
                                           workspace, cost, static_cast<hipStream_t>(stream));
}

int pct_instance_label_map_f32(const float *planes, int num_planes, int plane_height, int plane_width, const int32_t *plane_start,
                               const int32_t *plane_count, int batch, int height, int width, int32_t *labels, void *stream)
{
  if (num_planes < 0 || plane_height <= 0 || plane_width <= 0 || batch < 0 || height <= 0 || width <= 0) return PCT_ERR_BAD_ARG;
  if (batch == 0) return PCT_OK;
  if ((!planes && num_planes > 0) || !plane_start || !plane_count || !labels) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)planes | (uintptr_t)plane_start | (uintptr_t)plane_count | (uintptr_t)labels) & 3u) return PCT_ERR_ALIGNMENT;
  return pct::launch_instance_label_map(planes, num_planes, plane_height, plane_width, plane_start, plane_count, batch, height,
                                        width, labels, static_cast<hipStream_t>(stream));
}

int pct_discriminative_loss_forward_f32(const float *embedding, const int32_t *labels, int batch, int channels, int height,
                                        int width, int num_labels, float delta_v, float delta_d, float alpha, float beta,
                                        float gama, void *workspace, float *table, float *loss, int32_t *status, void *stream)
{
  if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0 || num_labels <= 0) return PCT_ERR_BAD_ARG;
  if (!embedding || !labels || !workspace || !table || !loss || !status) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)embedding | (uintptr_t)labels | (uintptr_t)table | (uintptr_t)loss | (uintptr_t)status) & 3u) ||
      ((uintptr_t)workspace & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_emb_loss_forward(embedding, labels, batch, channels, height, width, num_labels, delta_v, delta_d, alpha, beta,
                                      gama, workspace, table, loss, status, static_cast<hipStream_t>(stream));
}

int pct_discriminative_loss_backward_f32(const float *embedding, const int32_t *labels, const float *table, const float *grad_out,
                                         int batch, int channels, int height, int width, int num_labels, float delta_v,
                                         float *grad_embedding, void *stream)
{
  if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0 || num_labels <= 0) return PCT_ERR_BAD_ARG;
  if (!embedding || !labels || !table || !grad_out || !grad_embedding) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)embedding | (uintptr_t)labels | (uintptr_t)table | (uintptr_t)grad_out | (uintptr_t)grad_embedding) & 3u)
    return PCT_ERR_ALIGNMENT;
  return pct::launch_emb_loss_backward(embedding, labels, table, grad_out, batch, channels, height, width, num_labels, delta_v,
                                       grad_embedding, static_cast<hipStream_t>(stream));
}

int pct_reid_dice_rows_forward_f32(const float *logits, const int32_t *image_start, const int32_t *key, int batch, int num_query,
                                   int height, int width, int num_rows, void *workspace, float *sums, float *dice, int32_t *status,
                                   void *stream)
{
  if (batch <= 0 || num_query <= 0 || height <= 0 || width <= 0 || num_rows < 0) return PCT_ERR_BAD_ARG;
  if (num_rows == 0) return PCT_OK;
  if (!logits || !image_start || !key || !workspace || !sums || !dice || !status) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)logits | (uintptr_t)image_start | (uintptr_t)key | (uintptr_t)sums | (uintptr_t)dice | (uintptr_t)status) & 3u) ||
      ((uintptr_t)workspace & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_reid_dice_forward(logits, image_start, key, batch, num_query, height, width, num_rows, workspace, sums, dice,
                                       status, static_cast<hipStream_t>(stream));
}

int pct_reid_dice_rows_backward_f32(const float *logits, const int32_t *image_start, const int32_t *key, const float *dice,
                                    const float *sums, const float *grad_dice, int batch, int num_query, int height, int width,
                                    int num_rows, void *workspace, float *grad_logits, void *stream)
{
  if (batch <= 0 || num_query <= 0 || height <= 0 || width <= 0 || num_rows < 0) return PCT_ERR_BAD_ARG;
  if (!logits || !image_start || !workspace || !grad_logits) return PCT_ERR_BAD_ARG;
  if (num_rows > 0 && (!key || !dice || !sums || !grad_dice)) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)logits | (uintptr_t)image_start | (uintptr_t)key | (uintptr_t)dice | (uintptr_t)sums | (uintptr_t)grad_dice |
        (uintptr_t)grad_logits) & 3u) || ((uintptr_t)workspace & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_reid_dice_backward(logits, image_start, key, dice, sums, grad_dice, batch, num_query, height, width, num_rows,
                                        workspace, grad_logits, static_cast<hipStream_t>(stream));
}

int pct_refpoint_l1_forward_f32(const float *points, const float *target_points, const int32_t *src, const int32_t *tgt, int heads,
                                long long rows, int dims, int num_targets, int pairs, float num_masks, float *loss,
                                int32_t *status, void *stream)
{
  if (heads < 0 || rows < 0 || dims <= 0 || num_targets < 0 || pairs < 0) return PCT_ERR_BAD_ARG;
  if (heads == 0) return PCT_OK;
  if (!loss || !status || (pairs > 0 && (!points || !target_points || !src || !tgt))) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)points | (uintptr_t)target_points | (uintptr_t)src | (uintptr_t)tgt | (uintptr_t)loss | (uintptr_t)status) & 3u)
    return PCT_ERR_ALIGNMENT;
  return pct::launch_refpoint_l1_forward(points, target_points, src, tgt, heads, rows, dims, num_targets, pairs, num_masks, loss,
                                         status, static_cast<hipStream_t>(stream));
}

int pct_refpoint_l1_backward_f32(const float *points, const float *target_points, const int32_t *src, const int32_t *tgt,
                                 const float *grad_loss, int heads, long long rows, int dims, int num_targets, int pairs,
                                 float num_masks, float *grad_points, void *stream)
{
  if (heads < 0 || rows < 0 || dims <= 0 || num_targets < 0 || pairs < 0) return PCT_ERR_BAD_ARG;
  if (heads == 0 || rows == 0) return PCT_OK;
  if (!points || !grad_loss || !grad_points || (pairs > 0 && (!target_points || !src || !tgt))) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)points | (uintptr_t)target_points | (uintptr_t)src | (uintptr_t)tgt | (uintptr_t)grad_loss |
       (uintptr_t)grad_points) & 3u)
    return PCT_ERR_ALIGNMENT;
  return pct::launch_refpoint_l1_backward(points, target_points, src, tgt, grad_loss, heads, rows, dims, num_targets, pairs,
                                          num_masks, grad_points, static_cast<hipStream_t>(stream));
}

int pct_sigmoid_focal_strided_forward_f32(const float *logits, const void *fg, int fg_dtype, int batch, int out_h, int out_w,
                                          int height, int width, int stride, float alpha, void *workspace, float *loss,
                                          float *num_pos, void *stream)
{
  if (batch <= 0 || out_h <= 0 || out_w <= 0 || height <= 0 || width <= 0 || stride <= 0) return PCT_ERR_BAD_ARG;
  if (!logits || !fg || !workspace || !loss || !num_pos) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)logits | (uintptr_t)loss | (uintptr_t)num_pos | (fg_dtype == 4 ? (uintptr_t)fg : 0)) & 3u) ||
      ((uintptr_t)workspace & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_sigmoid_focal_strided_forward(logits, fg, fg_dtype, batch, out_h, out_w, height, width, stride, alpha,
                                                   workspace, loss, num_pos, static_cast<hipStream_t>(stream));
}

int pct_sigmoid_focal_strided_backward_f32(const float *logits, const void *fg, int fg_dtype, const float *num_pos,
                                           const float *grad_loss, int batch, int out_h, int out_w, int height, int width,
                                           int stride, float alpha, float *grad_logits, void *stream)
{
  if (batch <= 0 || out_h <= 0 || out_w <= 0 || height <= 0 || width <= 0 || stride <= 0) return PCT_ERR_BAD_ARG;
  if (!logits || !fg || !num_pos || !grad_loss || !grad_logits) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)logits | (uintptr_t)num_pos | (uintptr_t)grad_loss | (uintptr_t)grad_logits |
       (fg_dtype == 4 ? (uintptr_t)fg : 0)) & 3u)
    return PCT_ERR_ALIGNMENT;
  return pct::launch_sigmoid_focal_strided_backward(logits, fg, fg_dtype, num_pos, grad_loss, batch, out_h, out_w, height, width,
                                                    stride, alpha, grad_logits, static_cast<hipStream_t>(stream));
}

int pct_reid_nearest_positive_f32(const float *query, const int32_t *pos, int num_query, int batch, int channels, int max_pos,
                                  int32_t *nearest, void *stream)
{
  if (num_query <= 0 || batch <= 0 || channels <= 0 || max_pos <= 0) return PCT_ERR_BAD_ARG;
  if (!query || !pos || !nearest) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)query & 15u) || (((uintptr_t)pos | (uintptr_t)nearest) & 3u)) return PCT_ERR_ALIGNMENT;
  return pct::launch_reid_nearest_positive(query, pos, num_query, batch, channels, max_pos, nearest,
                                           static_cast<hipStream_t>(stream));
}

int pct_reid_query_rows_forward_f32(const float *query, const int32_t *image_start, const int32_t *key, int num_query, int batch,
                                    int channels, int num_rows, float *norm, float *dots, float *cosines, void *stream)
{
  if (num_query <= 0 || batch <= 0 || channels <= 0 || num_rows < 0) return PCT_ERR_BAD_ARG;
  if (num_rows == 0) return PCT_OK;
  if (!query || !image_start || !key || !norm || !dots || !cosines) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)query & 15u) ||
      (((uintptr_t)image_start | (uintptr_t)key | (uintptr_t)norm | (uintptr_t)dots | (uintptr_t)cosines) & 3u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_reid_query_rows_forward(query, image_start, key, num_query, batch, channels, num_rows, norm, dots, cosines,
                                             static_cast<hipStream_t>(stream));
}

int pct_reid_query_rows_backward_f32(const float *query, const int32_t *image_start, const int32_t *key, const float *norm,
                                     const float *cosines, const float *grad_dots, const float *grad_cosines, int num_query,
                                     int batch, int channels, int num_rows, void *workspace, float *grad_query, void *stream)
{
  if (num_query <= 0 || batch <= 0 || channels <= 0 || num_rows < 0) return PCT_ERR_BAD_ARG;
  if (!query || !image_start || !workspace || !grad_query) return PCT_ERR_BAD_ARG;
  if (num_rows > 0 && (!key || !norm || !cosines || !grad_dots || !grad_cosines)) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)query | (uintptr_t)workspace | (uintptr_t)grad_query) & 15u) ||
      (((uintptr_t)image_start | (uintptr_t)key | (uintptr_t)norm | (uintptr_t)cosines | (uintptr_t)grad_dots |
        (uintptr_t)grad_cosines) & 3u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_reid_query_rows_backward(query, image_start, key, norm, cosines, grad_dots, grad_cosines, num_query, batch,
                                              channels, num_rows, workspace, grad_query, static_cast<hipStream_t>(stream));
}

int pct_contrast_loss_rows_f32(const float *rows, const int32_t *image_of, const int32_t *key, const int32_t *owner, int num_rows,
                               int num_query, int batch, float inv_temperature, float *loss, float *coef, void *stream)
{
  if (num_rows < 0 || num_query <= 0 || batch <= 0 || !(inv_temperature > 0.f)) return PCT_ERR_BAD_ARG;
  if (num_rows == 0) return PCT_OK;
  if (!rows || !image_of || !key || !owner || !loss || !coef) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)rows | (uintptr_t)image_of | (uintptr_t)key | (uintptr_t)owner | (uintptr_t)loss | (uintptr_t)coef) & 3u)
    return PCT_ERR_ALIGNMENT;
  return pct::launch_contrast_loss_rows(rows, image_of, key, owner, num_rows, num_query, batch, inv_temperature, loss, coef,
                                        static_cast<hipStream_t>(stream));
}

int pct_instance_targets_census(const void *labels, int dtype, int batch, int height, int width, int ignore_label, void *workspace,
                                int32_t *ids, int32_t *pixels, float *centres, int32_t *num, int32_t *status, void *stream)
{
  if (batch <= 0 || height <= 0 || width <= 0) return PCT_ERR_BAD_ARG;
  if (!labels || !workspace || !ids || !pixels || !centres || !num || !status) return PCT_ERR_BAD_ARG;
  static const uintptr_t elem[5] = {1, 2, 4, 8, 4};
  if (dtype < 0 || dtype > 4) return PCT_ERR_UNSUPPORTED;
  if (((uintptr_t)labels & (elem[dtype] - 1)) || (((uintptr_t)ids | (uintptr_t)pixels | (uintptr_t)num | (uintptr_t)status) & 3u) ||
      ((uintptr_t)centres & 7u) || ((uintptr_t)workspace & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_instance_targets_census(labels, dtype, batch, height, width, ignore_label, workspace, ids, pixels, centres, num,
                                             status, static_cast<hipStream_t>(stream));
}

int pct_instance_targets_planes(const void *labels, int dtype, int batch, int height, int width, const void *workspace,
                                const int32_t *counts, long long total_planes, int max_count, int32_t *starts, uint8_t *masks,
                                float *planes, uint8_t *fg, void *stream)
{
  if (batch <= 0 || height <= 0 || width <= 0 || total_planes <= 0 || max_count <= 0) return PCT_ERR_BAD_ARG;
  if (!labels || !workspace || !counts || !starts || !masks) return PCT_ERR_BAD_ARG;
  static const uintptr_t elem[5] = {1, 2, 4, 8, 4};
  if (dtype < 0 || dtype > 4 || max_count > PCT_TARGETS_MAX_INSTANCES) return PCT_ERR_UNSUPPORTED;
  if (((uintptr_t)labels & (elem[dtype] - 1)) || (((uintptr_t)counts | (uintptr_t)starts) & 3u) ||
      (((uintptr_t)workspace | (uintptr_t)masks | (uintptr_t)planes | (uintptr_t)fg) & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_instance_targets_planes(labels, dtype, batch, height, width, workspace, counts, total_planes, max_count, starts,
                                             masks, planes, fg, static_cast<hipStream_t>(stream));
}

int pct_label_overlap(const void *pred, int pred_dtype, const void *gt, int gt_dtype, const uint8_t *fg, int batch, int height,
                      int width, void *workspace, int32_t *values, int32_t *areas, int32_t *num, int32_t *range, int32_t *table,
                      int32_t *status, void *stream)
{
  if (height <= 0 || width <= 0) return PCT_ERR_BAD_ARG;
  const int rc = pct::label_metrics_geometry_status(pred_dtype, gt_dtype, batch, height, width);
  if (rc != PCT_OK) return rc;
  if (!pred || !gt || !workspace || !values || !areas || !num || !range || !table || !status) return PCT_ERR_BAD_ARG;
  static const uintptr_t elem[5] = {1, 2, 4, 8, 4};
  if (((uintptr_t)pred & (elem[pred_dtype] - 1)) || ((uintptr_t)gt & (elem[gt_dtype] - 1)) ||
      (((uintptr_t)values | (uintptr_t)areas | (uintptr_t)num | (uintptr_t)range | (uintptr_t)status) & 3u) ||
      (((uintptr_t)workspace | (uintptr_t)table) & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_label_overlap(pred, pred_dtype, gt, gt_dtype, fg, batch, height, width, workspace, values, areas, num, range,
                                   table, status, static_cast<hipStream_t>(stream));
}

int pct_label_metrics(const int32_t *values, const int32_t *areas, const int32_t *num, const int32_t *range, const int32_t *table,
                      int batch, double *metrics, int32_t *counts, void *stream)
{
  if (batch <= 0 || batch > 65535) return PCT_ERR_UNSUPPORTED;
  if (!values || !areas || !num || !range || !table || !metrics || !counts) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)values | (uintptr_t)areas | (uintptr_t)num | (uintptr_t)range | (uintptr_t)table | (uintptr_t)counts) & 3u) ||
      ((uintptr_t)metrics & 7u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_label_metrics(values, areas, num, range, table, batch, metrics, counts, static_cast<hipStream_t>(stream));
}

int pct_label_merge_small(const void *labels, int dtype, const uint8_t *fg, int batch, int height, int width,
                          const int32_t *passes, int num_passes, void *workspace, void *out, int32_t *values, int32_t *final,
                          int32_t *areas_before, int32_t *areas_after, int32_t *num, int32_t *merges, int32_t *status,
                          void *stream)
{
  const int rc = pct::label_merge_status(dtype, batch, height, width, passes, num_passes);
  if (rc != PCT_OK) return rc;
  if (!labels || !workspace || !out || !values || !final || !areas_before || !areas_after || !num || !merges || !status)
    return PCT_ERR_BAD_ARG;
  static const uintptr_t elem[5] = {1, 2, 4, 8, 4};
  if ((((uintptr_t)labels | (uintptr_t)out) & (elem[dtype] - 1)) ||
      (((uintptr_t)values | (uintptr_t)final | (uintptr_t)areas_before | (uintptr_t)areas_after | (uintptr_t)num |
        (uintptr_t)merges | (uintptr_t)status) & 3u) ||
      ((uintptr_t)workspace & 15u))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_label_merge_small(labels, dtype, fg, batch, height, width, passes, num_passes, workspace, out, values, final,
                                       areas_before, areas_after, num, merges, status, static_cast<hipStream_t>(stream));
}

int pct_add_layernorm_f32(const float *x, const float *y, const float *gamma, const float *beta, float eps,
                          long long rows, int cols, float *out, void *stream)
{
  if (rows < 0 || cols <= 0) return PCT_ERR_BAD_ARG;
  if (rows == 0) return PCT_OK;
  if (!x || !gamma || !beta || !out) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15u) return PCT_ERR_ALIGNMENT;
  return pct::launch_add_layernorm(x, y, gamma, beta, eps, rows, cols, out, static_cast<hipStream_t>(stream));
}

int pct_linear_k128_f32(const float *x, long long ldx, const float *x_add, long long ld_add, long long add_period,
                        const float *w, const float *bias, long long rows, int n, int act, float *y, long long ldy,
                        void *stream)
{
  if (rows < 0 || n <= 0 || ldx < 128 || ldy < n || (act != 0 && act != 1)) return PCT_ERR_BAD_ARG;
  if (const int rc = check_x_add(x_add, ld_add, add_period); rc != PCT_OK) return rc;
  if (rows == 0) return PCT_OK;
  if (!x || !w || !y) return PCT_ERR_BAD_ARG;
  if (n % 32) return PCT_ERR_UNSUPPORTED;
  if ((((uintptr_t)x | (uintptr_t)w) & 15u) || (ldx & 3)) return PCT_ERR_ALIGNMENT;
  return pct::launch_linear_k128(x, ldx, x_add, ld_add, add_period, w, bias, rows, n, act, y, ldy, nullptr, 0, nullptr, nullptr, 0.f,
                                 static_cast<hipStream_t>(stream));
}

void pct_msda_set_kernel_choice(int choice) { pct::set_msda_kernel_choice(choice); }

int pct_msda_last_kernel(void) { return pct::msda_last_kernel(); }

void pct_msda_set_bwd_kernel_choice(int choice) { pct::set_msda_bwd_kernel_choice(choice); }

int pct_msda_last_bwd_kernel(void) { return pct::msda_bwd_last_kernel(); }

int pct_linear_k128_multi_f32(const float *x, long long ldx, const float *x_add, long long ld_add, long long add_period,
                              int nseg, const float *const *w, const float *const *bias, const int *n, const int *use_add,
                              float *const *y, const long long *ldy, long long rows, void *stream)
{
  if (rows < 0 || nseg < 1 || nseg > 4 || ldx < 128 || !w || !bias || !n || !use_add || !y || !ldy) return PCT_ERR_BAD_ARG;
  if (const int rc = check_x_add(x_add, ld_add, add_period); rc != PCT_OK) return rc;
  if (rows == 0) return PCT_OK;
  if (!x) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)x & 15u) || (ldx & 3)) return PCT_ERR_ALIGNMENT;
  for (int s = 0; s < nseg; ++s) {
    if (!w[s] || !y[s] || n[s] <= 0 || ldy[s] < n[s]) return PCT_ERR_BAD_ARG;
    if (n[s] % 32) return PCT_ERR_UNSUPPORTED;
  }
  // (this launcher's PCT_NOT_COVERED: w[s], bias[s] or y[s] not 16-byte aligned or ldy[s] % 4 != 0, and no other kernel takes the call)
  return abi_status(pct::launch_linear_k128_split_multi(x, ldx, x_add, ld_add, add_period, nseg, w, bias, n, use_add, y, ldy, rows,
                                                        static_cast<hipStream_t>(stream)),
                    PCT_ERR_ALIGNMENT);
}

int pct_linear_k128_add_layernorm_f32(const float *x, long long ldx, const float *w, const float *bias,
                                      const float *residual, long long ldr, const float *gamma, const float *beta,
                                      float eps, long long rows, float *out, long long ldo, void *stream)
{
  if (rows < 0 || ldx < 128 || ldr < 128 || ldo < 128) return PCT_ERR_BAD_ARG;
  if (rows == 0) return PCT_OK;
  if (!x || !w || !residual || !gamma || !beta || !out) return PCT_ERR_BAD_ARG;
  if ((((uintptr_t)x | (uintptr_t)w) & 15u) || (ldx & 3)) return PCT_ERR_ALIGNMENT;
  return pct::launch_linear_k128(x, ldx, nullptr, 0, 0, w, bias, rows, 128, 2, out, ldo, residual, ldr, gamma, beta, eps,
                                 static_cast<hipStream_t>(stream));
}

int pct_linear_add_layernorm_f32(const float *x, long long ldx, int k, const float *w, void *w_split_ws, const float *bias,
                                 const float *residual, long long ldr, const float *gamma, const float *beta, float eps,
                                 long long rows, float *out, long long ldo, void *stream)
{
  if (rows < 0 || k <= 0 || ldx < k || ldr < 128 || ldo < 128) return PCT_ERR_BAD_ARG;
  if (rows == 0) return PCT_OK;
  if (!x || !w || !w_split_ws || !residual || !gamma || !beta || !out) return PCT_ERR_BAD_ARG;
  if (k % 32) return PCT_ERR_UNSUPPORTED;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)w_split_ws | (uintptr_t)residual | (uintptr_t)out | (uintptr_t)bias |
        (uintptr_t)gamma | (uintptr_t)beta) & 15u) || (ldx & 3) || (ldr & 3) || (ldo & 3))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_linear_ln_split(x, ldx, w, static_cast<unsigned short *>(w_split_ws), k, bias, residual, ldr, gamma, beta, eps,
                                     rows, out, ldo, static_cast<hipStream_t>(stream));
}

int pct_groupnorm_flatten_f32(const float *x, const float *gamma, const float *beta, int batch, int channels, int hw,
                              int groups, float eps, float *stats, float *out, long long out_batch_stride,
                              long long out_offset, void *stream)
{
  if (batch < 0 || channels <= 0 || hw < 0 || groups <= 0 || out_batch_stride < 0 || out_offset < 0) return PCT_ERR_BAD_ARG;
  if (batch == 0 || hw == 0) return PCT_OK;
  if (!x || !gamma || !beta || !stats || !out) return PCT_ERR_BAD_ARG;
  if (channels != 128 || channels % groups || (channels / groups) % 4) return PCT_ERR_UNSUPPORTED;
  if ((uintptr_t)x & 15u) return PCT_ERR_ALIGNMENT;
  return pct::launch_groupnorm_flatten(x, gamma, beta, batch, channels, hw, groups, eps, stats, out, out_batch_stride,
                                       out_offset, static_cast<hipStream_t>(stream));
}

int pct_conv1x1_nchw_f32(const float *x, const float *w, const float *bias, void *w_split_ws, int batch, int in_channels,
                         int out_channels, int hw, float *out, void *stream)
{
  if (batch < 0 || in_channels <= 0 || out_channels <= 0 || hw < 0) return PCT_ERR_BAD_ARG;
  if (batch == 0 || hw == 0) return PCT_OK;
  if (!x || !w || !w_split_ws || !out) return PCT_ERR_BAD_ARG;
  if (out_channels != 128) return PCT_ERR_UNSUPPORTED;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)w_split_ws | (uintptr_t)out | (uintptr_t)bias) & 15u) return PCT_ERR_ALIGNMENT;
  return pct::launch_conv1x1_nchw_split(x, w, bias, static_cast<unsigned short *>(w_split_ws), batch, in_channels, hw, out,
                                        static_cast<hipStream_t>(stream));
}

int pct_conv1x1_groupnorm_tokens_f32(const float *x, const float *w, const float *bias, void *w_split_ws, const float *gamma,
                                     const float *beta, int groups, float eps, int batch, int in_channels, int out_channels, int hw,
                                     float *partial_ws, float *stats, float *out, long long out_batch_stride, long long out_offset,
                                     void *stream)
{
  if (batch < 0 || in_channels <= 0 || out_channels <= 0 || hw < 0 || out_batch_stride < 0 || out_offset < 0) return PCT_ERR_BAD_ARG;
  if (batch == 0 || hw == 0) return PCT_OK;
  if (!x || !w || !w_split_ws || !gamma || !beta || !partial_ws || !stats || !out) return PCT_ERR_BAD_ARG;
  if (out_channels != 128 || groups != 32) return PCT_ERR_UNSUPPORTED;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)w_split_ws | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta |
        (uintptr_t)partial_ws | (uintptr_t)stats) & 15u) || (out_batch_stride & 3) || (out_offset & 3))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_conv1x1_groupnorm_tokens(x, w, bias, static_cast<unsigned short *>(w_split_ws), gamma, beta, eps, batch,
                                              in_channels, hw, partial_ws, stats, out + out_offset, out_batch_stride,
                                              static_cast<hipStream_t>(stream));
}

int pct_ffn_layernorm_f32(const float *x, long long ldx, const float *w1, const float *b1, const float *w2, const float *b2,
                          const float *gamma, const float *beta, float eps, int hidden, long long rows, void *w_image_ws, float *out,
                          long long ldo, void *stream)
{
  if (rows < 0 || hidden <= 0 || ldx < 128 || ldo < 128) return PCT_ERR_BAD_ARG;
  if (rows == 0) return PCT_OK;
  if (!x || !w1 || !b1 || !w2 || !gamma || !beta || !w_image_ws || !out) return PCT_ERR_BAD_ARG;
  if (hidden % 32) return PCT_ERR_UNSUPPORTED;
  if ((((uintptr_t)x | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)gamma | (uintptr_t)beta |
        (uintptr_t)w_image_ws | (uintptr_t)out) & 15u) || (ldx & 3) || (ldo & 3))
    return PCT_ERR_ALIGNMENT;
  return pct::launch_ffn_fused_split(x, ldx, w1, b1, w2, b2, gamma, beta, eps, hidden, rows, w_image_ws, out, ldo,
                                     static_cast<hipStream_t>(stream));
}

int pct_lsap_f32(const float *cost, int batch, int num_query, int ld_target, const int *num_target, int *row_for_target,
                 int *status, void *stream)
{
  if (batch < 0 || num_query <= 0 || ld_target <= 0) return PCT_ERR_BAD_ARG;
  if (batch == 0) return PCT_OK;
  if (!cost || !num_target || !row_for_target || !status) return PCT_ERR_BAD_ARG;
  return pct::launch_lsap(cost, batch, num_query, ld_target, num_target, row_for_target, status, static_cast<hipStream_t>(stream));
}

int pct_masked_attention_bf16(const void *q, const void *k, const void *vT, const unsigned char *mask, int batch,
                              int heads, int num_query, int num_key, int head_dim, int v_head_dim, float scale,
                              int out_dtype, void *out, void *stream)
{
  if (batch < 0 || heads <= 0 || num_query < 0 || num_key <= 0) return PCT_ERR_BAD_ARG;
  if (batch == 0 || num_query == 0) return PCT_OK;
  if (!q || !k || !vT || !out) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)q | (uintptr_t)k) & 15u) return PCT_ERR_ALIGNMENT;
  if (((uintptr_t)vT | (uintptr_t)out) & 7u) return PCT_ERR_ALIGNMENT;
  return pct::launch_masked_attention(q, k, vT, mask, batch, heads, num_query, num_key, head_dim, v_head_dim, scale,
                                      out_dtype, out, static_cast<hipStream_t>(stream));
}

int pct_prepare_device(void)
{
  const int a = pct::prepare_win_queue_device();
  const int b = pct::prepare_msda_backward_col_device();
  const int c = pct::prepare_ffn_device();
  return a ? a : (b ? b : c);
}

const char *pct_build_info(void) { return "target=gfx950"; }

int pct_cross_attention_bf16(const void *q_content, const void *q_pos, const void *k_content, const void *k_pos, const void *v,
                             const unsigned char *mask, const unsigned char *row_open, int batch, int heads, int num_query,
                             int num_key, float scale, void *out, void *stream)
{
  if (batch < 0 || heads <= 0 || num_query < 0 || num_key <= 0) return PCT_ERR_BAD_ARG;
  if (batch == 0 || num_query == 0) return PCT_OK;
  if (!q_content || !q_pos || !k_content || !k_pos || !v || !out) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)q_content | (uintptr_t)q_pos | (uintptr_t)k_content | (uintptr_t)k_pos | (uintptr_t)v) & 15u)
    return PCT_ERR_ALIGNMENT;
  if ((uintptr_t)out & 7u) return PCT_ERR_ALIGNMENT;
  return abi_status(pct::launch_cross_attention(q_content, q_pos, k_content, k_pos, v, mask, mask ? row_open : nullptr, batch, heads,
                                                num_query, num_key, scale, out, static_cast<hipStream_t>(stream)));
}

int pct_cross_attention_ragged_bf16(const void *q_content, const void *q_pos, const void *k_content, const void *k_pos,
                                    const void *v, const unsigned char *mask, int mask_pitch, const unsigned char *row_open,
                                    int batch, int heads, int num_query, int num_key, float scale, void *out, void *stream)
{
  if (batch < 0 || heads <= 0 || num_query < 0 || num_key < 1) return PCT_ERR_BAD_ARG;
  if (mask && (mask_pitch < num_key || mask_pitch % 16 != 0)) return PCT_ERR_BAD_ARG;
  if (batch == 0 || num_query == 0) return PCT_OK;
  if (!q_content || !q_pos || !k_content || !k_pos || !v || !out) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)q_content | (uintptr_t)q_pos | (uintptr_t)k_content | (uintptr_t)k_pos | (uintptr_t)v | (uintptr_t)mask) & 15u)
    return PCT_ERR_ALIGNMENT;
  if ((uintptr_t)out & 7u) return PCT_ERR_ALIGNMENT;
  return abi_status(pct::launch_cross_attention_ragged(q_content, q_pos, k_content, k_pos, v, mask, mask ? mask_pitch : 0,
                                                       mask ? row_open : nullptr, batch, heads, num_query, num_key, scale, out,
                                                       static_cast<hipStream_t>(stream)));
}

long long pct_cross_attention_split_keys_workspace(int batch, int heads, int num_query, int splits)
{
  if (batch < 0 || heads <= 0 || num_query < 0 || splits < 1 || splits > 16) return PCT_ERR_BAD_ARG;
  if (heads % 4 != 0) return PCT_ERR_UNSUPPORTED;
  return pct::cross_attention_split_keys_workspace(batch, heads, num_query, splits);
}

// the ragged entry's checks in its order; the launcher goes on with that launcher's coverage, then `splits` and the workspace
int pct_cross_attention_split_keys_bf16(const void *q_content, const void *q_pos, const void *k_content, const void *k_pos,
                                        const void *v, const unsigned char *mask, int mask_pitch, const unsigned char *row_open,
                                        int batch, int heads, int num_query, int num_key, float scale, int splits, void *workspace,
                                        long long workspace_bytes, void *out, void *stream)
{
  if (batch < 0 || heads <= 0 || num_query < 0 || num_key < 1) return PCT_ERR_BAD_ARG;
  if (mask && (mask_pitch < num_key || mask_pitch % 16 != 0)) return PCT_ERR_BAD_ARG;
  if (batch == 0 || num_query == 0) return PCT_OK;
  if (!q_content || !q_pos || !k_content || !k_pos || !v || !out) return PCT_ERR_BAD_ARG;
  if (((uintptr_t)q_content | (uintptr_t)q_pos | (uintptr_t)k_content | (uintptr_t)k_pos | (uintptr_t)v | (uintptr_t)mask) & 15u)
    return PCT_ERR_ALIGNMENT;
  if ((uintptr_t)out & 7u) return PCT_ERR_ALIGNMENT;
  return abi_status(pct::launch_cross_attention_split_keys(q_content, q_pos, k_content, k_pos, v, mask, mask ? mask_pitch : 0,
                                                           mask ? row_open : nullptr, batch, heads, num_query, num_key, scale,
                                                           splits, workspace, workspace_bytes, out,
                                                           static_cast<hipStream_t>(stream)));
}

// The argument checks of the four differentiable fp32 attention entries, of the two split-key ones and of the two evaluation ones, in the order the ABI fixes: a negative size or no head,
// the empty call (nothing is read, every pointer may be null), a null pointer, a pointer off 16 bytes (self-attention:
// num_key = num_query).  -> true: launch; false: return *status.
static bool attn_train_args(int batch, int heads, int num_query, int num_key, std::initializer_list<const void *> ptrs,
                            int *status)
{
  *status = PCT_OK;
  if (batch < 0 || heads <= 0 || num_query < 0 || num_key < 0) *status = PCT_ERR_BAD_ARG;
  if (*status != PCT_OK || batch == 0 || num_query == 0 || num_key == 0) return false;
  uintptr_t bits = 0;
  for (const void *p : ptrs) {
    if (!p) *status = PCT_ERR_BAD_ARG;
    bits |= (uintptr_t)p;
  }
  if (*status == PCT_OK && (bits & 15u)) *status = PCT_ERR_ALIGNMENT;
  return *status == PCT_OK;
}

int pct_cross_attention_forward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                    const float *v, const unsigned char *mask, const unsigned char *row_open, int batch, int heads,
                                    int num_query, int num_key, float scale, float *out, float *lse, void *stream)
{
  int status;
  if (!attn_train_args(batch, heads, num_query, num_key, {q_content, q_pos, k_content, k_pos, v, out, lse}, &status)) return status;
  return abi_status(pct::launch_cross_attention_fwd_f32(q_content, q_pos, k_content, k_pos, v, mask, mask ? row_open : nullptr, batch,
                                                        heads, num_query, num_key, scale, out, lse,
                                                        static_cast<hipStream_t>(stream)));
}

int pct_cross_attention_backward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                     const float *v, const unsigned char *mask, const unsigned char *row_open, const float *out,
                                     const float *lse, const float *grad_out, int batch, int heads, int num_query, int num_key,
                                     float scale, float *workspace, float *grad_q_content, float *grad_q_pos, float *grad_k_content,
                                     float *grad_k_pos, float *grad_v, void *stream)
{
  int status;
  if (!attn_train_args(batch, heads, num_query, num_key,
                       {q_content, q_pos, k_content, k_pos, v, lse, grad_out, workspace, grad_q_content, grad_q_pos,
                        grad_k_content, grad_k_pos, grad_v},
                       &status))
    return status;
  return abi_status(pct::launch_cross_attention_bwd_f32(q_content, q_pos, k_content, k_pos, v, mask, mask ? row_open : nullptr, out, lse,
                                                        grad_out, batch, heads, num_query, num_key, scale, workspace, grad_q_content,
                                                        grad_q_pos, grad_k_content, grad_k_pos, grad_v,
                                                        static_cast<hipStream_t>(stream)));
}

long long pct_cross_attention_split_train_workspace(int batch, int heads, int num_query, int splits)
{
  if (batch < 0 || heads <= 0 || num_query < 0 || splits < 1 || splits > 16) return PCT_ERR_BAD_ARG;
  if (heads != 4 && heads != 8) return PCT_ERR_UNSUPPORTED;
  return pct::cross_attention_split_train_workspace(batch, heads, num_query, splits);
}

// the unsplit entries' checks with the workspace among the pointers; the launchers go on with the geometry, `splits` and
// workspace_bytes, all before their first launch
int pct_cross_attention_split_forward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                          const float *v, const unsigned char *mask, const unsigned char *row_open, int batch,
                                          int heads, int num_query, int num_key, float scale, int splits, void *workspace,
                                          long long workspace_bytes, float *out, float *lse, void *stream)
{
  int status;
  if (!attn_train_args(batch, heads, num_query, num_key, {q_content, q_pos, k_content, k_pos, v, out, lse, workspace}, &status))
    return status;
  return abi_status(pct::launch_cross_attention_split_fwd_f32(q_content, q_pos, k_content, k_pos, v, mask, mask ? row_open : nullptr,
                                                              batch, heads, num_query, num_key, scale, splits, workspace,
                                                              workspace_bytes, out, lse, static_cast<hipStream_t>(stream)));
}

int pct_cross_attention_split_backward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                           const float *v, const unsigned char *mask, const unsigned char *row_open,
                                           const float *out, const float *lse, const float *grad_out, int batch, int heads,
                                           int num_query, int num_key, float scale, int splits, void *workspace,
                                           long long workspace_bytes, float *grad_q_content, float *grad_q_pos,
                                           float *grad_k_content, float *grad_k_pos, float *grad_v, void *stream)
{
  int status;
  if (!attn_train_args(batch, heads, num_query, num_key,
                       {q_content, q_pos, k_content, k_pos, v, lse, grad_out, workspace, grad_q_content, grad_q_pos,
                        grad_k_content, grad_k_pos, grad_v},
                       &status))
    return status;
  (void)out;
  return abi_status(pct::launch_cross_attention_split_bwd_f32(q_content, q_pos, k_content, k_pos, v, mask, mask ? row_open : nullptr,
                                                              lse, grad_out, batch, heads, num_query, num_key, scale, splits,
                                                              workspace, workspace_bytes, grad_q_content, grad_q_pos,
                                                              grad_k_content, grad_k_pos, grad_v,
                                                              static_cast<hipStream_t>(stream)));
}

int pct_self_attention_forward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                   const float *v, int batch, int heads, int num_query, float scale, float *out, float *lse,
                                   void *stream)
{
  int status;
  if (!attn_train_args(batch, heads, num_query, num_query, {q_content, q_pos, k_content, k_pos, v, out, lse}, &status))
    return status;
  return abi_status(pct::launch_self_attention_fwd_f32(q_content, q_pos, k_content, k_pos, v, batch, heads, num_query, scale, out,
                                                       lse, static_cast<hipStream_t>(stream)));
}

int pct_self_attention_backward_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                    const float *v, const float *out, const float *lse, const float *grad_out, int batch,
                                    int heads, int num_query, float scale, float *workspace, float *grad_q, float *grad_k,
                                    float *grad_v, void *stream)
{
  int status;
  if (!attn_train_args(batch, heads, num_query, num_query,
                       {q_content, q_pos, k_content, k_pos, v, lse, grad_out, workspace, grad_q, grad_k, grad_v}, &status))
    return status;
  (void)out;
  return abi_status(pct::launch_self_attention_bwd_f32(q_content, q_pos, k_content, k_pos, v, lse, grad_out, batch, heads,
                                                       num_query, scale, workspace, grad_q, grad_k, grad_v,
                                                       static_cast<hipStream_t>(stream)));
}

int pct_cross_attention_eval_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                 const float *v, const unsigned char *mask, const unsigned char *row_open, int batch, int heads,
                                 int num_query, int num_key, float scale, float *out, void *stream)
{
  int status;
  if (!attn_train_args(batch, heads, num_query, num_key, {q_content, q_pos, k_content, k_pos, v, out}, &status)) return status;
  return abi_status(pct::launch_cross_attention_eval_f32(q_content, q_pos, k_content, k_pos, v, mask, mask ? row_open : nullptr, batch,
                                                         heads, num_query, num_key, scale, out, static_cast<hipStream_t>(stream)));
}

int pct_self_attention_eval_f32(const float *q_content, const float *q_pos, const float *k_content, const float *k_pos,
                                const float *v, int batch, int heads, int num_query, float scale, float *out, void *stream)
{
  int status;
  if (!attn_train_args(batch, heads, num_query, num_query, {q_content, q_pos, k_content, k_pos, v, out}, &status)) return status;
  return abi_status(pct::launch_self_attention_eval_f32(q_content, q_pos, k_content, k_pos, v, batch, heads, num_query, scale, out,
                                                        static_cast<hipStream_t>(stream)));
}

}  // extern "C"
