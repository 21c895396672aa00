// Differentiable fp32 cross-attention of the decoder (include/pctrans_hip_attn_train.h): the two-half, masked instance of
// attn_train_common.hpp, which holds the algorithm, the register layouts, the arithmetic and the summation orders.  Operands in
// the split form the projection GEMMs write, all fp32:
//   q_c, q_s [Q, N, heads * 16]   k_c, k_p, v [S, N, heads * 16]   mask [N, Q, S] bytes   row_open [N, Q] bytes
// Per head the query is [content 16 | position 16] and the key likewise; the concatenations are never formed:
//   score(q, k) = scale * (q_c[q] . k_c[k] + q_s[q] . k_p[k]).
// Forward one launch.  Backward three, everything read from global memory: D to the caller's workspace (xat_delta_kernel), the
// key pass (xat_bwd_k_kernel: grad_k_c, grad_k_p, grad_v), the query pass (xat_bwd_q_kernel: grad_q_c, grad_q_s).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_train_common.hpp"
#include "launchers.hpp"

namespace pct {
namespace {

__global__ __launch_bounds__(AT_THREADS) void xat_fwd_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                              const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                              const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                              const unsigned char *__restrict__ row_open, const Geo geo,
                                                              const float scale, float *__restrict__ out, float *__restrict__ lse)
{
  attn_fwd<Cross, true, false>(q_c, q_s, k_c, k_p, v, mask, row_open, geo, scale, out, lse);
}

__global__ __launch_bounds__(AT_THREADS) void xat_delta_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                const unsigned char *__restrict__ row_open,
                                                                const float *__restrict__ lse, const float *__restrict__ grad_out,
                                                                const Geo geo, const float scale, float *__restrict__ delta)
{
  const GlobalKeys<Cross> keys = {k_c, k_p, v};
  attn_bwd_q<Cross, true, false>(q_c, q_s, keys, mask, row_open, lse, grad_out, geo, scale, delta, nullptr, nullptr);
}

__global__ __launch_bounds__(AT_THREADS) void xat_bwd_q_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                const unsigned char *__restrict__ row_open,
                                                                const float *__restrict__ lse, const float *__restrict__ delta,
                                                                const float *__restrict__ grad_out, const Geo geo, const float scale,
                                                                float *__restrict__ grad_q_c, float *__restrict__ grad_q_s)
{
  const GlobalKeys<Cross> keys = {k_c, k_p, v};
  attn_bwd_q<Cross, false, true>(q_c, q_s, keys, mask, row_open, lse, grad_out, geo, scale, delta, grad_q_c, grad_q_s);
}

__global__ __launch_bounds__(AT_THREADS) void xat_bwd_k_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                const unsigned char *__restrict__ row_open,
                                                                const float *__restrict__ lse, const float *__restrict__ delta,
                                                                const float *__restrict__ grad_out, const Geo geo, const float scale,
                                                                float *__restrict__ grad_k_c, float *__restrict__ grad_k_p,
                                                                float *__restrict__ grad_v)
{
  attn_bwd_k<Cross>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, delta, grad_out, geo, scale, grad_k_c, grad_k_p, grad_v);
}

}  // namespace

int launch_cross_attention_fwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                   const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S,
                                   float scale, float *out, float *lse, hipStream_t stream)
{
  if (!attn_train_covered(N, heads, Q, S)) return PCT_NOT_COVERED;
  const Geo geo = attn_geo(N, heads, Q, S);
  xat_fwd_kernel<<<query_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, geo, scale, out, lse);
  return (int)hipGetLastError();
}

int launch_cross_attention_bwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                   const unsigned char *mask, const unsigned char *row_open, const float *out, const float *lse,
                                   const float *grad_out, int N, int heads, int Q, int S, float scale, float *workspace,
                                   float *grad_q_c, float *grad_q_s, float *grad_k_c, float *grad_k_p, float *grad_v,
                                   hipStream_t stream)
{
  if (!attn_train_covered(N, heads, Q, S)) return PCT_NOT_COVERED;
  const Geo geo = attn_geo(N, heads, Q, S);
  xat_delta_kernel<<<query_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, grad_out, geo, scale,
                                                               workspace);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  xat_bwd_k_kernel<<<key_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, workspace, grad_out, geo,
                                                             scale, grad_k_c, grad_k_p, grad_v);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  xat_bwd_q_kernel<<<query_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, workspace, grad_out, geo,
                                                               scale, grad_q_c, grad_q_s);
  return (int)hipGetLastError();
}

}  // namespace pct
