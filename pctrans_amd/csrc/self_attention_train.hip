// Differentiable fp32 self-attention of the decoder (include/pctrans_hip_self_attn_train.h): the one-half, unmasked instance of
// attn_train_common.hpp, which holds the algorithm, the register layouts, the arithmetic and the summation orders.  Operands as
// SelfAttentionLayer's five projections write them, all fp32:
//   q_c, q_p, k_c, k_p, v [Q, N, heads * 16]
// Per head  q = fl32(q_c + q_p),  k = fl32(k_c + k_p),  score(q, k) = scale * q . k,  softmax over all Q keys.  There is no mask
// and so no row without an attendable key: keys are the queries, and Q >= 1.
// Forward one launch; nothing is staged, a workgroup reads every key and value row once.  Backward two:
//   sat_bwd_q_kernel: the workgroup first stages k = fl32(k_c + k_p) and v of its whole (image, head) in LDS as [Q][16] floats
//   each (the add is made once per element, not once per use), because it sweeps the keys twice (D, written to the caller's
//   workspace, then grad_q) and reads k both by rows (the score's operand) and by columns (dq's operand).  The LDS image bounds
//   the query count: SAT_MAX_Q = 512 rows are 64 KiB of the 160 KiB of a gfx950 CU, two workgroups per CU.  Rows are 64 bytes:
//   a row read (lane (c, g): row c, floats 4 g ..) covers 1 KiB contiguously, a column read (row g + 4 r, float c) 64
//   consecutive words per group of rows: neither has a bank conflict.
//   sat_bwd_k_kernel: the key pass; each wave reads every query row once, so nothing is staged here.
// grad_q is the gradient of q_c and of q_p, grad_k of k_c and of k_p (the add's backward is the identity): each is written once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_train_common.hpp"
#include "launchers.hpp"

namespace pct {
namespace {

constexpr int SAT_MAX_Q = 512;             // rows of the LDS image of k and v in sat_bwd_q_kernel

__global__ __launch_bounds__(AT_THREADS) void sat_fwd_kernel(const float *__restrict__ q_c, const float *__restrict__ q_p,
                                                              const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                              const float *__restrict__ v, const Geo geo, const float scale,
                                                              float *__restrict__ out, float *__restrict__ lse)
{
  attn_fwd<Self, true, false>(q_c, q_p, k_c, k_p, v, nullptr, nullptr, geo, scale, out, lse);
}

__global__ __launch_bounds__(AT_THREADS) void sat_bwd_q_kernel(const float *__restrict__ q_c, const float *__restrict__ q_p,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const float *__restrict__ lse,
                                                                const float *__restrict__ grad_out, const Geo geo,
                                                                const float scale, float *__restrict__ delta,
                                                                float *__restrict__ grad_q)
{
  __shared__ __attribute__((aligned(16))) float s_k[SAT_MAX_Q * 16], s_v[SAT_MAX_Q * 16];
  const Head hd(geo);
  for (int i = threadIdx.x; i < 4 * geo.Q; i += AT_THREADS) {         // float4 i: row i / 4, floats 4 (i % 4) ..; Q <= SAT_MAX_Q
    const size_t at = (size_t)(i >> 2) * hd.rs + hd.hoff + 4 * (i & 3);
    *reinterpret_cast<float4 *>(s_k + 4 * i) = add4(ld4(k_c + at), ld4(k_p + at));
    *reinterpret_cast<float4 *>(s_v + 4 * i) = ld4(v + at);
  }
  const LdsKeys<Self> keys = {s_k, s_v};
  attn_bwd_q<Self, true, true>(q_c, q_p, keys, nullptr, nullptr, lse, grad_out, geo, scale, delta, grad_q, nullptr);
}

__global__ __launch_bounds__(AT_THREADS) void sat_bwd_k_kernel(const float *__restrict__ q_c, const float *__restrict__ q_p,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const float *__restrict__ lse,
                                                                const float *__restrict__ delta, const float *__restrict__ grad_out,
                                                                const Geo geo, const float scale, float *__restrict__ grad_k,
                                                                float *__restrict__ grad_v)
{
  attn_bwd_k<Self>(q_c, q_p, k_c, k_p, v, nullptr, nullptr, lse, delta, grad_out, geo, scale, grad_k, nullptr, grad_v);
}

}  // namespace

int launch_self_attention_fwd_f32(const float *q_c, const float *q_p, const float *k_c, const float *k_p, const float *v, int N,
                                  int heads, int Q, float scale, float *out, float *lse, hipStream_t stream)
{
  if (!attn_train_covered(N, heads, Q, Q, SAT_MAX_Q)) return PCT_NOT_COVERED;
  const Geo geo = attn_geo(N, heads, Q, Q);
  sat_fwd_kernel<<<query_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_p, k_c, k_p, v, geo, scale, out, lse);
  return (int)hipGetLastError();
}

int launch_self_attention_bwd_f32(const float *q_c, const float *q_p, const float *k_c, const float *k_p, const float *v,
                                  const float *lse, const float *grad_out, int N, int heads, int Q, float scale, float *workspace,
                                  float *grad_q, float *grad_k, float *grad_v, hipStream_t stream)
{
  if (!attn_train_covered(N, heads, Q, Q, SAT_MAX_Q)) return PCT_NOT_COVERED;
  const Geo geo = attn_geo(N, heads, Q, Q);
  sat_bwd_q_kernel<<<query_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_p, k_c, k_p, v, lse, grad_out, geo, scale, workspace, grad_q);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  sat_bwd_k_kernel<<<key_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_p, k_c, k_p, v, lse, workspace, grad_out, geo, scale, grad_k,
                                                             grad_v);
  return (int)hipGetLastError();
}

}  // namespace pct
