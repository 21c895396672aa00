// The decoder's attention in fp32 evaluation (include/pctrans_hip_attn_eval.h): the forward of attn_train_common.hpp without a
// backward to serve, for the key counts of whole images (4 096 - 5 655 on the finest level, where the training kernels stop at
// 1 024) and any query count.  Operands, layouts, the arithmetic and its summation orders are those of the training forwards
// (cross_attention_train.hip, self_attention_train.hip), and `out` has the same bits; two things differ (attn_fwd's LSE and AHEAD):
//   no lse      the row statistics have no reader
//   one step ahead   a wave issues the loads of its next 16-key step -- the key row of both operands, four value words, four
//                    mask bytes -- before the arithmetic of the current one, and holds that one set in registers.  A wave
//                    walks ceil(S / 64) steps one after the other (89 at 5 655 keys); in the training form each begins by
//                    waiting for its own loads.  The last step of a wave loads nothing: no address lies behind row S - 1.
// The self form has no query limit: the 512 of self_attention_train.hip is the LDS image of its backward.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_train_common.hpp"
#include "launchers.hpp"

namespace pct {
namespace {

__global__ __launch_bounds__(AT_THREADS) void xat_eval_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                               const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                               const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                               const unsigned char *__restrict__ row_open, const Geo geo,
                                                               const float scale, float *__restrict__ out)
{
  attn_fwd<Cross, false, true>(q_c, q_s, k_c, k_p, v, mask, row_open, geo, scale, out, nullptr);
}

__global__ __launch_bounds__(AT_THREADS) void sat_eval_kernel(const float *__restrict__ q_c, const float *__restrict__ q_p,
                                                               const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                               const float *__restrict__ v, const Geo geo, const float scale,
                                                               float *__restrict__ out)
{
  attn_fwd<Self, false, true>(q_c, q_p, k_c, k_p, v, nullptr, nullptr, geo, scale, out, nullptr);
}

}  // namespace

int launch_cross_attention_eval_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                    const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S,
                                    float scale, float *out, hipStream_t stream)
{
  if (!attn_train_covered(N, heads, Q, S)) return PCT_NOT_COVERED;
  const Geo geo = attn_geo(N, heads, Q, S);
  xat_eval_kernel<<<query_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, geo, scale, out);
  return (int)hipGetLastError();
}

int launch_self_attention_eval_f32(const float *q_c, const float *q_p, const float *k_c, const float *k_p, const float *v, int N,
                                   int heads, int Q, float scale, float *out, hipStream_t stream)
{
  if (!attn_train_covered(N, heads, Q, Q)) return PCT_NOT_COVERED;
  const Geo geo = attn_geo(N, heads, Q, Q);
  sat_eval_kernel<<<query_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_p, k_c, k_p, v, geo, scale, out);
  return (int)hipGetLastError();
}

}  // namespace pct
