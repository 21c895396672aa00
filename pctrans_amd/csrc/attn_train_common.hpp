// The small device helpers the differentiable fp32 attention kernels share (cross_attention_train.hip, self_attention_train.hip):
// the two MFMA forms on a lane's float4 of an operand row, the widening, the row permutation that lines an fp32 tile up with an
// fp64 one, and the column maximum in fp64.  The register layouts they rely on are described in cross_attention_train.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "attn_common.hpp"   // f32x4

namespace pct {
namespace {

__device__ __forceinline__ f32x4 mfma4(const float a, const float b, const f32x4 c)
{
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// += over the 4 dims a lane's float4 holds of each operand (16 dims in all over the four lane groups)
__device__ __forceinline__ f32x4 mfma16(const float4 a, const float4 b, f32x4 c)
{
  c = mfma4(a.x, b.x, c);
  c = mfma4(a.y, b.y, c);
  c = mfma4(a.z, b.z, c);
  return mfma4(a.w, b.w, c);
}
// The scores run on v_mfma_f64_16x16x4_f64 on the operands widened to fp64 (exact products, fp64 accumulation), and the
// exponent x - m (forward) or x - lse (backward) is formed in fp64 and rounded to fp32 once.  An fp32 chain leaves scale * s
// with an error that grows with |x| (32 roundings of partial sums, then |x| 2^-24 for the stored value), and the exponential
// turns it into a relative error of every probability: 1e-5 at the scores of +-300 of the underflowing family.  Operands as
// the fp32 form; the result differs: register r of lane group g is row g + 4 r (not 4 g + r).
typedef double f64x4 __attribute__((ext_vector_type(4)));
struct d4 {
  double x, y, z, w;
};
__device__ __forceinline__ d4 widen(const float4 a) { return {(double)a.x, (double)a.y, (double)a.z, (double)a.w}; }
__device__ __forceinline__ f64x4 mfma16d(const d4 a, const d4 b, f64x4 c)
{
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a.z, b.z, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a.w, b.w, c, 0, 0, 0);
}
// max over the four lane groups of a column (lane ^ 16, lane ^ 32)
__device__ __forceinline__ double xgroup_max_f64(double v)
{
  v = fmax(v, __shfl_xor(v, 16, 64));
  return fmax(v, __shfl_xor(v, 32, 64));
}
// An fp32 tile (rows 4 g + r) that must line up with an fp64 tile (rows g + 4 r) takes its A rows in this order: lane c
// supplies row pi(c), so that register r of group g holds row pi(4 g + r) = g + 4 r.
__device__ __forceinline__ int pi16(const int c) { return (c >> 2) + 4 * (c & 3); }
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

}  // namespace
}  // namespace pct
