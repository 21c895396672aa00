// Reductions over the 64 lanes of a wave for the loss, target and metric kernels.
//
// The order is contractual: a 6-step xor butterfly with the masks 32, 16, 8, 4, 2, 1.  Each step combines the same two numbers in
// both lanes of a pair, so every lane ends with the same bits, and a floating-point sum is one fixed tree whatever the kernel:
// the tests assert bit-identical repeats and float64 bounds derived from this chain of 6 additions.  A kernel with another
// order, or a butterfly over part of the wave, keeps its own loop.
#pragma once
#include <hip/hip_runtime.h>

namespace pct {

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}

}  // namespace pct
