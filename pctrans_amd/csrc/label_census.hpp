// The census of label values that instance_targets.hip and label_metrics.hip share: which of the 65 536 covered values a label
// map holds, as a presence bitmap per image, and their ascending ranks.  The two files walk the pixels differently (strips with
// run detection in instance_targets.hip, a lane per pixel in label_metrics.hip) and keep their own bitmap kernels; what a label
// value is, how a workgroup's bitmap joins the image's and how the set bits become ranks is stated in this header once, so that
// the two cannot disagree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pct {

constexpr int LC_MAX = 512;                     // values kept per map and image (the matcher's column limit)
constexpr int LC_VALUES = 65536;                // label values covered
constexpr int LC_WORDS = LC_VALUES / 32;        // words of a presence bitmap
constexpr unsigned LC_NONE = 0xFFFFu;           // value -> rank table entry of a value without a rank

// label value of a pixel, or -1 for a value the tables do not cover (negative, above 65 535, not integral, NaN)
template <typename T>
__device__ __forceinline__ int label_value(const T v)
{
  const long long w = (long long)v;                                             // (65 535 is no int16 value: compare widened)
  return (w >= 0 && w < LC_VALUES) ? (int)w : -1;
}
template <>
__device__ __forceinline__ int label_value<float>(const float v)
{
  return (v >= 0.f && v <= (float)(LC_VALUES - 1) && v == truncf(v)) ? (int)v : -1;
}

// the `words` bitmap words a workgroup of BLOCK threads holds in LDS, OR-ed into the image's global bitmap: only a non-zero
// word costs an atomic
template <int BLOCK>
__device__ __forceinline__ void census_merge(const unsigned *bits, const int words, unsigned *gb)
{
  for (int i = threadIdx.x; i < words; i += BLOCK) {
    const unsigned w = bits[i];
    if (w) atomicOr(&gb[i], w);
  }
}

// Rank step, by one workgroup of BLOCK threads on one image's bitmap `gb`: the bit of `clear` dropped (a value outside the covered
// ones clears nothing), then the set bits in ascending order -> out[base + rank] = value and index[value] = rank for the first
// LC_MAX of them, the rest of out[base .. base + LC_MAX) zeroed.  `base` keeps a caller's 32-bit index into a batch-wide array
// (a caller with a ready pointer passes 0): one int add per store, no 64-bit address arithmetic.  A thread takes LC_WORDS / BLOCK consecutive words; thread 0 makes the prefix of
// the popcounts in `first` (LDS, BLOCK + 1 ints).  -> the number of set bits, which may exceed LC_MAX.
// RANGE: also the lowest and highest set value into *lo and *hi (LDS; LC_VALUES and -1 for an empty bitmap), valid once the
// routine returns.  Without it lo and hi are not touched and cost nothing.
template <int BLOCK, bool RANGE>
__device__ __forceinline__ int census_rank(const unsigned *gb, const int clear, int *out, const int base, unsigned short *index,
                                           int *first, int *lo, int *hi)
{
  constexpr int PER = LC_WORDS / BLOCK;
  const int t = threadIdx.x;
  unsigned w[PER];
  int mine = 0, mylo = LC_VALUES, myhi = -1;
  if (RANGE && t == 0) {
    *lo = LC_VALUES;
    *hi = -1;
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int word = t * PER + k;
    w[k] = gb[word];
    if ((unsigned)clear < (unsigned)LC_VALUES && (clear >> 5) == word) w[k] &= ~(1u << (clear & 31));
    mine += __popc(w[k]);
    if (RANGE && w[k]) {
      mylo = min(mylo, word * 32 + __ffs(w[k]) - 1);
      myhi = max(myhi, word * 32 + 31 - __clz(w[k]));
    }
  }
  first[t + 1] = mine;
  __syncthreads();
  if (RANGE && mine) {
    atomicMin(lo, mylo);
    atomicMax(hi, myhi);
  }
  if (t == 0) {
    first[0] = 0;
    for (int i = 1; i <= BLOCK; ++i) first[i] += first[i - 1];
  }
  __syncthreads();
  int at = first[t];
  const int total = first[BLOCK];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    unsigned m = w[k];
    while (m) {
      const int b = __ffs(m) - 1;
      m &= m - 1;
      if (at < LC_MAX) {
        const int v = (t * PER + k) * 32 + b;
        out[base + at] = v;
        index[v] = (unsigned short)at;
      }
      ++at;
    }
  }
  for (int i = total + t; i < LC_MAX; i += BLOCK) out[base + i] = 0;
  return total;
}

}  // namespace pct
