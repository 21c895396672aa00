// The split-bf16 arithmetic of the encoder's GEMMs (linear_k128_split.hip, linear_ln_split.hip, ffn_fused_split.hip,
// conv1x1_split.hip), stated once.  An fp32 number with 2^-110 <= |a| < 0x7F7F8000 (3.396e38), or zero, is EXACTLY the sum of
// three bf16 numbers
//     a = a1 + a2 + a3,   a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)
// (below 2^-110 the bits of a under 2^-133, the last bf16 subnormal, can be lost; from 0x7F7F8000 on a1 rounds to inf and
// a2 = -inf, a3 = NaN: like an inf or a NaN, such an operand makes its whole output row NaN; tests/split_gemm_hard_inputs.py)
// and a product a.w is evaluated from its six leading partial products on the bf16 matrix cores with fp32 accumulation
// (linear_k128_split.hip has the error analysis).  Staging layouts and epilogues stay with the kernels; what they share is
// the split, the order of the six products, the vector types and the wave's 2 x 2 accumulator tile -- the GEMMs agree bit for
// bit only while these agree.  (split_tr_gemm.hpp: the weight-step stream and the step loop of the transposed-B kernels.)
#pragma once
#include <hip/hip_runtime.h>

namespace pct {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// (x, y) -> three packed bf16 pairs (low half = x's piece), x = x1 + x2 + x3 exactly
__device__ __forceinline__ void split_bf16x3(const float x, const float y, unsigned &p1, unsigned &p2, unsigned &p3)
{
  p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x, y}, bf16x2));               // v_cvt_pk_bf16_f32 (RNE)
  const float rx = x - __uint_as_float(p1 << 16), ry = y - __uint_as_float(p1 & 0xffff0000u);   // exact
  p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{rx, ry}, bf16x2));
  const float sx = rx - __uint_as_float(p2 << 16), sy = ry - __uint_as_float(p2 & 0xffff0000u); // exact
  p3 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{sx, sy}, bf16x2));
}

// the three pieces of a pair, one per plane: d, d + plane, d + 2 plane (in bf16 elements)
__device__ __forceinline__ void store_planes(unsigned short *d, const long long plane, const unsigned p1, const unsigned p2,
                                             const unsigned p3)
{
  *reinterpret_cast<unsigned *>(d) = p1;
  *reinterpret_cast<unsigned *>(d + plane) = p2;
  *reinterpret_cast<unsigned *>(d + 2 * plane) = p3;
}

// eight consecutive floats -> three bf16x8 pieces
__device__ __forceinline__ void split_bf16x3_8(const f32x4 a, const f32x4 b, bf16x8 (&out)[3])
{
  unsigned p[3][4];
  split_bf16x3(a[0], a[1], p[0][0], p[1][0], p[2][0]);
  split_bf16x3(a[2], a[3], p[0][1], p[1][1], p[2][1]);
  split_bf16x3(b[0], b[1], p[0][2], p[1][2], p[2][2]);
  split_bf16x3(b[2], b[3], p[0][3], p[1][3], p[2][3]);
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q] = __builtin_bit_cast(bf16x8, i32x4{(int)p[q][0], (int)p[q][1], (int)p[q][2], (int)p[q][3]});
}

// ... and staged: piece q as one 16-byte store at d + q * plane (bytes)
__device__ __forceinline__ void split_bf16x3_8_store(const f32x4 a, const f32x4 b, unsigned char *d, const int plane)
{
  bf16x8 p[3];
  split_bf16x3_8(a, b, p);
#pragma unroll
  for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x8 *>(d + q * plane) = p[q];
}

// One k-step of the product of w = w1 + w2 + w3 (A operand) and a = a1 + a2 + a3 (B operand): the six leading terms
//     w1a1 | w1a2 + w2a1 | w2a2 + w1a3 + w3a1          (relative size 1 | 2^-9 | 2^-18)
// Two accumulators: the w1a1 chain alone in `hi`, the five small terms in `lo`, so that the small terms are rounded at their
// own magnitude and not at the product's; the caller adds hi + lo once at the end.  The order below is the order everywhere:
// fp32 accumulation does not commute, and the kernels' results (tests/test_ffn_bitwise_gpu.py) are pinned to it.
// The accumulator type selects the instruction: f32x16 v_mfma_f32_32x32x16_bf16, f32x4 v_mfma_f32_16x16x32_bf16.
__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 w, bf16x8 a, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, a, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 w, bf16x8 a, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, c, 0, 0, 0); }
template <typename Acc>
__device__ __forceinline__ void split_mfma6(const bf16x8 w1, const bf16x8 w2, const bf16x8 w3, const bf16x8 a1, const bf16x8 a2,
                                            const bf16x8 a3, Acc &hi, Acc &lo)
{
  lo = mfma_bf16(w1, a3, lo);
  hi = mfma_bf16(w1, a1, hi);
  lo = mfma_bf16(w3, a1, lo);
  lo = mfma_bf16(w2, a2, lo);
  lo = mfma_bf16(w1, a2, lo);
  lo = mfma_bf16(w2, a1, lo);
}

// A wave's tile of the 128-wide GEMMs: 2 x 2 blocks of 32 x 32 outputs, each a hi / lo accumulator pair (128 VGPRs).
struct SplitTile2x2 {
  f32x16 hi[2][2], lo[2][2];                                        // [row block][column block]
  __device__ __forceinline__ void zero()
  {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int j = 0; j < 16; ++j) hi[rb][cb][j] = lo[rb][cb][j] = 0.f;
  }
  // one k-step, rows outer.  The A operand's three pieces w[.] belong to the row blocks; with W_BY_COLUMN to the column
  // blocks (linear_ln_split.hip computes the transposed tile) and b[.] to the row blocks
  template <bool W_BY_COLUMN = false>
  __device__ __forceinline__ void mac(const bf16x8 (&w)[2][3], const bf16x8 (&b)[2][3])
  {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const bf16x8(&wp)[3] = w[W_BY_COLUMN ? cb : rb], (&bp)[3] = b[W_BY_COLUMN ? rb : cb];
        split_mfma6(wp[0], wp[1], wp[2], bp[0], bp[1], bp[2], hi[rb][cb], lo[rb][cb]);
      }
  }
  // element j of block (rb, cb): the one addition of hi and lo
  __device__ __forceinline__ float sum(const int rb, const int cb, const int j) const { return hi[rb][cb][j] + lo[rb][cb][j]; }
};

// ReLU of the bias / ReLU epilogues: a NaN passes through as in torch.relu (fmaxf(v, 0.f) returns 0 for it, so a NaN of the
// product would vanish from the output); every other v, -0 included, gives the bits fmaxf gave
__device__ __forceinline__ float relu_keep_nan(const float v) { return (v > 0.f || v != v) ? v : 0.f; }

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, true));
}

// sum over the 32 lanes of each wave half (lanes 0-31 / 32-63); result valid in every lane of the half
__device__ __forceinline__ float half_wave_sum(float v)
{
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);   // row_half_mirror
  v += dpp_mov<0x140>(v);   // row_mirror  -> every lane of a 16-lane row holds the row's sum
  const int vi = __float_as_int(v);                                 // (readlane takes and returns the bit pattern)
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(vi, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(vi, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(vi, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(vi, 48));
  return (threadIdx.x & 32) ? r2 + r3 : r0 + r1;
}

}  // namespace pct
