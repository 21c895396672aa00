// Fused residual add + LayerNorm over the last dimension for MI355X (gfx950, wave64):  out = LN(x + y) * gamma + beta.
//
// Replaces the `src = src + dropout(src2); src = norm(src)` pairs of the encoder / decoder layers in eval mode
// (pixel_decoder/msdeformattn.py:116-131, transformer_decoder/mask2former_transformer_decoder.py:97-99,179-181,216-224
// of the reference): torch runs an elementwise add (read 2, write 1) followed by a LayerNorm kernel that reaches only
// ~1 TB/s at hidden = 128 (one block per 512-byte row).  Here a row is held by COLS/4 lanes as one float4 each (two rows
// per wave at COLS = 128), x and y are read once, mean / variance are two-pass in registers (sum, then centred sum of
// squares, reduced with wave shuffles) and the result is written once: 3 HBM passes instead of 5, all 16-byte coalesced.
#include "msda_common.hpp"
#include "launchers.hpp"

namespace pct {

constexpr int ALN_BLOCK = 256;

template <int COLS, bool HAS_Y>
__global__ __launch_bounds__(ALN_BLOCK) void add_layernorm_kernel(const float *__restrict__ x,
                                                                  const float *__restrict__ y,
                                                                  const float *__restrict__ gamma,
                                                                  const float *__restrict__ beta, const float eps,
                                                                  const long long rows, float *__restrict__ out)
{
  constexpr int LPR = COLS / 4;                       // lanes per row (power of two, <= 64)
  constexpr int RPB = ALN_BLOCK / LPR;                // rows per block
  using f4 = vec_t<float, 4>;
  const int lane = threadIdx.x % LPR;
  const f4 g = *reinterpret_cast<const f4 *>(gamma + lane * 4);
  const f4 bt = *reinterpret_cast<const f4 *>(beta + lane * 4);
  for (long long row = (long long)blockIdx.x * RPB + threadIdx.x / LPR; row < rows; row += (long long)gridDim.x * RPB) {
    const size_t off = (size_t)row * COLS + lane * 4;
    f4 v = *reinterpret_cast<const f4 *>(x + off);
    if constexpr (HAS_Y) {
      const f4 w = *reinterpret_cast<const f4 *>(y + off);
      v = v + w;
    }
    float s = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / COLS);
    const f4 d = v - mean;
    float q = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q * (1.0f / COLS) + eps);
    *reinterpret_cast<f4 *>(out + off) = d * rstd * g + bt;
  }
}

int launch_add_layernorm(const float *x, const float *y, const float *gamma, const float *beta, float eps,
                         long long rows, int cols, float *out, hipStream_t stream)
{
  if (rows == 0) return 0;
  if (cols != 128 && cols != 256 && cols != 64) return PCT_ERR_UNSUPPORTED;
  const int rpb = ALN_BLOCK / (cols / 4);
  long long nblk = (rows + rpb - 1) / rpb;
  if (nblk > 256 * 16) nblk = 256 * 16;               // grid-stride beyond 16 blocks per CU
  const dim3 grid((unsigned)nblk), block(ALN_BLOCK);
#define PCT_ALN(C_)                                                                                               \
  if (y) hipLaunchKernelGGL((add_layernorm_kernel<C_, true>), grid, block, 0, stream, x, y, gamma, beta, eps, rows, out); \
  else hipLaunchKernelGGL((add_layernorm_kernel<C_, false>), grid, block, 0, stream, x, y, gamma, beta, eps, rows, out)
  if (cols == 128) { PCT_ALN(128); }
  else if (cols == 256) { PCT_ALN(256); }
  else { PCT_ALN(64); }
#undef PCT_ALN
  return (int)hipGetLastError();
}

}  // namespace pct
