// Point-sampled mask losses (include/pctrans_hip_train.h: pct_point_sample_f32, pct_point_mask_loss_forward_f32,
// pct_point_mask_loss_backward_f32): the gather, the fused BCE + dice sums and the scatter of their gradient that
// loss/matcher.py and loss/maskformer_criterion.py otherwise run as grid_sample forward / backward plus elementwise and reduce
// launches.
//
// Sampling is F.grid_sample(input, 2c - 1, "bilinear", "zeros", align_corners=False): x = c_x * W - 0.5 (one fma),
// y = c_y * H - 0.5, taps at floor and floor + 1, weights (1 - tx)(1 - ty) .. tx ty, a tap outside the plane adds nothing.
// Every tap address is formed only after 0 <= xi < W and 0 <= yi < H held, whatever the coordinate (NaN, negative, huge).
//
// Backward.  No floating-point atomic: workgroup (pair k, band of PL_BAND_ROWS rows) zeroes one signed 64-bit accumulator per
// band pixel in LDS, walks the pair's P points and adds llrint(w * grad_x * s) for the taps that fall in its band
// (ds_add_u64, workgroup scope: integer adds commute, so the sum is the same for every arrival order), then stores
// float(acc) / s for the whole band with plain stores.  s is a power of two chosen per pair on the device:
//     bound = |alpha| + (|beta| + |gamma|) / 4  >=  |grad_x|  for labels in [0, 1]   (|sigma - t| <= 1, sigma' <= 1/4)
//     bound = m * 2^e, m in [0.5, 1)   ->   s = 2^(30 - e)  (exponent clamped to [-126, 126])
// so |w * grad_x * s| < 2^30 (1 + 2^-20) and the P <= 2^31 - 1 contributions one pixel can receive stay below 2^62: no
// overflow.  Multiplying by s is exact, the rounding to an integer moves a contribution by at most half a quantum,
// 1 / (2 s) <= bound * 2^-30; a pixel that receives n contributions is off by at most n * bound * 2^-30 from the exact sum of
// the fp32 products, plus the one rounding of the final int64 -> fp32 conversion.  (fp32 atomics would add n roundings of
// 2^-24 relative to the running sum, in an order that changes from run to run.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.hpp"

namespace pct {

namespace {

constexpr int PL_BAND_ROWS = 32;      // rows of a backward band (pctrans_amd/point_loss.py: BAND_ROWS)
constexpr int PL_MAX_WIDTH = 256;     // 32 rows x 256 pixels x 8 B = 64 KiB of LDS: two workgroups per CU
constexpr int PL_GATHER_BLOCK = 256;
constexpr int PL_FWD_BLOCK = 1024;
constexpr int PL_BWD_BLOCK = 512;

struct Taps {
  int x0, y0;
  float w00, w01, w10, w11;          // (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)
};

__device__ __forceinline__ Taps make_taps(const float cx, const float cy, const int H, const int W)
{
  const float x = fmaf(cx, (float)W, -0.5f), y = fmaf(cy, (float)H, -0.5f);
  // clamped before the conversion: a coordinate outside [0, 1] (or NaN: fmaxf returns the other operand) lands on taps that
  // are all outside the plane
  const float fx = fminf(fmaxf(floorf(x), -2.f), (float)W), fy = fminf(fmaxf(floorf(y), -2.f), (float)H);
  const float tx = x - fx, ty = y - fy;
  Taps t;
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  t.w00 = (1.f - tx) * (1.f - ty);
  t.w01 = tx * (1.f - ty);
  t.w10 = (1.f - tx) * ty;
  t.w11 = tx * ty;
  return t;
}

__device__ __forceinline__ float sample_plane(const float *__restrict__ plane, const Taps &t, const int H, const int W)
{
  const bool xa = (unsigned)t.x0 < (unsigned)W, xb = (unsigned)(t.x0 + 1) < (unsigned)W;
  const bool ya = (unsigned)t.y0 < (unsigned)H, yb = (unsigned)(t.y0 + 1) < (unsigned)H;
  const float *r0 = plane + (size_t)(ya ? t.y0 : 0) * W, *r1 = plane + (size_t)(yb ? t.y0 + 1 : 0) * W;
  const int c0 = xa ? t.x0 : 0, c1 = xb ? t.x0 + 1 : 0;
  const float v00 = (ya && xa) ? r0[c0] : 0.f, v01 = (ya && xb) ? r0[c1] : 0.f;
  const float v10 = (yb && xa) ? r1[c0] : 0.f, v11 = (yb && xb) ? r1[c1] : 0.f;
  float acc = 0.f;
  if (ya && xa) acc = t.w00 * v00;
  if (ya && xb) acc = fmaf(t.w01, v01, acc);
  if (yb && xa) acc = fmaf(t.w10, v10, acc);
  if (yb && xb) acc = fmaf(t.w11, v11, acc);
  return acc;
}

// sigma(x), sigma'(x) and bce_with_logits(x, t) from one exp: e = exp(-|x|) never overflows
__device__ __forceinline__ void sigmoid_terms(const float x, float &sg, float &dsg, float &softplus_neg_abs)
{
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  sg = x >= 0.f ? r : e * r;
  dsg = e * r * r;
  softplus_neg_abs = log1pf(e);
}

__global__ __launch_bounds__(PL_GATHER_BLOCK) void point_sample_kernel(const float *__restrict__ planes,
                                                                       const int *__restrict__ plane_index,
                                                                       const float2 *__restrict__ coords, const int num_planes,
                                                                       const int H, const int W, const int P, const int chunks,
                                                                       const int per_row, float *__restrict__ out)
{
  const int k = blockIdx.x / chunks;
  const int p = (blockIdx.x - k * chunks) * PL_GATHER_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int plane = plane_index ? plane_index[k] : k;
  float v = __builtin_nanf("");                                            // an index outside the planes: loud, and no access
  if ((unsigned)plane < (unsigned)num_planes) {
    const float2 c = coords[(size_t)(k / per_row) * P + p];
    v = sample_plane(planes + (size_t)plane * H * W, make_taps(c.x, c.y, H, W), H, W);
  }
  out[(size_t)k * P + p] = v;
}

// one workgroup per pair: every thread a fixed subset of the points in ascending order, then a fixed tree over the lanes and
// the waves in ascending order
__global__ __launch_bounds__(PL_FWD_BLOCK) void point_loss_forward_kernel(
    const float *__restrict__ pred, const int *__restrict__ src_index, const int num_pred, const int H, const int W,
    const float *__restrict__ tgt, const int *__restrict__ tgt_index, const int num_tgt, const int Ht, const int Wt,
    const float2 *__restrict__ coords, const int P, float *__restrict__ xs, float *__restrict__ ts, float *__restrict__ sums)
{
  __shared__ float part[PL_FWD_BLOCK / 64][4];
  const int k = blockIdx.x;
  const int sp = src_index ? src_index[k] : k, tp = tgt_index ? tgt_index[k] : k;
  const bool ok = (unsigned)sp < (unsigned)num_pred && (unsigned)tp < (unsigned)num_tgt;
  const float *pp = pred + (size_t)(ok ? sp : 0) * H * W, *tq = tgt + (size_t)(ok ? tp : 0) * Ht * Wt;
  const float nan = __builtin_nanf("");
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int p = threadIdx.x; p < P; p += PL_FWD_BLOCK) {
    const size_t o = (size_t)k * P + p;
    float x = nan, t = nan;
    if (ok) {
      const float2 c = coords[o];
      x = sample_plane(pp, make_taps(c.x, c.y, H, W), H, W);
      t = sample_plane(tq, make_taps(c.x, c.y, Ht, Wt), Ht, Wt);
    }
    xs[o] = x;
    ts[o] = t;
    float sg, dsg, sp_;
    sigmoid_terms(x, sg, dsg, sp_);
    s[0] += fmaxf(x, 0.f) - x * t + sp_;
    s[1] += sg * t;
    s[2] += sg;
    s[3] += t;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s[i] += __shfl_xor(s[i], d, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][i] = s[i];
  __syncthreads();
  if (threadIdx.x < 4) {
    float a = 0.f;
    for (int w = 0; w < PL_FWD_BLOCK / 64; ++w) a += part[w][threadIdx.x];
    sums[(size_t)k * 4 + threadIdx.x] = a;
  }
}

__global__ __launch_bounds__(PL_BWD_BLOCK) void point_loss_backward_kernel(
    const float *__restrict__ xs, const float *__restrict__ ts, const float2 *__restrict__ coords,
    const float *__restrict__ alpha, const float *__restrict__ beta, const float *__restrict__ gamma, const int P, const int H,
    const int W, const int bands, float *__restrict__ grad)
{
  extern __shared__ unsigned long long acc[];                              // [rows of this band][W]
  const int k = blockIdx.x / bands, band = blockIdx.x - k * bands;
  const int y_lo = band * PL_BAND_ROWS, rows = min(PL_BAND_ROWS, H - y_lo);
  const int cells = rows * W;
  const float a = alpha[k], b = beta[k], g = gamma[k];
  const float bound = fabsf(a) + 0.25f * (fabsf(b) + fabsf(g));
  float *out = grad + ((size_t)k * H + y_lo) * W;
  if (!(bound < __builtin_inff())) {                                      // NaN or infinite coefficients: as torch, not a number
    for (int i = threadIdx.x; i < cells; i += PL_BWD_BLOCK) out[i] = __builtin_nanf("");
    return;
  }
  int e = 0;
  (void)frexpf(bound, &e);                                                 // bound = m * 2^e, m in [0.5, 1); bound == 0: e = 0
  const int se = max(-126, min(126, 30 - e));
  const float scale = ldexpf(1.f, se), inv_scale = ldexpf(1.f, -se);
  for (int i = threadIdx.x; i < cells; i += PL_BWD_BLOCK) acc[i] = 0ull;
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += PL_BWD_BLOCK) {
    const size_t o = (size_t)k * P + p;
    const float2 c = coords[o];
    const Taps tp = make_taps(c.x, c.y, H, W);
    const int r0 = tp.y0 - y_lo, r1 = r0 + 1;                              // rows of the two tap rows inside the band
    const bool ya = (unsigned)r0 < (unsigned)rows, yb = (unsigned)r1 < (unsigned)rows;
    if (!(ya || yb)) continue;
    const bool xa = (unsigned)tp.x0 < (unsigned)W, xb = (unsigned)(tp.x0 + 1) < (unsigned)W;
    if (!(xa || xb)) continue;
    const float x = xs[o], t = ts[o];
    float sg, dsg, unused;
    sigmoid_terms(x, sg, dsg, unused);
    const float gx = fmaf(a, sg - t, dsg * (b - g * t)) * scale;          // (the power of two commutes with the roundings)
    auto add = [&](const bool inside, const int r, const int col, const float w) {
      if (!inside) return;
      const long long q = __float2ll_rn(w * gx);
      if (q != 0)
        __hip_atomic_fetch_add(&acc[r * W + col], (unsigned long long)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    add(ya && xa, r0, tp.x0, tp.w00);
    add(ya && xb, r0, tp.x0 + 1, tp.w01);
    add(yb && xa, r1, tp.x0, tp.w10);
    add(yb && xb, r1, tp.x0 + 1, tp.w11);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += PL_BWD_BLOCK) out[i] = (float)(long long)acc[i] * inv_scale;
}

// what the kernels cover: 32-bit offsets inside a plane, a one-dimensional grid, and for the losses a band that fits LDS
int point_sample_geometry_status(int H, int W, long long K, int P, int block)
{
  if ((long long)H * W >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  const long long chunks = ((long long)P + block - 1) / block;
  if (K * chunks >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

int point_loss_geometry_status(int H, int W, int Ht, int Wt, int K)
{
  if ((long long)H * W >= 0x7fffffffLL || (long long)Ht * Wt >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  if (W > PL_MAX_WIDTH) return PCT_ERR_UNSUPPORTED;
  if ((long long)K * ((H + PL_BAND_ROWS - 1) / PL_BAND_ROWS) >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

}  // namespace

int launch_point_sample(const float *planes, const int *plane_index, const float *coords, int num_planes, int H, int W, int K,
                        int P, int per_row, float *out, hipStream_t stream)
{
  if (const int rc = point_sample_geometry_status(H, W, K, P, PL_GATHER_BLOCK); rc != PCT_OK) return rc;
  const int chunks = (P + PL_GATHER_BLOCK - 1) / PL_GATHER_BLOCK;
  point_sample_kernel<<<dim3((unsigned)(K * chunks)), dim3(PL_GATHER_BLOCK), 0, stream>>>(
      planes, plane_index, reinterpret_cast<const float2 *>(coords), num_planes, H, W, P, chunks, per_row, out);
  return (int)hipGetLastError();
}

int launch_point_loss_forward(const float *pred, const int *src_index, int num_pred, int H, int W, const float *tgt,
                              const int *tgt_index, int num_tgt, int Ht, int Wt, const float *coords, int K, int P, float *x,
                              float *t, float *sums, hipStream_t stream)
{
  if (const int rc = point_loss_geometry_status(H, W, Ht, Wt, K); rc != PCT_OK) return rc;
  point_loss_forward_kernel<<<dim3((unsigned)K), dim3(PL_FWD_BLOCK), 0, stream>>>(
      pred, src_index, num_pred, H, W, tgt, tgt_index, num_tgt, Ht, Wt, reinterpret_cast<const float2 *>(coords), P, x, t, sums);
  return (int)hipGetLastError();
}

int launch_point_loss_backward(const float *x, const float *t, const float *coords, const float *alpha, const float *beta,
                               const float *gamma, int K, int P, int H, int W, float *grad_planes, hipStream_t stream)
{
  if (const int rc = point_loss_geometry_status(H, W, 1, 1, K); rc != PCT_OK) return rc;
  const int bands = (H + PL_BAND_ROWS - 1) / PL_BAND_ROWS;
  const size_t lds = (size_t)(H < PL_BAND_ROWS ? H : PL_BAND_ROWS) * W * sizeof(unsigned long long);
  point_loss_backward_kernel<<<dim3((unsigned)(K * bands)), dim3(PL_BWD_BLOCK), lds, stream>>>(
      x, t, reinterpret_cast<const float2 *>(coords), alpha, beta, gamma, P, H, W, bands, grad_planes);
  return (int)hipGetLastError();
}

}  // namespace pct
