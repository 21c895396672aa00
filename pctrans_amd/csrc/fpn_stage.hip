// One FPN level of the pixel decoder in eval mode on MI355X (gfx950), fp32 in and out, every product in exact split-bf16
// (pixel_decoder/msdeformattn.py: lateral 1x1 conv + norm of res2, bilinear resize DOWN to the finest encoder map, add, 3x3 conv
// + norm + ReLU -- the stage that produces `mask_features` with three encoder levels).  With s[c], t[c] the per-channel affine a
// norm with fixed statistics reduces to (s = gamma / sqrt(var + eps), t = beta - mean * s; identity: s = 1, t = 0):
//     lat[n][co][p] = s1[co] * (b1[co] + sum_ci W1[co][ci] * down(x)[n][ci][p]) + t1[co]
//     y             = enc + lat
//     out[n][co][p] = relu( s3[co] * (b3[co] + sum_{ci,ky,kx} W3[co][ci][ky][kx] * y[n][ci][p + (ky - 1, kx - 1)]) + t3[co] )
// x is [N, Cin, 2H, 2W]: at the exact ratio 2 the bilinear resize (align_corners = False) is the 2 x 2 mean, and since the lateral
// convolution and its affine are linear the mean is taken FIRST -- the 1x1 GEMM runs on a quarter of the pixels and the first
// kernel is bound by reading x once.
//
// Arithmetic: split_bf16.hpp -- every fp32 operand is exactly three bf16 numbers (for 2^-110 <= |a| < 0x7F7F8000 and zero; an
// operand above makes the outputs it reaches NaN, and the ReLU passes a NaN on), a product is its six leading terms on
// v_mfma_f32_32x32x16_bf16, the w1 a1 chain and the five small terms in accumulators of their own (hi / lo), summed once.
//
// fpn_lateral_kernel: workgroup (4 waves) = (image, 4 rows x 32 columns of the output map), all 128 output channels; per step of
// 16 input channels a thread loads 2 rows of 4 floats for 4 (channel, pixel pair) items as they lie in memory (8-byte loads, 16
// lanes = 256 contiguous bytes; a pair that hangs over the right edge loads its left half, pixels outside nothing), means them, splits
// the pair and writes three 4-byte words into the [16 k][128 pixels] planes that conv1x1_split.hip's transposing read
// (ds_read_b64_tr_b16) turns into B fragments.  Waves = 2 x 2 blocks of 64 channels x 64 pixels, the step loop is the same one
// (split_tr_gemm.hpp).  Epilogue: affine, + enc
// read where it lies (channels-last token rows: one 16-byte load per 4 channels; NCHW: 4 loads along the pixels), y written as
// [N][8 slabs][H W][16 channels] fp32: what the second kernel stages as contiguous 64-byte pixels.
//
// fpn_output_kernel: implicit GEMM [128 co] x [1152 = 8 slabs of 16 ci x 9 taps] x [pixels].  LDS on paper, for two workgroups per
// CU (80 KB each): three bf16 planes of the seg-head kernel's 340-pixel x 32-channel block are 81.6 KB before any weights.  With
// 16-channel slabs (one MFMA k-step per tap) and a tile of 4 rows x 32 columns: input block 6 x 34 = 204 pixels x 48 B (32 + 16
// pad: the 16-lane groups of a ds_read_b128 fall on distinct 16-byte slots, 3 being odd) x 3 planes = 29 376 B; weight image of a
// (slab, tap) step [3 planes][128 co][16 ci] at the same 48-byte stride = 18 432 B, double-buffered 36 864 B; affine 1 KB:
// 67 264 B.  Waves = 2 channel halves x 2 row pairs, 2 x 2 MFMA tiles with hi / lo = 128 accumulators; per step 12 ds_read_b128
// for 24 MFMAs.  The weights stream from L2 (884 736 B image, resident) through registers into the other buffer; the next slab's
// pixels are fetched during taps 0 and 1 and split + written behind a barrier after tap 8.  Pixels outside the image are staged
// as zeros (the padding), stores outside are masked: any H, W >= 1.
//
// The weight images are re-split on every call by fpn_weight_images_kernel into the caller's workspace.

#include "split_tr_gemm.hpp"    // split_bf16.hpp
#include "launchers.hpp"

namespace pct {

constexpr int FP_C = 128;                        // channels of enc, y and out
constexpr int FP_KS = 16;                        // reduction channels per step (both kernels)
constexpr int FP_BLOCK = 256;
constexpr int FP_TH = 4, FP_TW = 32;             // output tile of both kernels
constexpr int FP_WROW = 48;                      // bytes per weight row / staged pixel in LDS (16 bf16 + 16 pad)
constexpr int FP_WPLANE = FP_C * FP_WROW;        // 6 144
constexpr int FP_WBUF = 3 * FP_WPLANE;           // 18 432
constexpr int FP_WSTEP = 3 * FP_C * FP_KS;       // 6 144 bf16 per step image in memory ([plane][co][16], unpadded)
// lateral kernel: x planes as in conv1x1_split.hip
constexpr int FL_XROW = 320;                     // bytes per k-row of a plane (128 px x 2 B + 64 pad)
constexpr int FL_XPLANE = FP_KS * FL_XROW;
constexpr int FL_XBUF = 3 * FL_XPLANE;           // 15 360
// output kernel: halo block
constexpr int FO_HW = FP_TW + 2;                 // 34
constexpr int FO_HP = (FP_TH + 2) * FO_HW;       // 204 staged pixels
constexpr int FO_XPLANE = FO_HP * FP_WROW;       // 9 792
constexpr int FO_TASKS = FO_HP * 2;              // (pixel, 8-channel group)
constexpr int FO_ROUNDS = (FO_TASKS + FP_BLOCK - 1) / FP_BLOCK;      // 2

// W1 [128][K] -> img1 [K / 16][3][128][16]; W3 [128][128][3][3] -> img3 [slab * 9 + tap][3][128][16]: one thread per pair of
// consecutive input channels
__global__ __launch_bounds__(256) void fpn_weight_images_kernel(const float *__restrict__ w1, const int K,
                                                                const float *__restrict__ w3, unsigned short *__restrict__ img1,
                                                                unsigned short *__restrict__ img3)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int n1 = FP_C * K / 2;
  unsigned p1, p2, p3;
  unsigned short *dst;
  if (e < n1) {
    const int co = (2 * e) / K, k = 2 * e - co * K;
    split_bf16x3(w1[2 * e], w1[2 * e + 1], p1, p2, p3);
    dst = img1 + (size_t)(k / FP_KS) * FP_WSTEP + co * FP_KS + (k % FP_KS);
  } else {
    const int f = e - n1;                                          // (co, ci pair, tap), tap fastest
    if (f >= FP_C * (FP_C / 2) * 9) return;
    const int tap = f % 9, cp = (f / 9) % (FP_C / 2), co = f / (9 * (FP_C / 2)), ci = 2 * cp;
    const float *p = w3 + ((size_t)co * FP_C + ci) * 9 + tap;
    split_bf16x3(p[0], p[9], p1, p2, p3);
    dst = img3 + (size_t)((ci / FP_KS) * 9 + tap) * FP_WSTEP + co * FP_KS + (ci % FP_KS);
  }
  store_planes(dst, FP_C * FP_KS, p1, p2, p3);
}

// out = fmaf(s, acc, t): s = gamma / sqrt(var + eps), t = s * (bias - mean) + beta; without statistics s = 1, t = bias
__device__ __forceinline__ f32x2 fpn_affine(const int c, const float *bias, const float *mean, const float *var, const float *gamma,
                                            const float *beta, const float eps)
{
  const float b = bias ? bias[c] : 0.f;
  if (!mean) return f32x2{1.f, b};
  const float s = gamma[c] / sqrtf(var[c] + eps);
  return f32x2{s, fmaf(s, b - mean[c], beta[c])};
}

// a step's weight image in padded rows: chunk (plane i, row tid / 2, half tid % 2) for i = 0 .. 2
struct FpnWeightStream : WeightStepStream<FP_WPLANE, FP_WSTEP, FP_BLOCK> {
  __device__ __forceinline__ void init(const int tid) { loff = (tid >> 1) * FP_WROW + (tid & 1) * 16; }
};

template <bool ENC_NHWC>
__global__ __launch_bounds__(FP_BLOCK, 2) void fpn_lateral_kernel(
    const float *__restrict__ x, const unsigned short *__restrict__ img1, const float *__restrict__ bias,
    const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float eps, const float *__restrict__ enc, const long long enc_batch_stride, const int K, const int H, const int W,
    const int tiles_x, const int tiles_y, float *__restrict__ y)
{
  __shared__ __attribute__((aligned(16))) unsigned char xs[2][FL_XBUF];
  __shared__ __attribute__((aligned(16))) unsigned char wsm[2][FP_WBUF];
  __shared__ f32x2 aff[FP_C];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int tyi = tile / tiles_x, y0 = tyi * FP_TH, x0 = (tile - tyi * tiles_x) * FP_TW;
  const int HWp = H * W;
  const size_t plane_in = (size_t)4 * HWp;                         // floats per channel of x
  const int nsteps = K / FP_KS;

  if (tid < FP_C) aff[tid] = fpn_affine(tid, bias, mean, var, gamma, beta, eps);

  // staging items j = 0 .. 3: channel (tid / 64) + 4 j of the step, output row (tid / 16) % 4, pixel pair tid % 16
  const int s_pr = tid & 15, s_row = (tid >> 4) & 3, s_c = tid >> 6;
  const int soy = y0 + s_row, sox = x0 + 2 * s_pr;
  const int s_mode = soy < H ? (sox + 1 < W ? 2 : (sox < W ? 1 : 0)) : 0;      // 2: both pixels, 1: the left one, 0: none
  const float *xsrc = x + ((size_t)n * K + s_c) * plane_in + (size_t)(2 * soy) * (2 * W) + 2 * sox;
  const int s_off = s_c * FL_XROW + (s_row * FP_TW + 2 * s_pr) * 2;
  f32x4 ga[4], gb[4];
  FpnWeightStream wst;
  wst.init(tid);
  auto fetch = [&](const int step) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float *p = xsrc + (size_t)(step * FP_KS + 4 * j) * plane_in;
      // predicated 8-byte loads: the left pixel's columns, then the right pixel's (an odd row of x is only 8-byte aligned when W is odd)
      const f32x2 z = f32x2{0.f, 0.f};
      const f32x2 a0 = s_mode >= 1 ? *reinterpret_cast<const f32x2 *>(p) : z;
      const f32x2 b0 = s_mode >= 1 ? *reinterpret_cast<const f32x2 *>(p + 2 * W) : z;
      const f32x2 a1 = s_mode == 2 ? *reinterpret_cast<const f32x2 *>(p + 2) : z;
      const f32x2 b1 = s_mode == 2 ? *reinterpret_cast<const f32x2 *>(p + 2 * W + 2) : z;
      ga[j] = f32x4{a0[0], a0[1], a1[0], a1[1]};
      gb[j] = f32x4{b0[0], b0[1], b1[0], b1[1]};
    }
    wst.fetch(img1, step, tid);
  };
  auto stash = [&](const int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float m0 = 0.25f * ((ga[j][0] + ga[j][1]) + (gb[j][0] + gb[j][1]));
      const float m1 = 0.25f * ((ga[j][2] + ga[j][3]) + (gb[j][2] + gb[j][3]));
      unsigned a, b, c;
      split_bf16x3(m0, m1, a, b, c);
      unsigned char *d = xs[buf] + s_off + 4 * j * FL_XROW;
      *reinterpret_cast<unsigned *>(d) = a;
      *reinterpret_cast<unsigned *>(d + FL_XPLANE) = b;
      *reinterpret_cast<unsigned *>(d + 2 * FL_XPLANE) = c;
    }
    wst.stash(wsm[buf]);
  };

  // fragment addresses (fixed): wave = (channel half, pixel half = rows 2 px_half, 2 px_half + 1 of the tile)
  const int r = lane & 31, h = lane >> 5;
  const int co_half = wave >> 1, px_half = wave & 1;
  int a_off[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) a_off[rb] = (co_half * 64 + rb * 32 + r) * FP_WROW + h * 16;
  const SplitTile2x2 acc = split_tr_gemm<FL_XROW, FP_WPLANE>(xs[0], wsm[0], a_off, lane, px_half * 64, nsteps, fetch, stash);

  // epilogue: acc[4 q + t] = lat[co = block + 8 q + 4 h + t][row 2 px_half + cb][column r]; y [n][co / 16][pixel][co % 16]
  const int gx = x0 + r;
  const float *en = enc + (size_t)n * enc_batch_stride;
  float *yn = y + (size_t)n * FP_C * HWp;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int gy = y0 + 2 * px_half + cb;
    if (gy >= H || gx >= W) continue;
    const int pix = gy * W + gx;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co0 = co_half * 64 + rb * 32 + 8 * q + 4 * h;
        f32x4 e;
        if constexpr (ENC_NHWC) {
          e = *reinterpret_cast<const f32x4 *>(en + (size_t)pix * FP_C + co0);
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) e[t] = en[(size_t)(co0 + t) * HWp + pix];
        }
        f32x4 v;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x2 c = aff[co0 + t];
          v[t] = fmaf(c[0], acc.sum(rb, cb, 4 * q + t), c[1]) + e[t];
        }
        *reinterpret_cast<f32x4 *>(yn + ((size_t)(co0 >> 4) * HWp + pix) * FP_KS + (co0 & 15)) = v;
      }
  }
}

__global__ __launch_bounds__(FP_BLOCK, 2) void fpn_output_kernel(
    const float *__restrict__ y, const unsigned short *__restrict__ img3, const float *__restrict__ bias,
    const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float eps, const int H, const int W, const int tiles_x, const int tiles_y, float *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) unsigned char xs[3 * FO_XPLANE];
  __shared__ __attribute__((aligned(16))) unsigned char wsm[2][FP_WBUF];
  __shared__ f32x2 aff[FP_C];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int tyi = tile / tiles_x, y0 = tyi * FP_TH, x0 = (tile - tyi * tiles_x) * FP_TW;
  const int HWp = H * W;
  const float *yn = y + (size_t)n * FP_C * HWp;
  constexpr int NSLAB = FP_C / FP_KS;

  if (tid < FP_C) aff[tid] = fpn_affine(tid, bias, mean, var, gamma, beta, eps);

  // staging tasks of this thread (the same for every slab): 8 channels (cg) of a pixel of the halo block; -1 = zeros / no task
  int goff[FO_ROUNDS], loff[FO_ROUNDS];
#pragma unroll
  for (int rd = 0; rd < FO_ROUNDS; ++rd) {
    const int task = rd * FP_BLOCK + tid, p = task >> 1, cg = task & 1;
    const int py = p / FO_HW, px = p - py * FO_HW;
    const int gy = y0 - 1 + py, gx = x0 - 1 + px;
    const bool live = task < FO_TASKS;
    goff[rd] = (live && gy >= 0 && gy < H && gx >= 0 && gx < W) ? (gy * W + gx) * FP_KS + cg * 8 : -1;
    loff[rd] = live ? p * FP_WROW + cg * 16 : -1;
  }
  f32x4 gin[FO_ROUNDS][2];
  FpnWeightStream wst;
  wst.init(tid);
  auto load_x = [&](const int slab, const int rd) {
    if (goff[rd] >= 0) {
      const float *p = yn + (size_t)slab * HWp * FP_KS + goff[rd];
      gin[rd][0] = *reinterpret_cast<const f32x4 *>(p);
      gin[rd][1] = *reinterpret_cast<const f32x4 *>(p + 4);
    } else {
      gin[rd][0] = gin[rd][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto stash_x = [&]() {
#pragma unroll
    for (int rd = 0; rd < FO_ROUNDS; ++rd) {
      if (loff[rd] < 0) continue;
      split_bf16x3_8_store(gin[rd][0], gin[rd][1], xs + loff[rd], FO_XPLANE);
    }
  };

  // fragment addresses: lane = (r, h); wave = (channel half, row pair).  A: W[co][ci 8 h .. + 7], B: pixel (row 2 rp + cb, column r)
  const int r = lane & 31, h = lane >> 5;
  const int co_half = wave >> 1, rp = wave & 1;
  const int a_off = (co_half * 64 + r) * FP_WROW + h * 16;
  const int b_off = (2 * rp * FO_HW + r) * FP_WROW + h * 16;

  SplitTile2x2 acc;
  acc.zero();

  wst.fetch(img3, 0, tid);
#pragma unroll
  for (int rd = 0; rd < FO_ROUNDS; ++rd) load_x(0, rd);
  stash_x();
  wst.stash(wsm[0]);
  __syncthreads();

  for (int slab = 0; slab < NSLAB; ++slab) {
    const bool more_x = slab + 1 < NSLAB;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int step = slab * 9 + tap, buf = step & 1;
      const bool more_w = more_x || tap < 8;
      if (more_w) wst.fetch(img3, step + 1, tid);
      if (tap < FO_ROUNDS && more_x) load_x(slab + 1, tap);
      __builtin_amdgcn_sched_barrier(0);                           // the fetches ahead of the MFMAs
      const unsigned char *bp = xs + b_off + ((tap / 3) * FO_HW + tap % 3) * FP_WROW;
      const unsigned char *ap = wsm[buf] + a_off;
      bf16x8 wa[2][3], xb[2][3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) xb[cb][pl] = *reinterpret_cast<const bf16x8 *>(bp + pl * FO_XPLANE + cb * FO_HW * FP_WROW);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) wa[rb][pl] = *reinterpret_cast<const bf16x8 *>(ap + pl * FP_WPLANE + rb * 32 * FP_WROW);
      }
      acc.mac(wa, xb);
      if (tap == 8 && more_x) {
        __syncthreads();                                           // every wave has left the input block
        stash_x();
      }
      if (more_w) wst.stash(wsm[buf ^ 1]);                         // (everyone left that buffer before the previous barrier)
      __syncthreads();
    }
  }

  // epilogue: acc[4 q + t] = z[co = 64 co_half + 32 rb + 8 q + 4 h + t][row 2 rp + cb][column r]; out NCHW, lanes along the pixels
  const int gx = x0 + r;
  float *on = out + (size_t)n * FP_C * HWp;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int gy = y0 + 2 * rp + cb;
    if (gy >= H || gx >= W) continue;
    const int pix = gy * W + gx;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int co = co_half * 64 + rb * 32 + 8 * q + 4 * h + t;
          const f32x2 c = aff[co];
          on[(size_t)co * HWp + pix] = relu_keep_nan(fmaf(c[0], acc.sum(rb, cb, 4 * q + t), c[1]));
        }
  }
}

// Three launches on `stream`.  norm1 / norm3: {mean, var, gamma, beta}, a null mean = no norm.  w_ws: fpn weight images,
// (K / 16 + 72) * 12 288 bytes; y_ws: N * 128 * H * W floats.  PCT_NOT_COVERED: K % 16 != 0 or an image of 2^24 pixels or more
int launch_fpn_stage(const float *x, const float *enc, long long enc_batch_stride, int enc_nhwc, const float *w1, const float *b1,
                     const float *const *norm1, float eps1, const float *w3, const float *b3, const float *const *norm3, float eps3,
                     void *w_ws, float *y_ws, int N, int K, int H, int W, float *out, hipStream_t stream)
{
  if (K <= 0 || K % FP_KS != 0 || H <= 0 || W <= 0 || (long long)H * W >= (1LL << 24)) return PCT_NOT_COVERED;
  if (N == 0) return 0;
  const int tx = (W + FP_TW - 1) / FP_TW, ty = (H + FP_TH - 1) / FP_TH;
  const long long grid = (long long)N * tx * ty;
  if (grid >= 0x7fffffffLL) return PCT_NOT_COVERED;
  unsigned short *img1 = static_cast<unsigned short *>(w_ws), *img3 = img1 + (size_t)(K / FP_KS) * FP_WSTEP;
  const int pairs = FP_C * K / 2 + FP_C * (FP_C / 2) * 9;
  hipLaunchKernelGGL(fpn_weight_images_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, stream, w1, K, w3, img1, img3);
  const auto lateral = enc_nhwc ? fpn_lateral_kernel<true> : fpn_lateral_kernel<false>;
  hipLaunchKernelGGL(lateral, dim3((unsigned)grid), dim3(FP_BLOCK), 0, stream, x, img1, b1, norm1[0], norm1[1], norm1[2], norm1[3],
                     eps1, enc, enc_batch_stride, K, H, W, tx, ty, y_ws);
  hipLaunchKernelGGL(fpn_output_kernel, dim3((unsigned)grid), dim3(FP_BLOCK), 0, stream, y_ws, img3, b3, norm3[0], norm3[1],
                     norm3[2], norm3[3], eps3, H, W, tx, ty, out);
  return (int)hipGetLastError();
}

}  // namespace pct
