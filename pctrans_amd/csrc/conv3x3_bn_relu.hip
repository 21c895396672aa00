// The decoder's semantic head in eval mode on MI355X (gfx950): 3x3 convolution + BatchNorm (running statistics) + ReLU on bf16
// maps with 128 channels (NCHW, or channels-last as the mask features lie in memory), and, for the head's second block, the 1x1 convolution to one channel behind it
// (transformer_decoder/mask2former_transformer_decoder.py: `self.logits(self.seg_head(mf_lp))` under bf16 autocast):
//     z[n][co][y][x] = bf16( sum_{ci, ky, kx} bf16(W[co][ci][ky][kx]) * x[n][ci][y + ky - 1][x + kx - 1] )       (fp32 accumulation)
//     a[n][co][y][x] = relu( bf16( (z - mean[co]) * rsqrt(var[co] + eps) * gamma[co] + beta[co] ) )              (fp32 arithmetic)
//     LOGITS: out[n][0][y][x] = bf16( sum_co a[n][co][y][x] * bf16(w1[co]) + b1 )                                (fp32 accumulation)
// The rounding points are those of the library chain this replaces (convolution, batch norm, clamp and 1x1 convolution each
// writing a bf16 map); what differs is the order of the fp32 summation.
//
// Implicit GEMM, [128 co] x [1152 = 4 slabs of 32 ci x 9 taps] x [pixels], v_mfma_f32_32x32x16_bf16 with the weights as the A operand
// and the pixels as the columns.  A workgroup (4 waves) owns all 128 output channels of a tile of 8 rows x 32 columns; wave w
// owns rows 2 w and 2 w + 1: 4 x 2 MFMA tiles, 128 accumulators.  Per slab the [10 x 34 pixels incl. halo] x [32 channels] input
// block is staged ONCE as [pixel][channel]: a thread loads one pixel of 8 channels as the map lies in memory (NCHW: 8 two-byte
// loads, lanes along x; channels-last: one 16-byte load) and writes their 16 bytes, so that a B fragment -- 8 consecutive channels of a pixel per lane -- is one ds_read_b128 and the 9
// taps are whole-pixel offsets into the block (always aligned).  Pixels outside the image are staged as zeros: the padding.
// Pixel stride 80 B (64 + 16): the 16-lane groups of a ds_read_b128 and the 8-lane groups of a ds_write_b128 fall on distinct
// 16-byte slots.  The weights are rounded and laid out per call by a small kernel as the LDS image of each (slab, tap) step
// ([128 co][32 ci], 8 KB, same 80-byte stride in LDS) and streamed step by step from L2 through registers, double-buffered; the
// next slab's input is fetched into registers during taps 0 .. 5 of the current one and written behind a barrier after tap 8.
// One barrier per step of 16 MFMAs per wave; 50 KB of LDS, two workgroups per CU.
// With all 128 channels in one wave the LOGITS sum needs one cross-half shuffle and no LDS; that block's 128-channel output is
// never written.

#include "launchers.hpp"
#include "split_bf16.hpp"

namespace pct {

constexpr int S3_C = 128;                      // channels in and out
constexpr int S3_TH = 8, S3_TW = 32;           // output tile
constexpr int S3_HW = S3_TW + 2;               // staged row: 34 pixels
constexpr int S3_HP = (S3_TH + 2) * S3_HW;     // 340 staged pixels
constexpr int S3_CS = 32;                      // channels per slab
constexpr int S3_PS = 80;                      // bytes per staged pixel / per weight row in LDS
constexpr int S3_XBUF = S3_HP * S3_PS;         // 27 200
constexpr int S3_WBUF = S3_C * S3_PS;          // 10 240
constexpr int S3_BLOCK = 256;
constexpr int S3_TASKS = S3_HP * (S3_CS / 8);  // 1 360 (pixel, 8-channel group) staging tasks per slab
constexpr int S3_ROUNDS = (S3_TASKS + S3_BLOCK - 1) / S3_BLOCK;      // 6
constexpr int S3_STEP_ELEMS = S3_C * S3_CS;    // 4 096 bf16 per (slab, tap) weight image
constexpr int S3_W_ELEMS = S3_C * S3_C * 9;

__device__ __forceinline__ float s3_round_bf16(const float v) { return (float)(__bf16)v; }
__device__ __forceinline__ unsigned short s3_bits_bf16(const float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

// W [128][128][3][3] fp32 -> ws [slab][tap][co][32 ci] bf16 (round to nearest even, as autocast's cast); blockIdx.y: weight set
__global__ __launch_bounds__(256) void conv3x3_weight_image_kernel(const float *__restrict__ w0, const float *__restrict__ w1,
                                                                   unsigned short *__restrict__ ws)
{
  const int e = blockIdx.x * 256 + threadIdx.x;                    // index into the image
  if (e >= S3_W_ELEMS) return;
  const float *w = blockIdx.y ? w1 : w0;
  const int ci_l = e & 31, co = (e >> 5) & 127, st = e >> 12, slab = st / 9, tap = st - slab * 9;
  ws[(size_t)blockIdx.y * S3_W_ELEMS + e] = s3_bits_bf16(w[((size_t)co * S3_C + slab * S3_CS + ci_l) * 9 + tap]);
}

// NHWC: the maps (input, and the 128-channel output) are channels-last, [N][H][W][128]; else NCHW
template <bool LOGITS, bool NHWC>
__global__ __launch_bounds__(S3_BLOCK, 2) void conv3x3_bn_relu_kernel(
    const unsigned short *__restrict__ x, const unsigned short *__restrict__ ws, const float *__restrict__ bn_mean,
    const float *__restrict__ bn_var, const float *__restrict__ bn_gamma, const float *__restrict__ bn_beta, const float eps,
    const float *__restrict__ w1, const float *__restrict__ b1, const int H, const int W, const int tiles_x, const int tiles_y,
    unsigned short *__restrict__ y)
{
  __shared__ __attribute__((aligned(16))) unsigned char xs[S3_XBUF];
  __shared__ __attribute__((aligned(16))) unsigned char wsm[2][S3_WBUF];
  __shared__ f32x4 bn[S3_C];                                       // mean, rsqrt(var + eps), gamma, beta
  __shared__ float w1s[S3_C];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int tyi = tile / tiles_x, y0 = tyi * S3_TH, x0 = (tile - tyi * tiles_x) * S3_TW;
  const int HWp = H * W;
  const unsigned short *xn = x + (size_t)n * S3_C * HWp;

  if (tid < S3_C) {
    bn[tid] = f32x4{bn_mean[tid], rsqrtf(bn_var[tid] + eps), bn_gamma[tid], bn_beta[tid]};
    if constexpr (LOGITS) w1s[tid] = s3_round_bf16(w1[tid]);
  }

  // staging tasks of this thread (the same for every slab): element offset of channel 8 cg of the pixel inside the slab, -1 = zeros.
  // NCHW: lanes along the pixels, 8 two-byte loads a channel plane apart; NHWC: 4 lanes per pixel, one 16-byte load
  int goff[S3_ROUNDS], loff[S3_ROUNDS];
#pragma unroll
  for (int rd = 0; rd < S3_ROUNDS; ++rd) {
    const int task = rd * S3_BLOCK + tid;
    const int cg = NHWC ? (task & 3) : task / S3_HP, p = NHWC ? (task >> 2) : task - cg * S3_HP;
    const int py = p / S3_HW, px = p - py * S3_HW;
    const int gy = y0 - 1 + py, gx = x0 - 1 + px;
    const bool live = task < S3_TASKS;
    const int pix = gy * W + gx;
    goff[rd] = (live && gy >= 0 && gy < H && gx >= 0 && gx < W) ? (NHWC ? pix * S3_C + cg * 8 : cg * 8 * HWp + pix) : -1;
    loff[rd] = live ? p * S3_PS + cg * 16 : -1;
  }
  unsigned short raw[8];
  i32x4 gin[S3_ROUNDS], gw[2];
  auto load_x = [&](const int slab, const int rd) {
    if constexpr (NHWC) {
      gin[rd] = goff[rd] >= 0 ? *reinterpret_cast<const i32x4 *>(xn + slab * S3_CS + goff[rd]) : i32x4{0, 0, 0, 0};
    } else {
      const unsigned short *p = xn + (size_t)slab * S3_CS * HWp + (goff[rd] >= 0 ? goff[rd] : 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[j] = goff[rd] >= 0 ? p[(size_t)j * HWp] : (unsigned short)0;
    }
  };
  auto pack_x = [&](const int rd) {
    if constexpr (!NHWC)
      gin[rd] = i32x4{(int)(raw[0] | ((unsigned)raw[1] << 16)), (int)(raw[2] | ((unsigned)raw[3] << 16)),
                      (int)(raw[4] | ((unsigned)raw[5] << 16)), (int)(raw[6] | ((unsigned)raw[7] << 16))};
  };
  auto stash_x = [&]() {
#pragma unroll
    for (int rd = 0; rd < S3_ROUNDS; ++rd)
      if (loff[rd] >= 0) *reinterpret_cast<i32x4 *>(xs + loff[rd]) = gin[rd];
  };
  // weights: 512 chunks of 16 bytes per step, chunk c = row c / 4, part c % 4
  const int wl0 = (tid >> 2) * S3_PS + (tid & 3) * 16, wl1 = wl0 + 64 * S3_PS;
  auto fetch_w = [&](const int step) {
    const i32x4 *p = reinterpret_cast<const i32x4 *>(ws + (size_t)step * S3_STEP_ELEMS) + tid;
    gw[0] = p[0];
    gw[1] = p[S3_BLOCK];
  };
  auto stash_w = [&](const int buf) {
    *reinterpret_cast<i32x4 *>(wsm[buf] + wl0) = gw[0];
    *reinterpret_cast<i32x4 *>(wsm[buf] + wl1) = gw[1];
  };

  // fragment addresses: lane = (r, h); A: W[co = 32 rb + r][ci 8 h .. + 7 (+ 16 kk)], B: pixel (row 2 wave + cb, column r), same ci
  const int r = lane & 31, h = lane >> 5;
  const int a_off = r * S3_PS + h * 16;
  const int b_off = (2 * wave * S3_HW + r) * S3_PS + h * 16;

  f32x16 acc[4][2];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[rb][cb][j] = 0.f;

  fetch_w(0);
#pragma unroll
  for (int rd = 0; rd < S3_ROUNDS; ++rd) {
    load_x(0, rd);
    pack_x(rd);
  }
  stash_x();
  stash_w(0);
  __syncthreads();

  for (int slab = 0; slab < S3_C / S3_CS; ++slab) {
    const bool more_x = slab + 1 < S3_C / S3_CS;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int step = slab * 9 + tap, buf = step & 1;
      const bool more_w = more_x || tap < 8;
      if (more_w) fetch_w(step + 1);
      if (tap < S3_ROUNDS && more_x) load_x(slab + 1, tap);
      __builtin_amdgcn_sched_barrier(0);                           // the fetches ahead of the MFMAs
      const unsigned char *bp = xs + b_off + ((tap / 3) * S3_HW + tap % 3) * S3_PS;
      const unsigned char *ap = wsm[buf] + a_off;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 wa[4], xb[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) xb[cb] = *reinterpret_cast<const bf16x8 *>(bp + cb * S3_HW * S3_PS + kk * 32);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) wa[rb] = *reinterpret_cast<const bf16x8 *>(ap + rb * 32 * S3_PS + kk * 32);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) acc[rb][cb] = mfma_bf16(wa[rb], xb[cb], acc[rb][cb]);
      }
      if (tap < S3_ROUNDS && more_x) pack_x(tap);
      if (tap == 8 && more_x) {
        __syncthreads();                                           // every wave has left the input block
        stash_x();
      }
      if (more_w) stash_w(buf ^ 1);                                // (everyone left that buffer before the previous barrier)
      __syncthreads();
    }
  }

  // epilogue: acc[rb][cb][4 q + t] = z[co = 32 rb + 8 q + 4 h + t][row 2 wave + cb][column r]
  const int gx = x0 + r;
  if constexpr (LOGITS) {
    const float bias = b1 ? b1[0] : 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float s = 0.f;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int co = rb * 32 + 8 * q + 4 * h + t;
            const f32x4 c = bn[co];
            const float z = s3_round_bf16(acc[rb][cb][4 * q + t]);
            const float a = fmaxf(s3_round_bf16(fmaf(c[2], (z - c[0]) * c[1], c[3])), 0.f);
            s = fmaf(a, w1s[co], s);
          }
      s += __shfl_xor(s, 32);
      const int gy = y0 + 2 * wave + cb;
      if (h == 0 && gy < H && gx < W) y[((size_t)n * H + gy) * W + gx] = s3_bits_bf16(s + bias);
    }
    return;
  }
  unsigned short *yn = y + (size_t)n * S3_C * HWp;
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co0 = rb * 32 + 8 * q + 4 * h;
      f32x4 c[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = bn[co0 + t];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int gy = y0 + 2 * wave + cb;
        const bool live = gy < H && gx < W;
        const size_t pix = (size_t)gy * W + gx;
        float a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float z = s3_round_bf16(acc[rb][cb][4 * q + t]);
          a[t] = fmaxf(s3_round_bf16(fmaf(c[t][2], (z - c[t][0]) * c[t][1], c[t][3])), 0.f);
        }
        if constexpr (NHWC) {                                      // a lane's 4 consecutive channels: one 8-byte store
          const unsigned lo = s3_bits_bf16(a[0]) | ((unsigned)s3_bits_bf16(a[1]) << 16);
          const unsigned hi = s3_bits_bf16(a[2]) | ((unsigned)s3_bits_bf16(a[3]) << 16);
          if (live) *reinterpret_cast<uint2 *>(yn + pix * S3_C + co0) = uint2{lo, hi};
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (live) yn[(size_t)(co0 + t) * HWp + pix] = s3_bits_bf16(a[t]);
        }
      }
    }
}

namespace {

bool s3_geometry_ok(int C, int H, int W, int &tiles_x, int &tiles_y)
{
  if (C != S3_C || H <= 0 || W <= 0 || (long long)H * W >= (1LL << 24)) return false;     // 32-bit offsets inside an image
  tiles_x = (W + S3_TW - 1) / S3_TW;
  tiles_y = (H + S3_TH - 1) / S3_TH;
  return true;
}

template <bool LOGITS>
void s3_launch(bool nhwc, long long grid, hipStream_t stream, const void *x, const unsigned short *ws, const float *const *bnp, float eps,
               const float *w1, const float *b1, int H, int W, int tx, int ty, void *y)
{
  const auto kernel = nhwc ? conv3x3_bn_relu_kernel<LOGITS, true> : conv3x3_bn_relu_kernel<LOGITS, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(S3_BLOCK), 0, stream, static_cast<const unsigned short *>(x), ws, bnp[0],
                     bnp[1], bnp[2], bnp[3], eps, w1, b1, H, W, tx, ty, static_cast<unsigned short *>(y));
}

}  // namespace

// PCT_NOT_COVERED: anything but 128 channels, or an image of 2^24 pixels or more.  nhwc: x and out are channels-last
int launch_conv3x3_bn_relu(const void *x, int nhwc, const float *w, const float *const *bnp, float eps, void *w_ws, int N, int C, int H,
                           int W, void *out, hipStream_t stream)
{
  int tx, ty;
  if (!s3_geometry_ok(C, H, W, tx, ty)) return PCT_NOT_COVERED;
  if (N == 0) return 0;
  const long long grid = (long long)N * tx * ty;
  if (grid >= 0x7fffffffLL) return PCT_NOT_COVERED;
  unsigned short *ws = static_cast<unsigned short *>(w_ws);
  hipLaunchKernelGGL(conv3x3_weight_image_kernel, dim3((S3_W_ELEMS + 255) / 256, 1), dim3(256), 0, stream, w, w, ws);
  s3_launch<false>(nhwc != 0, grid, stream, x, ws, bnp, eps, nullptr, nullptr, H, W, tx, ty, out);
  return (int)hipGetLastError();
}

// both blocks and the 1x1 convolution: three launches.  bn_a / bn_b: {mean, var, gamma, beta}; mid has the layout of x
int launch_seg_head(const void *x, int nhwc, const float *w_a, const float *const *bn_a, float eps_a, const float *w_b,
                    const float *const *bn_b, float eps_b, const float *w_logits, const float *b_logits, void *w_ws, void *mid,
                    int N, int C, int H, int W, void *out, hipStream_t stream)
{
  int tx, ty;
  if (!s3_geometry_ok(C, H, W, tx, ty)) return PCT_NOT_COVERED;
  if (N == 0) return 0;
  const long long grid = (long long)N * tx * ty;
  if (grid >= 0x7fffffffLL) return PCT_NOT_COVERED;
  unsigned short *ws = static_cast<unsigned short *>(w_ws);
  hipLaunchKernelGGL(conv3x3_weight_image_kernel, dim3((S3_W_ELEMS + 255) / 256, 2), dim3(256), 0, stream, w_a, w_b, ws);
  s3_launch<false>(nhwc != 0, grid, stream, x, ws, bn_a, eps_a, nullptr, nullptr, H, W, tx, ty, mid);
  s3_launch<true>(nhwc != 0, grid, stream, mid, ws + S3_W_ELEMS, bn_b, eps_b, w_logits, b_logits, H, W, tx, ty, out);
  return (int)hipGetLastError();
}

}  // namespace pct
