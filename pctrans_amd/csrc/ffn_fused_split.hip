// The encoder layer's whole feed-forward block in ONE kernel on MI355X (gfx950):
//     y = LayerNorm(x + W2 . relu(W1 . x + b1) + b2),        x, y [rows, 128] fp32, W1 [F, 128], W2 [128, F], F % 32 == 0
// (pixel_decoder/msdeformattn.py:122-131 of the reference: linear1, activation, dropout2, linear2, dropout3, norm2; F = 1024.)
// As two kernels (linear_k128_split.hip + linear_ln_split.hip) the [rows, F] hidden tensor -- 11.4 GB at the bench's 2.8 M rows --
// is written by one and read back by the other: 21 + 25 ms of the 102 ms step, both kernels' matrix pipes 47-62 % busy, half
// of their time memory.  Here the hidden activations never leave the registers.
//
// Same arithmetic as those kernels: every fp32 operand is the exact sum of three bf16 pieces, a product is evaluated from its six
// leading partial products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, the a1w1 chain and the five small terms in separate
// accumulators; the hidden value is the fp32 number (hi + lo) + b1, ReLU'd, split again exactly.
//
// Structure.  Workgroup = 4 waves = 128 rows, ONE workgroup per CU with the whole register file (512 registers per lane) and
// 112 KB of LDS.  A wave owns 32 rows for both products, so nothing but weights is shared:
//   * its rows of x are split once per tile into the B fragments of GEMM 1 (8 k-steps x 3 planes, 96 registers);
//   * the hidden dimension is walked in chunks of 32 units: GEMM 1 gives D1[hidden 32][rows 32] -- W1 pieces as the A operand,
//     the transposed product as everywhere in this library -- whose accumulator layout holds, per lane (row r, half h), hidden
//     units 8 q + 4 h + t: after bias, ReLU and split these registers ARE the B fragments of GEMM 2, y[cols][rows] += W2 . h,
//     under a permutation of the k slots that the W2 image in LDS is written in (slot (h, e) of k-step s <-> hidden
//     16 s + 4 h + e for e < 4, 16 s + 8 + 4 h + e - 4 else): no LDS round trip, no shuffles;
//   * both weight matrices are pre-split per call into the exact LDS image of every chunk (W1: 32 rows x 128 k, row stride
//     272 B; W2: 128 rows x 32 permuted k, row stride 80 B; both conflict-free for ds_read_b128), 56 KB per chunk, streamed from
//     L2 by LDS-DMA into a double-buffered stage, one barrier per chunk;
//   * a tile's LayerNorm and stores run under the next tile's first product;
//   * the row statistics of the LayerNorm are complete inside a wave (a lane and its partner in the other half hold a row's 128
//     columns).
#include <stdlib.h>
#include <type_traits>
#include "msda_win_common.hpp"    // func_attr_per_device
#include "launchers.hpp"
#include "split_bf16.hpp"

namespace pct {

constexpr int FF_BLOCK = 256;
constexpr int FF_BM = 128;                        // rows per workgroup tile
constexpr int FF_D = 128;                         // model width
constexpr int FF_CH = 32;                         // hidden units per chunk
constexpr int FF_W1ROW = 272;                     // bytes per W1 row of a plane (128 bf16 + 16 pad)
constexpr int FF_W1PLANE = FF_CH * FF_W1ROW;      // 8 704
constexpr int FF_W2ROW = 80;                      // bytes per W2 row of a plane (32 bf16 + 16 pad)
constexpr int FF_W2PLANE = FF_D * FF_W2ROW;       // 10 240
constexpr int FF_W2OFF = 3 * FF_W1PLANE;          // 26 112
constexpr int FF_STAGE = 57344;                   // 26 112 + 30 720 = 56 832, padded to 256 threads x 14 x 16 B
constexpr int FF_PIECES = FF_STAGE / (FF_BLOCK * 16);   // 14
constexpr int FF_HALF = FF_PIECES / 2;                  // 7
constexpr int FF_LDS = 2 * FF_STAGE + 3 * FF_D * 4;     // two stages, then b2, gamma, beta
constexpr int FF_B1OFF = 56832;                         // the chunk's 32 biases, in the padding

// W1 [F][128], W2 [128][F], b1 [F] fp32 -> img [F / 32][FF_STAGE bytes]: image c holds W2 and b1 of chunk c and W1 of chunk c + 1
// (mod F / 32): what one iteration of the kernel's chunk loop reads (see the header); one thread per element pair
__global__ __launch_bounds__(256) void ffn_split_weights_kernel(const float *__restrict__ w1, const float *__restrict__ w2,
                                                                const float *__restrict__ b1, const int F,
                                                                unsigned short *__restrict__ img)
{
  const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
  const long long n1 = (long long)F * FF_D;
  const int nch = F / FF_CH;
  unsigned p1, p2, p3;
  if (e < n1) {                                                   // W1[u][k], k even: row u % 32, k-contiguous
    const int u = (int)(e / FF_D), k = (int)(e - (long long)u * FF_D);
    split_bf16x3(w1[e], w1[e + 1], p1, p2, p3);
    const int c = (u / FF_CH + nch - 1) % nch;
    unsigned short *d = img + (size_t)c * (FF_STAGE / 2) + (size_t)(u % FF_CH) * (FF_W1ROW / 2) + k;
    store_planes(d, FF_W1PLANE / 2, p1, p2, p3);
  } else if (e < 2 * n1) {                                        // W2[c][u], u even: chunk u / 32, row c, slot of u in the chunk
    const long long e2 = e - n1;
    const int c = (int)(e2 / F), u = (int)(e2 - (long long)c * F);
    split_bf16x3(w2[e2], w2[e2 + 1], p1, p2, p3);
    const int uu = u % FF_CH;                                     // 0 .. 31 (even): s = uu / 16, inside: v = uu % 16
    const int s = uu >> 4, v = uu & 15;
    // hidden 16 s + v with v = 8 g + 4 h + t (g = 0, 1; h = 0, 1; t = 0 .. 3) sits in slot (h, e = 4 g + t) of k-step s:
    // bf16 index inside the row = (2 s + h) * 8 + 4 g + t
    const int g = v >> 3, h = (v >> 2) & 1, t = v & 3;
    unsigned short *d = img + (size_t)(u / FF_CH) * (FF_STAGE / 2) + (size_t)(FF_W2OFF / 2) + (size_t)c * (FF_W2ROW / 2) +
                        (2 * s + h) * 8 + 4 * g + t;
    store_planes(d, FF_W2PLANE / 2, p1, p2, p3);                  // (t even: t and t + 1 are adjacent slots)
  } else if (e < 2 * n1 + F) {                                    // b1[u], u even
    const int u = (int)(e - 2 * n1);
    float *d = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(img) + (size_t)(u / FF_CH) * FF_STAGE + FF_B1OFF) + u % FF_CH;
    d[0] = b1[u];
    d[1] = b1[u + 1];
  }
}

__global__ __launch_bounds__(FF_BLOCK, 1) void ffn_fused_split_kernel(
    const float *__restrict__ X, const long long ldx, const unsigned short *__restrict__ img, const int F,
    const float *__restrict__ b2, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float eps, const long long M, float *__restrict__ Y, const long long ldy)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char ff_smem[];    // two stages
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const long long ntiles = (M + FF_BM - 1) / FF_BM;
  const int nch = F / FF_CH;

  // An image travels to LDS by LDS-DMA: piece p (0 .. 13) of 4 KiB is ONE 16-byte buffer_load ... lds per thread, wave w writing
  // bytes 1024 w .. + 1023 of the piece lane-linearly -- the global image is the exact LDS image (ffn_split_weights_kernel), so no
  // register holds it on the way and the 272 / 80 B row strides stay as they are.  A stage's DMAs are retired by a counted vmcnt
  // before the barrier that precedes its first read (never __syncthreads(): its fence would drain every DMA in flight).  Image
  // c + 1 into the free stage: its W2 / bias pieces 7 .. 13 behind the barrier of chunk c - 1 (the W1 part of that stage may still
  // be read at a tile seam), its W1 pieces 0 .. 6 in phase A of chunk c.  (The buffer form: one lane offset and a scalar one per
  // DMA, where global_load_lds's 64-bit lane addresses of the loop-invariant images were hoisted and spilled.)
  const auto img_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(img), 0, (int)((long long)nch * FF_STAGE),
                                                          0x00020000);
  auto t_dma = [&](const int piece, const int image, unsigned char *stage) {
    auto *dst = (__attribute__((address_space(3))) void *)(stage + piece * (FF_BLOCK * 16) + wave * 1024);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(img_rsrc, dst, 16, tid * 16, image * FF_STAGE + piece * (FF_BLOCK * 16), 0, 0);
  };

  // fragment addresses inside a stage: W1 (A operand of GEMM 1): hidden row r, k = 16 s + 8 h ..; W2 (A operand of GEMM 2):
  // output column 32 cb + r, slots of k-step s and half h
  const int w1_off = r * FF_W1ROW + 16 * h;                       // + 32 s, + plane
  const int w2_off = FF_W2OFF + r * FF_W2ROW + 16 * h;            // + cb * 32 rows, + 32 s, + plane

  // s_waitcnt vmcnt(n) lgkmcnt(0) as the builtin, so that hipcc's own wait bookkeeping sees the DMAs retired (while it counts one
  // as pending it waits vmcnt(0) at the next use of any loaded register), then the barrier
  auto wait_barrier = [](auto n_tag) {
    constexpr int n = decltype(n_tag)::value;
    static_assert(n >= 0 && n < 16, "vmcnt field");
    __builtin_amdgcn_s_waitcnt(0x70 | n);                         // gfx9 encoding: vmcnt [3:0], expcnt [6:4] = 7 (no wait), lgkmcnt [11:8] = 0
    asm volatile("s_barrier" ::: "memory");
  };

  // stage 1 <- the last image (W1 of chunk 0), stage 0 <- image 0, retired before the barrier below
#pragma unroll
  for (int p = 0; p < FF_PIECES; ++p) {
    t_dma(p, nch - 1, ff_smem + FF_STAGE);
    t_dma(p, 0, ff_smem);
  }
  if (tid < FF_D) {                                               // b2, gamma, beta behind the stages
    float *par = reinterpret_cast<float *>(ff_smem + 2 * FF_STAGE);
    par[tid] = b2 ? b2[tid] : 0.f;
    par[FF_D + tid] = gamma[tid];
    par[2 * FF_D + tid] = beta[tid];
  }
  wait_barrier(std::integral_constant<int, 0>{});
  int cur = 0;                                                    // stage holding the image of the chunk about to be used

  // a tile's rows of x are requested one tile ahead (under GEMM 2 of the last chunk of the tile before, when the fragments of the
  // current rows are no longer needed; a row-strided load touches 32 lines: 16 of them back to back cost 3 k cycles): lane (r, h) takes k = 16 s + 8 h .. + 7 of row r, s = 0 .. 7
  i32x4 xraw[16];
  auto x_request = [&](const long long tile, const int s0, const int s1) {      // k-steps s0 .. s1 - 1
    const long long row0 = tile * FF_BM + 32 * wave;
    const long long left = M - row0;
    const unsigned xbytes = (unsigned)((left < 32 ? (left < 0 ? 0 : left) : 32) * ldx * 4);      // past the end: zeros
    const auto xq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(X + (left > 0 ? row0 : 0) * ldx), 0, (int)xbytes, 0x00020000);
    const int xoff = (int)((r * ldx + 8 * h) * 4);
#pragma unroll
    for (int s = s0; s < s1; ++s) {
      xraw[2 * s] = __builtin_amdgcn_raw_buffer_load_b128(xq, xoff, s * 64, 0);
      xraw[2 * s + 1] = __builtin_amdgcn_raw_buffer_load_b128(xq, xoff, s * 64 + 16, 0);
    }
  };

  // GEMM 1: D1[hidden 8 q + 4 h + t][row r] over k = 128 from the W1 part of stage `st`.  One wave per SIMD: nobody else covers an
  // LDS round trip, so the fragments of k-step s + 1 are requested before the MFMAs of step s
  bf16x8 xp[8][3];                                             // this wave's 32 rows of x as GEMM 1's B fragments
  f32x16 h_hi, h_lo;
  bf16x8 wa[2][3];
  auto split_x = [&](const int s) {
    split_bf16x3_8(__builtin_bit_cast(f32x4, xraw[2 * s]), __builtin_bit_cast(f32x4, xraw[2 * s + 1]), xp[s]);
  };
  auto w1_frags = [&](const unsigned char *st, const int s) {
#pragma unroll
    for (int p = 0; p < 3; ++p) wa[s & 1][p] = *reinterpret_cast<const bf16x8 *>(st + w1_off + 32 * s + p * FF_W1PLANE);
  };
  auto gemm1_step = [&](const int s) {
    const bf16x8 a1 = wa[s & 1][0], a2 = wa[s & 1][1], a3 = wa[s & 1][2];
    // split_mfma6(a1, a2, a3, xp[s], h_hi, h_lo) written out, here and in phase B: through the shared function this kernel's
    // schedule and register allocation come out different (the MFMAs are interleaved by hand below), the other GEMMs' do not
    h_lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xp[s][2], h_lo, 0, 0, 0);
    h_hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xp[s][0], h_hi, 0, 0, 0);
    h_lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, xp[s][0], h_lo, 0, 0, 0);
    h_lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, xp[s][1], h_lo, 0, 0, 0);
    h_lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xp[s][1], h_lo, 0, 0, 0);
    h_lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, xp[s][0], h_lo, 0, 0, 0);
  };
  // a tile's chunk 0 starts with its first product alone: its W1 is in the image the tile before ended on, in the stage that is not
  // `cur`.  Its k-step s + 1 of x is split under k-step s, with the LayerNorm of the tile before (`epi(s)`; nothing for the first
  // tile), and it takes image 1's W2 / bias pieces by DMA into the part of that stage it does not read; iteration 0 then refills the
  // W1 part
  auto first_gemm1 = [&](auto epi) {
    unsigned char *pst = ff_smem + (cur ^ 1) * FF_STAGE;
#pragma unroll
    for (int j = 0; j < 16; ++j) h_hi[j] = h_lo[j] = 0.f;
    w1_frags(pst, 0);
    split_x(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s < 7) w1_frags(pst, s + 1);
      gemm1_step(s);
      if (s < 7) split_x(s + 1);
      if (s < 7) t_dma(FF_HALF + s, 1 % nch, pst);
      epi(s);
      __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);          // the reads first (left alone the scheduler sinks them)
#pragma unroll
      for (int i = 0; i < 6; ++i) {                               // the epilogue's arithmetic and stores between the MFMAs
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 10, 0);
        if (i == 1 && s < 7) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        if (s >= 4 && i < 4) __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };

  x_request(blockIdx.x, 0, 8);
  first_gemm1([](int) {});

  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row0 = tile * FF_BM + 32 * wave;
    const long long left = M - row0;
    const unsigned xbytes = (unsigned)((left < 32 ? (left < 0 ? 0 : left) : 32) * ldx * 4);
    const auto xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(X + row0 * ldx), 0, (int)xbytes, 0x00020000);
    f32x16 y_hi[4], y_lo[4];                                   // D2[col block][cols 32][rows 32]
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int j = 0; j < 16; ++j) y_hi[cb][j] = y_lo[cb][j] = 0.f;
    f32x4 res[16];                                             // the residual: columns 32 cb + 8 q + 4 h .. + 3 of row r, [4 cb + q]

    // entering iteration `chunk`: wa[0] = step 0 of the W1 fragments and bq = the biases it needs, the W2 / bias pieces of image
    // chunk + 1 on their way
    f32x4 bq[4];
    auto load_bias = [&](const unsigned char *st) {
#pragma unroll
      for (int q = 0; q < 4; ++q) bq[q] = *reinterpret_cast<const f32x4 *>(st + FF_B1OFF + (8 * q + 4 * h) * 4);
    };
    w1_frags(ff_smem + cur * FF_STAGE, 0);
    load_bias(ff_smem + cur * FF_STAGE);

    auto chunk_body = [&](auto last_tag, const int chunk) {
      constexpr bool LAST = decltype(last_tag)::value;
      const unsigned char *st = ff_smem + cur * FF_STAGE;         // image `chunk`: W2 and b1 of this chunk, W1 of the next
      unsigned char *nst = ff_smem + (cur ^ 1) * FF_STAGE;        // nobody reads it since the previous barrier: image chunk + 1
      const int nxt = LAST ? 0 : chunk + 1, nxt2 = (chunk + 2) % nch;
      // this chunk's hidden accumulators move to the vector side; the same registers then take the next chunk's product
      const f32x16 c_hi = h_hi, c_lo = h_lo;
      if constexpr (!LAST) {
#pragma unroll
        for (int j = 0; j < 16; ++j) h_hi[j] = h_lo[j] = 0.f;
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- phase A: GEMM 1 of chunk + 1 under bias, ReLU, split of this chunk: value pair m of the B fragments of GEMM 2 is k-step
      // sg = m / 4, word w = m % 4 (accumulator quartet q = 2 sg + w / 2, elements 2 (w % 2) and + 1); pairs 0 - 3 (k-step 0) behind
      // the odd steps here, pairs 4 - 7 (k-step 1, first used by group 4) behind groups 0 - 3 of phase B; image chunk + 1: the W1
      // pieces 0 .. 6 by DMA into the stage nobody reads since the previous barrier, two per step in steps 0 - 3 (as early as that:
      // 6.545 -> 6.525 ms against one per step in steps 0 - 6).  The last chunk (no product here) requests the tile's residual rows
      // in steps 0 - 5: the barrier's wait, which leaves only the x loads of phase B in flight, retires them ---------------------
      unsigned hpw[2][3][4];
      bf16x8 wb[2][3], wc[3];
      auto valu_slice = [&](const int m) {
        const int sg = m >> 2, w = m & 3, q = 2 * sg + (w >> 1), t0 = 2 * (w & 1), j0 = 4 * q + t0;
        const float v0 = fmaxf((c_hi[j0] + c_lo[j0]) + bq[q][t0], 0.f);
        const float v1 = fmaxf((c_hi[j0 + 1] + c_lo[j0 + 1]) + bq[q][t0 + 1], 0.f);
        split_bf16x3(v0, v1, hpw[sg][0][w], hpw[sg][1][w], hpw[sg][2][w]);
      };
      auto h_frag = [&](const int sg, const int p) {
        return __builtin_bit_cast(bf16x8, i32x4{(int)hpw[sg][p][0], (int)hpw[sg][p][1], (int)hpw[sg][p][2], (int)hpw[sg][p][3]});
      };
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        if constexpr (!LAST) {
          if (s < 7) w1_frags(st, s + 1);
          gemm1_step(s);
        }
        if (s == 7) {
#pragma unroll
          for (int p = 0; p < 3; ++p) wb[0][p] = *reinterpret_cast<const bf16x8 *>(st + w2_off + p * FF_W2PLANE);
        }
        if (s & 1) valu_slice(s >> 1);
        if constexpr (LAST) {
          if (s < 6) {
#pragma unroll
            for (int i = s < 4 ? 3 * s : 2 * s + 4; i < (s < 4 ? 3 * s + 3 : 2 * s + 6); ++i)     // column 8 i + 4 h
              res[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, (int)((r * ldx + 4 * h) * 4), 32 * i, 0));
          }
        }
        if (s < 3) {
          t_dma(2 * s, nxt, nst);
          t_dma(2 * s + 1, nxt, nst);
        }
        if (s == 3) t_dma(6, nxt, nst);
        if constexpr (!LAST) {                                    // reads first; vector instructions, the load and the store between MFMAs
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (s & 1) __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            if (!(i & 1)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // fragment reads spread between the MFMAs
            if ((i == 1 || (i == 3 && s < 3)) && s < 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- phase B: GEMM 2: D2[col 32 cb + 8 q + 4 h + t][row r] += W2 . h over this chunk's 32 hidden units; group g = (s, cb),
      // the next group's fragments requested before this group's MFMAs.  The last two groups' fragments are in registers before
      // group 6, so the chunk's barrier sits after group 5, behind the wait that retires image chunk + 1's DMAs: groups 6 and 7 cover
      // it, the first reads of the next iteration and the W2 / bias pieces of image chunk + 2 into the stage just read (the last
      // chunk leaves them to the next tile's first product: no DMA is in flight in the epilogue, whose loads then have counted waits)
      auto w2_frags = [&](bf16x8 (&dst)[3], const int g) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
          dst[p] = *reinterpret_cast<const bf16x8 *>(st + w2_off + (g & 3) * 32 * FF_W2ROW + 32 * (g >> 2) + p * FF_W2PLANE);
      };
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const int sg = g >> 2, cb = g & 3;
        if (g < 5) w2_frags(wb[(g + 1) & 1], g + 1);
        if (g == 5) {
          w2_frags(wb[0], 6);
          w2_frags(wc, 7);
        }
        if (g < 4) valu_slice(4 + g);
        if constexpr (LAST) x_request(tile + gridDim.x, g, g + 1);     // the next tile's rows, two row-strided loads per group
        if constexpr (!LAST) {                                    // behind the barrier: this stage is free, image chunk + 2
          if (g == 6) {
#pragma unroll
            for (int p = FF_HALF; p < FF_HALF + 4; ++p) t_dma(p, nxt2, const_cast<unsigned char *>(st));
            w1_frags(nst, 0);
            load_bias(nst);
          }
          if (g == 7)
#pragma unroll
            for (int p = FF_HALF + 4; p < FF_PIECES; ++p) t_dma(p, nxt2, const_cast<unsigned char *>(st));
        }
        const bf16x8 a1 = g == 7 ? wc[0] : wb[g & 1][0], a2 = g == 7 ? wc[1] : wb[g & 1][1], a3 = g == 7 ? wc[2] : wb[g & 1][2];
        y_lo[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, h_frag(sg, 2), y_lo[cb], 0, 0, 0);
        y_hi[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, h_frag(sg, 0), y_hi[cb], 0, 0, 0);
        y_lo[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, h_frag(sg, 0), y_lo[cb], 0, 0, 0);
        y_lo[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, h_frag(sg, 1), y_lo[cb], 0, 0, 0);
        y_lo[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, h_frag(sg, 1), y_lo[cb], 0, 0, 0);
        y_lo[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, h_frag(sg, 0), y_lo[cb], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if (g < 4) __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
          // fragment reads one (two, group 5 and 6) per MFMA, not in a burst
          if (g < 5 && !(i & 1)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          if (g == 5) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          if (g == 6 && !LAST) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          if (g == 6 && !LAST && i == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          if (g == 6 && !LAST && i < 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
          if (g == 7 && !LAST && i < 3) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (g == 5) {                                             // (the last chunk: the 12 x loads of groups 0 - 5 stay in flight)
          if constexpr (LAST) wait_barrier(std::integral_constant<int, 12>{});
          else wait_barrier(std::integral_constant<int, 0>{});
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      cur ^= 1;
    };
    for (int chunk = 0; chunk + 1 < nch; ++chunk) chunk_body(std::false_type{}, chunk);
    chunk_body(std::true_type{}, nch - 1);

    // ---- epilogue: y_*[cb][4 q + t] = y[row r][column 32 cb + 8 q + 4 h + t]; + b2 + residual, then the LayerNorm and the stores in
    // eight slices, one per k-step of the next tile's first product, which they run under ---------------------------------------
    const unsigned ybytes = (unsigned)((left < 32 ? (left < 0 ? 0 : left) : 32) * ldy * 4);
    const auto yr = __builtin_amdgcn_make_buffer_rsrc(Y + row0 * ldy, 0, (int)ybytes, 0x00020000);
    float v[64];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * cb + 8 * q + 4 * h;
        const f32x4 bb = *reinterpret_cast<const f32x4 *>(ff_smem + 2 * FF_STAGE + c0 * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[16 * cb + 4 * q + t] = ((y_hi[cb][4 * q + t] + y_lo[cb][4 * q + t]) + bb[t]) + res[4 * cb + q][t];
      }
    __builtin_amdgcn_sched_barrier(0);
    float sm = 0.f, s2 = 0.f, mean, rstd;
    auto epi = [&](const int s) {
      if (s < 2) {                                                // the row sum
#pragma unroll
        for (int j = 32 * s; j < 32 * s + 32; ++j) sm += v[j];
        if (s == 1) {
          sm += __shfl_xor(sm, 32);
          mean = sm * (1.f / 128.f);
        }
      } else if (s < 4) {                                         // centred, the sum of squares
#pragma unroll
        for (int j = 32 * (s - 2); j < 32 * (s - 2) + 32; ++j) {
          v[j] -= mean;
          s2 += v[j] * v[j];
        }
        if (s == 3) {
          s2 += __shfl_xor(s2, 32);
          rstd = rsqrtf(s2 * (1.f / 128.f) + eps);
        }
      } else {                                                    // scaled, shifted, stored: column block s - 4
        const int cb = s - 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c0 = 32 * cb + 8 * q + 4 * h;
          const f32x4 gq = *reinterpret_cast<const f32x4 *>(ff_smem + 2 * FF_STAGE + (FF_D + c0) * 4);
          const f32x4 eq = *reinterpret_cast<const f32x4 *>(ff_smem + 2 * FF_STAGE + (2 * FF_D + c0) * 4);
          f32x4 o;
#pragma unroll
          for (int t = 0; t < 4; ++t) o[t] = v[16 * cb + 4 * q + t] * rstd * gq[t] + eq[t];
          // (y rows with the non-temporal hint: 6.79 -> 6.97 ms)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, o), yr, (int)((r * ldy + 4 * h) * 4), 4 * (c0 - 4 * h), 0);
        }
      }
    };
    // (also after the last tile, on the zero rows x_request returns past the end: with a use on one path only, the compiler sinks
    // the x loads out of the last chunk into that path, behind the barrier whose counted wait assumes them)
    first_gemm1(epi);
  }
  __builtin_amdgcn_s_waitcnt(0x70);                               // no DMA outlives the workgroup's LDS
}

// the kernel's LDS attribute for the current device, outside any stream capture (pct_prepare_device)
int prepare_ffn_device() { return func_attr_per_device(reinterpret_cast<const void *>(&ffn_fused_split_kernel), FF_LDS) == hipSuccess ? 0 : PCT_ERR_UNSUPPORTED; }

// img_ws: (F / 32) * 57 344 bytes, 16-byte aligned, refilled on every call.  PCT_ERR_UNSUPPORTED: geometry not covered.
int launch_ffn_fused_split(const float *x, long long ldx, const float *w1, const float *b1, const float *w2, const float *b2,
                           const float *gamma, const float *beta, float eps, int F, long long rows, void *img_ws, float *out,
                           long long ldo, hipStream_t stream)
{
  if (rows <= 0) return 0;
  if (F <= 0 || F % FF_CH) return PCT_ERR_UNSUPPORTED;
  if ((long long)(F / FF_CH) * FF_STAGE > 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  if (32LL * (ldx > ldo ? ldx : ldo) * 4 > 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  if (func_attr_per_device(reinterpret_cast<const void *>(&ffn_fused_split_kernel), FF_LDS) != hipSuccess) return PCT_ERR_UNSUPPORTED;
  const long long pairs = (long long)F * FF_D + F / 2;            // element pairs of both matrices and the bias
  hipLaunchKernelGGL(ffn_split_weights_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, stream, w1, w2, b1, F,
                     static_cast<unsigned short *>(img_ws));
  const long long ntiles = (rows + FF_BM - 1) / FF_BM;
  const unsigned gx = (unsigned)(ntiles < 256 ? ntiles : 256);    // persistent: one workgroup per CU
  hipLaunchKernelGGL(ffn_fused_split_kernel, dim3(gx), dim3(FF_BLOCK), FF_LDS, stream, x, ldx,
                     static_cast<const unsigned short *>(img_ws), F, b2, gamma, beta, eps, rows, out, ldo);
  return (int)hipGetLastError();
}

}  // namespace pct
