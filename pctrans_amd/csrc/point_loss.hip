// Point-sampled mask losses (include/pctrans_hip_train.h: pct_point_sample_f32, pct_point_mask_loss_forward_f32,
// pct_point_mask_loss_backward_f32, pct_point_select_uncertain_f32, pct_point_match_cost_f32): the gather, the fused BCE + dice
// sums and the scatter of their gradient that loss/matcher.py and loss/maskformer_criterion.py otherwise run as grid_sample
// forward / backward plus elementwise and reduce launches, the choice of the most uncertain of the oversampled candidates that
// the criterion otherwise makes with a gather, topk, gather and cat, and the matcher's cost matrices that it otherwise forms
// from two gathers with a chain of elementwise launches and three einsum.  The selection, the loss forward and the cost pass
// serve up to PL_MAX_HEADS prediction heads in one launch (pct_point_select_uncertain_many_f32,
// pct_point_mask_loss_forward_many_f32, pct_point_match_cost_many_f32), the head taken from a grid dimension (HeadPlanes below);
// the single-head selection and loss forward are the same launch with one head.
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
#include "wave_reduce.hpp"

namespace pct {

namespace {

constexpr int PL_BAND_ROWS = 32;      // rows of a backward band (pctrans_amd/point_loss.py: BAND_ROWS)
constexpr int PL_MAX_WIDTH = 256;     // 32 rows x 256 pixels x 8 B = 64 KiB of LDS: two workgroups per CU
constexpr int PL_GATHER_BLOCK = 256;
constexpr int PL_FWD_BLOCK = 1024;
constexpr int PL_BWD_BLOCK = 512;
constexpr int PL_SELECT_BLOCK = 1024;
constexpr int PL_SELECT_MAX_CAND = 65536;   // 64 keys per thread in registers (pctrans_amd/point_loss.py: MAX_CANDIDATES)
constexpr int PL_SELECT_COPIES = 32;        // copies of the digit histogram: one per LDS bank

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

// The prediction planes of the heads of a launch: a by-value kernel argument (128 bytes of the kernarg segment, read with a
// scalar load at a uniform index), so that nothing is uploaded.  The *_many kernels take their head from a grid dimension, move
// every per-head array to that head's slice and run their *_body on it: a head's bits do not depend on how many heads the
// launch has.  A single-head selection or loss forward is a launch of one head (c_abi.hip); the cost pass alone keeps
// single-head kernels beside its *_many pair, because one head of that pair measured slower than they are.
// point_select_body and point_loss_forward_body now have one caller each and still stay device functions of their own, as
// the cost pass's two do: written out inside their kernels, hipcc schedules every one of the four differently
// (match_cost_partial_many_kernel then takes 228 VGPRs, not 165).
constexpr int PL_MAX_HEADS = 16;           // include/pctrans_hip_train.h: PCT_POINT_MAX_HEADS
static_assert(PL_MAX_HEADS == PCT_POINT_MAX_HEADS, "the header's limit");

struct HeadPlanes {
  const float *p[PL_MAX_HEADS];
};

// one workgroup per pair: every thread a fixed subset of the points in ascending order, then a fixed tree over the lanes and
// the waves in ascending order
__device__ __forceinline__ void point_loss_forward_body(
    const float *__restrict__ pred, const int *__restrict__ src_index, const int num_pred, const int H, const int W,
    const float *__restrict__ tgt, const int *__restrict__ tgt_index, const int num_tgt, const int Ht, const int Wt,
    const float2 *__restrict__ coords, const int P, float *__restrict__ xs, float *__restrict__ ts, float *__restrict__ sums,
    const int k)
{
  __shared__ float part[PL_FWD_BLOCK / 64][4];
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
  for (int i = 0; i < 4; ++i) s[i] = wave_sum(s[i]);
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

// grid (pair, head): the index vectors are [heads, K], coords [heads, K, P, 2], x, t [heads, K, P], sums [heads, K, 4]
__global__ __launch_bounds__(PL_FWD_BLOCK) void point_loss_forward_many_kernel(
    const HeadPlanes heads, const int *__restrict__ src_index, const int num_pred, const int H, const int W,
    const float *__restrict__ tgt, const int *__restrict__ tgt_index, const int num_tgt, const int Ht, const int Wt,
    const float2 *__restrict__ coords, const int K, const int P, float *__restrict__ xs, float *__restrict__ ts,
    float *__restrict__ sums)
{
  const size_t row0 = (size_t)blockIdx.y * K;
  point_loss_forward_body(heads.p[blockIdx.y], src_index ? src_index + row0 : nullptr, num_pred, H, W, tgt,
                          tgt_index ? tgt_index + row0 : nullptr, num_tgt, Ht, Wt, coords + row0 * P, P, xs + row0 * P,
                          ts + row0 * P, sums + row0 * 4, blockIdx.x);
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

// Selection of the num_keep most uncertain (smallest |logit|) of S candidates, one workgroup per pair, no sort and the logits
// never in memory.  key = bits of |x| (NaN: 0); unsigned order of the keys is the order of |x|.
//
// Candidates are dealt to the threads strided: round i, thread t holds candidate i * 1024 + t, so a wave's coordinate loads
// and stores are contiguous.  A blocked deal (thread t holds IPT consecutive candidates) would give each thread one run of
// candidate order and so one scan of per-thread counts, but 8-byte loads IPT * 8 bytes apart.  The strided deal keeps one scan
// as well: in round i the 64 candidates of a wave are consecutive, their order inside the wave is the lane order (a ballot
// and a population count of the lanes below), and the (round, wave) cells in ascending order are the candidate order.  So
// one workgroup-wide exclusive scan over the IPT * 16 <= 1024 cell counts, one cell per thread, places every candidate.
//
// 1. Every thread samples its IPT candidates (make_taps / sample_plane: the gather's code, the gather's bits) and keeps the
//    keys in registers; every loop over them is fully unrolled.  A thread's samples run one after the other (the taps sit
//    behind their bounds tests): this, not a throughput limit, is what the kernel's time is made of.
// 2. Radix select, most significant byte first, four passes.  A pass counts the byte of the keys that agree with the bytes
//    chosen so far in a 256-bin LDS histogram, finds the bin that holds rank `rank` and descends into it.  The histogram has
//    PL_SELECT_COPIES = 32 copies laid out [bin][copy] with copy = lane & 31: the 32 lanes the LDS serves together hit 32
//    different banks whatever their bins, so the adds (integer, workgroup scope, order-free) never conflict, also when every
//    key falls in one bin (an all-zero plane; logits of one exponent).  The copies are summed by all threads (bin t / 4, eight
//    copies each, rotated by the bin so that the 32 lanes again read 32 banks) and cleared for the next pass; wave 0 scans the
//    256 totals.  After the last pass `key_t` is the num_keep-th smallest key and `rank` the number of candidates equal to
//    it that are admitted: the first `rank` of them in candidate order.
// 3. Ballots of key < key_t and key == key_t per round and wave, the scan of their counts, and for candidate s with `lb` lower
//    and `eb` equal keys before it:  selected = lower or (equal and eb < rank),  position = lb + min(eb, rank).
template <int IPT>
__device__ __forceinline__ void point_select_body(const float *__restrict__ pred, const int *__restrict__ src_index,
                                                  const int num_pred, const int H, const int W, const float2 *__restrict__ cand,
                                                  const int S, const int num_keep, float2 *__restrict__ out,
                                                  const int out_row_points, int *__restrict__ out_index, const int k)
{
  constexpr int WAVES = PL_SELECT_BLOCK / 64, CELLS = IPT * WAVES;
  static_assert(CELLS <= PL_SELECT_BLOCK && IPT * PL_SELECT_BLOCK <= PL_SELECT_MAX_CAND, "one scan cell per thread");
  __shared__ unsigned hist[256 * PL_SELECT_COPIES];
  __shared__ unsigned total[256];
  __shared__ unsigned cell[2][PL_SELECT_BLOCK];                            // lower / equal keys per (round, wave), then before it
  __shared__ unsigned wave_total[2][WAVES];
  __shared__ unsigned pick[2];                                             // the chosen bin and the rank inside it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = src_index ? src_index[k] : k;
  float2 *orow = out + (size_t)k * out_row_points;
  int *irow = out_index ? out_index + (size_t)k * num_keep : nullptr;
  if (!((unsigned)plane < (unsigned)num_pred)) {                           // an index outside the planes: loud, and no access
    const float nan = __builtin_nanf("");
    for (int p = tid; p < num_keep; p += PL_SELECT_BLOCK) {
      orow[p] = make_float2(nan, nan);
      if (irow) irow[p] = -1;
    }
    return;
  }
  const float *pp = pred + (size_t)plane * H * W;
  const float2 *crow = cand + (size_t)k * S;

  for (int i = tid; i < 256 * PL_SELECT_COPIES; i += PL_SELECT_BLOCK) hist[i] = 0u;
  unsigned key[IPT];                                                       // 0xffffffff past S: above every key, in no later pass
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    key[i] = 0xffffffffu;
    if (tid < S - i * PL_SELECT_BLOCK) {
      const float2 c = (crow + i * PL_SELECT_BLOCK)[threadIdx.x];          // a uniform base and one 32-bit lane offset
      const unsigned bits = __float_as_uint(sample_plane(pp, make_taps(c.x, c.y, H, W), H, W)) & 0x7fffffffu;
      key[i] = bits > 0x7f800000u ? 0u : bits;
    }
  }
  __syncthreads();

  unsigned key_t = 0u, rank = (unsigned)num_keep;                          // rank counts from 1 among the keys that agree with key_t
#pragma unroll
  for (int shift = 24; shift >= 0; shift -= 8) {
    const unsigned above = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
#pragma unroll
    for (int i = 0; i < IPT; ++i)
      if (((key[i] ^ key_t) & above) == 0u)
        __hip_atomic_fetch_add(&hist[((key[i] >> shift) & 255u) * PL_SELECT_COPIES + (lane & 31)], 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    {
      const int bin = tid >> 2, quarter = tid & 3;
      unsigned a = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int at = bin * PL_SELECT_COPIES + quarter * 8 + ((j + bin) & 7);
        a += hist[at];
        hist[at] = 0u;
      }
      a += __shfl_xor(a, 1, 64);
      a += __shfl_xor(a, 2, 64);
      if (quarter == 0) total[bin] = a;
    }
    __syncthreads();
    if (wave == 0) {
      unsigned c[4], sum = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) sum += c[j] = total[4 * lane + j];
      unsigned incl = sum;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      unsigned before = incl - sum;
#pragma unroll
      for (int j = 0; j < 4; ++j) {                                        // one bin of one lane holds the rank: an empty one cannot
        if (before < rank && rank <= before + c[j]) {
          pick[0] = (unsigned)(4 * lane + j);
          pick[1] = rank - before;
        }
        before += c[j];
      }
    }
    __syncthreads();
    key_t |= pick[0] << shift;
    rank = pick[1];
  }

  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const unsigned long long lower = __ballot(key[i] < key_t), equal = __ballot(key[i] == key_t);
    if (lane == 0) {
      cell[0][i * WAVES + wave] = (unsigned)__popcll(lower);
      cell[1][i * WAVES + wave] = (unsigned)__popcll(equal);
    }
  }
  __syncthreads();
  {
    unsigned v[2], incl[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      incl[h] = v[h] = tid < CELLS ? cell[h][tid] : 0u;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl[h], d, 64);
        if (lane >= d) incl[h] += up;
      }
      if (lane == 63) wave_total[h][wave] = incl[h];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      unsigned before = incl[h] - v[h];
      for (int w = 0; w < wave; ++w) before += wave_total[h][w];
      if (tid < CELLS) cell[h][tid] = before;
    }
  }
  __syncthreads();
  // The compiler would otherwise keep IPT coordinate addresses and 2 IPT ballots of the loops above alive for the loop below
  // (common subexpressions: hundreds of registers, spilled); through these two it forms them again, a few instructions each.
  unsigned tid2 = threadIdx.x;
  asm volatile("" : "+v"(tid2), "+v"(key_t));
  constexpr int BATCH = 8;                                                 // coordinate pairs loaded together, then stored
  static_assert(IPT % BATCH == 0, "whole batches");
#pragma unroll
  for (int i0 = 0; i0 < IPT; i0 += BATCH) {
    float2 c[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) c[j] = crow[min((i0 + j) * PL_SELECT_BLOCK + (int)tid2, S - 1)];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = i0 + j;
      const bool is_lower = key[i] < key_t, is_equal = key[i] == key_t;
      const unsigned long long lower = __ballot(is_lower), equal = __ballot(is_equal);
      const unsigned lb = cell[0][i * WAVES + wave] + (unsigned)__popcll(lower & below);
      const unsigned eb = cell[1][i * WAVES + wave] + (unsigned)__popcll(equal & below);
      const unsigned at = lb + min(eb, rank);
      if ((is_lower || (is_equal && eb < rank)) && at < (unsigned)num_keep) {   // (at < num_keep always holds: the store's own guard)
        orow[at] = c[j];
        if (irow) irow[at] = i * PL_SELECT_BLOCK + (int)tid2;
      }
    }
  }
}

// grid (pair, head): src_index [heads, K], cand [heads, K, S], out [heads, K, out_row_points], out_index [heads, K, num_keep]
template <int IPT>
__global__ __launch_bounds__(PL_SELECT_BLOCK) void point_select_many_kernel(
    const HeadPlanes heads, const int *__restrict__ src_index, const int num_pred, const int H, const int W,
    const float2 *__restrict__ cand, const int K, const int S, const int num_keep, float2 *__restrict__ out,
    const int out_row_points, int *__restrict__ out_index)
{
  const size_t row0 = (size_t)blockIdx.y * K;
  point_select_body<IPT>(heads.p[blockIdx.y], src_index ? src_index + row0 : nullptr, num_pred, H, W, cand + row0 * S, S, num_keep,
                         out + row0 * out_row_points, out_row_points, out_index ? out_index + row0 * num_keep : nullptr,
                         blockIdx.x);
}

// Matcher cost matrices (pct_point_match_cost_f32): cost[b, q, g] of Point_HungarianMatcher._batched_costs from the planes, the
// point samples never in memory.  Three P-long contractions per (q, g) on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 sums):
//     ce  = sum_p softplus(-x) t + sum_p softplus(x) (1 - t)      (two non-negative products into ONE accumulator: nothing cancels)
//     st  = sum_p sigma(x) t
// plus the vectors sum_p sigma(x) per query and sum_p t per target.
//
// Workgroup (chunk of P, group of 128 queries x group of 64 targets, image), 4 waves, wave w the query tile 32 w .. 32 w + 31.
// The chunk is walked in passes of MC_SUB = 128 points:
//   1. every thread forms the taps of one point of the pass from the image's coordinate row, once for the prediction's geometry
//      (kept in LDS for pass 2) and once for the targets' (kept in registers), and samples its share of the group's target planes
//      into LDS as ts[point][target] (row stride 65 words: the writes, lanes along the points, and the reads, lanes along the
//      targets, both touch 32 different banks);
//   2. a wave's lane (i, kh) = (lane % 32, lane / 32) IS the A operand's element (row i, k = kh) of the matrix instruction: for step s
//      it samples query i at point 2 s + kh with the staged taps (make_taps / sample_plane: the gather's code and the gather's bits),
//      forms softplus(-x), softplus(x), sigma(x) from one e = exp(-|x|) and feeds them straight from registers; the B operand
//      (k = kh, column i) is ts[2 s + kh][i], and 1 - that.  No operand shuffle, no A tile in LDS.
// The accumulators (2 products x 2 target tiles x 16 registers) stay in registers over all passes of the chunk and go to the
// workspace once; sum sigma is a per-lane running sum (ascending points), sum t likewise from the B operands the lane reads anyway.
// Points past P: A operands and t are 0 (0 * (1 - 0) = 0).  Queries past Q: x = 0, nothing is read, the rows are not used.
// Targets past the image's count: t = 0, nothing is read; target tiles wholly past the count are skipped.
// match_cost_finish_kernel adds the chunks in ascending order and forms the cost; columns past the count are written as 0.
constexpr int MC_BLOCK = 256;
constexpr int MC_SUB = 128;                // points per pass
constexpr int MC_QGROUP = 128;             // queries per workgroup: 4 waves x 32
constexpr int MC_GTILES = 2;               // target tiles of 32 per workgroup
constexpr int MC_GGROUP = 32 * MC_GTILES;
constexpr int MC_TS = MC_GGROUP + 1;       // row stride of ts in words
constexpr int MC_MAX_CHUNKS = 32;          // of P: bounds the workspace
constexpr int MC_WANT_GROUPS = 512;        // workgroups the P split aims for (two per compute unit)

typedef float mc_f16 __attribute__((ext_vector_type(16)));

struct MatchCostPlan {
  int qgroups, ggroups, passes, chunks;    // passes of MC_SUB points per chunk
  long long per_chunk;                     // floats of one (image, chunk): 2 Qp Gp + Qp + Gp
};

__host__ __device__ inline MatchCostPlan match_cost_plan(const int B, const int Q, const int Gmax, const int P)
{
  MatchCostPlan m;
  m.qgroups = (Q + MC_QGROUP - 1) / MC_QGROUP;
  m.ggroups = (Gmax + MC_GGROUP - 1) / MC_GGROUP;
  const long long groups = (long long)B * m.qgroups * m.ggroups;
  const int subs = (P + MC_SUB - 1) / MC_SUB;
  long long want = (MC_WANT_GROUPS + groups - 1) / groups;
  if (want > MC_MAX_CHUNKS) want = MC_MAX_CHUNKS;
  if (want > subs) want = subs;
  if (want < 1) want = 1;
  m.passes = (int)((subs + want - 1) / want);
  m.chunks = (subs + m.passes - 1) / m.passes;                             // <= want
  const long long Qp = (long long)m.qgroups * MC_QGROUP, Gp = (long long)m.ggroups * MC_GGROUP;
  m.per_chunk = 2 * Qp * Gp + Qp + Gp;
  return m;
}

__device__ __forceinline__ void match_cost_partial_body(
    const float *__restrict__ pred, const float *__restrict__ tgt, const int *__restrict__ tgt_start,
    const int *__restrict__ tgt_count, const float2 *__restrict__ coords, const int Q, const int H, const int W, const int num_tgt,
    const int Ht, const int Wt, const int Gmax, const int P, const MatchCostPlan plan, float *__restrict__ ws, const int chunk,
    const unsigned group, const int b)
{
  __shared__ Taps taps[MC_SUB];
  __shared__ float ts[MC_SUB * MC_TS];
  const int qgrp = group / plan.ggroups, ggrp = group - qgrp * plan.ggroups;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, kh = lane >> 5;
  const int start = tgt_start[b];
  const int count = max(0, min(tgt_count[b], Gmax)) - ggrp * MC_GGROUP;    // targets of this group that the image has
  const int ntiles = max(0, min(MC_GTILES, (count + 31) / 32));
  const int q = qgrp * MC_QGROUP + wave * 32 + col;
  const bool q_ok = q < Q;
  const float *pp = pred + ((size_t)b * Q + (q_ok ? q : 0)) * H * W;
  const float2 *crow = coords + (size_t)b * P;

  mc_f16 acc_ce[MC_GTILES], acc_st[MC_GTILES];
  float tsum[MC_GTILES], ssig = 0.f;
#pragma unroll
  for (int gt = 0; gt < MC_GTILES; ++gt) {
    tsum[gt] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_ce[gt][r] = acc_st[gt][r] = 0.f;
  }

  for (int pass = 0; pass < plan.passes; ++pass) {
    const int p0 = (chunk * plan.passes + pass) * MC_SUB;
    if (p0 >= P) break;                                                     // (uniform)
    __syncthreads();                                                        // the previous pass has read taps and ts
    {
      const int pt = tid & (MC_SUB - 1), half = tid >> 7;
      const bool in = p0 + pt < P;
      const float2 c = in ? crow[p0 + pt] : make_float2(0.f, 0.f);
      if (half == 0) taps[pt] = make_taps(c.x, c.y, H, W);
      const Taps tt = make_taps(c.x, c.y, Ht, Wt);
      for (int j = half; j < ntiles * 32; j += MC_BLOCK / MC_SUB) {
        float v = 0.f;
        if (in && j < count) {
          const int plane = start + ggrp * MC_GGROUP + j;                   // outside the planes: loud, and no access
          v = (unsigned)plane < (unsigned)num_tgt ? sample_plane(tgt + (size_t)plane * Ht * Wt, tt, Ht, Wt) : __builtin_nanf("");
        }
        ts[pt * MC_TS + j] = v;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < MC_SUB / 2; ++s) {
      const int pt = 2 * s + kh;
      const Taps tp = taps[pt];
      const float x = q_ok ? sample_plane(pp, tp, H, W) : 0.f;
      const float e = expf(-fabsf(x));
      const float l = log1pf(e), r = 1.f / (1.f + e);
      const bool in = p0 + pt < P;
      const float pos = in ? fmaxf(-x, 0.f) + l : 0.f;                      // softplus(-x) = bce_with_logits(x, 1)
      const float neg = in ? fmaxf(x, 0.f) + l : 0.f;                       // softplus(x)  = bce_with_logits(x, 0)
      const float sg = in ? (x >= 0.f ? r : e * r) : 0.f;
      ssig += sg;
#pragma unroll
      for (int gt = 0; gt < MC_GTILES; ++gt) {
        if (gt < ntiles) {
          const float t = ts[pt * MC_TS + gt * 32 + col];
          tsum[gt] += t;
          acc_ce[gt] = __builtin_amdgcn_mfma_f32_32x32x2f32(pos, t, acc_ce[gt], 0, 0, 0);
          acc_ce[gt] = __builtin_amdgcn_mfma_f32_32x32x2f32(neg, 1.f - t, acc_ce[gt], 0, 0, 0);
          acc_st[gt] = __builtin_amdgcn_mfma_f32_32x32x2f32(sg, t, acc_st[gt], 0, 0, 0);
        }
      }
    }
  }

  // acc[r] = D[row 8 (r / 4) + 4 kh + r % 4][column col]: row = query of the wave's tile, column = target of the tile
  const long long Qp = (long long)plan.qgroups * MC_QGROUP, Gp = (long long)plan.ggroups * MC_GGROUP;
  float *wsb = ws + ((size_t)b * plan.chunks + chunk) * plan.per_chunk;
#pragma unroll
  for (int gt = 0; gt < MC_GTILES; ++gt) {
    if (gt < ntiles) {
      const long long g = (long long)ggrp * MC_GGROUP + gt * 32 + col;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long row = (long long)qgrp * MC_QGROUP + wave * 32 + 8 * (r / 4) + 4 * kh + r % 4;
        wsb[row * Gp + g] = acc_ce[gt][r];
        wsb[Qp * Gp + row * Gp + g] = acc_st[gt][r];
      }
      const float t2 = tsum[gt] + __shfl_xor(tsum[gt], 32, 64);             // even points + odd points
      if (qgrp == 0 && wave == 0 && kh == 0) wsb[2 * Qp * Gp + Qp + g] = t2;
    }
  }
  const float s2 = ssig + __shfl_xor(ssig, 32, 64);
  if (ggrp == 0 && kh == 0) wsb[2 * Qp * Gp + (long long)qgrp * MC_QGROUP + wave * 32 + col] = s2;
}

// The cost pass keeps single-head kernels of its own: a launch of one head of the *_many pair below measured 1.1 - 1.3 % slower
// than these (profiles/point_one_head.json).  The same bodies, so the same bits.
__global__ __launch_bounds__(MC_BLOCK, 2) void match_cost_partial_kernel(
    const float *__restrict__ pred, const float *__restrict__ tgt, const int *__restrict__ tgt_start,
    const int *__restrict__ tgt_count, const float2 *__restrict__ coords, const int Q, const int H, const int W, const int num_tgt,
    const int Ht, const int Wt, const int Gmax, const int P, const MatchCostPlan plan, float *__restrict__ ws)
{
  match_cost_partial_body(pred, tgt, tgt_start, tgt_count, coords, Q, H, W, num_tgt, Ht, Wt, Gmax, P, plan, ws, blockIdx.x,
                          blockIdx.y, blockIdx.z);
}

// grid z = head * B + image: coords [heads, B, P], one workspace of the single-head size per head; `plan` is the plan of B images
__global__ __launch_bounds__(MC_BLOCK, 2) void match_cost_partial_many_kernel(
    const HeadPlanes heads, const float *__restrict__ tgt, const int *__restrict__ tgt_start, const int *__restrict__ tgt_count,
    const float2 *__restrict__ coords, const int B, const int Q, const int H, const int W, const int num_tgt, const int Ht,
    const int Wt, const int Gmax, const int P, const MatchCostPlan plan, float *__restrict__ ws)
{
  const int head = blockIdx.z / (unsigned)B, b = blockIdx.z - head * B;
  match_cost_partial_body(heads.p[head], tgt, tgt_start, tgt_count, coords + (size_t)head * B * P, Q, H, W, num_tgt, Ht, Wt, Gmax, P,
                          plan, ws + (size_t)head * B * plan.chunks * plan.per_chunk, blockIdx.x, blockIdx.y, b);
}

__device__ __forceinline__ void match_cost_finish_body(const float *__restrict__ ws, const int *__restrict__ tgt_count, const int Q,
                                                       const int Gmax, const int P, const long long total,
                                                       const MatchCostPlan &plan, const float cost_mask, const float cost_dice,
                                                       float *__restrict__ cost)
{
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int g = (int)(i % Gmax);
  const long long bq = i / Gmax;
  const int q = (int)(bq % Q), b = (int)(bq / Q);
  float c = 0.f;
  if (g < tgt_count[b]) {
    const long long Qp = (long long)plan.qgroups * MC_QGROUP, Gp = (long long)plan.ggroups * MC_GGROUP;
    const float *w = ws + (size_t)b * plan.chunks * plan.per_chunk;
    float ce = 0.f, st = 0.f, sg = 0.f, t = 0.f;
    for (int k = 0; k < plan.chunks; ++k, w += plan.per_chunk) {
      ce += w[q * Gp + g];
      st += w[Qp * Gp + q * Gp + g];
      sg += w[2 * Qp * Gp + q];
      t += w[2 * Qp * Gp + Qp + g];
    }
    const float dice = 1.f - (2.f * st + 1.f) / (sg + t + 1.f);
    c = cost_mask * (ce / (float)P) + cost_dice * dice;
  }
  cost[i] = c;
}

__global__ __launch_bounds__(256) void match_cost_finish_kernel(const float *__restrict__ ws, const int *__restrict__ tgt_count,
                                                                const int Q, const int Gmax, const int P, const long long total,
                                                                const MatchCostPlan plan, const float cost_mask,
                                                                const float cost_dice, float *__restrict__ cost)
{
  match_cost_finish_body(ws, tgt_count, Q, Gmax, P, total, plan, cost_mask, cost_dice, cost);
}

// grid y = head: `total` elements of cost and one workspace of the single-head size per head
__global__ __launch_bounds__(256) void match_cost_finish_many_kernel(const float *__restrict__ ws, const int *__restrict__ tgt_count,
                                                                     const int B, const int Q, const int Gmax, const int P,
                                                                     const long long total, const MatchCostPlan plan,
                                                                     const float cost_mask, const float cost_dice,
                                                                     float *__restrict__ cost)
{
  match_cost_finish_body(ws + (size_t)blockIdx.y * B * plan.chunks * plan.per_chunk, tgt_count, Q, Gmax, P, total, plan, cost_mask,
                         cost_dice, cost + (size_t)blockIdx.y * total);
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

// the P split above bounds the grid's x; y and z hold the query / target groups and the images
int match_cost_geometry_status(int B, int Q, int H, int W, int Ht, int Wt, int Gmax, int P)
{
  if ((long long)H * W >= 0x7fffffffLL || (long long)Ht * Wt >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  if (B > 65535 || P > 0x40000000) return PCT_ERR_UNSUPPORTED;
  const long long qg = (Q + MC_QGROUP - 1) / MC_QGROUP, gg = (Gmax + MC_GGROUP - 1) / MC_GGROUP;
  if (qg * gg > 65535) return PCT_ERR_UNSUPPORTED;
  if ((long long)B * Q * Gmax >= 0x7fffffffLL * 256) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

}  // namespace

int launch_point_match_cost(const float *pred, int B, int Q, int H, int W, const float *tgt, int num_tgt, int Ht, int Wt,
                            const int *tgt_start, const int *tgt_count, int Gmax, const float *coords, int P, float cost_mask,
                            float cost_dice, void *workspace, float *cost, hipStream_t stream)
{
  if (const int rc = match_cost_geometry_status(B, Q, H, W, Ht, Wt, Gmax, P); rc != PCT_OK) return rc;
  const MatchCostPlan plan = match_cost_plan(B, Q, Gmax, P);
  float *ws = static_cast<float *>(workspace);
  match_cost_partial_kernel<<<dim3((unsigned)plan.chunks, (unsigned)(plan.qgroups * plan.ggroups), (unsigned)B), dim3(MC_BLOCK), 0,
                              stream>>>(pred, tgt, tgt_start, tgt_count, reinterpret_cast<const float2 *>(coords), Q, H, W, num_tgt,
                                        Ht, Wt, Gmax, P, plan, ws);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  const long long total = (long long)B * Q * Gmax;
  match_cost_finish_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(ws, tgt_count, Q, Gmax, P, total, plan,
                                                                                           cost_mask, cost_dice, cost);
  return (int)hipGetLastError();
}

int launch_point_sample(const float *planes, const int *plane_index, const float *coords, int num_planes, int H, int W, int K,
                        int P, int per_row, float *out, hipStream_t stream)
{
  if (const int rc = point_sample_geometry_status(H, W, K, P, PL_GATHER_BLOCK); rc != PCT_OK) return rc;
  const int chunks = (P + PL_GATHER_BLOCK - 1) / PL_GATHER_BLOCK;
  point_sample_kernel<<<dim3((unsigned)(K * chunks)), dim3(PL_GATHER_BLOCK), 0, stream>>>(
      planes, plane_index, reinterpret_cast<const float2 *>(coords), num_planes, H, W, P, chunks, per_row, out);
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

// ---- the launches with a head dimension: the C ABI has checked 0 < num_heads <= PL_MAX_HEADS and the entries
static HeadPlanes head_planes(const float *const *preds, int num_heads)
{
  HeadPlanes hp;
  for (int h = 0; h < PL_MAX_HEADS; ++h) hp.p[h] = h < num_heads ? preds[h] : nullptr;
  return hp;
}

int launch_point_select_many(const float *const *preds, int num_heads, const int *src_index, int num_pred, int H, int W,
                             const float *cand_coords, int K, int S, int num_keep, float *out_coords, int out_row_points,
                             int *out_index, hipStream_t stream)
{
  if ((long long)H * W >= 0x7fffffffLL || S > PL_SELECT_MAX_CAND) return PCT_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)K, (unsigned)num_heads), block(PL_SELECT_BLOCK);
  const HeadPlanes hp = head_planes(preds, num_heads);
  const float2 *cand = reinterpret_cast<const float2 *>(cand_coords);
  float2 *out = reinterpret_cast<float2 *>(out_coords);
  if (S <= 16 * PL_SELECT_BLOCK)
    point_select_many_kernel<16><<<grid, block, 0, stream>>>(hp, src_index, num_pred, H, W, cand, K, S, num_keep, out, out_row_points, out_index);
  else if (S <= 40 * PL_SELECT_BLOCK)
    point_select_many_kernel<40><<<grid, block, 0, stream>>>(hp, src_index, num_pred, H, W, cand, K, S, num_keep, out, out_row_points, out_index);
  else
    point_select_many_kernel<64><<<grid, block, 0, stream>>>(hp, src_index, num_pred, H, W, cand, K, S, num_keep, out, out_row_points, out_index);
  return (int)hipGetLastError();
}

int launch_point_loss_forward_many(const float *const *preds, int num_heads, const int *src_index, int num_pred, int H, int W,
                                   const float *tgt, const int *tgt_index, int num_tgt, int Ht, int Wt, const float *coords, int K,
                                   int P, float *x, float *t, float *sums, hipStream_t stream)
{
  if (const int rc = point_loss_geometry_status(H, W, Ht, Wt, K); rc != PCT_OK) return rc;
  point_loss_forward_many_kernel<<<dim3((unsigned)K, (unsigned)num_heads), dim3(PL_FWD_BLOCK), 0, stream>>>(
      head_planes(preds, num_heads), src_index, num_pred, H, W, tgt, tgt_index, num_tgt, Ht, Wt,
      reinterpret_cast<const float2 *>(coords), K, P, x, t, sums);
  return (int)hipGetLastError();
}

int launch_point_match_cost_many(const float *const *preds, int num_heads, int B, int Q, int H, int W, const float *tgt, int num_tgt,
                                 int Ht, int Wt, const int *tgt_start, const int *tgt_count, int Gmax, const float *coords, int P,
                                 float cost_mask, float cost_dice, void *workspace, float *cost, hipStream_t stream)
{
  if (const int rc = match_cost_geometry_status(B, Q, H, W, Ht, Wt, Gmax, P); rc != PCT_OK) return rc;
  if ((long long)num_heads * B > 65535) return PCT_ERR_UNSUPPORTED;         // the grid's z holds (head, image)
  const MatchCostPlan plan = match_cost_plan(B, Q, Gmax, P);                // of ONE head: no sum's order depends on num_heads
  float *ws = static_cast<float *>(workspace);
  match_cost_partial_many_kernel<<<dim3((unsigned)plan.chunks, (unsigned)(plan.qgroups * plan.ggroups), (unsigned)(num_heads * B)),
                                   dim3(MC_BLOCK), 0, stream>>>(head_planes(preds, num_heads), tgt, tgt_start, tgt_count,
                                                                reinterpret_cast<const float2 *>(coords), B, Q, H, W, num_tgt, Ht,
                                                                Wt, Gmax, P, plan, ws);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  const long long total = (long long)B * Q * Gmax;
  match_cost_finish_many_kernel<<<dim3((unsigned)((total + 255) / 256), (unsigned)num_heads), dim3(256), 0, stream>>>(
      ws, tgt_count, B, Q, Gmax, P, total, plan, cost_mask, cost_dice, cost);
  return (int)hipGetLastError();
}

}  // namespace pct
