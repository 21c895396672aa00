// Mask side of the query-contrast ("re-id") loss on the device (include/pctrans_hip_reid.h: pct_reid_dice_rows_forward_f32,
// pct_reid_dice_rows_backward_f32): the rows of dice_for (pctrans_amd/transformer_decoder/query_contrast.py) that
// select_pos_neg_mask keeps, and their backward, without the [N, Q, P] sigmoid tensor, the [N, Q, Q] Gram matrix and the
// batched GEMMs of autograd.  x = sigmoid(z) is recomputed wherever it is needed; fp32 throughout.
//
// Forward, three launches on one stream, nothing allocated, no host synchronisation, no floating-point atomic:
//   reid_fwd_kernel        one (chunk of pixels, group of 128 queries, image): [rows + 1] x [128] sums over the chunk's pixels on
//                          v_mfma_f32_32x32x2_f32 -- A = the sigmoid rows of the image's keys and one row of ones (its products
//                          are exact: that row is s), B = the sigmoid rows of the group's queries -- into the workspace
//   reid_fwd_sums_kernel   s[n, q]: the chunks added in ascending order
//   reid_fwd_dice_kernel   num[i, q]: the chunks added in ascending order; D = (2 num + 1) / (s_k + s_q + 1); the status word
// An accumulator is bit for bit an fmaf chain over its chunk's pixels in ascending order (RD_FWD_PIX pixels per pass, `passes`
// passes per chunk), so an output passes through at most passes * RD_FWD_PIX + chunks additions.
//
// Backward, three launches, with a = 2 G / den, b = -G D / den, den = s_k + s_q + 1:
//   reid_bwd_rows_kernel   one row i: a[i, :] (and its transpose), b[i, :], and sum_q b[i, q] in a fixed order
//   reid_bwd_const_kernel  c[n, q] = sum_{i of n} b[i, q] + sum_{i of n: k_i = q} sum_q' b[i, q'], rows in ascending order
//   reid_bwd_kernel        one (32 pixels, image): the sigmoid of all Q rows of those pixels in LDS, then per group of 64 rows
//                            acc[q, p] += sum_i a[i, q] x[k_i, p]                   ([Q x rows] . [rows x 32])
//                          and then per group of 64 rows
//                            y[i, p] = sum_q' a[i, q'] x[q', p]                     ([rows x Q] . [Q x 32], into LDS; two halves of
//                                                                                    the queries by two waves, added in order)
//                            acc[q, p] += sum_i (k_i == q) y[i, p]                  (a 0 / 1 operand: exact products, fixed order)
//                          and dz = (acc + c) x (1 - x).  An image without rows gets zeros.
// Every sum has one order that depends on the shapes alone: two calls on the same operands give the same bits.
//
// A key outside [0, Q) (and a row past the Q-th of its image) reads nothing: its operands are zeros, its row of D is 0, it adds
// nothing to any gradient, and the status word counts it.  image_start is clamped to [0, num_rows] before it indexes anything
// (row_ranges.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.hpp"
#include "msda_win_common.hpp"    // func_attr_per_device
#include "row_ranges.hpp"         // image_rows, row_image: the clamping rules, shared with reid_query.hip
#include "wave_reduce.hpp"

namespace pct {

namespace {

constexpr int RD_MAX_Q = 1024;            // the assignment kernel's query limit; rows per image <= Q
constexpr int RD_MAX_CHUNKS = 128;        // of the pixels of an image: bounds the workspace
constexpr int RD_FWD_PIX = 64;            // pixels of one forward pass
constexpr int RD_FWD_XS = RD_FWD_PIX + 1; // row stride of the forward's LDS tiles in words (odd: 32 rows on 32 banks)
constexpr int RD_FWD_COLS = 128;          // queries of one workgroup: 4 waves x 32
constexpr int RD_FWD_ROWS = 96;           // key rows (+ the row of ones) of one sweep over the chunk: 3 tiles of 32
constexpr int RD_BWD_PIX = 32;            // pixels of one backward workgroup
constexpr int RD_BWD_XS = RD_BWD_PIX + 1;
constexpr int RD_BWD_ROWS = 64;           // rows of one group of the backward
constexpr int RD_BWD_AHEAD = 8;           // operand loads from a / aT issued together, ahead of their MFMAs
constexpr int RD_BWD_PARTS = 2;           // y of a row is summed over the queries in two halves, by two waves
constexpr int RD_BWD_MAX_LDS = ((RD_MAX_Q + RD_BWD_PARTS * RD_BWD_ROWS) * RD_BWD_XS + RD_BWD_ROWS) * 4;   // 152 320 bytes of the CU's 160 KiB

typedef float rd_f16 __attribute__((ext_vector_type(16)));

// e = exp(-|z|) never overflows.  expf and the division are the compiler's accurate ones (no fast-math)
__device__ __forceinline__ float rd_sigmoid(const float z)
{
  const float e = expf(-fabsf(z));
  const float r = 1.f / (1.f + e);
  return z >= 0.f ? r : e * r;
}

__global__ __launch_bounds__(256) void reid_fwd_kernel(const float *__restrict__ z, const int *__restrict__ image_start,
                                                       const int *__restrict__ key, const int Q, const int P, const int I,
                                                       const int N, const ChunkPlan plan, float *__restrict__ ws)
{
  __shared__ float xs[RD_FWD_COLS * RD_FWD_XS];
  __shared__ float ks[RD_FWD_ROWS * RD_FWD_XS];
  __shared__ int krow[RD_FWD_ROWS];         // key of row r of the sweep; -1: the row of ones; -2: a row of zeros
  const int chunk = blockIdx.x, n = blockIdx.z, q0 = blockIdx.y * RD_FWD_COLS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, kh = lane >> 5;
  int first, rows;
  image_rows(image_start, n, I, Q, first, rows);
  const int total = rows + 1;               // the keys' rows, then the row of ones
  const float *zb = z + (size_t)n * Q * P;
  const int wq0 = q0 + wave * 32;
  const bool wave_live = wq0 < Q;           // (uniform in the wave)

  for (int g0 = 0; g0 < total; g0 += RD_FWD_ROWS) {
    const int gr = min(RD_FWD_ROWS, total - g0), tiles = (gr + 31) >> 5;
    __syncthreads();                        // the previous sweep has read krow
    if (tid < RD_FWD_ROWS) {
      const int idx = g0 + tid;
      int k = -2;
      if (idx < rows) {
        k = key[first + idx];
        if ((unsigned)k >= (unsigned)Q) k = -2;
      } else if (idx == rows) {
        k = -1;
      }
      krow[tid] = k;
    }
    rd_f16 acc[RD_FWD_ROWS / 32];
#pragma unroll
    for (int t = 0; t < RD_FWD_ROWS / 32; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int pass = 0; pass < plan.passes; ++pass) {
      const long long p0 = ((long long)chunk * plan.passes + pass) * RD_FWD_PIX;
      if (p0 >= P) break;                   // (uniform)
      __syncthreads();                      // krow is written; the previous pass has read xs and ks
      // every load is unconditional (row and pixel clamped into the image, the value dropped afterwards), so that the loads of
      // several rows are in flight together
      const int pix = tid % RD_FWD_PIX, r0 = tid / RD_FWD_PIX;
      const bool pix_ok = p0 + pix < P;
      const size_t pc = (size_t)(pix_ok ? p0 + pix : P - 1);
#pragma unroll 8
      for (int r = r0; r < RD_FWD_COLS; r += 256 / RD_FWD_PIX) {
        const int q = q0 + r;
        const float v = zb[(size_t)min(q, Q - 1) * P + pc];
        xs[r * RD_FWD_XS + pix] = (q < Q && pix_ok) ? rd_sigmoid(v) : 0.f;
      }
#pragma unroll 8
      for (int r = r0; r < tiles * 32; r += 256 / RD_FWD_PIX) {
        const int k = krow[r];
        const float v = zb[(size_t)max(k, 0) * P + pc];
        ks[r * RD_FWD_XS + pix] = !pix_ok ? 0.f : (k >= 0 ? rd_sigmoid(v) : (k == -1 ? 1.f : 0.f));
      }
      __syncthreads();
      if (wave_live) {
#pragma unroll 4
        for (int s = 0; s < RD_FWD_PIX / 2; ++s) {
          const int px = 2 * s + kh;
          const float b = xs[(wave * 32 + col) * RD_FWD_XS + px];
#pragma unroll
          for (int t = 0; t < RD_FWD_ROWS / 32; ++t)
            if (t < tiles) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[(t * 32 + col) * RD_FWD_XS + px], b, acc[t], 0, 0, 0);
        }
      }
    }

    // acc[t][r] = sum[row 32 t + 8 (r / 4) + 4 kh + r % 4 of the sweep][query wq0 + col]
    if (wave_live && wq0 + col < Q) {
#pragma unroll
      for (int t = 0; t < RD_FWD_ROWS / 32; ++t) {
        if (t >= tiles) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int idx = g0 + t * 32 + 8 * (r / 4) + 4 * kh + r % 4;
          if (idx > rows) continue;
          const size_t row = idx < rows ? (size_t)(first + idx) : (size_t)I + n;
          ws[((size_t)chunk * ((size_t)I + N) + row) * Q + wq0 + col] = acc[t][r];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void reid_fwd_sums_kernel(const float *__restrict__ ws, const int Q, const int I, const int N,
                                                            const int chunks, float *__restrict__ s)
{
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * Q) return;
  const int n = (int)(idx / Q), q = (int)(idx % Q);
  float sum = 0.f;
  for (int c = 0; c < chunks; ++c) sum += ws[((size_t)c * ((size_t)I + N) + (size_t)I + n) * Q + q];
  s[idx] = sum;
}

__global__ __launch_bounds__(256) void reid_fwd_dice_kernel(const float *__restrict__ ws, const float *__restrict__ s,
                                                            const int *__restrict__ image_start, const int *__restrict__ key,
                                                            const int Q, const int I, const int N, const int chunks,
                                                            const int qblocks, float *__restrict__ D, int *__restrict__ status)
{
  __shared__ int bad_rows;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {                                                    // the status word: an integer sum
    if (tid == 0) bad_rows = 0;
    __syncthreads();
    int bad = 0;
    for (int r = tid; r < I; r += 256) bad += row_image(image_start, key, N, I, Q, r) < 0 ? 1 : 0;
    if (bad) atomicAdd(&bad_rows, bad);
    __syncthreads();
    if (tid == 0) *status = bad_rows;
  }
  const int i = blockIdx.x / qblocks, q = (blockIdx.x % qblocks) * 256 + tid;
  if (q >= Q) return;
  const int n = row_image(image_start, key, N, I, Q, i);
  float d = 0.f;
  if (n >= 0) {
    float num = 0.f;
    for (int c = 0; c < chunks; ++c) num += ws[((size_t)c * ((size_t)I + N) + i) * Q + q];
    d = (2.f * num + 1.f) / (s[(size_t)n * Q + key[i]] + s[(size_t)n * Q + q] + 1.f);
  }
  D[(size_t)i * Q + q] = d;
}

__global__ __launch_bounds__(256) void reid_bwd_rows_kernel(const float *__restrict__ G, const float *__restrict__ D,
                                                            const float *__restrict__ s, const int *__restrict__ image_start,
                                                            const int *__restrict__ key, const int Q, const int I, const int N,
                                                            float *__restrict__ a, float *__restrict__ aT, float *__restrict__ b,
                                                            float *__restrict__ rowsum)
{
  __shared__ float part[4];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = row_image(image_start, key, N, I, Q, i);
  const float sk = n >= 0 ? s[(size_t)n * Q + key[i]] : 0.f;
  float sum = 0.f;
  for (int q = tid; q < Q; q += 256) {
    float av = 0.f, bv = 0.f;
    if (n >= 0) {
      const float den = sk + s[(size_t)n * Q + q] + 1.f, g = G[(size_t)i * Q + q];
      av = 2.f * g / den;
      bv = -g * D[(size_t)i * Q + q] / den;
    }
    a[(size_t)i * Q + q] = av;
    aT[(size_t)q * I + i] = av;
    b[(size_t)i * Q + q] = bv;
    sum += bv;
  }
  sum = wave_sum(sum);
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  if (tid == 0) rowsum[i] = ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(256) void reid_bwd_const_kernel(const float *__restrict__ b, const float *__restrict__ rowsum,
                                                             const int *__restrict__ image_start, const int *__restrict__ key,
                                                             const int Q, const int I, const int N, float *__restrict__ c)
{
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * Q) return;
  const int n = (int)(idx / Q), q = (int)(idx % Q);
  int first, rows;
  image_rows(image_start, n, I, Q, first, rows);
  float c1 = 0.f, c2 = 0.f;
  for (int r = 0; r < rows; ++r) {
    const int i = first + r;
    c1 += b[(size_t)i * Q + q];
    if (key[i] == q) c2 += rowsum[i];
  }
  c[idx] = c1 + c2;
}

// TILES: query tiles of 32 a wave owns (tile wave + 4 t): 4 covers Q <= 512 in half the registers, 8 covers RD_MAX_Q
template <int TILES>
__global__ __launch_bounds__(256) void reid_bwd_kernel(const float *__restrict__ z, const int *__restrict__ image_start,
                                                       const int *__restrict__ key, const float *__restrict__ a,
                                                       const float *__restrict__ aT, const float *__restrict__ c, const int Q,
                                                       const int P, const int I, float *__restrict__ dz)
{
  extern __shared__ __attribute__((aligned(16))) float rd_smem[];
  float *xs = rd_smem;                                   // [Q][RD_BWD_XS]: sigmoid of every query at this workgroup's pixels
  float *ys = xs + (size_t)Q * RD_BWD_XS;                // [RD_BWD_PARTS][RD_BWD_ROWS][RD_BWD_XS]: y of the group's rows, by halves
  int *kr = reinterpret_cast<int *>(ys + RD_BWD_PARTS * RD_BWD_ROWS * RD_BWD_XS);   // [RD_BWD_ROWS]: the group's keys, -1 = none
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, kh = lane >> 5;
  const long long p0 = (long long)blockIdx.x * RD_BWD_PIX;
  int first, rows;
  image_rows(image_start, n, I, Q, first, rows);
  const float *zb = z + (size_t)n * Q * P;
  float *dzb = dz + (size_t)n * Q * P;

  if (rows == 0) {                                       // (uniform) an image without rows: exact zeros
    for (int e = tid; e < Q * RD_BWD_PIX; e += 256) {
      const long long p = p0 + (e & 31);
      if (p < P) dzb[(size_t)(e >> 5) * P + p] = 0.f;
    }
    return;
  }
  {                                                      // unconditional loads (the pixel clamped into the image): many in flight
    const int pix = tid & 31;
    const bool pix_ok = p0 + pix < P;
    const size_t pc = (size_t)(pix_ok ? p0 + pix : P - 1);
#pragma unroll 8
    for (int q = tid >> 5; q < Q; q += 8) {
      const float v = zb[(size_t)q * P + pc];
      xs[q * RD_BWD_XS + pix] = pix_ok ? rd_sigmoid(v) : 0.f;
    }
  }

  const int qtiles = (Q + 31) >> 5;
  rd_f16 acc[TILES];                              // query tile wave + 4 t
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // First every a[i, q] x[k_i, p] in ascending row order, then every y in ascending row order: a row that counts for nothing adds
  // exact zeros wherever it stands, so the sums do not depend on the rows that do not count.
  for (int g0 = 0; g0 < rows; g0 += RD_BWD_ROWS) {
    const int gr = min(RD_BWD_ROWS, rows - g0);
    __syncthreads();                                     // xs is staged; the previous group has read kr
    if (tid < RD_BWD_ROWS) {
      int k = -1;
      if (tid < gr) {
        k = key[first + g0 + tid];
        if ((unsigned)k >= (unsigned)Q) k = -1;
      }
      kr[tid] = k;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      if (wave + 4 * t >= qtiles) continue;              // (uniform in the wave)
      const int qa = (wave + 4 * t) * 32 + col;
      const float *ap = a + ((size_t)first + g0) * Q + min(qa, Q - 1);   // the loads are unconditional: several in flight
      const int steps = (gr + 1) / 2;
      for (int s4 = 0; s4 < steps; s4 += RD_BWD_AHEAD) {
        float al[RD_BWD_AHEAD];
#pragma unroll
        for (int j = 0; j < RD_BWD_AHEAD; ++j) al[j] = ap[(size_t)min(2 * (s4 + j) + kh, gr - 1) * Q];
#pragma unroll
        for (int j = 0; j < RD_BWD_AHEAD; ++j) {
          if (s4 + j >= steps) break;                    // (uniform)
          const int il = 2 * (s4 + j) + kh;
          const bool live = il < gr;
          const int k = live ? kr[il] : -1;
          const float av = (live && qa < Q) ? al[j] : 0.f;
          const float bv = k >= 0 ? xs[k * RD_BWD_XS + col] : 0.f;
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
      }
    }
  }
  for (int g0 = 0; g0 < rows; g0 += RD_BWD_ROWS) {
    const int gr = min(RD_BWD_ROWS, rows - g0), rtiles = (gr + 31) >> 5;
    __syncthreads();                                     // the previous group has read ys and kr
    if (tid < RD_BWD_ROWS) {
      int k = -1;
      if (tid < gr) {
        k = key[first + g0 + tid];
        if ((unsigned)k >= (unsigned)Q) k = -1;
      }
      kr[tid] = k;
    }
    // y of row tile wave % 2 over half wave / 2 of the queries: [32 x Q / 2] . [Q / 2 x 32].  The halves are the same whatever
    // the rows are; they are added in order where y is read
    if ((wave & 1) < rtiles) {                           // (uniform in the wave)
      const int rt = wave & 1, part = wave >> 1;
      const int steps = (Q + 1) / 2, half = (steps + RD_BWD_PARTS - 1) / RD_BWD_PARTS;
      const int s0 = part * half, s1 = min(steps, s0 + half);
      rd_f16 y;
#pragma unroll
      for (int r = 0; r < 16; ++r) y[r] = 0.f;
      const bool row_ok = rt * 32 + col < gr;
      const float *atp = aT + (size_t)first + g0 + (row_ok ? rt * 32 + col : 0);   // unconditional loads: several in flight
      for (int s4 = s0; s4 < s1; s4 += RD_BWD_AHEAD) {
        float al[RD_BWD_AHEAD];
#pragma unroll
        for (int j = 0; j < RD_BWD_AHEAD; ++j) al[j] = atp[(size_t)min(2 * (s4 + j) + kh, Q - 1) * I];
#pragma unroll
        for (int j = 0; j < RD_BWD_AHEAD; ++j) {
          if (s4 + j >= s1) break;                       // (uniform)
          const int qq = 2 * (s4 + j) + kh;
          const float av = (row_ok && qq < Q) ? al[j] : 0.f;
          const float bv = qq < Q ? xs[qq * RD_BWD_XS + col] : 0.f;
          y = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, y, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ys[(part * RD_BWD_ROWS + rt * 32 + 8 * (r / 4) + 4 * kh + r % 4) * RD_BWD_XS + col] = y[r];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      if (wave + 4 * t >= qtiles) continue;              // (uniform in the wave)
      const int qa = (wave + 4 * t) * 32 + col;
      for (int s = 0; s < (gr + 1) / 2; ++s) {
        const int il = 2 * s + kh;
        const bool live = il < gr;
        const bool hit = live && kr[il] == qa;           // row il's key is this lane's query: its y joins that query's sum
        if (__any(hit)) {                                // (uniform in the wave)
          const float yv = live ? ys[il * RD_BWD_XS + col] + ys[(RD_BWD_ROWS + il) * RD_BWD_XS + col] : 0.f;
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(hit ? 1.f : 0.f, yv, acc[t], 0, 0, 0);
        }
      }
    }
  }

  // acc[t][r] = dL/dx[query 32 (wave + 4 t) + 8 (r / 4) + 4 kh + r % 4][pixel p0 + col] without its constant
  const long long p = p0 + col;
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    if (wave + 4 * t >= qtiles) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = (wave + 4 * t) * 32 + 8 * (r / 4) + 4 * kh + r % 4;
      if (q < Q && p < P) {
        const float x = xs[q * RD_BWD_XS + col];
        dzb[(size_t)q * P + p] = (acc[t][r] + c[(size_t)blockIdx.y * Q + q]) * (x * (1.f - x));
      }
    }
  }
}

inline int reid_dice_geometry_status(int N, int Q, int h, int w, int I)
{
  if (Q > RD_MAX_Q || N > 65535 || (long long)h * w >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  if ((long long)I > (long long)N * Q) return PCT_ERR_UNSUPPORTED;          // more than Q rows in some image
  return PCT_OK;
}

}  // namespace

int launch_reid_dice_forward(const float *logits, const int *image_start, const int *key, int N, int Q, int h, int w, int I,
                             void *workspace, float *sums, float *dice, int *status, hipStream_t stream)
{
  if (const int rc = reid_dice_geometry_status(N, Q, h, w, I); rc != PCT_OK) return rc;
  const int P = h * w;
  const ChunkPlan plan = chunk_plan(P, RD_FWD_PIX, RD_MAX_CHUNKS);          // passes of RD_FWD_PIX pixels per chunk; chunks of an image
  float *ws = static_cast<float *>(workspace);
  const int qgroups = (Q + RD_FWD_COLS - 1) / RD_FWD_COLS, qblocks = (Q + 255) / 256;
  reid_fwd_kernel<<<dim3((unsigned)plan.chunks, (unsigned)qgroups, (unsigned)N), dim3(256), 0, stream>>>(logits, image_start, key, Q,
                                                                                                      P, I, N, plan, ws);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  reid_fwd_sums_kernel<<<dim3((unsigned)(((long long)N * Q + 255) / 256)), dim3(256), 0, stream>>>(ws, Q, I, N, plan.chunks, sums);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  reid_fwd_dice_kernel<<<dim3((unsigned)((long long)I * qblocks)), dim3(256), 0, stream>>>(ws, sums, image_start, key, Q, I, N,
                                                                                          plan.chunks, qblocks, dice, status);
  return (int)hipGetLastError();
}

int launch_reid_dice_backward(const float *logits, const int *image_start, const int *key, const float *dice, const float *sums,
                              const float *grad_dice, int N, int Q, int h, int w, int I, void *workspace, float *grad_logits,
                              hipStream_t stream)
{
  if (const int rc = reid_dice_geometry_status(N, Q, h, w, I); rc != PCT_OK) return rc;
  const int P = h * w;
  const size_t IQ = (size_t)I * Q;
  float *a = static_cast<float *>(workspace), *aT = a + IQ, *b = aT + IQ, *rowsum = b + IQ, *c = rowsum + I;
  if (I > 0) {
    reid_bwd_rows_kernel<<<dim3((unsigned)I), dim3(256), 0, stream>>>(grad_dice, dice, sums, image_start, key, Q, I, N, a, aT, b,
                                                                     rowsum);
    if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
    reid_bwd_const_kernel<<<dim3((unsigned)(((long long)N * Q + 255) / 256)), dim3(256), 0, stream>>>(b, rowsum, image_start, key, Q,
                                                                                                     I, N, c);
    if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  }
  const int lds = ((Q + RD_BWD_PARTS * RD_BWD_ROWS) * RD_BWD_XS + RD_BWD_ROWS) * 4;
  const dim3 grid((unsigned)(((long long)P + RD_BWD_PIX - 1) / RD_BWD_PIX), (unsigned)N);
  if (Q <= 512) {                                                           // 85 KB of LDS at most
    if (lds > 64 * 1024 && func_attr_per_device(reinterpret_cast<const void *>(&reid_bwd_kernel<4>), RD_BWD_MAX_LDS) != hipSuccess)
      return PCT_ERR_UNSUPPORTED;
    reid_bwd_kernel<4><<<grid, dim3(256), (size_t)lds, stream>>>(logits, image_start, key, a, aT, c, Q, P, I, grad_logits);
  } else {
    if (func_attr_per_device(reinterpret_cast<const void *>(&reid_bwd_kernel<8>), RD_BWD_MAX_LDS) != hipSuccess)
      return PCT_ERR_UNSUPPORTED;
    reid_bwd_kernel<8><<<grid, dim3(256), (size_t)lds, stream>>>(logits, image_start, key, a, aT, c, Q, P, I, grad_logits);
  }
  return (int)hipGetLastError();
}

}  // namespace pct
