// Query side of the query-contrast ("re-id") loss on the device (include/pctrans_hip_reid_query.h): the nearest matched query of
// every query (what query_contrast._plan keeps of the [N, Q, Q] cosine table), the rows of the per-image Gram matrix X X^T that
// select_pos_neg_query keeps with their cosines and their backward, and the per-item reduction of SetCriterion.loss_reid_query /
// loss_reid_mask with its coefficients.  fp32 throughout, on the VALU: the work is a few MFLOP on rows that stay in L2, so the
// kernels are shaped for few launches and coalesced 16-byte row loads, not for the matrix cores.
//
// A row of X ([Q, N, C]: row (q, n) at (q N + n) C) lives in the registers of ONE wave: lane l holds the float4s l and l + 64 of
// the row (C <= 512).  A dot product of two rows is, in every kernel here, wave_sum(rq_lane_dot(a, b)): per lane an fmaf chain
// over its (at most 8) channels in ascending order, then a 6-step xor butterfly (wave_reduce.hpp).  It passes through at most
// RQ_LANE_CHANNELS + RQ_WAVE_STEPS = 14 additions, and equal operand rows give equal bits whichever kernel or wave computes them
// (the norms of the forward, of the nearest-positive table and of the keys are the same expression).
//
//   rq_nearest_kernel      one wave per (query, image): cosine to every matched query of the image in list order, first maximum
//   rq_rows_fwd_kernel     one wave per (query, image): its norm, and S, Cs against the key row of every item of the image
//   rq_bwd_coef_kernel     one workgroup per item: a[i, :], b[i, :] and sum_q b[i, q] (per thread ascending, butterfly, 4 partials)
//   rq_bwd_key_kernel      one workgroup per item: y[i, :] = sum_q' a[i, q'] x[n, q', :], the queries in `parts` contiguous ranges
//                          (ascending inside a range, the ranges added in ascending order)
//   rq_bwd_kernel          one wave per (query, image): sum_i a[i, q] x[k_i] (items ascending), + y[i] for the items whose key is q
//                          (ascending), + ((sum_i b[i, q]) + (sum_{i: k_i = q} rowsum_i)) / m_q^2 x[q] unless m_q was clamped
//   rq_contrast_kernel     one workgroup per item: two max-subtracted sums in LDS, the loss and its coefficients in one launch
// No floating-point atomic, every sum in one order that depends on the shapes alone: two calls give the same bits.
//
// A key outside [0, Q) reads nothing: its rows of S and Cs are 0 and it adds nothing to any gradient.  image_start is clamped to
// [0, num_rows] before it indexes anything (row_ranges.hpp, shared with reid_dice.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.hpp"
#include "row_ranges.hpp"     // image_rows, row_image: the clamping rules, shared with reid_dice.hip
#include "wave_reduce.hpp"    // wave_sum, wave_max: every lane ends with the same bits

namespace pct {

namespace {

constexpr int RQ_MAX_Q = 1024;            // queries of an image; rows per image <= Q
constexpr int RQ_MAX_C = 512;             // channels: 64 lanes x RQ_ROW_VECS float4
constexpr int RQ_ROW_VECS = 2;            // float4s of a row one lane holds
constexpr int RQ_LANE_CHANNELS = 8;       // fmaf chain of one lane's part of a dot product
constexpr int RQ_WAVE_STEPS = 6;          // additions of the butterfly over 64 lanes
constexpr int RQ_WAVES = 4;               // rows of one workgroup of the row kernels
constexpr int RQ_ITEM_SLOTS = RQ_MAX_Q / 256;   // scores one thread of rq_contrast_kernel holds

static_assert(RQ_ROW_VECS * 4 == RQ_LANE_CHANNELS && RQ_MAX_C == 64 * RQ_LANE_CHANNELS && (1 << RQ_WAVE_STEPS) == 64,
              "a row is one wave's registers");

struct RqRow {
  float4 v[RQ_ROW_VECS];
};

__device__ __forceinline__ RqRow rq_load_row(const float *__restrict__ row, const int C4, const int lane)
{
  RqRow r;
#pragma unroll
  for (int j = 0; j < RQ_ROW_VECS; ++j) {
    const int idx = lane + 64 * j;
    r.v[j] = idx < C4 ? reinterpret_cast<const float4 *>(row)[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  return r;
}

__device__ __forceinline__ float rq_lane_dot(const RqRow &a, const RqRow &b)
{
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < RQ_ROW_VECS; ++j) {
    s = fmaf(a.v[j].x, b.v[j].x, s);
    s = fmaf(a.v[j].y, b.v[j].y, s);
    s = fmaf(a.v[j].z, b.v[j].z, s);
    s = fmaf(a.v[j].w, b.v[j].w, s);
  }
  return s;
}

__device__ __forceinline__ void rq_axpy(RqRow &acc, const float a, const RqRow &x)
{
#pragma unroll
  for (int j = 0; j < RQ_ROW_VECS; ++j) {
    acc.v[j].x = fmaf(a, x.v[j].x, acc.v[j].x);
    acc.v[j].y = fmaf(a, x.v[j].y, acc.v[j].y);
    acc.v[j].z = fmaf(a, x.v[j].z, acc.v[j].z);
    acc.v[j].w = fmaf(a, x.v[j].w, acc.v[j].w);
  }
}

__global__ __launch_bounds__(256) void rq_nearest_kernel(const float *__restrict__ x, const int *__restrict__ pos, const int Q,
                                                         const int N, const int C, const int Pmax, int *__restrict__ nearest)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * RQ_WAVES + wave, n = blockIdx.y;
  if (q >= Q) return;                                                       // (uniform in the wave; the kernel has no barrier)
  const int C4 = C >> 2;
  const RqRow xr = rq_load_row(x + ((size_t)q * N + n) * C, C4, lane);
  const float nr = fmaxf(sqrtf(wave_sum(rq_lane_dot(xr, xr))), 1e-8f);
  float best = 0.f;
  int bestp = -1;
  for (int p = 0; p < Pmax; ++p) {
    const int k = pos[(size_t)n * Pmax + p];
    if ((unsigned)k >= (unsigned)Q) continue;                               // padding
    const RqRow xk = rq_load_row(x + ((size_t)k * N + n) * C, C4, lane);
    const float d = wave_sum(rq_lane_dot(xr, xk));
    const float nk = fmaxf(sqrtf(wave_sum(rq_lane_dot(xk, xk))), 1e-8f);
    const float c = d / (nr * nk);
    if (bestp < 0 || c > best) {                                            // the first maximum wins
      best = c;
      bestp = p;
    }
  }
  if (lane == 0) nearest[(size_t)n * Q + q] = bestp;
}

__global__ __launch_bounds__(256) void rq_rows_fwd_kernel(const float *__restrict__ x, const int *__restrict__ image_start,
                                                          const int *__restrict__ key, const int Q, const int N, const int C,
                                                          const int I, float *__restrict__ norm, float *__restrict__ S,
                                                          float *__restrict__ Cs)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * RQ_WAVES + wave, n = blockIdx.y;
  if (q >= Q) return;                                                       // (uniform in the wave; the kernel has no barrier)
  const int C4 = C >> 2;
  const RqRow xr = rq_load_row(x + ((size_t)q * N + n) * C, C4, lane);
  const float mq = fmaxf(sqrtf(wave_sum(rq_lane_dot(xr, xr))), 1e-12f);
  if (lane == 0) norm[(size_t)n * Q + q] = mq;
  int first, rows;
  image_rows(image_start, n, I, Q, first, rows);
  for (int r = 0; r < rows; ++r) {
    const int i = first + r, k = key[i];
    float s = 0.f, c = 0.f;
    if ((unsigned)k < (unsigned)Q) {
      const RqRow xk = rq_load_row(x + ((size_t)k * N + n) * C, C4, lane);
      s = wave_sum(rq_lane_dot(xr, xk));
      const float mk = fmaxf(sqrtf(wave_sum(rq_lane_dot(xk, xk))), 1e-12f);   // the bits of norm[n, k]
      c = s / (mq * mk);
    }
    if (lane == 0) {
      S[(size_t)i * Q + q] = s;
      Cs[(size_t)i * Q + q] = c;
    }
  }
}

__global__ __launch_bounds__(256) void rq_bwd_coef_kernel(const float *__restrict__ gS, const float *__restrict__ gC,
                                                          const float *__restrict__ Cs, const float *__restrict__ norm,
                                                          const int *__restrict__ image_start, const int *__restrict__ key,
                                                          const int Q, const int N, const int I, float *__restrict__ a,
                                                          float *__restrict__ b, float *__restrict__ rowsum)
{
  __shared__ float part[4];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = row_image(image_start, key, N, I, Q, i);
  const float mk = n >= 0 ? norm[(size_t)n * Q + key[i]] : 1.f;
  float sum = 0.f;
  for (int q = tid; q < Q; q += 256) {
    float av = 0.f, bv = 0.f;
    if (n >= 0) {
      const float gc = gC[(size_t)i * Q + q];
      av = gS[(size_t)i * Q + q] + gc / (norm[(size_t)n * Q + q] * mk);
      bv = -gc * Cs[(size_t)i * Q + q];
    }
    a[(size_t)i * Q + q] = av;
    b[(size_t)i * Q + q] = bv;
    sum += bv;
  }
  sum = wave_sum(sum);
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  if (tid == 0) rowsum[i] = ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(256) void rq_bwd_key_kernel(const float *__restrict__ x, const float *__restrict__ a,
                                                         const int *__restrict__ image_start, const int *__restrict__ key,
                                                         const int Q, const int N, const int C, const int I, float *__restrict__ y)
{
  __shared__ float4 ys[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int n = row_image(image_start, key, N, I, Q, i);
  const int C4 = C >> 2;
  const int colp = C4 <= 64 ? 64 : 128, parts = 256 / colp;                 // 4 ranges of queries, or 2
  const int col = tid % colp, part = tid / colp;
  const int chunk = (Q + parts - 1) / parts;
  const int q0 = part * chunk, q1 = min(Q, q0 + chunk);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n >= 0 && col < C4) {
    const float *ai = a + (size_t)i * Q;
    const float4 *xn = reinterpret_cast<const float4 *>(x) + (size_t)n * C4 + col;
#pragma unroll 4
    for (int q = q0; q < q1; ++q) {
      const float av = ai[q];
      const float4 xv = xn[(size_t)q * N * C4];
      acc.x = fmaf(av, xv.x, acc.x);
      acc.y = fmaf(av, xv.y, acc.y);
      acc.z = fmaf(av, xv.z, acc.z);
      acc.w = fmaf(av, xv.w, acc.w);
    }
  }
  ys[tid] = acc;
  __syncthreads();
  if (part == 0 && col < C4) {
    float4 sum = ys[col];
    for (int p = 1; p < parts; ++p) {
      const float4 v = ys[p * colp + col];
      sum.x += v.x;
      sum.y += v.y;
      sum.z += v.z;
      sum.w += v.w;
    }
    reinterpret_cast<float4 *>(y)[(size_t)i * C4 + col] = sum;
  }
}

__global__ __launch_bounds__(256) void rq_bwd_kernel(const float *__restrict__ x, const int *__restrict__ image_start,
                                                     const int *__restrict__ key, const float *__restrict__ norm,
                                                     const float *__restrict__ a, const float *__restrict__ b,
                                                     const float *__restrict__ rowsum, const float *__restrict__ y, const int Q,
                                                     const int N, const int C, const int I, float *__restrict__ gx)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * RQ_WAVES + wave, n = blockIdx.y;
  if (q >= Q) return;                                                       // (uniform in the wave; the kernel has no barrier)
  const int C4 = C >> 2;
  const size_t row = ((size_t)q * N + n) * C;
  RqRow acc;
#pragma unroll
  for (int j = 0; j < RQ_ROW_VECS; ++j) acc.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  int first, rows;
  image_rows(image_start, n, I, Q, first, rows);
  if (rows > 0) {                                                           // (uniform) an image without rows: exact zeros
    const RqRow xr = rq_load_row(x + row, C4, lane);
    float c1 = 0.f, c2 = 0.f;
    for (int r = 0; r < rows; ++r) {
      const int i = first + r, k = key[i];
      if ((unsigned)k >= (unsigned)Q) continue;
      const RqRow xk = rq_load_row(x + ((size_t)k * N + n) * C, C4, lane);
      rq_axpy(acc, a[(size_t)i * Q + q], xk);
      c1 += b[(size_t)i * Q + q];
    }
    for (int r = 0; r < rows; ++r) {
      const int i = first + r;
      if (key[i] != q) continue;
      const RqRow yi = rq_load_row(y + (size_t)i * C, C4, lane);
#pragma unroll
      for (int j = 0; j < RQ_ROW_VECS; ++j) {
        acc.v[j].x += yi.v[j].x;
        acc.v[j].y += yi.v[j].y;
        acc.v[j].z += yi.v[j].z;
        acc.v[j].w += yi.v[j].w;
      }
      c2 += rowsum[i];
    }
    const float m = norm[(size_t)n * Q + q];
    if (m > 1e-12f) rq_axpy(acc, (c1 + c2) / (m * m), xr);                  // a clamped norm is a constant: no b term
  }
#pragma unroll
  for (int j = 0; j < RQ_ROW_VECS; ++j) {
    const int idx = lane + 64 * j;
    if (idx < C4) reinterpret_cast<float4 *>(gx + row)[idx] = acc.v[j];
  }
}

// expf, logf, log1pf and the divisions are the compiler's accurate ones (no fast-math)
__global__ __launch_bounds__(256) void rq_contrast_kernel(const float *__restrict__ rows, const int *__restrict__ image_of,
                                                          const int *__restrict__ key, const int *__restrict__ owner, const int I,
                                                          const int Q, const int N, const float inv_t, float *__restrict__ loss,
                                                          float *__restrict__ coef)
{
  __shared__ float red[2][4];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = image_of[i], k = key[i];
  const bool valid = (unsigned)n < (unsigned)N;
  float z[RQ_ITEM_SLOTS];
  int cls[RQ_ITEM_SLOTS];                                                   // 0: the key, or past Q; 1: a negative; 2: a positive
  float mxn = -INFINITY, mxp = -INFINITY;
#pragma unroll
  for (int j = 0; j < RQ_ITEM_SLOTS; ++j) {
    const int q = tid + 256 * j;
    z[j] = 0.f;
    cls[j] = 0;
    if (valid && q < Q) {
      z[j] = rows[(size_t)i * Q + q] * inv_t;
      cls[j] = q == k ? 0 : (owner[(size_t)n * Q + q] == i ? 2 : 1);
      if (cls[j] == 1) mxn = fmaxf(mxn, z[j]);
      if (cls[j] == 2) mxp = fmaxf(mxp, -z[j]);
    }
  }
  mxn = wave_max(mxn);
  mxp = wave_max(mxp);
  if (lane == 0) {
    red[0][wave] = mxn;
    red[1][wave] = mxp;
  }
  __syncthreads();
  mxn = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  mxp = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  __syncthreads();                                                          // red is read before it is written again
  // an item without negatives (or without positives): logsumexp over nothing is -inf, the loss softplus(-inf) = 0
  const bool live = mxn > -INFINITY && mxp > -INFINITY && mxn < INFINITY && mxp < INFINITY;
  float en[RQ_ITEM_SLOTS], ep[RQ_ITEM_SLOTS];
  float sn = 0.f, sp = 0.f;
#pragma unroll
  for (int j = 0; j < RQ_ITEM_SLOTS; ++j) {
    en[j] = (live && cls[j] == 1) ? expf(z[j] - mxn) : 0.f;
    ep[j] = (live && cls[j] == 2) ? expf(-z[j] - mxp) : 0.f;
    sn += en[j];
    sp += ep[j];
  }
  sn = wave_sum(sn);
  sp = wave_sum(sp);
  if (lane == 0) {
    red[0][wave] = sn;
    red[1][wave] = sp;
  }
  __syncthreads();
  sn = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  sp = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  float l = 0.f, sig = 0.f;
  if (live) {
    const float t = (mxn + logf(sn)) + (mxp + logf(sp));
    const float e = expf(-fabsf(t));
    l = fmaxf(t, 0.f) + log1pf(e);
    sig = t >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  }
  if (tid == 0) loss[i] = l;
#pragma unroll
  for (int j = 0; j < RQ_ITEM_SLOTS; ++j) {
    const int q = tid + 256 * j;
    if (q >= Q) continue;
    float c = 0.f;
    if (live && cls[j] == 1) c = sig * (en[j] / sn) * inv_t;
    if (live && cls[j] == 2) c = -(sig * (ep[j] / sp) * inv_t);
    coef[(size_t)i * Q + q] = c;
  }
}

inline int reid_query_geometry_status(int Q, int N, int C, int I)
{
  if (Q > RQ_MAX_Q || N > 65535 || C > RQ_MAX_C || (C & 3)) return PCT_ERR_UNSUPPORTED;
  if ((long long)I > (long long)N * Q) return PCT_ERR_UNSUPPORTED;          // more than Q rows in some image
  return PCT_OK;
}

}  // namespace

int launch_reid_nearest_positive(const float *query, const int *pos, int Q, int N, int C, int max_pos, int *nearest,
                                 hipStream_t stream)
{
  if (const int rc = reid_query_geometry_status(Q, N, C, 0); rc != PCT_OK) return rc;
  if (max_pos > Q) return PCT_ERR_UNSUPPORTED;
  rq_nearest_kernel<<<dim3((unsigned)((Q + RQ_WAVES - 1) / RQ_WAVES), (unsigned)N), dim3(256), 0, stream>>>(query, pos, Q, N, C,
                                                                                                          max_pos, nearest);
  return (int)hipGetLastError();
}

int launch_reid_query_rows_forward(const float *query, const int *image_start, const int *key, int Q, int N, int C, int I,
                                   float *norm, float *dots, float *cosines, hipStream_t stream)
{
  if (const int rc = reid_query_geometry_status(Q, N, C, I); rc != PCT_OK) return rc;
  rq_rows_fwd_kernel<<<dim3((unsigned)((Q + RQ_WAVES - 1) / RQ_WAVES), (unsigned)N), dim3(256), 0, stream>>>(
      query, image_start, key, Q, N, C, I, norm, dots, cosines);
  return (int)hipGetLastError();
}

int launch_reid_query_rows_backward(const float *query, const int *image_start, const int *key, const float *norm,
                                    const float *cosines, const float *grad_dots, const float *grad_cosines, int Q, int N, int C,
                                    int I, void *workspace, float *grad_query, hipStream_t stream)
{
  if (const int rc = reid_query_geometry_status(Q, N, C, I); rc != PCT_OK) return rc;
  const size_t IQ = (size_t)I * Q;
  float *y = static_cast<float *>(workspace), *a = y + (size_t)I * C, *b = a + IQ, *rowsum = b + IQ;
  if (I > 0) {
    rq_bwd_coef_kernel<<<dim3((unsigned)I), dim3(256), 0, stream>>>(grad_dots, grad_cosines, cosines, norm, image_start, key, Q, N,
                                                                   I, a, b, rowsum);
    if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
    rq_bwd_key_kernel<<<dim3((unsigned)I), dim3(256), 0, stream>>>(query, a, image_start, key, Q, N, C, I, y);
    if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  }
  rq_bwd_kernel<<<dim3((unsigned)((Q + RQ_WAVES - 1) / RQ_WAVES), (unsigned)N), dim3(256), 0, stream>>>(
      query, image_start, key, norm, a, b, rowsum, y, Q, N, C, I, grad_query);
  return (int)hipGetLastError();
}

int launch_contrast_loss_rows(const float *rows, const int *image_of, const int *key, const int *owner, int I, int Q, int N,
                              float inv_temperature, float *loss, float *coef, hipStream_t stream)
{
  if (Q > RQ_MAX_Q || N > 65535) return PCT_ERR_UNSUPPORTED;
  rq_contrast_kernel<<<dim3((unsigned)I), dim3(256), 0, stream>>>(rows, image_of, key, owner, I, Q, N, inv_temperature, loss, coef);
  return (int)hipGetLastError();
}

}  // namespace pct
