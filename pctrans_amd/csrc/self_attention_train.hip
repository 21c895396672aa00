// Differentiable fp32 self-attention of the decoder: forward with the row statistics kept, and a backward that recomputes the
// probabilities (include/pctrans_hip_self_attn_train.h).  Operands as SelfAttentionLayer's five projections write them, all fp32:
//   q_c, q_p, k_c, k_p, v [Q, N, heads * 16]
// Per head  q = fl32(q_c + q_p),  k = fl32(k_c + k_p)  (one fp32 rounding each, as torch's add; the sums are never written),
//   score(q, k) = scale * q . k over the head's 16 dims,   P = softmax over all Q keys,   out = P v.
// There is no mask and so no row without an attendable key: keys are the queries, and Q >= 1.
//
// Arithmetic, register layouts and the reasons for them are those of cross_attention_train.hip (helpers: attn_train_common.hpp):
// the score products run on v_mfma_f64_16x16x4_f64 of the widened operands, the exponent x - m (forward) or x - lse (backward)
// is formed in fp64 and rounded to fp32 once, every other product runs on v_mfma_f32_16x16x4_f32 with fp32 accumulation.  With
// g = lane / 16 and c = lane % 16 a lane supplies A[row c][k slot g] and B[k slot g][column c]; register r receives
// D[row 4 g + r][column c] of an fp32 product and D[row g + 4 r][column c] of an fp64 one.
//
// Forward (sat_fwd_kernel), one launch: a workgroup of four waves owns 16 queries of one (image, head); wave w walks the 16-key
// steps w, w + 4, ...; the tile is S^T[key][query], so a lane holds one query's row statistics.  Online softmax per wave, then
// the four waves' (m, l, O) are merged through LDS in wave order.  lse = m + log(l) is written as two planes [2][N, heads, Q]:
// the fp32 value and what it leaves of the fp64 sum (lse enters the backward's exponent, where one fp32 word is a relative error
// of every probability of the row).  Nothing is staged: a workgroup reads every key and value row once.
//
// Backward, two launches.
//   sat_bwd_q_kernel: the same ownership.  The workgroup first stages k = fl32(k_c + k_p) and v of its whole (image, head) in
//   LDS as [Q][16] floats each (the add is made once per element, not once per use), because it sweeps the keys twice and reads
//   k both by rows (the score's operand) and by columns (dq's operand): sweep one forms D = sum_k P dP in fp64 (the form
//   torch's softmax backward evaluates, not the 16-term dot product with `out`), the four waves' partial sums are added in wave
//   order, D is rounded to fp32 once and written to the caller's workspace; sweep two recomputes P and dP, forms
//   dS = P (dP - D) and accumulates dq^T += k^T dS^T.  The four waves' dq go to LDS and are added in wave order, times scale.
//   The LDS image bounds the query count: SAT_MAX_Q = 512 rows are 64 KiB of the 160 KiB of a gfx950 CU, two workgroups per CU.
//   Rows are 64 bytes: a row read (lane (c, g): row c, floats 4 g ..) covers 1 KiB contiguously, a column read (row g + 4 r,
//   float c) 64 consecutive words per group of rows: neither has a bank conflict.
//   sat_bwd_k_kernel: one wave owns 16 keys of one (image, head) and loops over all queries in tiles of 16; the tile is
//   S[query][key], its registers feed dV^T += dO^T P and dK^T += Q^T dS; the wave stores its rows once.  It reads D from the
//   workspace.  Each wave reads every query row once, so nothing is staged here.
// grad_q is the gradient of q_c and of q_p, grad_k of k_c and of k_p (the add's backward is the identity): each is written once.
//
// No sum crosses a workgroup, there is no atomic and every order is fixed -- a gradient element is summed over its tiles in
// ascending order (per wave), inside a tile by the fmaf chain over the four k slots, for dq and D then over the four waves in
// ascending order: two calls on the same operands give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "attn_common.hpp"         // xgroup_sum, f32x4
#include "attn_train_common.hpp"   // mfma4, mfma16, mfma16d, widen, pi16, ld4, xgroup_max_f64
#include "launchers.hpp"

namespace pct {
namespace {

constexpr int ST_WAVES = 4;                // waves of a workgroup
constexpr int ST_THREADS = 64 * ST_WAVES;
constexpr int SAT_MAX_Q = 512;             // rows of the LDS image of k and v in sat_bwd_q_kernel

struct SGeo {
  int N, heads, Q;
  size_t rs;      // floats between two rows of an operand: N * heads * 16
};

// one fp32 rounding per element, as torch's add
__device__ __forceinline__ float4 add4(const float4 a, const float4 b)
{
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// ---- forward ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void sat_fwd_kernel(const float *__restrict__ q_c, const float *__restrict__ q_p,
                                                              const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                              const float *__restrict__ v, const SGeo geo, const float scale,
                                                              float *__restrict__ out, float *__restrict__ lse)
{
  __shared__ double s_m[ST_WAVES][16];
  __shared__ float s_l[ST_WAVES][16], s_o[ST_WAVES][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q;
  const size_t rs = geo.rs, hoff = (size_t)n * geo.heads * 16 + (size_t)h * 16;
  const int q = min(q0 + c, Q - 1);                                   // (a tile's surplus columns repeat the last query)
  const d4 qa = widen(add4(ld4(q_c + q * rs + hoff + 4 * g), ld4(q_p + q * rs + hoff + 4 * g)));
  const double dscale = (double)scale;

  double m_run = -INFINITY;
  float l_run = 0.f;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = wave * 16; k0 < Q; k0 += 16 * ST_WAVES) {
    const int key = min(k0 + c, Q - 1);
    const d4 ka = widen(add4(ld4(k_c + key * rs + hoff + 4 * g), ld4(k_p + key * rs + hoff + 4 * g)));
    float va[4], p[4];
    double x[4];
    double mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) va[r] = v[min(k0 + g + 4 * r, Q - 1) * rs + hoff + c];
    const f64x4 zd = {0., 0., 0., 0.};
    const f64x4 s = mfma16d(ka, qa, zd);                              // s[r] = score^T[key k0 + g + 4 r][query c] / scale
    bool dead[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dead[r] = k0 + g + 4 * r >= Q;
      x[r] = s[r] * dscale;
      mx = fmax(mx, dead[r] ? -INFINITY : x[r]);
    }
    mx = xgroup_max_f64(mx);                                          // finite: key k0 exists
    const double m_new = fmax(m_run, mx);
    const float alpha = expf((float)(m_run - m_new));                 // exp(-inf) = 0 on the wave's first step
    float rsum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = dead[r] ? 0.f : expf((float)(x[r] - m_new));
      rsum += p[r];
    }
    rsum = xgroup_sum(rsum);
    l_run = l_run * alpha + rsum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] *= alpha;
#pragma unroll
    for (int r = 0; r < 4; ++r) o = mfma4(va[r], p[r], o);            // o[r] = O[query c][value dim 4 g + r]
  }

  if (g == 0) {
    s_m[wave][c] = m_run;
    s_l[wave][c] = l_run;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) s_o[wave][c][4 * g + r] = o[r];
  __syncthreads();
  // the four waves' partial softmaxes, merged in wave order: thread (query tq, value dim td).  Wave 0 always has a key, so the
  // maximum is finite; a wave without a step holds (-inf, 0, 0) and enters with the factor exp(-inf) = 0
  const int tq = threadIdx.x >> 4, td = threadIdx.x & 15;
  double mm = -INFINITY;
#pragma unroll
  for (int w = 0; w < ST_WAVES; ++w) mm = fmax(mm, s_m[w][tq]);
  float l = 0.f, acc = 0.f;
#pragma unroll
  for (int w = 0; w < ST_WAVES; ++w) {
    const float f = expf((float)(s_m[w][tq] - mm));
    l += s_l[w][tq] * f;
    acc += s_o[w][tq][td] * f;
  }
  if (q0 + tq < Q) {
    out[(q0 + tq) * rs + hoff + td] = acc / l;
    if (td == 0) {
      // mm + log(l) in two fp32 words, formed in fp64 (cross_attention_train.hip says why)
      const double e = mm + log((double)l);
      const float hi = (float)e;
      const size_t at = ((size_t)n * geo.heads + h) * Q + q0 + tq;
      lse[at] = hi;
      lse[(size_t)geo.N * geo.heads * Q + at] = (float)(e - (double)hi);
    }
  }
}

// ---- backward, query side: D to the workspace, then grad_q ---------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void sat_bwd_q_kernel(const float *__restrict__ q_c, const float *__restrict__ q_p,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const float *__restrict__ lse,
                                                                const float *__restrict__ grad_out, const SGeo geo,
                                                                const float scale, float *__restrict__ delta,
                                                                float *__restrict__ grad_q)
{
  __shared__ __attribute__((aligned(16))) float s_k[SAT_MAX_Q * 16], s_v[SAT_MAX_Q * 16];
  __shared__ double s_sum[ST_WAVES][16];
  __shared__ float s_d[ST_WAVES][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q;                                                // <= SAT_MAX_Q (the launcher refuses more)
  const size_t rs = geo.rs, hoff = (size_t)n * geo.heads * 16 + (size_t)h * 16;
  for (int i = threadIdx.x; i < 4 * Q; i += ST_THREADS) {             // float4 i: row i / 4, floats 4 (i % 4) ..
    const size_t at = (size_t)(i >> 2) * rs + hoff + 4 * (i & 3);
    *reinterpret_cast<float4 *>(s_k + 4 * i) = add4(ld4(k_c + at), ld4(k_p + at));
    *reinterpret_cast<float4 *>(s_v + 4 * i) = ld4(v + at);
  }
  const int q = min(q0 + c, Q - 1);
  const d4 qa = widen(add4(ld4(q_c + q * rs + hoff + 4 * g), ld4(q_p + q * rs + hoff + 4 * g)));
  const float4 doa = ld4(grad_out + q * rs + hoff + 4 * g);
  const size_t stat = ((size_t)n * geo.heads + h) * Q + q, lo_plane = (size_t)geo.N * geo.heads * Q;
  const double lse_q = (double)lse[stat] + (double)lse[lo_plane + stat], dscale = (double)scale;
  const f64x4 zd = {0., 0., 0., 0.};
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  // sweep one: D[query c] = sum over the keys of P dP, fp64 running sums
  double sum = 0.;
  for (int k0 = wave * 16; k0 < Q; k0 += 16 * ST_WAVES) {
    const d4 ka = widen(ld4(s_k + min(k0 + c, Q - 1) * 16 + 4 * g));
    const float4 va = ld4(s_v + min(k0 + pi16(c), Q - 1) * 16 + 4 * g);
    const f64x4 s = mfma16d(ka, qa, zd);                              // score^T[key k0 + g + 4 r][query c] / scale
    const f32x4 dp = mfma16(va, doa, z);                              // dP^T[key k0 + g + 4 r][query] = v[key] . grad_out[query]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = expf((float)(s[r] * dscale - lse_q));
      sum += k0 + g + 4 * r >= Q ? 0. : (double)p * (double)dp[r];
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (g == 0) s_sum[wave][c] = sum;
  __syncthreads();
  double d = 0.;
#pragma unroll
  for (int w = 0; w < ST_WAVES; ++w) d += s_sum[w][c];
  const float d_q = (float)d;                                         // what the key pass reads back from the workspace
  if (threadIdx.x < 16 && q0 + (int)threadIdx.x < Q) delta[stat] = d_q;

  // sweep two: dq^T[dim c][query] += k^T[dim c][key] dS^T[key][query]
  f32x4 dq = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = wave * 16; k0 < Q; k0 += 16 * ST_WAVES) {
    const d4 ka = widen(ld4(s_k + min(k0 + c, Q - 1) * 16 + 4 * g));
    const float4 va = ld4(s_v + min(k0 + pi16(c), Q - 1) * 16 + 4 * g);
    float kt[4], ds[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) kt[r] = s_k[min(k0 + g + 4 * r, Q - 1) * 16 + c];
    const f64x4 s = mfma16d(ka, qa, zd);
    const f32x4 dp = mfma16(va, doa, z);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = expf((float)(s[r] * dscale - lse_q));
      ds[r] = k0 + g + 4 * r >= Q ? 0.f : p * (dp[r] - d_q);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dq = mfma4(kt[r], ds[r], dq);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) s_d[wave][c][4 * g + r] = dq[r];        // register r: dq[query c][dim 4 g + r]
  __syncthreads();
  const int tq = threadIdx.x >> 4, td = threadIdx.x & 15;
  if (q0 + tq < Q) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < ST_WAVES; ++w) a += s_d[w][tq][td];
    grad_q[(q0 + tq) * rs + hoff + td] = a * scale;
  }
}

// ---- backward, key side: grad_k, grad_v --------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void sat_bwd_k_kernel(const float *__restrict__ q_c, const float *__restrict__ q_p,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const float *__restrict__ lse,
                                                                const float *__restrict__ delta, const float *__restrict__ grad_out,
                                                                const SGeo geo, const float scale, float *__restrict__ grad_k,
                                                                float *__restrict__ grad_v)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int k0 = (blockIdx.x * ST_WAVES + wave) * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q;
  if (k0 >= Q) return;                                                // (whole waves; the kernel has no barrier)
  const size_t rs = geo.rs, hoff = (size_t)n * geo.heads * 16 + (size_t)h * 16;
  const size_t stat = ((size_t)n * geo.heads + h) * Q, lo_plane = (size_t)geo.N * geo.heads * Q;
  const bool key_ok = k0 + c < Q;
  const int key = min(k0 + c, Q - 1);
  const d4 ka = widen(add4(ld4(k_c + key * rs + hoff + 4 * g), ld4(k_p + key * rs + hoff + 4 * g)));
  const float4 va = ld4(v + key * rs + hoff + 4 * g);
  const double dscale = (double)scale;

  f32x4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < Q; q0 += 16) {
    const int q = min(q0 + c, Q - 1);
    const d4 qa = widen(add4(ld4(q_c + q * rs + hoff + 4 * g), ld4(q_p + q * rs + hoff + 4 * g)));
    const float4 doa = ld4(grad_out + min(q0 + pi16(c), Q - 1) * rs + hoff + 4 * g);
    float qt[4], dot[4], p[4], ds[4];
    const f64x4 zd = {0., 0., 0., 0.};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f64x4 s = mfma16d(qa, ka, zd);                              // score[query q0 + g + 4 r][key c] / scale
    const f32x4 dp = mfma16(doa, va, z);                              // dP[query q0 + g + 4 r][key]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qq = q0 + g + 4 * r, qr = min(qq, Q - 1);
      const size_t at = qr * rs + hoff + c;
      qt[r] = q_c[at] + q_p[at];
      dot[r] = grad_out[at];
      const bool dead = qq >= Q || !key_ok;
      const double l = (double)lse[stat + qr] + (double)lse[lo_plane + stat + qr];
      const float e = expf((float)(s[r] * dscale - l));
      p[r] = dead ? 0.f : e;
      ds[r] = dead ? 0.f : e * (dp[r] - delta[stat + qr]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                     // X^T[dim c][key] += Y^T[dim c][query] Z[query][key]
      dv = mfma4(dot[r], p[r], dv);
      dk = mfma4(qt[r], ds[r], dk);
    }
  }
  if (key_ok) {                                                       // register r: row `key`, dim 4 g + r
    const size_t at = key * rs + hoff + 4 * g;
    *reinterpret_cast<float4 *>(grad_v + at) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    *reinterpret_cast<float4 *>(grad_k + at) = make_float4(dk[0] * scale, dk[1] * scale, dk[2] * scale, dk[3] * scale);
  }
}

// heads 4 or 8 (what the decoder builds); at most SAT_MAX_Q queries (the LDS image of the query pass); an operand's element
// count below 2^31 (offsets are formed in 64 bits; the bound keeps the grid's z extent and the row arithmetic far from their limits)
bool sat_covered(const int N, const int heads, const int Q)
{
  if (heads != 4 && heads != 8) return false;
  if (N > 65535 || Q > SAT_MAX_Q) return false;
  return (long long)Q * N * heads * 16 < 0x7fffffffLL;
}

}  // namespace

int launch_self_attention_fwd_f32(const float *q_c, const float *q_p, const float *k_c, const float *k_p, const float *v, int N,
                                  int heads, int Q, float scale, float *out, float *lse, hipStream_t stream)
{
  if (!sat_covered(N, heads, Q)) return PCT_NOT_COVERED;
  const SGeo geo = {N, heads, Q, (size_t)N * heads * 16};
  sat_fwd_kernel<<<dim3((Q + 15) / 16, heads, N), ST_THREADS, 0, stream>>>(q_c, q_p, k_c, k_p, v, geo, scale, out, lse);
  return (int)hipGetLastError();
}

int launch_self_attention_bwd_f32(const float *q_c, const float *q_p, const float *k_c, const float *k_p, const float *v,
                                  const float *lse, const float *grad_out, int N, int heads, int Q, float scale, float *workspace,
                                  float *grad_q, float *grad_k, float *grad_v, hipStream_t stream)
{
  if (!sat_covered(N, heads, Q)) return PCT_NOT_COVERED;
  const SGeo geo = {N, heads, Q, (size_t)N * heads * 16};
  sat_bwd_q_kernel<<<dim3((Q + 15) / 16, heads, N), ST_THREADS, 0, stream>>>(q_c, q_p, k_c, k_p, v, lse, grad_out, geo, scale,
                                                                            workspace, grad_q);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  sat_bwd_k_kernel<<<dim3((Q + 16 * ST_WAVES - 1) / (16 * ST_WAVES), heads, N), ST_THREADS, 0, stream>>>(
      q_c, q_p, k_c, k_p, v, lse, workspace, grad_out, geo, scale, grad_k, grad_v);
  return (int)hipGetLastError();
}

}  // namespace pct
