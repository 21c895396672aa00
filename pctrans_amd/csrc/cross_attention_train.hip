// Differentiable fp32 cross-attention of the decoder: forward with the row statistics kept, and a backward that recomputes the
// probabilities (include/pctrans_hip_attn_train.h).  Operands in the split form the projection GEMMs write, all fp32:
//   q_c, q_s [Q, N, heads * 16]   k_c, k_p, v [S, N, heads * 16]   mask [N, Q, S] bytes   row_open [N, Q] bytes
// Per head the query is [content 16 | position 16] and the key likewise; the concatenations are never formed:
//   score(q, k) = scale * (q_c[q] . k_c[k] + q_s[q] . k_p[k]),   P = softmax over the attendable keys,   out = P v.
//
// The score products run on v_mfma_f64_16x16x4_f64 (the fp32 operands widened, see mfma16d in attn_train_common.hpp), every other product on
// v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulation: bit for bit an fmaf chain in ascending k slot).  With g = lane / 16
// and c = lane % 16, a lane supplies A[row c][k slot g] and B[k slot g][column c]; register r receives D[row 4 g + r][column c]
// of an fp32 product and D[row g + 4 r][column c] of an fp64 one.  The four k slots of one instruction need not be neighbours,
// so a lane loads ONE float4 (dims 4 g .. 4 g + 3 of row c) and instruction j of a group of four contracts component j: the 16
// dims of an operand half are summed in the order (j, g) = dim 4 g + j, j outermost.  An accumulator register r of a tile
// whose rows are the contracted index of the next product is that product's B operand for k slot g as it stands: no lane
// movement and no LDS between the score tile and the products that consume the probabilities.
//
// Forward (xat_fwd_kernel) and the query-gradient pass (xat_bwd_q_kernel): a workgroup of four waves owns 16 queries of one
// (image, head); wave w walks the 16-key steps w, w + 4, ...; the tile is S^T[key][query], so a lane holds one query's row
// statistics.  Forward: online softmax per wave, then the four waves' (m, l, O) are merged through LDS in wave order.
// Backward: each wave's partial dq (content and position half) goes to LDS and the four are added in wave order, times scale.
// The key/value-gradient pass (xat_bwd_k_kernel): one wave owns 16 keys of one (image, head) and loops over all queries in
// tiles of 16; the tile is S[query][key], its registers feed dV^T += dO^T P, dK_c^T += Q_c^T dS, dK_p^T += Q_s^T dS; the wave
// stores its rows once.  No sum crosses a workgroup, there is no atomic, and every order above is fixed: two calls give the
// same bits.
//
// Summation order of a gradient element: over its tiles in ascending order (per wave), inside a tile the fmaf chain over the
// four k slots, instruction m covering rows g + 4 m; for dq then over the four waves in ascending order.
//
// Backward recomputes P = exp(scale * s - lse), the difference in fp64, from the forward's lse = m + log(l) (row maximum + log
// of the row sum), which the forward writes as two planes [2][N, heads, Q]: the fp32 value and what it leaves of the fp64 sum.  lse enters an
// exponent: one fp32 word at |lse| in [4, 8) is off by up to 2.4e-7, a relative error of every probability of the row and so
// of the row's gradients, on top of what the torch chain's stored probabilities carry.  dP = dO V^T, dS = P (dP - D) with
// D = rowsum(dO * out) formed once by xat_delta_kernel in the caller's workspace (as sum_k P dP: see there).  A masked position has P = 0 and dS = 0
// exactly (selected, not multiplied).
//
// A row with nothing attendable (every key masked, row_open not set) follows attn_common.hpp: everything stays 0 -- out = 0,
// lse = 0 in both planes (the sentinel; never read for a live position), every gradient contribution of the row 0.  Torch's
// masked softmax gives NaN on such a row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "attn_common.hpp"   // xgroup_max, xgroup_sum, f32x4
#include "attn_train_common.hpp"   // mfma4, mfma16, mfma16d, widen, pi16, ld4, xgroup_max_f64
#include "launchers.hpp"

namespace pct {
namespace {

constexpr int XT_WAVES = 4;                // waves of a workgroup
constexpr int XT_THREADS = 64 * XT_WAVES;

struct Geo {
  int N, heads, Q, S;
  size_t rs;      // floats between two rows of an operand: N * heads * 16
};

// ---- forward ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XT_THREADS) void xat_fwd_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                              const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                              const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                              const unsigned char *__restrict__ row_open, const Geo geo,
                                                              const float scale, float *__restrict__ out, float *__restrict__ lse)
{
  __shared__ double s_m[XT_WAVES][16];
  __shared__ float s_l[XT_WAVES][16], s_o[XT_WAVES][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = geo.S;
  const size_t rs = geo.rs, hoff = (size_t)n * geo.heads * 16 + (size_t)h * 16;
  const int q = min(q0 + c, Q - 1);                                   // (a tile's surplus columns repeat the last query)
  const d4 qa = widen(ld4(q_c + q * rs + hoff + 4 * g)), qb = widen(ld4(q_s + q * rs + hoff + 4 * g));
  const bool open = !mask || (row_open && row_open[(size_t)n * Q + q]);
  const unsigned char *mrow = mask ? mask + ((size_t)n * Q + q) * S : nullptr;
  const double dscale = (double)scale;

  double m_run = -INFINITY;
  float l_run = 0.f;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = wave * 16; k0 < S; k0 += 16 * XT_WAVES) {
    const int key = min(k0 + c, S - 1);
    const d4 ka = widen(ld4(k_c + key * rs + hoff + 4 * g)), kb = widen(ld4(k_p + key * rs + hoff + 4 * g));
    float va[4], p[4];
    double x[4];
    double mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) va[r] = v[min(k0 + g + 4 * r, S - 1) * rs + hoff + c];
    const f64x4 zd = {0., 0., 0., 0.};
    // (content and position half in accumulators of their own: two chains of four dependent instructions instead of one of eight)
    const f64x4 s = mfma16d(ka, qa, zd) + mfma16d(kb, qb, zd);        // s[r] = score^T[key k0 + g + 4 r][query c] / scale
    bool dead[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = k0 + g + 4 * r;
      dead[r] = kk >= S || (!open && mrow[kk] != 0);
      x[r] = s[r] * dscale;
      mx = fmax(mx, dead[r] ? -INFINITY : x[r]);
    }
    mx = xgroup_max_f64(mx);
    const double m_new = fmax(m_run, mx);
    const double m_safe = m_new == -INFINITY ? 0. : m_new;            // nothing attendable yet: keep everything 0
    const float alpha = expf((float)(m_run - m_safe));                // exp(-inf) = 0 on the first live step
    float rsum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = dead[r] ? 0.f : expf((float)(x[r] - m_safe));
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
  // the four waves' partial softmaxes, merged in wave order: thread (query tq, value dim td)
  const int tq = threadIdx.x >> 4, td = threadIdx.x & 15;
  double mm = -INFINITY;
#pragma unroll
  for (int w = 0; w < XT_WAVES; ++w) mm = fmax(mm, s_m[w][tq]);
  float l = 0.f, acc = 0.f;
  if (mm != -INFINITY) {
#pragma unroll
    for (int w = 0; w < XT_WAVES; ++w) {
      const float f = expf((float)(s_m[w][tq] - mm));
      l += s_l[w][tq] * f;
      acc += s_o[w][tq][td] * f;
    }
  }
  if (q0 + tq < Q) {
    const bool live = l > 0.f;
    out[(q0 + tq) * rs + hoff + td] = live ? acc / l : 0.f;
    if (td == 0) {
      // mm + log(l) in two fp32 words (formed in fp64: fp32's logf alone is off by up to an ulp of a result near 8, 5e-7, and
      // the sum is rounded once more -- as a relative error of every recomputed probability of the row)
      const double e = live ? mm + log((double)l) : 0.0;
      const float hi = (float)e;
      const size_t at = ((size_t)n * geo.heads + h) * Q + q0 + tq;
      lse[at] = hi;
      lse[(size_t)geo.N * geo.heads * Q + at] = (float)(e - (double)hi);
    }
  }
}

// ---- D = rowsum(grad_out * out) = sum_k P dP, formed as the second sum from the backward's own P and dP: the forward's
// structure (four waves over interleaved key steps, merged in wave order).  The first form inherits the rounding of `out`
// through a 16-term dot product whose terms do not cancel the way dP - D must (measured: key gradients at 2 - 3.4 x the torch
// chain's error on rows with two or three live keys); the second is what torch's softmax backward evaluates, its error is
// common to dP and D, and a row with one key of weight 1 has D = dP and dS = 0 exactly, as in torch.  fp64 running sums.
__global__ __launch_bounds__(XT_THREADS) void xat_delta_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                const unsigned char *__restrict__ row_open,
                                                                const float *__restrict__ lse, const float *__restrict__ grad_out,
                                                                const Geo geo, const float scale, float *__restrict__ delta)
{
  __shared__ double s_sum[XT_WAVES][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = geo.S;
  const size_t rs = geo.rs, hoff = (size_t)n * geo.heads * 16 + (size_t)h * 16;
  const int q = min(q0 + c, Q - 1);
  const d4 qa = widen(ld4(q_c + q * rs + hoff + 4 * g)), qb = widen(ld4(q_s + q * rs + hoff + 4 * g));
  const float4 doa = ld4(grad_out + q * rs + hoff + 4 * g);
  const size_t stat = ((size_t)n * geo.heads + h) * Q + q, lo_plane = (size_t)geo.N * geo.heads * Q;
  const double lse_q = (double)lse[stat] + (double)lse[lo_plane + stat], dscale = (double)scale;
  const bool open = !mask || (row_open && row_open[(size_t)n * Q + q]);
  const unsigned char *mrow = mask ? mask + ((size_t)n * Q + q) * S : nullptr;

  double sum = 0.;
  for (int k0 = wave * 16; k0 < S; k0 += 16 * XT_WAVES) {
    const int key = min(k0 + c, S - 1);
    const d4 ka = widen(ld4(k_c + key * rs + hoff + 4 * g)), kb = widen(ld4(k_p + key * rs + hoff + 4 * g));
    const float4 va = ld4(v + min(k0 + pi16(c), S - 1) * rs + hoff + 4 * g);
    const f64x4 zd = {0., 0., 0., 0.};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f64x4 s = mfma16d(ka, qa, zd) + mfma16d(kb, qb, zd);        // score^T[key k0 + g + 4 r][query c] / scale
    const f32x4 dp = mfma16(va, doa, z);                              // dP^T[key k0 + g + 4 r][query]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = k0 + g + 4 * r;
      const bool dead = kk >= S || (!open && mrow[kk] != 0);
      const float p = expf((float)(s[r] * dscale - lse_q));
      sum += dead ? 0. : (double)p * (double)dp[r];
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (g == 0) s_sum[wave][c] = sum;
  __syncthreads();
  if (threadIdx.x < 16 && q0 + (int)threadIdx.x < Q) {
    double d = 0.;
#pragma unroll
    for (int w = 0; w < XT_WAVES; ++w) d += s_sum[w][threadIdx.x];
    delta[((size_t)n * geo.heads + h) * Q + q0 + threadIdx.x] = (float)d;
  }
}

// ---- backward, query side: grad_q_c, grad_q_s --------------------------------------------------------------------------------
__global__ __launch_bounds__(XT_THREADS) void xat_bwd_q_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                const unsigned char *__restrict__ row_open,
                                                                const float *__restrict__ lse, const float *__restrict__ delta,
                                                                const float *__restrict__ grad_out, const Geo geo, const float scale,
                                                                float *__restrict__ grad_q_c, float *__restrict__ grad_q_s)
{
  __shared__ float s_d[XT_WAVES][2][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = geo.S;
  const size_t rs = geo.rs, hoff = (size_t)n * geo.heads * 16 + (size_t)h * 16;
  const int q = min(q0 + c, Q - 1);
  const d4 qa = widen(ld4(q_c + q * rs + hoff + 4 * g)), qb = widen(ld4(q_s + q * rs + hoff + 4 * g));
  const float4 doa = ld4(grad_out + q * rs + hoff + 4 * g);
  const size_t stat = ((size_t)n * geo.heads + h) * Q + q, lo_plane = (size_t)geo.N * geo.heads * Q;
  const double lse_q = (double)lse[stat] + (double)lse[lo_plane + stat], dscale = (double)scale;
  const float d_q = delta[stat];
  const bool open = !mask || (row_open && row_open[(size_t)n * Q + q]);
  const unsigned char *mrow = mask ? mask + ((size_t)n * Q + q) * S : nullptr;

  f32x4 dqc = {0.f, 0.f, 0.f, 0.f}, dqs = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = wave * 16; k0 < S; k0 += 16 * XT_WAVES) {
    const int key = min(k0 + c, S - 1);
    const d4 ka = widen(ld4(k_c + key * rs + hoff + 4 * g)), kb = widen(ld4(k_p + key * rs + hoff + 4 * g));
    const float4 va = ld4(v + min(k0 + pi16(c), S - 1) * rs + hoff + 4 * g);
    float kct[4], kpt[4], ds[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t at = min(k0 + g + 4 * r, S - 1) * rs + hoff + c;
      kct[r] = k_c[at];
      kpt[r] = k_p[at];
    }
    const f64x4 zd = {0., 0., 0., 0.};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f64x4 s = mfma16d(ka, qa, zd) + mfma16d(kb, qb, zd);        // score^T[key k0 + g + 4 r][query c] / scale
    const f32x4 dp = mfma16(va, doa, z);                              // dP^T[key k0 + g + 4 r][query] = v[key] . grad_out[query]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = k0 + g + 4 * r;
      const bool dead = kk >= S || (!open && mrow[kk] != 0);
      const float p = expf((float)(s[r] * dscale - lse_q));
      ds[r] = dead ? 0.f : p * (dp[r] - d_q);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                     // dq^T[dim c][query] += k^T[dim c][key] dS^T[key][query]
      dqc = mfma4(kct[r], ds[r], dqc);
      dqs = mfma4(kpt[r], ds[r], dqs);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {                                       // register r: dq[query c][dim 4 g + r]
    s_d[wave][0][c][4 * g + r] = dqc[r];
    s_d[wave][1][c][4 * g + r] = dqs[r];
  }
  __syncthreads();
  const int tq = threadIdx.x >> 4, td = threadIdx.x & 15;
  if (q0 + tq < Q) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < XT_WAVES; ++w) {
      a += s_d[w][0][tq][td];
      b += s_d[w][1][tq][td];
    }
    grad_q_c[(q0 + tq) * rs + hoff + td] = a * scale;
    grad_q_s[(q0 + tq) * rs + hoff + td] = b * scale;
  }
}

// ---- backward, key side: grad_k_c, grad_k_p, grad_v --------------------------------------------------------------------------
__global__ __launch_bounds__(XT_THREADS) void xat_bwd_k_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                const unsigned char *__restrict__ row_open,
                                                                const float *__restrict__ lse, const float *__restrict__ delta,
                                                                const float *__restrict__ grad_out, const Geo geo, const float scale,
                                                                float *__restrict__ grad_k_c, float *__restrict__ grad_k_p,
                                                                float *__restrict__ grad_v)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int k0 = (blockIdx.x * XT_WAVES + wave) * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = geo.S;
  if (k0 >= S) return;                                                // (whole waves; the kernel has no barrier)
  const size_t rs = geo.rs, hoff = (size_t)n * geo.heads * 16 + (size_t)h * 16;
  const size_t stat = ((size_t)n * geo.heads + h) * Q, lo_plane = (size_t)geo.N * geo.heads * Q;
  const bool key_ok = k0 + c < S;
  const int key = min(k0 + c, S - 1);
  const d4 ka = widen(ld4(k_c + key * rs + hoff + 4 * g)), kb = widen(ld4(k_p + key * rs + hoff + 4 * g));
  const float4 va = ld4(v + key * rs + hoff + 4 * g);
  const double dscale = (double)scale;

  f32x4 dkc = {0.f, 0.f, 0.f, 0.f}, dkp = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < Q; q0 += 16) {
    const int q = min(q0 + c, Q - 1);
    const d4 qa = widen(ld4(q_c + q * rs + hoff + 4 * g)), qb = widen(ld4(q_s + q * rs + hoff + 4 * g));
    const float4 doa = ld4(grad_out + min(q0 + pi16(c), Q - 1) * rs + hoff + 4 * g);
    float qct[4], qst[4], dot[4], p[4], ds[4];
    const f64x4 zd = {0., 0., 0., 0.};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f64x4 s = mfma16d(qa, ka, zd) + mfma16d(qb, kb, zd);        // score[query q0 + g + 4 r][key c] / scale
    const f32x4 dp = mfma16(doa, va, z);                              // dP[query q0 + g + 4 r][key]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qq = q0 + g + 4 * r, qr = min(qq, Q - 1);
      const size_t at = qr * rs + hoff + c;
      qct[r] = q_c[at];
      qst[r] = q_s[at];
      dot[r] = grad_out[at];
      const bool masked = mask && !(row_open && row_open[(size_t)n * Q + qr]) && mask[((size_t)n * Q + qr) * S + key] != 0;
      const bool dead = qq >= Q || !key_ok || masked;
      const double l = (double)lse[stat + qr] + (double)lse[lo_plane + stat + qr];
      const float e = expf((float)(s[r] * dscale - l));
      p[r] = dead ? 0.f : e;
      ds[r] = dead ? 0.f : e * (dp[r] - delta[stat + qr]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                     // X^T[dim c][key] += Y^T[dim c][query] Z[query][key]
      dv = mfma4(dot[r], p[r], dv);
      dkc = mfma4(qct[r], ds[r], dkc);
      dkp = mfma4(qst[r], ds[r], dkp);
    }
  }
  if (key_ok) {                                                       // register r: row `key`, dim 4 g + r
    const size_t at = key * rs + hoff + 4 * g;
    *reinterpret_cast<float4 *>(grad_v + at) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    *reinterpret_cast<float4 *>(grad_k_c + at) = make_float4(dkc[0] * scale, dkc[1] * scale, dkc[2] * scale, dkc[3] * scale);
    *reinterpret_cast<float4 *>(grad_k_p + at) = make_float4(dkp[0] * scale, dkp[1] * scale, dkp[2] * scale, dkp[3] * scale);
  }
}

// heads 4 or 8 (what the decoder builds); a tensor's element count below 2^31 (offsets are formed in 64 bits; the bound keeps
// the grid's z extent and the row arithmetic far from their limits)
bool xat_covered(const int N, const int heads, const int Q, const int S)
{
  if (heads != 4 && heads != 8) return false;
  if (N > 65535) return false;
  const long long lim = 0x7fffffffLL, rs = (long long)N * heads * 16;
  return (long long)Q * rs < lim && (long long)S * rs < lim;
}

}  // namespace

int launch_cross_attention_fwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                   const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S,
                                   float scale, float *out, float *lse, hipStream_t stream)
{
  if (!xat_covered(N, heads, Q, S)) return PCT_NOT_COVERED;
  const Geo geo = {N, heads, Q, S, (size_t)N * heads * 16};
  xat_fwd_kernel<<<dim3((Q + 15) / 16, heads, N), XT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, geo, scale, out,
                                                                          lse);
  return (int)hipGetLastError();
}

int launch_cross_attention_bwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                   const unsigned char *mask, const unsigned char *row_open, const float *out, const float *lse,
                                   const float *grad_out, int N, int heads, int Q, int S, float scale, float *workspace,
                                   float *grad_q_c, float *grad_q_s, float *grad_k_c, float *grad_k_p, float *grad_v,
                                   hipStream_t stream)
{
  if (!xat_covered(N, heads, Q, S)) return PCT_NOT_COVERED;
  const Geo geo = {N, heads, Q, S, (size_t)N * heads * 16};
  xat_delta_kernel<<<dim3((Q + 15) / 16, heads, N), XT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, grad_out,
                                                                            geo, scale, workspace);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  xat_bwd_k_kernel<<<dim3((S + 16 * XT_WAVES - 1) / (16 * XT_WAVES), heads, N), XT_THREADS, 0, stream>>>(
      q_c, q_s, k_c, k_p, v, mask, row_open, lse, workspace, grad_out, geo, scale, grad_k_c, grad_k_p, grad_v);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  xat_bwd_q_kernel<<<dim3((Q + 15) / 16, heads, N), XT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, workspace,
                                                                            grad_out, geo, scale, grad_q_c, grad_q_s);
  return (int)hipGetLastError();
}

}  // namespace pct
