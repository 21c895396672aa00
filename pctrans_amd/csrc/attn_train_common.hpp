// The differentiable fp32 attention of the decoder, stated once for its two instances (cross_attention_train.hip,
// self_attention_train.hip): forward with the row statistics kept, and a backward that recomputes the probabilities; and the
// same forward without them for evaluation (attention_eval.hip: attn_fwd's LSE and AHEAD).  Operands
// are fp32 rows [rows, N, heads * 16]; per head a query or key row has two 16-dim halves (a, b), and a policy F says what the
// score makes of them:
//   F::HALVES == 2 (cross)  the row is [a | b]: score = scale * (q_a . k_a + q_b . k_b), every half has a gradient of its own
//   F::HALVES == 1 (self)   the row is fl32(a + b) (one fp32 rounding per element, as torch's add; the sum is never written):
//                           score = scale * q . k, and the one gradient is that of a and of b
//   F::MASKED               a byte mask [N, Q, S] may take keys out of a row (row_open [N, Q] set: the row ignores its mask
//                           row), and a row may be left with nothing attendable.  Not MASKED: no mask code is compiled.
//   F::keys(geo)            the key count S (self: the query count, held once)
//   P = softmax over the attendable keys,   out = P v.
//
// The score products run on v_mfma_f64_16x16x4_f64 (the fp32 operands widened, see mfma16d), every other product on
// v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulation: bit for bit an fmaf chain in ascending k slot).  With g = lane / 16
// and c = lane % 16, a lane supplies A[row c][k slot g] and B[k slot g][column c]; register r receives D[row 4 g + r][column c]
// of an fp32 product and D[row g + 4 r][column c] of an fp64 one.  The four k slots of one instruction need not be neighbours,
// so a lane loads ONE float4 (dims 4 g .. 4 g + 3 of row c) and instruction j of a group of four contracts component j: the 16
// dims of an operand half are summed in the order (j, g) = dim 4 g + j, j outermost.  An accumulator register r of a tile
// whose rows are the contracted index of the next product is that product's B operand for k slot g as it stands: no lane
// movement and no LDS between the score tile and the products that consume the probabilities.
//
// Forward (attn_fwd) and the query pass (attn_bwd_q): a workgroup of four waves owns 16 queries of one (image, head); wave w
// walks the 16-key steps w, w + 4, ...; the tile is S^T[key][query], so a lane holds one query's row statistics.  Forward:
// online softmax per wave, then the four waves' (m, l, O) are merged through LDS in wave order.  Query pass: sweep D forms
// D = sum_k P dP per query, sweep DQ accumulates dq^T += k^T dS^T; each wave's partial result goes to LDS and the four are added
// in wave order (dq then times scale).  A kernel runs one sweep or both, on keys read from global memory or from an LDS image.
// The key pass (attn_bwd_k): one wave owns 16 keys of one (image, head) and loops over all queries in tiles of 16; the tile is
// S[query][key], its registers feed dV^T += dO^T P and, per half, dK^T += Q^T dS; the wave stores its rows once.  No sum crosses
// a workgroup, there is no atomic, and every order is fixed: two calls give the same bits.
//
// Summation order of a gradient element: over its tiles in ascending order (per wave), inside a tile the fmaf chain over the
// four k slots, instruction m covering rows g + 4 m; for dq and D then over the four waves in ascending order.
//
// Backward recomputes P = exp(scale * s - lse), the difference in fp64, from the forward's lse = m + log(l) (row maximum + log
// of the row sum), which the forward writes as two planes [2][N, heads, Q]: the fp32 value and what it leaves of the fp64 sum.
// lse enters an exponent: one fp32 word at |lse| in [4, 8) is off by up to 2.4e-7, a relative error of every probability of
// the row and so of the row's gradients, on top of what the torch chain's stored probabilities carry.  dP = dO V^T,
// dS = P (dP - D).  D = rowsum(dO * out) is formed as sum_k P dP from the backward's own P and dP, in fp64 running sums: the
// first form inherits the rounding of `out` through a 16-term dot product whose terms do not cancel the way dP - D must
// (measured: key gradients at 2 - 3.4 x the torch chain's error on rows with two or three live keys); the second is what
// torch's softmax backward evaluates, its error is common to dP and D, and a row with one key of weight 1 has D = dP and
// dS = 0 exactly, as in torch.  A masked position has P = 0 and dS = 0 exactly (selected, not multiplied).
//
// A row with nothing attendable (every key masked, row_open not set) follows attn_common.hpp: everything stays 0 -- out = 0,
// lse = 0 in both planes (the sentinel; never read for a live position), every gradient contribution of the row 0.  Torch's
// masked softmax gives NaN on such a row.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include <type_traits>

#include "attn_common.hpp"   // xgroup_sum, f32x4

namespace pct {
namespace {

constexpr int AT_WAVES = 4;                // waves of a workgroup
constexpr int AT_THREADS = 64 * AT_WAVES;

__device__ __forceinline__ f32x4 mfma4(const float a, const float b, const f32x4 c)
{
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// += over the 4 dims a lane's float4 holds of each operand (16 dims in all over the four lane groups)
__device__ __forceinline__ f32x4 mfma16(const float4 a, const float4 b, f32x4 c)
{
  c = mfma4(a.x, b.x, c);
  c = mfma4(a.y, b.y, c);
  c = mfma4(a.z, b.z, c);
  return mfma4(a.w, b.w, c);
}
// The scores run on v_mfma_f64_16x16x4_f64 on the operands widened to fp64 (exact products, fp64 accumulation), and the
// exponent x - m (forward) or x - lse (backward) is formed in fp64 and rounded to fp32 once.  An fp32 chain leaves scale * s
// with an error that grows with |x| (32 roundings of partial sums, then |x| 2^-24 for the stored value), and the exponential
// turns it into a relative error of every probability: 1e-5 at the scores of +-300 of the underflowing family.  Operands as
// the fp32 form; the result differs: register r of lane group g is row g + 4 r (not 4 g + r).
typedef double f64x4 __attribute__((ext_vector_type(4)));
struct d4 {
  double x, y, z, w;
};
__device__ __forceinline__ d4 widen(const float4 a) { return {(double)a.x, (double)a.y, (double)a.z, (double)a.w}; }
__device__ __forceinline__ f64x4 mfma16d(const d4 a, const d4 b, f64x4 c)
{
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a.z, b.z, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a.w, b.w, c, 0, 0, 0);
}
// max over the four lane groups of a column (lane ^ 16, lane ^ 32)
__device__ __forceinline__ double xgroup_max_f64(double v)
{
  v = fmax(v, __shfl_xor(v, 16, 64));
  return fmax(v, __shfl_xor(v, 32, 64));
}
// An fp32 tile (rows 4 g + r) that must line up with an fp64 tile (rows g + 4 r) takes its A rows in this order: lane c
// supplies row pi(c), so that register r of group g holds row pi(4 g + r) = g + 4 r.
__device__ __forceinline__ int pi16(const int c) { return (c >> 2) + 4 * (c & 3); }
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 add4(const float4 a, const float4 b)
{
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

struct Geo {
  int N, heads, Q, S;   // self-attention: S = Q
  size_t rs;            // floats between two rows of an operand: N * heads * 16
};
// the 16 floats per row of the workgroup's (image blockIdx.z, head blockIdx.y) in an operand [rows, N, heads * 16]
struct Head {
  size_t rs, hoff;
  __device__ __forceinline__ explicit Head(const Geo &geo)
  {
    const int h = blockIdx.y, n = blockIdx.z;
    rs = geo.rs;
    hoff = (size_t)n * geo.heads * 16 + (size_t)h * 16;
  }
  __device__ __forceinline__ size_t idx(const int row, const int dim) const { return row * rs + hoff + dim; }
  // float4 number g of a row: dims 4 g .. 4 g + 3
  __device__ __forceinline__ float4 row4(const float *p, const int row, const int g) const
  {
    return ld4(p + row * rs + hoff + 4 * g);
  }
};

// the two policies: the decoder's cross-attention (cross_attention_train.hip, attention_eval.hip) ...
struct Cross {
  static constexpr int HALVES = 2;
  static constexpr bool MASKED = true;
  static __device__ int keys(const Geo &geo) { return geo.S; }
};
// ... and its self-attention (self_attention_train.hip, attention_eval.hip)
struct Self {
  static constexpr int HALVES = 1;
  static constexpr bool MASKED = false;
  static __device__ int keys(const Geo &geo) { return geo.Q; }   // the keys are the queries: one register
};

// ---- operands and the score tile ------------------------------------------------------------------------------------------
template <class F>
struct Row {   // a lane's four dims of a query or key row, as the score takes them
  d4 h[F::HALVES];
};
struct RawRow {   // the same four dims as the two loads deliver them: what a wave can hold ahead of the arithmetic
  float4 a, b;
};
__device__ __forceinline__ RawRow load_raw(const float *a, const float *b, const Head &hd, const int row, const int g)
{
  return {hd.row4(a, row, g), hd.row4(b, row, g)};
}
template <class F>
__device__ __forceinline__ Row<F> cook(const RawRow &w)
{
  if constexpr (F::HALVES == 2) return {{widen(w.a), widen(w.b)}};
  else return {{widen(add4(w.a, w.b))}};
}
template <class F>
__device__ __forceinline__ Row<F> load_row(const float *a, const float *b, const Head &hd, const int row, const int g)
{
  return cook<F>(load_raw(a, b, hd, row, g));
}
// dim c of a row, one float per half: the A operand of the fp32 product that contracts over rows
template <class F>
__device__ __forceinline__ void load_col(const float *a, const float *b, const size_t at, float (&t)[F::HALVES])
{
  if constexpr (F::HALVES == 2) {
    t[0] = a[at];
    t[1] = b[at];
  } else {
    t[0] = a[at] + b[at];
  }
}
// the score / scale of 16 rows x against 16 rows y: register r is [row g + 4 r of x][row c of y]
template <class F>
__device__ __forceinline__ f64x4 score(const Row<F> &x, const Row<F> &y)
{
  const f64x4 zd = {0., 0., 0., 0.};
  // (two halves in accumulators of their own: two chains of four dependent instructions instead of one of eight)
  if constexpr (F::HALVES == 2) return mfma16d(x.h[0], y.h[0], zd) + mfma16d(x.h[1], y.h[1], zd);
  else return mfma16d(x.h[0], y.h[0], zd);
}

// the keys of one (image, head) as the query pass reads them: from global memory ...
template <class F>
struct GlobalKeys {
  static constexpr bool STAGED = false;
  const float *k_a, *k_b, *v;
  __device__ __forceinline__ Row<F> row(const Head &hd, const int key, const int g) const
  {
    return load_row<F>(k_a, k_b, hd, key, g);
  }
  __device__ __forceinline__ float4 vrow(const Head &hd, const int key, const int g) const { return hd.row4(v, key, g); }
  __device__ __forceinline__ void col(const Head &hd, const int key, const int c, float (&t)[F::HALVES]) const
  {
    load_col<F>(k_a, k_b, hd.idx(key, c), t);
  }
};
// ... or from an image [S][16] of the summed key and of v that the workgroup has written to LDS (no barrier yet)
template <class F>
struct LdsKeys {
  static_assert(F::HALVES == 1);
  static constexpr bool STAGED = true;
  const float *s_k, *s_v;
  __device__ __forceinline__ Row<F> row(const Head &, const int key, const int g) const
  {
    return {{widen(ld4(s_k + key * 16 + 4 * g))}};
  }
  __device__ __forceinline__ float4 vrow(const Head &, const int key, const int g) const { return ld4(s_v + key * 16 + 4 * g); }
  __device__ __forceinline__ void col(const Head &, const int key, const int c, float (&t)[1]) const { t[0] = s_k[key * 16 + c]; }
};

// a query's mask row, seen from the lane that owns the query
struct MaskRow {
  bool open;
  const unsigned char *row;
};
template <class F>
__device__ __forceinline__ MaskRow mask_row(const unsigned char *mask, const unsigned char *row_open, const int n, const int Q,
                                            const int S, const int q)
{
  if constexpr (F::MASKED)
    return {!mask || (row_open && row_open[(size_t)n * Q + q]), mask ? mask + ((size_t)n * Q + q) * S : nullptr};
  else
    return {true, nullptr};
}
template <class F>
__device__ __forceinline__ bool key_dead(const MaskRow &m, const int kk, const int S)
{
  if constexpr (F::MASKED) return kk >= S || (!m.open && m.row[kk] != 0);
  else return kk >= S;
}

// lse in two fp32 words (formed in fp64: fp32's logf alone is off by up to an ulp of a result near 8, 5e-7, and the sum is
// rounded once more -- as a relative error of every recomputed probability of the row)
__device__ __forceinline__ void write_lse(float *lse, const double e, const size_t at, const size_t lo_plane)
{
  const float hi = (float)e;
  lse[at] = hi;
  lse[lo_plane + at] = (float)(e - (double)hi);
}
__device__ __forceinline__ double read_lse(const float *lse, const size_t at, const size_t lo_plane)
{
  return (double)lse[at] + (double)lse[lo_plane + at];
}
// the backward's probability of element r of a score tile
__device__ __forceinline__ float prob(const f64x4 s, const int r, const double dscale, const double lse)
{
  return expf((float)(s[r] * dscale - lse));
}

// ---- forward --------------------------------------------------------------------------------------------------------------
// What a wave reads from memory for one 16-key step, unconverted: lane (c, g)'s four dims of key row k0 + c (both operands), dim
// c of the value rows k0 + g + 4 r and the mask bytes of those keys in the lane's query row.  Rows beyond S - 1 repeat row
// S - 1 and are dead in fwd_step; no address lies behind the last row.  A masked position's byte is read only where the row
// has a mask and is not open (key_dead's rule, taken at load time: mk[r] != 0 is "masked")
template <class F>
struct FwdTile {
  RawRow k;
  float va[4];
  unsigned char mk[4];
};
template <class F>
__device__ __forceinline__ FwdTile<F> fwd_load(const float *k_a, const float *k_b, const float *v, const Head &hd, const MaskRow &m,
                                               const int k0, const int S, const int c, const int g)
{
  FwdTile<F> t;
  t.k = load_raw(k_a, k_b, hd, min(k0 + c, S - 1), g);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kk = k0 + g + 4 * r;
    t.va[r] = v[hd.idx(min(kk, S - 1), c)];
    t.mk[r] = 0;
    if constexpr (F::MASKED)
      if (!m.open && kk < S) t.mk[r] = m.row[kk];
  }
  return t;
}
// a wave's running softmax of its steps: per lane the row maximum and row sum of query c, and O[query c][value dim 4 g + r]
struct FwdState {
  double m_run;
  float l_run;
  f32x4 o;
};
// one step of the online softmax on the tile at k0
template <class F>
__device__ __forceinline__ void fwd_step(FwdState &st, const FwdTile<F> &t, const Row<F> &qa, const int k0, const int S, const int g,
                                         const double dscale)
{
  const Row<F> ka = cook<F>(t.k);
  float p[4];
  double x[4];
  double mx = -INFINITY;
  const f64x4 s = score<F>(ka, qa);                                   // s[r] = score^T[key k0 + g + 4 r][query c] / scale
  bool dead[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dead[r] = k0 + g + 4 * r >= S || (F::MASKED && t.mk[r] != 0);
    x[r] = s[r] * dscale;
    mx = fmax(mx, dead[r] ? -INFINITY : x[r]);
  }
  mx = xgroup_max_f64(mx);                                            // not MASKED: finite, key k0 exists
  const double m_new = fmax(st.m_run, mx);
  double m_safe = m_new;
  if constexpr (F::MASKED) m_safe = m_new == -INFINITY ? 0. : m_new;     // nothing attendable yet: keep everything 0
  const float alpha = expf((float)(st.m_run - m_safe));               // exp(-inf) = 0 on the first live step
  float rsum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    p[r] = dead[r] ? 0.f : expf((float)(x[r] - m_safe));
    rsum += p[r];
  }
  rsum = xgroup_sum(rsum);
  st.l_run = fmaf(st.l_run, alpha, rsum);                            // (fused by name, here and in the merge: see attn_fwd)
  st.m_run = m_new;
#pragma unroll
  for (int r = 0; r < 4; ++r) st.o[r] *= alpha;
#pragma unroll
  for (int r = 0; r < 4; ++r) st.o = mfma4(t.va[r], p[r], st.o);      // o[r] = O[query c][value dim 4 g + r]
}

// LSE: the row statistics are written for a backward (training).  AHEAD: the wave issues the loads of its next step before the
// arithmetic of the current one and keeps that one FwdTile in registers (evaluation: thousands of keys, 89 steps a wave at 5 655,
// each of which would otherwise begin with its own trip to memory).  Neither changes an operation on the way to `out`: the
// two forms give the same bits.  Every multiply-add of the forward is an fmaf by name: left to the compiler, whether a
// product and a sum are fused is decided per instantiation (with lse to form, the merge's came out as v_pk_mul_f32 and adds;
// without, as v_pk_fma_f32 -- one ulp apart).
template <class F, bool LSE, bool AHEAD>
__device__ __forceinline__ void attn_fwd(const float *q_a, const float *q_b, const float *k_a, const float *k_b, const float *v,
                                         const unsigned char *mask, const unsigned char *row_open, const Geo geo,
                                         const float scale, float *out, float *lse)
{
  __shared__ double s_m[AT_WAVES][16];
  __shared__ float s_l[AT_WAVES][16], s_o[AT_WAVES][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = F::keys(geo);
  const Head hd(geo);
  const int q = min(q0 + c, Q - 1);                                   // (a tile's surplus columns repeat the last query)
  const Row<F> qa = load_row<F>(q_a, q_b, hd, q, g);
  const MaskRow m = mask_row<F>(mask, row_open, n, Q, S, q);
  const double dscale = (double)scale;
  constexpr int STEP = 16 * AT_WAVES;

  FwdState st = {-INFINITY, 0.f, {0.f, 0.f, 0.f, 0.f}};
  if constexpr (AHEAD) {
    int k0 = wave * 16;
    if (k0 < S) {
      FwdTile<F> cur = fwd_load<F>(k_a, k_b, v, hd, m, k0, S, c, g);
      for (; k0 + STEP < S; k0 += STEP) {
        const FwdTile<F> nxt = fwd_load<F>(k_a, k_b, v, hd, m, k0 + STEP, S, c, g);   // in flight during the step below
        fwd_step<F>(st, cur, qa, k0, S, g, dscale);
        cur = nxt;
      }
      fwd_step<F>(st, cur, qa, k0, S, g, dscale);                     // the wave's last step: nothing is loaded behind it
    }
  } else {
    for (int k0 = wave * 16; k0 < S; k0 += STEP) fwd_step<F>(st, fwd_load<F>(k_a, k_b, v, hd, m, k0, S, c, g), qa, k0, S, g, dscale);
  }

  if (g == 0) {
    s_m[wave][c] = st.m_run;
    s_l[wave][c] = st.l_run;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) s_o[wave][c][4 * g + r] = st.o[r];
  __syncthreads();
  // the four waves' partial softmaxes, merged in wave order: thread (query tq, value dim td).  A wave without a live step holds
  // (-inf, 0, 0) and enters with the factor exp(-inf) = 0; not MASKED, wave 0 always has a key and the maximum is finite
  const int tq = threadIdx.x >> 4, td = threadIdx.x & 15;
  double mm = -INFINITY;
#pragma unroll
  for (int w = 0; w < AT_WAVES; ++w) mm = fmax(mm, s_m[w][tq]);
  float l = 0.f, acc = 0.f;
  if (!F::MASKED || mm != -INFINITY) {
#pragma unroll
    for (int w = 0; w < AT_WAVES; ++w) {
      const float f = expf((float)(s_m[w][tq] - mm));
      l = fmaf(s_l[w][tq], f, l);
      acc = fmaf(s_o[w][tq][td], f, acc);
    }
  }
  if (q0 + tq < Q) {
    const bool live = !F::MASKED || l > 0.f;
    out[hd.idx(q0 + tq, td)] = live ? acc / l : 0.f;
    if constexpr (LSE) {
      if (td == 0) {
        const double e = live ? mm + log((double)l) : 0.0;
        write_lse(lse, e, ((size_t)n * geo.heads + h) * Q + q0 + tq, (size_t)geo.N * geo.heads * Q);
      }
    }
  }
}

// ---- backward, query pass: D to `delta` (sweep D) and/or grad_q (sweep DQ, on the D it formed or reads from `delta`) ----------
template <class F, bool D, bool DQ, class Keys>
__device__ __forceinline__ void attn_bwd_q(const float *q_a, const float *q_b, const Keys keys, const unsigned char *mask,
                                           const unsigned char *row_open, const float *lse, const float *grad_out, const Geo geo,
                                           const float scale, std::conditional_t<D, float, const float> *delta, float *grad_q_a,
                                           float *grad_q_b)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = F::keys(geo);
  const Head hd(geo);
  const int q = min(q0 + c, Q - 1);
  const Row<F> qa = load_row<F>(q_a, q_b, hd, q, g);
  const float4 doa = hd.row4(grad_out, q, g);
  const size_t stat = ((size_t)n * geo.heads + h) * Q + q;
  const double lse_q = read_lse(lse, stat, (size_t)geo.N * geo.heads * Q), dscale = (double)scale;
  float d_q = 0.f;
  if constexpr (!D) d_q = delta[stat];
  const MaskRow m = mask_row<F>(mask, row_open, n, Q, S, q);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if constexpr (Keys::STAGED) __syncthreads();                        // the LDS image is complete (the loads above overlap its writes)

  if constexpr (D) {
    __shared__ double s_sum[AT_WAVES][16];
    double sum = 0.;
    for (int k0 = wave * 16; k0 < S; k0 += 16 * AT_WAVES) {
      const Row<F> ka = keys.row(hd, min(k0 + c, S - 1), g);
      const float4 va = keys.vrow(hd, min(k0 + pi16(c), S - 1), g);
      const f64x4 s = score<F>(ka, qa);                               // score^T[key k0 + g + 4 r][query c] / scale
      const f32x4 dp = mfma16(va, doa, z);                            // dP^T[key k0 + g + 4 r][query] = v[key] . grad_out[query]
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool dead = key_dead<F>(m, k0 + g + 4 * r, S);
        const float p = prob(s, r, dscale, lse_q);
        sum += dead ? 0. : (double)p * (double)dp[r];
      }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (g == 0) s_sum[wave][c] = sum;
    __syncthreads();
    const auto d_of = [&](const int col) {                            // the four waves' sums in wave order, rounded once
      double d = 0.;
#pragma unroll
      for (int w = 0; w < AT_WAVES; ++w) d += s_sum[w][col];
      return (float)d;
    };
    const bool writer = threadIdx.x < 16 && q0 + (int)threadIdx.x < Q;
    if constexpr (DQ) {                                               // every lane needs its query's D: what the key pass reads back
      d_q = d_of(c);
      if (writer) delta[stat] = d_q;
    } else if (writer) {
      delta[((size_t)n * geo.heads + h) * Q + q0 + threadIdx.x] = d_of(threadIdx.x);
    }
  }

  if constexpr (DQ) {
    __shared__ float s_d[AT_WAVES][F::HALVES][16][17];
    f32x4 dq[F::HALVES] = {};
    for (int k0 = wave * 16; k0 < S; k0 += 16 * AT_WAVES) {
      const Row<F> ka = keys.row(hd, min(k0 + c, S - 1), g);
      const float4 va = keys.vrow(hd, min(k0 + pi16(c), S - 1), g);
      float kt[4][F::HALVES], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) keys.col(hd, min(k0 + g + 4 * r, S - 1), c, kt[r]);
      const f64x4 s = score<F>(ka, qa);
      const f32x4 dp = mfma16(va, doa, z);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool dead = key_dead<F>(m, k0 + g + 4 * r, S);
        const float p = prob(s, r, dscale, lse_q);
        ds[r] = dead ? 0.f : p * (dp[r] - d_q);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)                                     // dq^T[dim c][query] += k^T[dim c][key] dS^T[key][query]
#pragma unroll
        for (int hf = 0; hf < F::HALVES; ++hf) dq[hf] = mfma4(kt[r][hf], ds[r], dq[hf]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)                                       // register r: dq[query c][dim 4 g + r]
#pragma unroll
      for (int hf = 0; hf < F::HALVES; ++hf) s_d[wave][hf][c][4 * g + r] = dq[hf][r];
    __syncthreads();
    const int tq = threadIdx.x >> 4, td = threadIdx.x & 15;
    if (q0 + tq < Q) {
      float a[F::HALVES] = {};
#pragma unroll
      for (int w = 0; w < AT_WAVES; ++w)
#pragma unroll
        for (int hf = 0; hf < F::HALVES; ++hf) a[hf] += s_d[w][hf][tq][td];
      grad_q_a[hd.idx(q0 + tq, td)] = a[0] * scale;
      if constexpr (F::HALVES == 2) grad_q_b[hd.idx(q0 + tq, td)] = a[1] * scale;
    }
  }
}

// ---- backward, key pass: grad_k per half, grad_v ------------------------------------------------------------------------------
template <class F>
__device__ __forceinline__ void attn_bwd_k(const float *q_a, const float *q_b, const float *k_a, const float *k_b, const float *v,
                                           const unsigned char *mask, const unsigned char *row_open, const float *lse,
                                           const float *delta, const float *grad_out, const Geo geo, const float scale,
                                           float *grad_k_a, float *grad_k_b, float *grad_v)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int k0 = (blockIdx.x * AT_WAVES + wave) * 16, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = F::keys(geo);
  if (k0 >= S) return;                                                // (whole waves; the pass has no barrier)
  const Head hd(geo);
  const size_t stat = ((size_t)n * geo.heads + h) * Q, lo_plane = (size_t)geo.N * geo.heads * Q;
  const bool key_ok = k0 + c < S;
  const int key = min(k0 + c, S - 1);
  const Row<F> ka = load_row<F>(k_a, k_b, hd, key, g);
  const float4 va = hd.row4(v, key, g);
  const double dscale = (double)scale;

  f32x4 dk[F::HALVES] = {}, dv = {0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < Q; q0 += 16) {
    const Row<F> qa = load_row<F>(q_a, q_b, hd, min(q0 + c, Q - 1), g);
    const float4 doa = hd.row4(grad_out, min(q0 + pi16(c), Q - 1), g);
    float qt[4][F::HALVES], dot[4], p[4], ds[4];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f64x4 s = score<F>(qa, ka);                                 // score[query q0 + g + 4 r][key c] / scale
    const f32x4 dp = mfma16(doa, va, z);                              // dP[query q0 + g + 4 r][key]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qq = q0 + g + 4 * r, qr = min(qq, Q - 1);
      const size_t at = hd.idx(qr, c);
      load_col<F>(q_a, q_b, at, qt[r]);
      dot[r] = grad_out[at];
      bool masked = false;
      if constexpr (F::MASKED)
        masked = mask && !(row_open && row_open[(size_t)n * Q + qr]) && mask[((size_t)n * Q + qr) * S + key] != 0;
      const bool dead = qq >= Q || !key_ok || masked;
      const float e = prob(s, r, dscale, read_lse(lse, stat + qr, lo_plane));
      p[r] = dead ? 0.f : e;
      ds[r] = dead ? 0.f : e * (dp[r] - delta[stat + qr]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                     // X^T[dim c][key] += Y^T[dim c][query] Z[query][key]
      dv = mfma4(dot[r], p[r], dv);
#pragma unroll
      for (int hf = 0; hf < F::HALVES; ++hf) dk[hf] = mfma4(qt[r][hf], ds[r], dk[hf]);
    }
  }
  if (key_ok) {                                                       // register r: row `key`, dim 4 g + r
    const size_t at = hd.idx(key, 4 * g);
    *reinterpret_cast<float4 *>(grad_v + at) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    float *const grad_k[2] = {grad_k_a, grad_k_b};
#pragma unroll
    for (int hf = 0; hf < F::HALVES; ++hf)
      *reinterpret_cast<float4 *>(grad_k[hf] + at) = make_float4(dk[hf][0] * scale, dk[hf][1] * scale, dk[hf][2] * scale, dk[hf][3] * scale);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// heads 4 or 8 (what the decoder builds); at most max_q queries; a tensor's element count below 2^31 (offsets are formed in 64
// bits; the bound keeps the grid's z extent and the row arithmetic far from their limits)
inline bool attn_train_covered(const int N, const int heads, const int Q, const int S, const int max_q = INT_MAX)
{
  if (heads != 4 && heads != 8) return false;
  if (N > 65535 || Q > max_q) return false;
  const long long lim = 0x7fffffffLL, rs = (long long)N * heads * 16;
  return (long long)Q * rs < lim && (long long)S * rs < lim;
}
inline Geo attn_geo(const int N, const int heads, const int Q, const int S) { return {N, heads, Q, S, (size_t)N * heads * 16}; }
// forward and query pass: a workgroup per 16 queries; key pass: a wave per 16 keys
inline dim3 query_grid(const Geo &geo) { return dim3((geo.Q + 15) / 16, geo.heads, geo.N); }
inline dim3 key_grid(const Geo &geo) { return dim3((geo.S + 16 * AT_WAVES - 1) / (16 * AT_WAVES), geo.heads, geo.N); }

}  // namespace
}  // namespace pct
