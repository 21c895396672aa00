// Differentiable fp32 cross-attention of the decoder with the keys of a workgroup divided over several workgroups
// (include/pctrans_hip_attn_train_split.h): cross_attention_train.hip for the key counts at which its query-side kernels leave
// most of the device idle -- 16 queries of one (image, head) per workgroup, every workgroup walking all keys: 112 workgroups of
// 49 dependent steps per wave at 100 queries, 2 images and 3 136 keys.  The arithmetic of a step, the register layouts and the
// policies are those of attn_train_common.hpp (fwd_load, fwd_step, score, prob, Head, MaskRow, key_dead, the wave merges); this file
// restricts the forward and the two sweeps of the query pass to a key range and adds what joins the ranges again.
//
// Key ranges.  The unit is a chunk of 64 keys, one 16-key step of each of the four waves; C = ceil(S / 64).  Split j of `splits`
// owns the chunks [j C / splits, (j + 1) C / splits), and inside its range wave w walks the steps w, w + 4, ... of the range: ranges
// begin at multiples of four steps, so these are a subsequence of the steps that wave walks in the unsplit kernel.  The
// launchers use min(splits, C) splits, so no range is empty.
//
// Forward, 2 launches:
//   xats_fwd_kernel      grid (ceil(Q / 16) * splits, heads, N): the unsplit forward up to and including the four-wave merge on
//                        the range; per (split, image, head, query) the merged maximum (fp64), the merged row sum l (fp32) and the
//                        16 unnormalised sums (fp32) go to the workspace.  Nothing attendable in the range: (-inf, 0, 0 ...)
//   xats_fwd_combine     thread = (query, value dim): M = max_j m_j; l = sum_j l_j exp(m_j - M) and acc likewise, over the splits
//                        in ascending order in fp64 (fma by name), each rounded once to fp32; out = acc / l in fp32 as attn_fwd;
//                        lse = M + log(l) from the fp64 sum, in write_lse's two planes.  Every split at -inf: out = 0, lse = 0
// Backward, 4 launches:
//   xats_delta_kernel    sweep D on the range: the four waves' fp64 sums added in wave order, written as fp64 per (split, row)
//   xats_bwd_q_kernel    D of a row = the splits' fp64 partials added in ascending order, rounded once to fp32 (every workgroup
//                        forms it for its 16 queries; the workgroups of split 0 write it to `delta`); then sweep DQ on the range:
//                        the four waves' dq added in wave order, unscaled, to the workspace
//   xats_bwd_k_kernel    attn_bwd_k<Cross> as it is, on lse and `delta` (launched after xats_bwd_q_kernel, which writes `delta`)
//   xats_dq_combine      grad_q = (0 + the splits' dq in ascending order) * scale
// No floating-point atomic, no counter: plain launches in a fixed order; two calls give the same bits.
//
// What follows from the construction (tests/test_split_key_attention_train_gpu.py):
//   splits == 1           every result has the bits of cross_attention_train.hip: one term with the factor exp(0) = 1, sums that
//                         start from 0, and an fp64 round trip of fp32 values
//   any splits            a query whose live keys all lie in one split's range has the unsplit kernels' out, lse, D and grad_q:
//                         the other splits enter with the factor exp(-inf) = 0 or with exact zeros
//
// Workspace (cross_attention_split_train_workspace), R = N * heads * Q rows, sp = the requested splits:
//   forward    double m[sp][R] | float l[sp][R] | float acc[sp][R][16]                      76 sp R bytes
//   backward   double d[sp][R] | float delta[R] (padded to 16 bytes) | float dq[sp][R][2][16]   136 sp R + 4 R bytes: the need
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_train_common.hpp"
#include "launchers.hpp"

namespace pct {
namespace {

constexpr int XS_CHUNK = 16 * AT_WAVES;   // keys per chunk
constexpr int XS_MAX_SPLITS = 16;
constexpr int XS_CT = 256;                // threads of a combine workgroup: 16 rows of 16 dims

struct KeyRange {
  int begin, end;   // keys [begin, end); begin a multiple of XS_CHUNK, end one or S
};
__device__ __forceinline__ KeyRange key_range(const int S, const int j, const int splits)
{
  const int nch = (S + XS_CHUNK - 1) / XS_CHUNK;
  return {j * nch / splits * XS_CHUNK, min((j + 1) * nch / splits * XS_CHUNK, S)};
}
// a workgroup's query tile and split: blockIdx.x = tile * splits + split
struct TileSplit {
  int q0, j;
  __device__ __forceinline__ explicit TileSplit(const int splits)
  {
    const int tile = blockIdx.x / splits;
    q0 = tile * 16;
    j = blockIdx.x - tile * splits;
  }
};
struct BwdWs {
  double *d;      // [splits][R]
  float *delta;   // [R]
  float *dq;      // [splits][R][2][16]
};

// ---- forward ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AT_THREADS) void xats_fwd_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                               const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                               const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                               const unsigned char *__restrict__ row_open, const Geo geo,
                                                               const float scale, const int splits, double *__restrict__ ws_m,
                                                               float *__restrict__ ws_l, float *__restrict__ ws_acc)
{
  using F = Cross;
  __shared__ double s_m[AT_WAVES][16];
  __shared__ float s_l[AT_WAVES][16], s_o[AT_WAVES][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const TileSplit ts(splits);
  const int q0 = ts.q0, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = F::keys(geo);
  const Head hd(geo);
  const int q = min(q0 + c, Q - 1);
  const Row<F> qa = load_row<F>(q_c, q_s, hd, q, g);
  const MaskRow m = mask_row<F>(mask, row_open, n, Q, S, q);
  const double dscale = (double)scale;
  const KeyRange kr = key_range(S, ts.j, splits);

  FwdState st = {-INFINITY, 0.f, {0.f, 0.f, 0.f, 0.f}};
  for (int k0 = kr.begin + wave * 16; k0 < kr.end; k0 += XS_CHUNK)
    fwd_step<F>(st, fwd_load<F>(k_c, k_p, v, hd, m, k0, S, c, g), qa, k0, S, g, dscale);

  if (g == 0) {
    s_m[wave][c] = st.m_run;
    s_l[wave][c] = st.l_run;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) s_o[wave][c][4 * g + r] = st.o[r];
  __syncthreads();
  // attn_fwd's merge of the four waves in wave order: thread (query tq, value dim td)
  const int tq = threadIdx.x >> 4, td = threadIdx.x & 15;
  double mm = -INFINITY;
#pragma unroll
  for (int w = 0; w < AT_WAVES; ++w) mm = fmax(mm, s_m[w][tq]);
  float l = 0.f, acc = 0.f;
  if (mm != -INFINITY) {
#pragma unroll
    for (int w = 0; w < AT_WAVES; ++w) {
      const float f = expf((float)(s_m[w][tq] - mm));
      l = fmaf(s_l[w][tq], f, l);
      acc = fmaf(s_o[w][tq][td], f, acc);
    }
  }
  if (q0 + tq < Q) {
    const size_t rows = (size_t)geo.N * geo.heads * Q;
    const size_t at = ts.j * rows + ((size_t)n * geo.heads + h) * Q + q0 + tq;
    if (td == 0) {
      ws_m[at] = mm;
      ws_l[at] = l;
    }
    ws_acc[at * 16 + td] = acc;
  }
}

__global__ __launch_bounds__(XS_CT) void xats_fwd_combine(const Geo geo, const int splits, const double *__restrict__ ws_m,
                                                           const float *__restrict__ ws_l, const float *__restrict__ ws_acc,
                                                           float *__restrict__ out, float *__restrict__ lse)
{
  const size_t rows = (size_t)geo.N * geo.heads * geo.Q;
  const size_t row = (size_t)blockIdx.x * (XS_CT / 16) + (threadIdx.x >> 4);
  const int td = threadIdx.x & 15;
  if (row >= rows) return;
  const int q = (int)(row % geo.Q);
  const size_t nh = row / geo.Q;                                       // n * heads + h
  double M = -INFINITY;
  for (int j = 0; j < splits; ++j) M = fmax(M, ws_m[j * rows + row]);
  float o = 0.f;
  double e = 0.;
  if (M != -INFINITY) {
    double L = 0., A = 0.;
    for (int j = 0; j < splits; ++j) {
      const size_t at = j * rows + row;
      const double f = exp(ws_m[at] - M);                              // exp(-inf) = 0: a split without a live key for the row
      L = fma((double)ws_l[at], f, L);
      A = fma((double)ws_acc[at * 16 + td], f, A);
    }
    o = (float)A / (float)L;
    e = M + log(L);
  }
  out[(size_t)q * geo.rs + nh * 16 + td] = o;
  if (td == 0) write_lse(lse, e, row, rows);
}

// ---- backward, query side -------------------------------------------------------------------------------------------------------
// sweep D of attn_bwd_q on the workgroup's key range: the fp64 sum of the row, not yet rounded
__global__ __launch_bounds__(AT_THREADS) void xats_delta_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                 const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                 const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                 const unsigned char *__restrict__ row_open,
                                                                 const float *__restrict__ lse, const float *__restrict__ grad_out,
                                                                 const Geo geo, const float scale, const int splits,
                                                                 double *__restrict__ ws_d)
{
  using F = Cross;
  __shared__ double s_sum[AT_WAVES][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const TileSplit ts(splits);
  const int q0 = ts.q0, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = F::keys(geo);
  const Head hd(geo);
  const GlobalKeys<F> keys = {k_c, k_p, v};
  const int q = min(q0 + c, Q - 1);
  const Row<F> qa = load_row<F>(q_c, q_s, hd, q, g);
  const float4 doa = hd.row4(grad_out, q, g);
  const size_t rows = (size_t)geo.N * geo.heads * Q, stat = ((size_t)n * geo.heads + h) * Q + q;
  const double lse_q = read_lse(lse, stat, rows), dscale = (double)scale;
  const MaskRow m = mask_row<F>(mask, row_open, n, Q, S, q);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const KeyRange kr = key_range(S, ts.j, splits);

  double sum = 0.;
  for (int k0 = kr.begin + wave * 16; k0 < kr.end; k0 += XS_CHUNK) {
    const Row<F> ka = keys.row(hd, min(k0 + c, S - 1), g);
    const float4 va = keys.vrow(hd, min(k0 + pi16(c), S - 1), g);
    const f64x4 s = score<F>(ka, qa);
    const f32x4 dp = mfma16(va, doa, z);
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
  if (threadIdx.x < 16 && q0 + (int)threadIdx.x < Q) {
    double d = 0.;
#pragma unroll
    for (int w = 0; w < AT_WAVES; ++w) d += s_sum[w][threadIdx.x];
    ws_d[ts.j * rows + ((size_t)n * geo.heads + h) * Q + q0 + threadIdx.x] = d;
  }
}

// D from the splits' partial sums, then sweep DQ of attn_bwd_q on the workgroup's key range
__global__ __launch_bounds__(AT_THREADS) void xats_bwd_q_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                 const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                 const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                 const unsigned char *__restrict__ row_open,
                                                                 const float *__restrict__ lse, const float *__restrict__ grad_out,
                                                                 const Geo geo, const float scale, const int splits, const BwdWs ws)
{
  using F = Cross;
  __shared__ float s_d[AT_WAVES][F::HALVES][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const TileSplit ts(splits);
  const int q0 = ts.q0, h = blockIdx.y, n = blockIdx.z;
  const int Q = geo.Q, S = F::keys(geo);
  const Head hd(geo);
  const GlobalKeys<F> keys = {k_c, k_p, v};
  const int q = min(q0 + c, Q - 1);
  const Row<F> qa = load_row<F>(q_c, q_s, hd, q, g);
  const float4 doa = hd.row4(grad_out, q, g);
  const size_t rows = (size_t)geo.N * geo.heads * Q, stat = ((size_t)n * geo.heads + h) * Q + q;
  const double lse_q = read_lse(lse, stat, rows), dscale = (double)scale;
  double d = 0.;
  for (int j = 0; j < splits; ++j) d += ws.d[j * rows + stat];
  const float d_q = (float)d;
  if (ts.j == 0 && threadIdx.x < 16 && q0 + (int)threadIdx.x < Q) ws.delta[stat] = d_q;   // (lanes 0 .. 15: q = q0 + lane)
  const MaskRow m = mask_row<F>(mask, row_open, n, Q, S, q);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const KeyRange kr = key_range(S, ts.j, splits);

  f32x4 dq[F::HALVES] = {};
  for (int k0 = kr.begin + wave * 16; k0 < kr.end; k0 += XS_CHUNK) {
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
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int hf = 0; hf < F::HALVES; ++hf) dq[hf] = mfma4(kt[r][hf], ds[r], dq[hf]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
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
    float *const to = ws.dq + (ts.j * rows + ((size_t)n * geo.heads + h) * Q + q0 + tq) * (16 * F::HALVES);
#pragma unroll
    for (int hf = 0; hf < F::HALVES; ++hf) to[16 * hf + td] = a[hf];
  }
}

__global__ __launch_bounds__(XS_CT) void xats_dq_combine(const Geo geo, const float scale, const int splits,
                                                          const float *__restrict__ ws_dq, float *__restrict__ grad_q_c,
                                                          float *__restrict__ grad_q_s)
{
  const size_t rows = (size_t)geo.N * geo.heads * geo.Q;
  const size_t row = (size_t)blockIdx.x * (XS_CT / 16) + (threadIdx.x >> 4);
  const int td = threadIdx.x & 15;
  if (row >= rows) return;
  const int q = (int)(row % geo.Q);
  const size_t nh = row / geo.Q;
  float a[2] = {0.f, 0.f};
  for (int j = 0; j < splits; ++j)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) a[hf] += ws_dq[(j * rows + row) * 32 + 16 * hf + td];
  const size_t at = (size_t)q * geo.rs + nh * 16 + td;
  grad_q_c[at] = a[0] * scale;
  grad_q_s[at] = a[1] * scale;
}

// ---- backward, key side: the unsplit pass ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(AT_THREADS) void xats_bwd_k_kernel(const float *__restrict__ q_c, const float *__restrict__ q_s,
                                                                 const float *__restrict__ k_c, const float *__restrict__ k_p,
                                                                 const float *__restrict__ v, const unsigned char *__restrict__ mask,
                                                                 const unsigned char *__restrict__ row_open,
                                                                 const float *__restrict__ lse, const float *__restrict__ delta,
                                                                 const float *__restrict__ grad_out, const Geo geo, const float scale,
                                                                 float *__restrict__ grad_k_c, float *__restrict__ grad_k_p,
                                                                 float *__restrict__ grad_v)
{
  attn_bwd_k<Cross>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, delta, grad_out, geo, scale, grad_k_c, grad_k_p, grad_v);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline long long round16(const long long b) { return (b + 15) / 16 * 16; }
inline int used_splits(const int S, const int splits) { return min(splits, (S + XS_CHUNK - 1) / XS_CHUNK); }
inline dim3 split_grid(const Geo &geo, const int splits) { return dim3((geo.Q + 15) / 16 * splits, geo.heads, geo.N); }
inline unsigned combine_blocks(const Geo &geo) { return (unsigned)(((long long)geo.N * geo.heads * geo.Q + XS_CT / 16 - 1) / (XS_CT / 16)); }
// PCT_OK, or why the launchers refuse `splits` and the workspace
inline int split_args(const int N, const int heads, const int Q, const int splits, const void *workspace, const long long workspace_bytes)
{
  if (splits < 1 || splits > XS_MAX_SPLITS || !workspace) return PCT_ERR_BAD_ARG;
  if (workspace_bytes < cross_attention_split_train_workspace(N, heads, Q, splits)) return PCT_ERR_BAD_ARG;
  return ((uintptr_t)workspace & 15u) ? PCT_ERR_ALIGNMENT : PCT_OK;
}

}  // namespace

long long cross_attention_split_train_workspace(int N, int heads, int Q, int splits)
{
  const long long rows = (long long)N * heads * Q;
  return round16(8 * splits * rows + round16(4 * rows) + 128 * splits * rows);
}

int launch_cross_attention_split_fwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                         const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S,
                                         float scale, int splits, void *workspace, long long workspace_bytes, float *out,
                                         float *lse, hipStream_t stream)
{
  if (!attn_train_covered(N, heads, Q, S)) return PCT_NOT_COVERED;
  const int bad = split_args(N, heads, Q, splits, workspace, workspace_bytes);
  if (bad != PCT_OK) return bad;
  const Geo geo = attn_geo(N, heads, Q, S);
  const int sp = used_splits(S, splits);
  const size_t rows = (size_t)N * heads * Q;
  double *const ws_m = static_cast<double *>(workspace);
  float *const ws_l = reinterpret_cast<float *>(ws_m + sp * rows), *const ws_acc = ws_l + sp * rows;
  xats_fwd_kernel<<<split_grid(geo, sp), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, geo, scale, sp, ws_m, ws_l,
                                                                  ws_acc);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  xats_fwd_combine<<<combine_blocks(geo), XS_CT, 0, stream>>>(geo, sp, ws_m, ws_l, ws_acc, out, lse);
  return (int)hipGetLastError();
}

int launch_cross_attention_split_bwd_f32(const float *q_c, const float *q_s, const float *k_c, const float *k_p, const float *v,
                                         const unsigned char *mask, const unsigned char *row_open, const float *lse,
                                         const float *grad_out, int N, int heads, int Q, int S, float scale, int splits,
                                         void *workspace, long long workspace_bytes, float *grad_q_c, float *grad_q_s,
                                         float *grad_k_c, float *grad_k_p, float *grad_v, hipStream_t stream)
{
  if (!attn_train_covered(N, heads, Q, S)) return PCT_NOT_COVERED;
  const int bad = split_args(N, heads, Q, splits, workspace, workspace_bytes);
  if (bad != PCT_OK) return bad;
  const Geo geo = attn_geo(N, heads, Q, S);
  const int sp = used_splits(S, splits);
  const size_t rows = (size_t)N * heads * Q;
  BwdWs ws;
  ws.d = static_cast<double *>(workspace);
  ws.delta = reinterpret_cast<float *>(ws.d + sp * rows);
  ws.dq = ws.delta + round16(4 * (long long)rows) / 4;
  xats_delta_kernel<<<split_grid(geo, sp), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, grad_out, geo, scale,
                                                                    sp, ws.d);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  xats_bwd_q_kernel<<<split_grid(geo, sp), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, grad_out, geo, scale,
                                                                    sp, ws);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  xats_bwd_k_kernel<<<key_grid(geo), AT_THREADS, 0, stream>>>(q_c, q_s, k_c, k_p, v, mask, row_open, lse, ws.delta, grad_out, geo,
                                                              scale, grad_k_c, grad_k_p, grad_v);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  xats_dq_combine<<<combine_blocks(geo), XS_CT, 0, stream>>>(geo, scale, sp, ws.dq, grad_q_c, grad_q_s);
  return (int)hipGetLastError();
}

}  // namespace pct
