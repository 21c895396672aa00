// Backward of MSDeformAttn with the module front-end fused in (pct_ms_deform_attn_fused_backward_f32,
// include/pctrans_hip_msda_train.h): two small kernels around the routed backward of msda_route.hip.
//
//   expand   offsets, logits, reference points  ->  workspace: sampling locations [R][L*P][2] and softmax weights [R][L*P]
//   (routed backward at the workspace's locations and weights; its grad_sampling_loc / grad_attn_weight land in the
//    caller's grad_offsets / grad_logits buffers)
//   fold     in place:  grad_offsets = gloc / (W_l, H_l),  grad_logits = w * (gw - sum_k w_k gw_k)
//
// R = batch * num_query * heads (image, query, head) records.  Both kernels are bound by their bytes, so every global access
// is a 16-byte one on consecutive addresses: a workgroup is one wave that owns 64 consecutive records, i.e. one contiguous
// span of each tensor.  The two reductions over a record (softmax, the weighted sum of gw) are done one record per lane; the
// span goes through LDS on its way from the line-covering loads to the lanes' rows.  A row is padded to an odd number of 16-byte
// slots: the 16 lanes of a ds_read_b128 group then sit on 16 different slots of the 256-byte bank row.  The location
// arithmetic has no reduction and stays element-wise on the 16-byte pieces (two (x, y) points of one level: P is even).
// The last workgroup may hold fewer than 64 records.
//
// Arithmetic: the exact formulation of the torch chain (expf, IEEE division and addition), not the forward kernels' exp2 / rcp.
#include <math.h>

#include "launchers.hpp"
#include "msda_common.hpp"

namespace pct {

namespace {

constexpr int FB_RECS = 64;         // records per workgroup = lanes of its one wave
constexpr int FB_MAX_POINTS = 64;   // L * P of a record
constexpr int FB_MAX_LEVELS = 32;   // ... with P >= 2

using f4 = vec_t<float, 4>;

// 16-byte slots per record row in LDS: odd
__host__ __device__ inline int fb_row_slots(int c4) { return c4 | 1; }

// (W_l, H_l) as floats, the divisors of the location arithmetic, and the level of each 16-byte piece of a record of (x, y)
// pairs: piece j holds points 2j and 2j + 1 of the record's L * P, both of level 2j / P
__device__ __forceinline__ void fb_stage_levels(float *wh, int *piece_level, const int64_t *shapes, int L, int P, int lane)
{
  if (lane < 2 * L) wh[lane] = (float)shapes[lane ^ 1];      // shapes[l] = (H, W)  ->  wh[l] = (W, H)
  if (lane < L * P / 2) piece_level[lane] = 2 * lane / P;
}

// nrec consecutive rows of c4 16-byte pieces: global span -> padded LDS rows, and back
__device__ __forceinline__ void fb_rows_in(f4 *rows, const f4 *span, int nrec, int c4, int lane)
{
  const int s4 = fb_row_slots(c4);
  for (int i = lane; i < nrec * c4; i += FB_RECS) {
    const int rec = i / c4;
    rows[rec * s4 + (i - rec * c4)] = span[i];
  }
}
__device__ __forceinline__ void fb_rows_out(f4 *span, const f4 *rows, int nrec, int c4, int lane)
{
  const int s4 = fb_row_slots(c4);
  for (int i = lane; i < nrec * c4; i += FB_RECS) {
    const int rec = i / c4;
    span[i] = rows[rec * s4 + (i - rec * c4)];
  }
}

__global__ __launch_bounds__(FB_RECS) void msda_fused_expand_kernel(const f4 *__restrict__ logits, const f4 *__restrict__ offsets,
                                                                   const float *__restrict__ ref, long long ref_batch_stride,
                                                                   const int64_t *__restrict__ shapes, long long R, int M, int Lq,
                                                                   int L, int P, f4 *__restrict__ loc, f4 *__restrict__ w)
{
  extern __shared__ f4 fb_lds[];
  __shared__ float wh[2 * FB_MAX_LEVELS];
  __shared__ int piece_level[FB_MAX_POINTS / 2];
  __shared__ long long ref_row[FB_RECS];                        // a record's reference points: offset of ref[image][query][0]
  const int lane = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * FB_RECS;
  const int nrec = (int)(R - r0 < FB_RECS ? R - r0 : FB_RECS);
  const int c4 = L * P / 4, s4 = fb_row_slots(c4);

  fb_stage_levels(wh, piece_level, shapes, L, P, lane);
  if (lane < nrec) {
    const long long q = (r0 + lane) / M;                        // image * Lq + query
    ref_row[lane] = (q / Lq) * ref_batch_stride + (q % Lq) * L * 2;
  }
  fb_rows_in(fb_lds, logits + r0 * c4, nrec, c4, lane);
  __syncthreads();
  if (lane < nrec) {                                            // softmax over the record, as torch forms it: exp(x - max) / sum
    f4 *row = fb_lds + lane * s4;
    float m = -INFINITY;
    for (int k = 0; k < c4; ++k) {
      const f4 x = row[k];
      m = fmaxf(fmaxf(m, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
    }
    float s = 0.f;
    for (int k = 0; k < c4; ++k) {
      f4 x = row[k];
      x.x = expf(x.x - m), x.y = expf(x.y - m), x.z = expf(x.z - m), x.w = expf(x.w - m);
      s += (x.x + x.y) + (x.z + x.w);
      row[k] = x;
    }
    for (int k = 0; k < c4; ++k) {
      f4 x = row[k];
      x.x /= s, x.y /= s, x.z /= s, x.w /= s;
      row[k] = x;
    }
  }
  __syncthreads();
  fb_rows_out(w + r0 * c4, fb_lds, nrec, c4, lane);

  // loc = ref + offsets / (W_l, H_l), element-wise on the 16-byte pieces
  const int c2 = 2 * c4;
  const f4 *off = offsets + r0 * c2;
  f4 *lo = loc + r0 * c2;
  for (int i = lane; i < nrec * c2; i += FB_RECS) {
    const int rec = i / c2, l = piece_level[i - rec * c2];
    const float *rp = ref + ref_row[rec] + 2 * l;
    const float rx = rp[0], ry = rp[1], W = wh[2 * l], H = wh[2 * l + 1];
    f4 o = off[i];
    o.x = rx + o.x / W, o.y = ry + o.y / H, o.z = rx + o.z / W, o.w = ry + o.w / H;
    lo[i] = o;
  }
}

// In place on the routed backward's results: every record is read whole (into LDS) before any of it is stored, and no other
// workgroup touches it.
__global__ __launch_bounds__(FB_RECS) void msda_fused_fold_kernel(const f4 *__restrict__ w, const int64_t *__restrict__ shapes,
                                                                 long long R, int L, int P, f4 *grad_offsets, f4 *grad_logits)
{
  extern __shared__ f4 fb_lds[];
  __shared__ float wh[2 * FB_MAX_LEVELS];
  __shared__ int piece_level[FB_MAX_POINTS / 2];
  const int lane = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * FB_RECS;
  const int nrec = (int)(R - r0 < FB_RECS ? R - r0 : FB_RECS);
  const int c4 = L * P / 4, s4 = fb_row_slots(c4);
  f4 *w_rows = fb_lds, *g_rows = fb_lds + FB_RECS * s4;

  fb_stage_levels(wh, piece_level, shapes, L, P, lane);
  fb_rows_in(w_rows, w + r0 * c4, nrec, c4, lane);
  fb_rows_in(g_rows, grad_logits + r0 * c4, nrec, c4, lane);
  __syncthreads();
  if (lane < nrec) {                                            // softmax adjoint: w * (gw - sum_k w_k gw_k)
    const f4 *wr = w_rows + lane * s4;
    f4 *gr = g_rows + lane * s4;
    float dot = 0.f;
    for (int k = 0; k < c4; ++k) {
      const f4 a = wr[k], g = gr[k];
      dot += (a.x * g.x + a.y * g.y) + (a.z * g.z + a.w * g.w);
    }
    for (int k = 0; k < c4; ++k) {
      const f4 a = wr[k];
      f4 g = gr[k];
      g.x = a.x * (g.x - dot), g.y = a.y * (g.y - dot), g.z = a.z * (g.z - dot), g.w = a.w * (g.w - dot);
      gr[k] = g;
    }
  }
  __syncthreads();
  fb_rows_out(grad_logits + r0 * c4, g_rows, nrec, c4, lane);

  // grad_offsets = gloc / (W_l, H_l), element-wise (a sample gated out by the sampling kernel keeps its exact zero)
  const int c2 = 2 * c4;
  f4 *go = grad_offsets + r0 * c2;
  for (int i = lane; i < nrec * c2; i += FB_RECS) {
    const int l = piece_level[i % c2];
    const float W = wh[2 * l], H = wh[2 * l + 1];
    f4 g = go[i];
    g.x /= W, g.y /= H, g.z /= W, g.w /= H;
    go[i] = g;
  }
}

inline bool fb_geometry_ok(int L, int P) { return L >= 1 && P >= 2 && P % 2 == 0 && (L * P) % 4 == 0 && L * P <= FB_MAX_POINTS; }

}  // namespace

// PCT_NOT_COVERED: L * P above 64 or no multiple of 4, an odd P, or more workgroups than one grid dimension holds (2^37 records)
int launch_msda_fused_expand(const float *logits, const float *offsets, const float *ref, long long ref_batch_stride,
                             const int64_t *shapes, long long R, int M, int Lq, int L, int P, float *loc, float *w,
                             hipStream_t stream)
{
  if (!fb_geometry_ok(L, P)) return PCT_NOT_COVERED;
  const long long blocks = (R + FB_RECS - 1) / FB_RECS;
  if (blocks <= 0 || blocks >= 0x7fffffffLL) return PCT_NOT_COVERED;
  const size_t lds = sizeof(f4) * FB_RECS * fb_row_slots(L * P / 4);
  hipLaunchKernelGGL(msda_fused_expand_kernel, dim3((unsigned)blocks), dim3(FB_RECS), lds, stream,
                     reinterpret_cast<const f4 *>(logits), reinterpret_cast<const f4 *>(offsets), ref, ref_batch_stride, shapes, R,
                     M, Lq, L, P, reinterpret_cast<f4 *>(loc), reinterpret_cast<f4 *>(w));
  return (int)hipGetLastError();
}

int launch_msda_fused_fold(const float *w, const int64_t *shapes, long long R, int L, int P, float *grad_offsets,
                           float *grad_logits, hipStream_t stream)
{
  if (!fb_geometry_ok(L, P)) return PCT_NOT_COVERED;
  const long long blocks = (R + FB_RECS - 1) / FB_RECS;
  if (blocks <= 0 || blocks >= 0x7fffffffLL) return PCT_NOT_COVERED;
  const size_t lds = sizeof(f4) * 2 * FB_RECS * fb_row_slots(L * P / 4);
  hipLaunchKernelGGL(msda_fused_fold_kernel, dim3((unsigned)blocks), dim3(FB_RECS), lds, stream,
                     reinterpret_cast<const f4 *>(w), shapes, R, L, P, reinterpret_cast<f4 *>(grad_offsets),
                     reinterpret_cast<f4 *>(grad_logits));
  return (int)hipGetLastError();
}

}  // namespace pct
