// The criterion's two small losses on the device (include/pctrans_hip_aux_loss.h): the reference-point L1 loss of all supervised
// heads (pct_refpoint_l1_forward_f32, pct_refpoint_l1_backward_f32: SetCriterion.loss_refpoints, nine calls per step) and the
// semantic focal loss on the strided foreground map (pct_sigmoid_focal_strided_forward_f32, pct_sigmoid_focal_strided_backward_f32:
// SetCriterion.loss_sem).  Both work on a few thousand numbers: their cost is launches, so each is one small grid.  fp32
// throughout, no floating-point atomic: every sum has one order that depends on the shapes alone, and two calls on the same
// operands give the same bits.
//
// Reference points, one launch each way:
//   refpoint_fwd_kernel   one workgroup per head.  Thread t adds the terms of pairs t, t + 256, ... in ascending pair order, each
//                         pair's coordinates in ascending d; the 64 lanes of a wave by wave_sum, the four waves in ascending order;
//                         then the division by num_masks.  Workgroup 0 also counts the pairs with an index out of range
//   refpoint_bwd_kernel   one thread per (head, row): it walks the head's pairs in ascending order (their src staged in LDS) and
//                         adds sgn(points - target) g for every pair that lists its row, g = grad_loss[h] / num_masks; a row no
//                         pair lists keeps its exact zeros.  Every element of grad_points is written: no fill pass
// A pair whose src is outside [0, rows) or whose tgt is outside [0, num_targets) reads nothing and adds nothing, either way.
//
// Focal loss, two launches forward and one backward:
//   focal_fwd_kernel      one workgroup per chunk of FL_PER_PASS * passes consecutive outputs: thread t adds elements
//                         t, t + 256, ... of the chunk in ascending order, lanes by wave_sum, waves in ascending order; the chunk's
//                         loss sum and its count of positive targets go to the workspace
//   focal_final_kernel    one thread adds the chunks in ascending order: loss = sum / max(num_pos, 1), and num_pos
//   focal_bwd_kernel      one thread per output; p, ce and m recomputed from the logit
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.hpp"
#include "wave_reduce.hpp"

namespace pct {

namespace {

constexpr int RP_MAX_DIMS = 8;            // 2 * points_num of a reference point
constexpr int RP_STAGE = 1024;            // pairs of one LDS stage of the backward
constexpr int FL_PER_PASS = 1024;         // outputs of one pass of a forward workgroup: 4 per thread
constexpr int FL_MAX_CHUNKS = 256;        // workgroups of the forward: bounds the workspace (PCT_FOCAL_WORKSPACE_BYTES)
constexpr int FL_FG_BYTE = 0, FL_FG_F32 = 4;   // dtype codes of fg: those of the instance targets' label maps

// the four waves' sums in ascending order; the result is valid in thread 0
template <typename T>
__device__ __forceinline__ T block_sum_256(T v, T *part)
{
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

__device__ __forceinline__ bool rp_pair_ok(const int s, const int t, const int rows, const int num_targets)
{
  return (unsigned)s < (unsigned)rows && (unsigned)t < (unsigned)num_targets;
}

__global__ __launch_bounds__(256) void refpoint_fwd_kernel(const float *__restrict__ points, const float *__restrict__ target,
                                                           const int *__restrict__ src, const int *__restrict__ tgt,
                                                           const int heads, const int rows, const int dims,
                                                           const int num_targets, const int pairs, const float num_masks,
                                                           float *__restrict__ loss, int *__restrict__ status)
{
  __shared__ float part[4];
  __shared__ int bad_part[4];
  const int h = blockIdx.x, tid = threadIdx.x;
  const float *ph = points + (size_t)h * rows * dims;
  float sum = 0.f;
  for (int k = tid; k < pairs; k += 256) {
    const int s = src[(size_t)h * pairs + k], t = tgt[(size_t)h * pairs + k];
    if (!rp_pair_ok(s, t, rows, num_targets)) continue;
    const float *p = ph + (size_t)s * dims, *q = target + (size_t)t * dims;
    for (int d = 0; d < dims; ++d) sum += fabsf(p[d] - q[d]);
  }
  sum = block_sum_256(sum, part);
  if (tid == 0) loss[h] = sum / num_masks;
  if (h == 0) {                                                             // the status word: an integer sum
    int bad = 0;
    for (long long k = tid; k < (long long)heads * pairs; k += 256) bad += rp_pair_ok(src[k], tgt[k], rows, num_targets) ? 0 : 1;
    bad = block_sum_256(bad, bad_part);
    if (tid == 0) *status = bad;
  }
}

__global__ __launch_bounds__(256) void refpoint_bwd_kernel(const float *__restrict__ points, const float *__restrict__ target,
                                                           const int *__restrict__ src, const int *__restrict__ tgt,
                                                           const float *__restrict__ grad_loss, const int rows, const int dims,
                                                           const int num_targets, const int pairs, const float num_masks,
                                                           float *__restrict__ grad_points)
{
  __shared__ int srow[RP_STAGE];            // src of the stage's pairs; -1: the pair does not count
  const int h = blockIdx.y, tid = threadIdx.x;
  const long long row = (long long)blockIdx.x * 256 + tid;
  const bool live = row < rows;
  const float g = grad_loss[h] / num_masks;
  const float *p = points + ((size_t)h * rows + (size_t)(live ? row : 0)) * dims;
  float x[RP_MAX_DIMS], acc[RP_MAX_DIMS];
#pragma unroll
  for (int d = 0; d < RP_MAX_DIMS; ++d) {
    x[d] = (live && d < dims) ? p[d] : 0.f;
    acc[d] = 0.f;
  }
  for (int k0 = 0; k0 < pairs; k0 += RP_STAGE) {
    const int n = min(RP_STAGE, pairs - k0);
    __syncthreads();                        // the previous stage has been read
    for (int k = tid; k < n; k += 256) {
      const int s = src[(size_t)h * pairs + k0 + k], t = tgt[(size_t)h * pairs + k0 + k];
      srow[k] = rp_pair_ok(s, t, rows, num_targets) ? s : -1;
    }
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < n; ++k) {
      if (srow[k] != (int)row) continue;
      const float *q = target + (size_t)tgt[(size_t)h * pairs + k0 + k] * dims;
#pragma unroll
      for (int d = 0; d < RP_MAX_DIMS; ++d) {
        if (d >= dims) break;
        const float diff = x[d] - q[d];
        acc[d] += diff > 0.f ? g : (diff < 0.f ? -g : 0.f);
      }
    }
  }
  if (!live) return;
  float *o = grad_points + ((size_t)h * rows + (size_t)row) * dims;
#pragma unroll
  for (int d = 0; d < RP_MAX_DIMS; ++d)
    if (d < dims) o[d] = acc[d];
}

// p = sigmoid(x), ce = max(x, 0) - x t + log1p(exp(-|x|)), m = 1 - (p t + (1 - p)(1 - t)): e = exp(-|x|) never overflows.
// expf, log1pf and the division are the compiler's accurate ones (no fast-math)
struct FocalTerms {
  float p, ce, m, w;
};
__device__ __forceinline__ FocalTerms focal_terms(const float x, const float t, const float alpha)
{
  FocalTerms f;
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  f.p = x >= 0.f ? r : e * r;
  f.ce = fmaxf(x, 0.f) - x * t + log1pf(e);
  f.m = 1.f - (f.p * t + (1.f - f.p) * (1.f - t));
  f.w = alpha >= 0.f ? alpha * t + (1.f - alpha) * (1.f - t) : 1.f;
  return f;
}

// the target of output e = (n, i, j): fg[n, stride / 2 + i stride, stride / 2 + j stride] as a float
template <typename F>
__device__ __forceinline__ float focal_target(const F *__restrict__ fg, const int e, const int out_h, const int out_w,
                                              const int height, const int width, const int stride)
{
  const int j = e % out_w, ni = e / out_w, i = ni % out_h, n = ni / out_h;
  return (float)fg[((size_t)n * height + (size_t)(stride / 2 + i * stride)) * width + (size_t)(stride / 2 + j * stride)];
}

template <typename F>
__global__ __launch_bounds__(256) void focal_fwd_kernel(const float *__restrict__ logits, const F *__restrict__ fg, const int total,
                                                        const int out_h, const int out_w, const int height, const int width,
                                                        const int stride, const float alpha, const ChunkPlan plan,
                                                        float *__restrict__ ws_loss, int *__restrict__ ws_pos)
{
  __shared__ float part[4];
  __shared__ int pos_part[4];
  const int tid = threadIdx.x;
  const long long e0 = (long long)blockIdx.x * plan.passes * FL_PER_PASS;
  const long long e1 = min((long long)total, e0 + (long long)plan.passes * FL_PER_PASS);
  float sum = 0.f;
  int pos = 0;
  for (long long e = e0 + tid; e < e1; e += 256) {
    const float t = focal_target(fg, (int)e, out_h, out_w, height, width, stride);
    const FocalTerms f = focal_terms(logits[e], t, alpha);
    sum += f.w * (f.ce * (f.m * f.m));
    pos += t > 0.f ? 1 : 0;
  }
  sum = block_sum_256(sum, part);
  pos = block_sum_256(pos, pos_part);
  if (tid == 0) {
    ws_loss[blockIdx.x] = sum;
    ws_pos[blockIdx.x] = pos;
  }
}

__global__ void focal_final_kernel(const float *__restrict__ ws_loss, const int *__restrict__ ws_pos, const int chunks,
                                   float *__restrict__ loss, float *__restrict__ num_pos)
{
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float sum = 0.f;
  long long pos = 0;
  for (int c = 0; c < chunks; ++c) {
    sum += ws_loss[c];
    pos += ws_pos[c];
  }
  const float np = (float)pos;
  *num_pos = np;
  *loss = sum / fmaxf(np, 1.f);
}

template <typename F>
__global__ __launch_bounds__(256) void focal_bwd_kernel(const float *__restrict__ logits, const F *__restrict__ fg,
                                                        const float *__restrict__ num_pos, const float *__restrict__ grad_loss,
                                                        const int total, const int out_h, const int out_w, const int height,
                                                        const int width, const int stride, const float alpha,
                                                        float *__restrict__ grad_logits)
{
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const float t = focal_target(fg, (int)e, out_h, out_w, height, width, stride);
  const FocalTerms f = focal_terms(logits[e], t, alpha);
  const float d = (f.p - t) * (f.m * f.m) - 2.f * f.ce * f.m * (2.f * t - 1.f) * f.p * (1.f - f.p);
  grad_logits[e] = grad_loss[0] * f.w * d / fmaxf(num_pos[0], 1.f);
}

inline int refpoint_geometry_status(int heads, long long rows, int dims)
{
  if (heads > PCT_POINT_MAX_HEADS || dims > RP_MAX_DIMS || rows >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

// PCT_ERR_BAD_ARG for an output size that is not the strided slice's, PCT_ERR_UNSUPPORTED for what the kernels do not cover
inline int focal_geometry_status(int fg_dtype, int batch, int out_h, int out_w, int height, int width, int stride)
{
  const int first = stride / 2;
  if (height <= first || width <= first) return PCT_ERR_BAD_ARG;
  if (out_h != (height - first + stride - 1) / stride || out_w != (width - first + stride - 1) / stride) return PCT_ERR_BAD_ARG;
  if (fg_dtype != FL_FG_BYTE && fg_dtype != FL_FG_F32) return PCT_ERR_UNSUPPORTED;
  if ((long long)batch * out_h * out_w >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

}  // namespace

int launch_refpoint_l1_forward(const float *points, const float *target_points, const int *src, const int *tgt, int heads,
                               long long rows, int dims, int num_targets, int pairs, float num_masks, float *loss, int *status,
                               hipStream_t stream)
{
  if (const int rc = refpoint_geometry_status(heads, rows, dims); rc != PCT_OK) return rc;
  if (heads == 0) return PCT_OK;
  refpoint_fwd_kernel<<<dim3((unsigned)heads), dim3(256), 0, stream>>>(points, target_points, src, tgt, heads, (int)rows, dims,
                                                                       num_targets, pairs, num_masks, loss, status);
  return (int)hipGetLastError();
}

int launch_refpoint_l1_backward(const float *points, const float *target_points, const int *src, const int *tgt,
                                const float *grad_loss, int heads, long long rows, int dims, int num_targets, int pairs,
                                float num_masks, float *grad_points, hipStream_t stream)
{
  if (const int rc = refpoint_geometry_status(heads, rows, dims); rc != PCT_OK) return rc;
  if (heads == 0 || rows == 0) return PCT_OK;
  refpoint_bwd_kernel<<<dim3((unsigned)((rows + 255) / 256), (unsigned)heads), dim3(256), 0, stream>>>(
      points, target_points, src, tgt, grad_loss, (int)rows, dims, num_targets, pairs, num_masks, grad_points);
  return (int)hipGetLastError();
}

int launch_sigmoid_focal_strided_forward(const float *logits, const void *fg, int fg_dtype, int batch, int out_h, int out_w,
                                         int height, int width, int stride, float alpha, void *workspace, float *loss,
                                         float *num_pos, hipStream_t stream)
{
  if (const int rc = focal_geometry_status(fg_dtype, batch, out_h, out_w, height, width, stride); rc != PCT_OK) return rc;
  const int total = batch * out_h * out_w;
  const ChunkPlan plan = chunk_plan(total, FL_PER_PASS, FL_MAX_CHUNKS);
  float *ws_loss = static_cast<float *>(workspace);
  int *ws_pos = reinterpret_cast<int *>(ws_loss + FL_MAX_CHUNKS);
  if (fg_dtype == FL_FG_BYTE)
    focal_fwd_kernel<<<dim3((unsigned)plan.chunks), dim3(256), 0, stream>>>(logits, static_cast<const uint8_t *>(fg), total, out_h,
                                                                            out_w, height, width, stride, alpha, plan, ws_loss,
                                                                            ws_pos);
  else
    focal_fwd_kernel<<<dim3((unsigned)plan.chunks), dim3(256), 0, stream>>>(logits, static_cast<const float *>(fg), total, out_h,
                                                                            out_w, height, width, stride, alpha, plan, ws_loss,
                                                                            ws_pos);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  focal_final_kernel<<<dim3(1), dim3(64), 0, stream>>>(ws_loss, ws_pos, plan.chunks, loss, num_pos);
  return (int)hipGetLastError();
}

int launch_sigmoid_focal_strided_backward(const float *logits, const void *fg, int fg_dtype, const float *num_pos,
                                          const float *grad_loss, int batch, int out_h, int out_w, int height, int width,
                                          int stride, float alpha, float *grad_logits, hipStream_t stream)
{
  if (const int rc = focal_geometry_status(fg_dtype, batch, out_h, out_w, height, width, stride); rc != PCT_OK) return rc;
  const int total = batch * out_h * out_w;
  const dim3 grid((unsigned)(((long long)total + 255) / 256));
  if (fg_dtype == FL_FG_BYTE)
    focal_bwd_kernel<<<grid, dim3(256), 0, stream>>>(logits, static_cast<const uint8_t *>(fg), num_pos, grad_loss, total, out_h,
                                                     out_w, height, width, stride, alpha, grad_logits);
  else
    focal_bwd_kernel<<<grid, dim3(256), 0, stream>>>(logits, static_cast<const float *>(fg), num_pos, grad_loss, total, out_h, out_w,
                                                     height, width, stride, alpha, grad_logits);
  return (int)hipGetLastError();
}

}  // namespace pct
