// Instance targets from label maps on the device (include/pctrans_hip_targets.h: pct_instance_targets_census,
// pct_instance_targets_planes): what the reference trainer's prepare_intance_targets computes on the host with torch.unique,
// one `map == id`, nonzero and float mean per instance, a stack and a pageable copy of the [G, H, W] masks.
//
// Census, five launches on one stream, nothing allocated, no host synchronisation, integer arithmetic only:
//   init_kernel         the workspace: bitmaps and totals 0, the value -> plane tables "none", the status words 0
//   bitmap_kernel<T>    presence of each of the 65 536 label values: an 8 KB bitmap per workgroup in LDS, its non-zero words
//                       OR-ed into the image's global bitmap; a value that is negative, above 65 535 or not integral sets
//                       bit 0 of the image's status word and is otherwise left out
//   rank_kernel         one workgroup per image: `ignore_label` cleared, the set bits ranked in ascending order -> ids, the kept
//                       count, table[value] = plane index for the first LC_MAX kept values; more than LC_MAX sets status bit 1
//   accumulate_kernel<T> per kept id the pixel count, sum x and sum y: a thread walks 16 consecutive pixels and adds a run of
//                       equal labels at once (an instance is a blob: most runs are whole strips), LDS integer atomics inside the
//                       workgroup, 64-bit integer atomic adds of the non-empty entries into the image's totals.  Integer addition
//                       is associative: the totals are exact and the same from call to call whatever the order
//   centres_kernel      (sum x / count / W, sum y / count / W) in fp64, rounded to fp32 once
// What a label value is, the merge of a workgroup's bitmap and the rank step are label_census.hpp's, shared with label_metrics.hip.
//
// Planes, two launches: starts_kernel (exclusive prefix sum of the plane counts), then one of
//   planes_strip_kernel<T>  H * W a multiple of 16: a thread owns 16 consecutive pixels, reads their labels once (once per
//                           group of planes: blockIdx.z splits an image's planes so that the grid fills the device), looks up
//                           their plane indices and writes, for each plane of its group, 16 bool bytes in one 16-byte store and
//                           16 floats in four; plane group 0 also writes the 16 foreground bytes
//   planes_flat_kernel<T>   any other size: a plane then starts at an address that is no multiple of 16, so the thread owns 16
//                           consecutive ELEMENTS of the whole [sum G, H, W] output instead (the allocation is padded to 16) and
//                           finds each element's (image, plane, pixel); stores stay 16 bytes wide and aligned, plane and row
//                           tails included, at the price of reading a label once per plane.  The foreground bytes likewise
// Both are pure write streams of sum G * H * W * (1 + 4) bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "label_census.hpp"    // LC_MAX kept ids per image, LC_VALUES, LC_WORDS, LC_NONE; label_value, census_merge, census_rank
#include "launchers.hpp"

namespace pct {

namespace {

constexpr int IT_BLOCK = 256;
constexpr int IT_STRIP = 16;                    // consecutive pixels of one thread
constexpr int IT_PASS = IT_BLOCK * IT_STRIP;    // pixels of one workgroup pass
constexpr int IT_MAX_CHUNKS = 256;              // workgroups per image of the census kernels

// workspace of one image, in bytes: bitmap, totals (count, sum x, sum y: 64-bit each), table (16-bit plane index per value)
constexpr size_t IT_WS_BITMAP = 0;
constexpr size_t IT_WS_TOTALS = IT_WS_BITMAP + LC_WORDS * 4;
constexpr size_t IT_WS_TABLE = IT_WS_TOTALS + (size_t)LC_MAX * 3 * 8;
constexpr size_t IT_WS_IMAGE = IT_WS_TABLE + (size_t)LC_VALUES * 2;
static_assert(LC_MAX == PCT_TARGETS_MAX_INSTANCES && IT_WS_IMAGE == PCT_TARGETS_WORKSPACE_PER_IMAGE, "the header's limits");

__device__ __forceinline__ unsigned *ws_bitmap(void *ws, int n) { return (unsigned *)((char *)ws + n * IT_WS_IMAGE + IT_WS_BITMAP); }
__device__ __forceinline__ unsigned long long *ws_totals(void *ws, int n)
{
  return (unsigned long long *)((char *)ws + n * IT_WS_IMAGE + IT_WS_TOTALS);
}
__device__ __forceinline__ unsigned short *ws_table(const void *ws, int n)
{
  return (unsigned short *)((char *)ws + n * IT_WS_IMAGE + IT_WS_TABLE);
}

__global__ __launch_bounds__(IT_BLOCK) void init_kernel(void *__restrict__ ws, int *__restrict__ num, int *__restrict__ status)
{
  const int n = blockIdx.y;
  unsigned *zero = (unsigned *)((char *)ws + n * IT_WS_IMAGE);                  // bitmap and totals are adjacent
  unsigned *none = (unsigned *)ws_table(ws, n);
  const int step = gridDim.x * IT_BLOCK, t = blockIdx.x * IT_BLOCK + threadIdx.x;
  for (int i = t; i < (int)(IT_WS_TABLE / 4); i += step) zero[i] = 0u;
  for (int i = t; i < LC_VALUES / 2; i += step) none[i] = 0xFFFFFFFFu;
  if (t == 0) {
    num[n] = 0;
    status[n] = 0;
  }
}

template <typename T>
__global__ __launch_bounds__(IT_BLOCK) void bitmap_kernel(const T *__restrict__ labels, const int P, const ChunkPlan plan,
                                                          void *__restrict__ ws, int *__restrict__ status)
{
  __shared__ unsigned bits[LC_WORDS];
  const int n = blockIdx.y;
  const T *lb = labels + (size_t)n * P;
  for (int i = threadIdx.x; i < LC_WORDS; i += IT_BLOCK) bits[i] = 0u;
  __syncthreads();
  bool bad = false;
  int last = -1;
  for (int pass = 0; pass < plan.passes; ++pass) {
    const long long p0 = ((long long)blockIdx.x * plan.passes + pass) * IT_PASS + (long long)threadIdx.x * IT_STRIP;
    if (p0 >= P) break;
    const int cnt = (int)min((long long)IT_STRIP, P - p0);
    for (int k = 0; k < cnt; ++k) {
      const int v = label_value<T>(lb[p0 + k]);
      if (v < 0) {
        bad = true;
      } else if (v != last) {
        atomicOr(&bits[v >> 5], 1u << (v & 31));
        last = v;
      }
    }
  }
  __syncthreads();
  census_merge<IT_BLOCK>(bits, LC_WORDS, ws_bitmap(ws, n));
  if (bad) atomicOr(&status[n], 1);
}

__global__ __launch_bounds__(IT_BLOCK) void rank_kernel(void *__restrict__ ws, const int ignore_label, int *__restrict__ ids,
                                                        int *__restrict__ num, int *__restrict__ status)
{
  __shared__ int first[IT_BLOCK + 1];
  const int n = blockIdx.x;
  const int total = census_rank<IT_BLOCK, false>(ws_bitmap(ws, n), ignore_label, ids, n * LC_MAX, ws_table(ws, n), first, nullptr,
                                                 nullptr);
  if (threadIdx.x == 0) {
    num[n] = total;
    if (total > LC_MAX) atomicOr(&status[n], 2);
  }
}

template <typename T>
__global__ __launch_bounds__(IT_BLOCK) void accumulate_kernel(const T *__restrict__ labels, const int P, const int W,
                                                              const ChunkPlan plan, void *__restrict__ ws)
{
  __shared__ unsigned long long sx[LC_MAX], sy[LC_MAX];
  __shared__ unsigned cn[LC_MAX];
  const int n = blockIdx.y;
  const T *lb = labels + (size_t)n * P;
  const unsigned short *table = ws_table(ws, n);
  for (int i = threadIdx.x; i < LC_MAX; i += IT_BLOCK) {
    sx[i] = 0ull;
    sy[i] = 0ull;
    cn[i] = 0u;
  }
  __syncthreads();
  for (int pass = 0; pass < plan.passes; ++pass) {
    const long long p0 = ((long long)blockIdx.x * plan.passes + pass) * IT_PASS + (long long)threadIdx.x * IT_STRIP;
    if (p0 >= P) break;
    const int cnt = (int)min((long long)IT_STRIP, P - p0);
    int y = (int)(p0 / W), x = (int)(p0 - (long long)y * W);
    unsigned run = LC_NONE, rc = 0u;                                            // the current run: plane index, pixels
    unsigned long long rx = 0ull, ry = 0ull;
    for (int k = 0; k < cnt; ++k) {
      const int v = label_value<T>(lb[p0 + k]);
      const unsigned g = v < 0 ? LC_NONE : (unsigned)table[v];
      if (g != run) {
        if (rc) {
          atomicAdd(&cn[run], rc);
          atomicAdd(&sx[run], rx);
          atomicAdd(&sy[run], ry);
        }
        run = g;
        rc = 0u;
        rx = ry = 0ull;
      }
      if (g != LC_NONE) {
        ++rc;
        rx += (unsigned)x;
        ry += (unsigned)y;
      }
      if (++x == W) {
        x = 0;
        ++y;
      }
    }
    if (rc) {
      atomicAdd(&cn[run], rc);
      atomicAdd(&sx[run], rx);
      atomicAdd(&sy[run], ry);
    }
  }
  __syncthreads();
  unsigned long long *tot = ws_totals(ws, n);
  for (int i = threadIdx.x; i < LC_MAX; i += IT_BLOCK)
    if (cn[i]) {
      atomicAdd(&tot[i * 3 + 0], (unsigned long long)cn[i]);
      atomicAdd(&tot[i * 3 + 1], sx[i]);
      atomicAdd(&tot[i * 3 + 2], sy[i]);
    }
}

__global__ __launch_bounds__(LC_MAX) void centres_kernel(void *__restrict__ ws, const int W, const int *__restrict__ num,
                                                         int *__restrict__ pixels, float *__restrict__ centres)
{
  const int n = blockIdx.x, g = threadIdx.x;
  const unsigned long long *tot = ws_totals(ws, n);
  const unsigned long long c = tot[g * 3];
  float cx = 0.f, cy = 0.f;
  if (g < num[n] && c) {
    cx = (float)((double)tot[g * 3 + 1] / (double)c / (double)W);
    cy = (float)((double)tot[g * 3 + 2] / (double)c / (double)W);               // (the reference divides both by the width)
  }
  pixels[n * LC_MAX + g] = (int)c;
  centres[(n * LC_MAX + g) * 2] = cx;
  centres[(n * LC_MAX + g) * 2 + 1] = cy;
}

// starts[n] = counts[0] + ... + counts[n - 1]: one workgroup, a thread adds a run of consecutive images
__global__ __launch_bounds__(1024) void starts_kernel(const int *__restrict__ counts, const int N, int *__restrict__ starts)
{
  __shared__ int first[1025];
  const int t = threadIdx.x, per = (N + 1023) / 1024;
  const int a = min(N, t * per), b = min(N, a + per);
  int s = 0;
  for (int i = a; i < b; ++i) s += counts[i];
  first[t + 1] = s;
  __syncthreads();
  if (t == 0) {
    first[0] = 0;
    for (int i = 1; i <= 1024; ++i) first[i] += first[i - 1];
  }
  __syncthreads();
  s = first[t];
  for (int i = a; i < b; ++i) {
    starts[i] = s;
    s += counts[i];
  }
}

__device__ __forceinline__ unsigned bool_word(const unsigned *idx, const unsigned g)
{
  return (idx[0] == g ? 1u : 0u) | (idx[1] == g ? 0x100u : 0u) | (idx[2] == g ? 0x10000u : 0u) | (idx[3] == g ? 0x1000000u : 0u);
}

template <typename T>
__global__ __launch_bounds__(IT_BLOCK) void planes_strip_kernel(const T *__restrict__ labels, const int P, const void *__restrict__ ws,
                                                                const int *__restrict__ starts, const int *__restrict__ counts,
                                                                uint8_t *__restrict__ masks, float *__restrict__ planes,
                                                                uint8_t *__restrict__ fg)
{
  const int n = blockIdx.y;
  const long long p0 = ((long long)blockIdx.x * IT_BLOCK + threadIdx.x) * IT_STRIP;
  if (p0 >= P) return;                                                          // (P is a multiple of IT_STRIP: whole strips only)
  const T *lb = labels + (size_t)n * P + p0;
  const unsigned short *table = ws_table(ws, n);
  unsigned idx[IT_STRIP];
  unsigned fgw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < IT_STRIP; ++k) {
    const T raw = lb[k];
    const int v = label_value<T>(raw);
    idx[k] = v < 0 ? LC_NONE : (unsigned)table[v];
    if (raw > (T)0) fgw[k >> 2] |= 1u << (8 * (k & 3));
  }
  if (fg && blockIdx.z == 0) *(uint4 *)(fg + (size_t)n * P + p0) = make_uint4(fgw[0], fgw[1], fgw[2], fgw[3]);
  const int G = counts[n];
  const size_t base = (size_t)starts[n] * P + p0;
  for (int g = blockIdx.z; g < G; g += gridDim.z) {
    const size_t at = base + (size_t)g * P;
    *(uint4 *)(masks + at) = make_uint4(bool_word(idx, g), bool_word(idx + 4, g), bool_word(idx + 8, g), bool_word(idx + 12, g));
    if (planes) {
      float4 *dst = (float4 *)(planes + at);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        dst[q] = make_float4(idx[4 * q] == (unsigned)g ? 1.f : 0.f, idx[4 * q + 1] == (unsigned)g ? 1.f : 0.f,
                             idx[4 * q + 2] == (unsigned)g ? 1.f : 0.f, idx[4 * q + 3] == (unsigned)g ? 1.f : 0.f);
    }
  }
}

// the image that owns global plane `plane`: the last n with starts[n] <= plane (images without planes share their successor's
// start and come before it).  Not row_ranges.hpp's image_of: a 64-bit key and an inclusive upper bound, other instructions
__device__ __forceinline__ int image_of_plane(const int *__restrict__ starts, const int N, const long long plane)
{
  int lo = 0, hi = N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (starts[mid] <= plane) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <typename T>
__global__ __launch_bounds__(IT_BLOCK) void planes_flat_kernel(const T *__restrict__ labels, const int N, const int P,
                                                               const void *__restrict__ ws, const int *__restrict__ starts,
                                                               const long long total, uint8_t *__restrict__ masks,
                                                               float *__restrict__ planes)
{
  const long long e0 = ((long long)blockIdx.x * IT_BLOCK + threadIdx.x) * IT_STRIP;
  if (e0 >= total) return;                                                      // (the outputs are padded to whole strips)
  long long plane = e0 / P;
  int p = (int)(e0 - plane * P);
  int n = image_of_plane(starts, N, plane);
  unsigned hit[IT_STRIP];
#pragma unroll
  for (int k = 0; k < IT_STRIP; ++k) {
    hit[k] = 0u;
    if (e0 + k < total) {
      const int v = label_value<T>(labels[(size_t)n * P + p]);
      const unsigned g = (unsigned)(plane - starts[n]);
      hit[k] = (v >= 0 && (unsigned)ws_table(ws, n)[v] == g) ? 1u : 0u;
      if (++p == P) {
        p = 0;
        ++plane;
        if (e0 + k + 1 < total) n = image_of_plane(starts, N, plane);
      }
    }
  }
  *(uint4 *)(masks + e0) = make_uint4(hit[0] | hit[1] << 8 | hit[2] << 16 | hit[3] << 24, hit[4] | hit[5] << 8 | hit[6] << 16 | hit[7] << 24,
                                      hit[8] | hit[9] << 8 | hit[10] << 16 | hit[11] << 24,
                                      hit[12] | hit[13] << 8 | hit[14] << 16 | hit[15] << 24);
  if (planes) {
    float4 *dst = (float4 *)(planes + e0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      dst[q] = make_float4((float)hit[4 * q], (float)hit[4 * q + 1], (float)hit[4 * q + 2], (float)hit[4 * q + 3]);
  }
}

// foreground bytes of [N, P] maps, 16 consecutive elements per thread (the buffer is padded to whole strips)
template <typename T>
__global__ __launch_bounds__(IT_BLOCK) void fg_flat_kernel(const T *__restrict__ labels, const long long total, uint8_t *__restrict__ fg)
{
  const long long e0 = ((long long)blockIdx.x * IT_BLOCK + threadIdx.x) * IT_STRIP;
  if (e0 >= total) return;
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < IT_STRIP; ++k)
    if (e0 + k < total && labels[e0 + k] > (T)0) w[k >> 2] |= 1u << (8 * (k & 3));
  *(uint4 *)(fg + e0) = make_uint4(w[0], w[1], w[2], w[3]);
}

template <typename T>
int census_typed(const void *labels, int N, int P, int W, int ignore_label, void *ws, int *ids, int *pixels, float *centres, int *num,
                 int *status, hipStream_t stream)
{
  const ChunkPlan plan = chunk_plan(P, IT_PASS, IT_MAX_CHUNKS);                 // passes of IT_PASS pixels; workgroups per image
  const T *lb = static_cast<const T *>(labels);
  init_kernel<<<dim3(16, N), IT_BLOCK, 0, stream>>>(ws, num, status);
  bitmap_kernel<T><<<dim3(plan.chunks, N), IT_BLOCK, 0, stream>>>(lb, P, plan, ws, status);
  rank_kernel<<<N, IT_BLOCK, 0, stream>>>(ws, ignore_label, ids, num, status);
  accumulate_kernel<T><<<dim3(plan.chunks, N), IT_BLOCK, 0, stream>>>(lb, P, W, plan, ws);
  centres_kernel<<<N, LC_MAX, 0, stream>>>(ws, W, num, pixels, centres);
  return (int)hipGetLastError();
}

template <typename T>
int planes_typed(const void *labels, int N, int P, const void *ws, const int *counts, long long total_planes, int max_count,
                 int *starts, uint8_t *masks, float *planes, uint8_t *fg, hipStream_t stream)
{
  const T *lb = static_cast<const T *>(labels);
  starts_kernel<<<1, 1024, 0, stream>>>(counts, N, starts);
  if (P % IT_STRIP == 0) {
    const int blocks = (P / IT_STRIP + IT_BLOCK - 1) / IT_BLOCK;
    const long long want = 2048 / ((long long)blocks * N);                      // plane groups: enough workgroups for the device
    const int groups = (int)std::max(1ll, std::min((long long)max_count, want));
    planes_strip_kernel<T><<<dim3(blocks, N, groups), IT_BLOCK, 0, stream>>>(lb, P, ws, starts, counts, masks, planes, fg);
  } else {
    const long long total = total_planes * P, blocks = (total + IT_PASS - 1) / IT_PASS;
    const long long fg_total = (long long)N * P, fg_blocks = (fg_total + IT_PASS - 1) / IT_PASS;
    if (blocks > 0x7FFFFFFFll || fg_blocks > 0x7FFFFFFFll) return PCT_ERR_UNSUPPORTED;
    planes_flat_kernel<T><<<(unsigned)blocks, IT_BLOCK, 0, stream>>>(lb, N, P, ws, starts, total, masks, planes);
    if (fg) fg_flat_kernel<T><<<(unsigned)fg_blocks, IT_BLOCK, 0, stream>>>(lb, fg_total, fg);
  }
  return (int)hipGetLastError();
}

}  // namespace

int instance_targets_geometry_status(int dtype, int N, int H, int W)
{
  if (dtype < 0 || dtype > 4) return PCT_ERR_UNSUPPORTED;
  if (N > 65535 || (long long)H * W >= 0x7FFFFFFFll) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

int launch_instance_targets_census(const void *labels, int dtype, int N, int H, int W, int ignore_label, void *workspace, int *ids,
                                   int *pixels, float *centres, int *num, int *status, hipStream_t stream)
{
  const int rc = instance_targets_geometry_status(dtype, N, H, W);
  if (rc != PCT_OK) return rc;
  const int P = H * W;
  switch (dtype) {
    case 0: return census_typed<uint8_t>(labels, N, P, W, ignore_label, workspace, ids, pixels, centres, num, status, stream);
    case 1: return census_typed<int16_t>(labels, N, P, W, ignore_label, workspace, ids, pixels, centres, num, status, stream);
    case 2: return census_typed<int32_t>(labels, N, P, W, ignore_label, workspace, ids, pixels, centres, num, status, stream);
    case 3: return census_typed<int64_t>(labels, N, P, W, ignore_label, workspace, ids, pixels, centres, num, status, stream);
    default: return census_typed<float>(labels, N, P, W, ignore_label, workspace, ids, pixels, centres, num, status, stream);
  }
}

int launch_instance_targets_planes(const void *labels, int dtype, int N, int H, int W, const void *workspace, const int *counts,
                                   long long total_planes, int max_count, int *starts, uint8_t *masks, float *planes, uint8_t *fg,
                                   hipStream_t stream)
{
  const int rc = instance_targets_geometry_status(dtype, N, H, W);
  if (rc != PCT_OK) return rc;
  const int P = H * W;
  switch (dtype) {
    case 0: return planes_typed<uint8_t>(labels, N, P, workspace, counts, total_planes, max_count, starts, masks, planes, fg, stream);
    case 1: return planes_typed<int16_t>(labels, N, P, workspace, counts, total_planes, max_count, starts, masks, planes, fg, stream);
    case 2: return planes_typed<int32_t>(labels, N, P, workspace, counts, total_planes, max_count, starts, masks, planes, fg, stream);
    case 3: return planes_typed<int64_t>(labels, N, P, workspace, counts, total_planes, max_count, starts, masks, planes, fg, stream);
    default: return planes_typed<float>(labels, N, P, workspace, counts, total_planes, max_count, starts, masks, planes, fg, stream);
  }
}

}  // namespace pct
