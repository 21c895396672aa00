// Small-object merging of label maps on the device (include/pctrans_hip_merge.h: pct_label_merge_small): the reference's
// merge_func / merge_small_object (connectomics/engine/trainer.py:744-777), which runs on the host after a copy of every label
// map.  `seg[seg == ids] = max_ids` moves ALL pixels of one current label to another: the current map is cur[original value], and a
// label's pixel count, row sum and column sum are additive under a merge.  So no per-label pass over the image is needed.
//
// Six launches on one stream, nothing allocated, no host synchronisation, integer arithmetic only:
//   init_kernel      the workspace (bitmap 0, value -> rank table "none", the sums 0), the counts 0, the status words 0
//   bitmap_kernel    presence of each of the 65 536 values of the map read through the foreground map: an 8 KB bitmap per workgroup
//                    in LDS (a lane sets a bit only where its value differs from its neighbour's), OR-ed into the image's
//   rank_kernel      one workgroup per image: the set bits ranked in ascending order -> values, num, rank table; COUNT status bit
//   sums_kernel      a workgroup walks a contiguous run of pixels, 256 per pass, a lane per pixel.  Every lane compares its rank
//                    with the lane before (lane 0 and the first pixel of an image row always start a run); the head of a run adds
//                    the run's length, length * row and the sum of its columns to the workgroup's LDS tables in one integer
//                    atomic each; the non-zero rows of the tables join the image's with global integer atomics (64-bit sums)
//   plan_kernel      one workgroup per image runs all passes in order on the 512-row tables in LDS: see there
//   apply_kernel     out = final[rank(gated value)], 16 bytes per lane where the pointers allow, scalar at the ragged end
// What a label value is, the merge of a workgroup's bitmap and the rank step are label_census.hpp's, shared with
// instance_targets.hip and label_metrics.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "label_census.hpp"    // LC_MAX distinct values per image, LC_VALUES, LC_WORDS, LC_NONE; label_value, census_merge, census_rank
#include "launchers.hpp"

namespace pct {

namespace {

constexpr int MG_BLOCK = 256;                   // threads of every kernel here = pixels of one workgroup pass
constexpr int MG_MAX_CHUNKS = 256;              // workgroups per image of the map kernels
constexpr int MG_PER_LANE = (PCT_MERGE_MAX_WINDOW * PCT_MERGE_MAX_WINDOW + MG_BLOCK - 1) / MG_BLOCK;   // crop pixels of a lane
constexpr int MG_KEY_BITS = 9;                  // decision key = count << 9 | (511 - rank): count descending, then value ascending
static_assert(LC_MAX == 1 << MG_KEY_BITS && LC_MAX == 2 * MG_BLOCK, "two table rows per thread; a rank fits the key's low bits");

// workspace of one image, in bytes: bitmap, value -> rank table (16 bit per value), row sums, column sums (64 bit per rank)
constexpr size_t MG_WS_BITMAP = 0;
constexpr size_t MG_WS_INDEX = MG_WS_BITMAP + (size_t)LC_WORDS * 4;
constexpr size_t MG_WS_ROWS = MG_WS_INDEX + (size_t)LC_VALUES * 2;
constexpr size_t MG_WS_COLS = MG_WS_ROWS + (size_t)LC_MAX * 8;
constexpr size_t MG_WS_IMAGE = MG_WS_COLS + (size_t)LC_MAX * 8;
static_assert(LC_MAX == PCT_MERGE_MAX_VALUES && MG_WS_IMAGE == PCT_MERGE_WORKSPACE_PER_IMAGE, "the header's limits");

__device__ __forceinline__ unsigned *ws_bitmap(void *ws, int n) { return (unsigned *)((char *)ws + n * MG_WS_IMAGE + MG_WS_BITMAP); }
__device__ __forceinline__ unsigned short *ws_index(const void *ws, int n)
{
  return (unsigned short *)((char *)ws + n * MG_WS_IMAGE + MG_WS_INDEX);
}
__device__ __forceinline__ unsigned long long *ws_rows(const void *ws, int n)
{
  return (unsigned long long *)((char *)ws + n * MG_WS_IMAGE + MG_WS_ROWS);
}
__device__ __forceinline__ unsigned long long *ws_cols(const void *ws, int n)
{
  return (unsigned long long *)((char *)ws + n * MG_WS_IMAGE + MG_WS_COLS);
}

struct Map {
  const void *labels;
  const uint8_t *fg;
  int dtype, H, W, P;
};

struct Passes {
  int num, threshold[PCT_MERGE_MAX_PASSES], window[PCT_MERGE_MAX_PASSES];
};

// label_value of element i of the map read through the foreground map.  `dtype` is uniform over the launch
__device__ __forceinline__ int gated_label(const Map &m, const size_t i)
{
  if (m.fg && m.fg[i] == 0) return 0;
  switch (m.dtype) {
    case 0: return label_value(((const uint8_t *)m.labels)[i]);
    case 1: return label_value(((const int16_t *)m.labels)[i]);
    case 2: return label_value(((const int32_t *)m.labels)[i]);
    case 3: return label_value(((const int64_t *)m.labels)[i]);
    default: return label_value(((const float *)m.labels)[i]);
  }
}

__global__ __launch_bounds__(MG_BLOCK) void init_kernel(void *__restrict__ ws, int *__restrict__ before, int *__restrict__ status)
{
  const int n = blockIdx.y;
  uint4 *zero = (uint4 *)((char *)ws + n * MG_WS_IMAGE + MG_WS_BITMAP);
  uint4 *none = (uint4 *)((char *)ws + n * MG_WS_IMAGE + MG_WS_INDEX);
  uint4 *sums = (uint4 *)((char *)ws + n * MG_WS_IMAGE + MG_WS_ROWS);
  const int step = gridDim.x * MG_BLOCK, t = blockIdx.x * MG_BLOCK + threadIdx.x;
  for (int i = t; i < (int)(LC_WORDS * 4 / 16); i += step) zero[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int i = t; i < (int)(LC_VALUES * 2 / 16); i += step) none[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  for (int i = t; i < (int)(2 * LC_MAX * 8 / 16); i += step) sums[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int i = t; i < LC_MAX; i += step) before[(size_t)n * LC_MAX + i] = 0;
  if (t == 0) status[n] = 0;
}

__global__ __launch_bounds__(MG_BLOCK) void bitmap_kernel(const Map m, const ChunkPlan plan, void *__restrict__ ws,
                                                          int *__restrict__ status)
{
  __shared__ unsigned bits[LC_WORDS];
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const size_t base = (size_t)n * m.P;
  for (int i = threadIdx.x; i < LC_WORDS; i += MG_BLOCK) bits[i] = 0u;
  __syncthreads();
  int bad = 0;
  for (int pass = 0; pass < plan.passes; ++pass) {
    const int start = (blockIdx.x * plan.passes + pass) * MG_BLOCK;             // (uniform: the whole workgroup leaves together)
    if (start >= m.P) break;
    const int i = start + threadIdx.x;
    int v = -2;                                                                 // -2: no pixel
    if (i < m.P) {
      v = gated_label(m, base + i);
      if (v < 0) bad = PCT_MERGE_STATUS_VALUE;
    }
    const int b = __shfl_up(v, 1);
    if (v >= 0 && (lane == 0 || v != b)) atomicOr(&bits[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
  census_merge<MG_BLOCK>(bits, LC_WORDS, ws_bitmap(ws, n));
  if (bad) atomicOr(&status[n], bad);
}

__global__ __launch_bounds__(MG_BLOCK) void rank_kernel(void *__restrict__ ws, int *__restrict__ values, int *__restrict__ num,
                                                        int *__restrict__ status)
{
  __shared__ int first[MG_BLOCK + 1];
  const int n = blockIdx.x;
  const int total = census_rank<MG_BLOCK, false>(ws_bitmap(ws, n), -1, values + (size_t)n * LC_MAX, 0, ws_index(ws, n), first,
                                                 nullptr, nullptr);
  if (threadIdx.x == 0) {
    num[n] = total;
    if (total > LC_MAX) atomicOr(&status[n], PCT_MERGE_STATUS_COUNT);
  }
}

__global__ __launch_bounds__(MG_BLOCK) void sums_kernel(const Map m, const ChunkPlan plan, void *__restrict__ ws,
                                                        int *__restrict__ before)
{
  __shared__ int cnt[LC_MAX];
  __shared__ unsigned long long rows[LC_MAX], cols[LC_MAX];
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const size_t base = (size_t)n * m.P;
  const unsigned short *index = ws_index(ws, n);
  for (int i = threadIdx.x; i < LC_MAX; i += MG_BLOCK) {
    cnt[i] = 0;
    rows[i] = cols[i] = 0ull;
  }
  __syncthreads();
  for (int pass = 0; pass < plan.passes; ++pass) {
    const int start = (blockIdx.x * plan.passes + pass) * MG_BLOCK;             // (uniform)
    if (start >= m.P) break;
    const int i = start + threadIdx.x;
    unsigned key = LC_NONE;                                                     // a pixel that is in no table row
    int y = 0, x = -1;
    if (i < m.P) {
      y = i / m.W;
      x = i - y * m.W;
      const int v = gated_label(m, base + i);
      if (v >= 0) key = index[v];                                               // LC_NONE past the first LC_MAX values
    }
    const unsigned prev = __shfl_up(key, 1);
    const bool head = lane == 0 || key != prev || x == 0;                       // a run stays inside one image row
    const unsigned long long heads = __ballot(head);
    if (head && key != LC_NONE) {
      const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = later ? __ffsll(later) : 64 - lane;                       // up to the next head, or to the wave's end
      atomicAdd(&cnt[key], len);                                                // (lanes past the image hold LC_NONE: they are heads)
      atomicAdd(&rows[key], (unsigned long long)len * (unsigned)y);
      atomicAdd(&cols[key], (unsigned long long)len * (unsigned)x + (unsigned long long)(len * (len - 1) / 2));
    }
  }
  __syncthreads();
  unsigned long long *grows = ws_rows(ws, n), *gcols = ws_cols(ws, n);
  for (int i = threadIdx.x; i < LC_MAX; i += MG_BLOCK) {
    const int c = cnt[i];
    if (c) {
      atomicAdd(&before[(size_t)n * LC_MAX + i], c);
      atomicAdd(&grows[i], rows[i]);
      atomicAdd(&gcols[i], cols[i]);
    }
  }
}

// numpy's seg[start : start + window] on an axis of n (start + window > 0: the centroid is not negative): a negative start wraps
__device__ __forceinline__ void crop_range(const int start, const int window, const int n, int &lo, int &hi)
{
  lo = start < 0 ? max(start + n, 0) : min(start, n);
  hi = min(start + window, n);
}

// One workgroup of 256 threads per image; thread t owns the table rows t and t + 256 (a row = one distinct value of the gated map,
// by ascending rank).  cur[row] = the row whose label the row's pixels carry now; cnt / sr / sc = live pixel count, row sum and
// column sum of each label.  Per pass: snap = cnt; every row with 0 < snap <= threshold is visited in ascending order:
//   crop       from the live centroid, numpy's slice rules
//   histogram  a lane per crop pixel: the pixel's current label through the gate, the rank table and cur; LDS atomics by rank
//   scan       every thread offers its two rows: the number of distinct labels, the best key of all, the best key of the labels
//              other than 0 and the visited one (key = count << 9 | 511 - rank: count descending, then value ascending)
//   decision   fewer than three labels: nothing.  0 first -> the best eligible label; else the best of all, nothing if it is the
//              visited one.  TIE: 0 and the visited label share the top count, or another eligible label has the best count
//   merge      the sums move (thread 0), the rows that carry the visited label are redirected (their owners)
// Three barriers per visit; a row that is not visited costs the test alone.  The histogram is cleared by the lanes that filled it.
__global__ __launch_bounds__(MG_BLOCK) void plan_kernel(const Map m, const Passes ps, const void *__restrict__ ws,
                                                        const int *__restrict__ values, const int *__restrict__ num,
                                                        const int *__restrict__ before, int *__restrict__ final_,
                                                        int *__restrict__ after, int *__restrict__ merges, int *__restrict__ status)
{
  __shared__ unsigned short cur[LC_MAX];
  __shared__ int cnt[LC_MAX], snap[LC_MAX], hist[LC_MAX];
  __shared__ long long sr[LC_MAX], sc[LC_MAX];
  __shared__ int best_all, best_elig, distinct, h_zero, h_visited, tie;
  const int n = blockIdx.x, t = threadIdx.x;
  const size_t base = (size_t)n * m.P;
  const unsigned short *index = ws_index(ws, n);
  const int *val = values + (size_t)n * LC_MAX;
  const int K = min(num[n], LC_MAX);
  const int zr = (K > 0 && val[0] == 0) ? 0 : -1;                               // the row of label 0: the lowest value, if present
  for (int r = t; r < LC_MAX; r += MG_BLOCK) {
    cur[r] = (unsigned short)r;
    cnt[r] = r < K ? before[(size_t)n * LC_MAX + r] : 0;
    sr[r] = r < K ? (long long)ws_rows(ws, n)[r] : 0ll;
    sc[r] = r < K ? (long long)ws_cols(ws, n)[r] : 0ll;
    hist[r] = 0;
  }
  if (t == 0) tie = 0;
  int merged[PCT_MERGE_MAX_PASSES];
#pragma unroll
  for (int p = 0; p < PCT_MERGE_MAX_PASSES; ++p) merged[p] = 0;

#pragma unroll 1
  for (int p = 0; p < ps.num; ++p) {
    const int threshold = ps.threshold[p], window = ps.window[p];
    __syncthreads();
    for (int r = t; r < LC_MAX; r += MG_BLOCK) snap[r] = cnt[r];
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < K; ++k) {                                               // (everything up to the histogram is uniform)
      const int size = snap[k];
      if (size <= 0 || size > threshold) continue;
      const int live = cnt[k];
      if (live <= 0) continue;                                                  // (never: only the visited label vanishes)
      int r0, r1, c0, c1;
      crop_range((int)(sr[k] / live) - window / 2, window, m.H, r0, r1);
      crop_range((int)(sc[k] / live) - window / 2, window, m.W, c0, c1);
      const int ch = r1 - r0, cw = c1 - c0;
      if (ch <= 0 || cw <= 0) continue;
      const int pixels = ch * cw;                                               // <= window^2 <= 961

      if (t == 0) {
        best_all = best_elig = -1;
        distinct = 0;
      }
      unsigned lab[MG_PER_LANE];
#pragma unroll
      for (int j = 0; j < MG_PER_LANE; ++j) {
        lab[j] = LC_NONE;
        const int q = t + j * MG_BLOCK;
        if (q < pixels) {
          const int dy = q / cw, y = r0 + dy, x = c0 + q - dy * cw;
          const int v = gated_label(m, base + (size_t)y * m.W + x);
          const unsigned rank = v >= 0 ? index[v] : LC_NONE;
          if (rank < (unsigned)LC_MAX) {
            lab[j] = cur[rank];
            atomicAdd(&hist[lab[j]], 1);
          }
        }
      }
      __syncthreads();

      int h[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = t + j * MG_BLOCK;
        h[j] = hist[r];
        if (r == zr) h_zero = h[j];
        if (r == k) h_visited = h[j];
        if (h[j] > 0) {
          const int key = (h[j] << MG_KEY_BITS) | (LC_MAX - 1 - r);
          atomicAdd(&distinct, 1);
          atomicMax(&best_all, key);
          if (r != zr && r != k) atomicMax(&best_elig, key);
        }
      }
      __syncthreads();

      if (distinct >= 3) {                                                      // (uniform from here to the merge)
        const int top = best_all >> MG_KEY_BITS;
        const bool zero_first = zr >= 0 && h_zero == top;
        const int sel = zero_first ? best_elig : best_all;                      // (three labels: an eligible one exists)
        const int count = sel >> MG_KEY_BITS, target = LC_MAX - 1 - (sel & (LC_MAX - 1));
        bool tied = t == 0 && zero_first && k != zr && h_visited == top;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int r = t + j * MG_BLOCK;
          if (h[j] == count && r != target && (!zero_first || (r != zr && r != k))) tied = true;
        }
        if (tied) tie = 1;
        if (sel >= 0 && target != k) {
          ++merged[p];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int r = t + j * MG_BLOCK;
            if (cur[r] == k) cur[r] = (unsigned short)target;
          }
          if (t == 0) {
            cnt[target] += cnt[k];
            sr[target] += sr[k];
            sc[target] += sc[k];
            cnt[k] = 0;
            sr[k] = sc[k] = 0ll;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < MG_PER_LANE; ++j)
        if (lab[j] != LC_NONE) hist[lab[j]] = 0;
      __syncthreads();
    }
  }
  __syncthreads();
  for (int r = t; r < LC_MAX; r += MG_BLOCK) {
    final_[(size_t)n * LC_MAX + r] = r < K ? val[cur[r]] : 0;
    after[(size_t)n * LC_MAX + r] = r < K ? cnt[r] : 0;
  }
  if (t < PCT_MERGE_MAX_PASSES) {
    int mine = 0;
#pragma unroll
    for (int p = 0; p < PCT_MERGE_MAX_PASSES; ++p) mine = t == p ? merged[p] : mine;
    merges[n * PCT_MERGE_MAX_PASSES + t] = mine;
  }
  if (t == 0 && tie) atomicOr(&status[n], PCT_MERGE_STATUS_TIE);
}

template <typename T>
__device__ __forceinline__ T merged_label(const T raw, const bool gate, const unsigned short *__restrict__ index,
                                          const int *__restrict__ fin)
{
  const T in = gate ? raw : (T)0;
  const int v = label_value(in);
  if (v < 0) return in;                                                         // (VALUE status: the caller discards the image)
  const unsigned rank = index[v];
  return rank < (unsigned)LC_MAX ? (T)fin[rank] : in;                           // (COUNT status likewise)
}

// Element e of the flat [batch * P] map: 16 bytes of labels (VEC of them) per lane while whole vectors remain and the pointers are
// 16-byte aligned (`vectors` = 0 otherwise), single elements past them.  A vector may straddle two images.
template <typename T>
__global__ __launch_bounds__(MG_BLOCK) void apply_kernel(const T *__restrict__ in, const uint8_t *__restrict__ fg,
                                                         T *__restrict__ out, const long long total, const long long vectors,
                                                         const int P, const void *__restrict__ ws, const int *__restrict__ final_)
{
  constexpr int VEC = 16 / (int)sizeof(T);
  struct alignas(16) Labels {
    T e[VEC];
  };
  struct alignas(VEC) Gates {
    uint8_t b[VEC];
  };
  const long long step = (long long)gridDim.x * MG_BLOCK, first = (long long)blockIdx.x * MG_BLOCK + threadIdx.x;
  for (long long g = first; g < vectors; g += step) {
    const long long e = g * VEC;
    const Labels a = *(const Labels *)(in + e);
    Gates f;
    if (fg) f = *(const Gates *)(fg + e);
    int n = (int)(e / P), at = (int)(e - (long long)n * P);
    Labels o;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      while (at >= P) {
        at -= P;
        ++n;
      }
      o.e[j] = merged_label<T>(a.e[j], !fg || f.b[j] != 0, ws_index(ws, n), final_ + (size_t)n * LC_MAX);
      ++at;
    }
    *(Labels *)(out + e) = o;
  }
  for (long long e = vectors * VEC + first; e < total; e += step) {
    const int n = (int)(e / P);
    out[e] = merged_label<T>(in[e], !fg || fg[e] != 0, ws_index(ws, n), final_ + (size_t)n * LC_MAX);
  }
}

template <typename T>
void launch_apply(const Map &m, int N, void *out, const void *ws, const int *final_, hipStream_t stream)
{
  constexpr int VEC = 16 / (int)sizeof(T);
  const long long total = (long long)N * m.P;
  const bool aligned = !(((uintptr_t)m.labels | (uintptr_t)out | (uintptr_t)m.fg) & 15u);
  const long long vectors = aligned ? total / VEC : 0;
  const long long items = vectors + (total - vectors * VEC);
  const long long blocks = (items + MG_BLOCK - 1) / MG_BLOCK;
  const int grid = (int)(blocks < 65536 ? blocks : 65536);
  apply_kernel<T><<<grid, MG_BLOCK, 0, stream>>>((const T *)m.labels, m.fg, (T *)out, total, vectors, m.P, ws, final_);
}

}  // namespace

int label_merge_status(int dtype, int N, int H, int W, const int *passes, int num_passes)
{
  if (H <= 0 || W <= 0 || !passes || num_passes < 1 || num_passes > PCT_MERGE_MAX_PASSES) return PCT_ERR_BAD_ARG;
  for (int p = 0; p < num_passes; ++p)
    if (passes[2 * p] < 0 || passes[2 * p + 1] < 1 || passes[2 * p + 1] > PCT_MERGE_MAX_WINDOW) return PCT_ERR_BAD_ARG;
  if (dtype < 0 || dtype > 4) return PCT_ERR_UNSUPPORTED;
  if (N <= 0 || N > 65535 || (long long)H * W >= (1ll << 24)) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

int launch_label_merge_small(const void *labels, int dtype, const uint8_t *fg, int N, int H, int W, const int *passes,
                             int num_passes, void *workspace, void *out, int *values, int *final_, int *areas_before,
                             int *areas_after, int *num, int *merges, int *status, hipStream_t stream)
{
  const int rc = label_merge_status(dtype, N, H, W, passes, num_passes);
  if (rc != PCT_OK) return rc;
  Map m;
  m.labels = labels;
  m.fg = fg;
  m.dtype = dtype;
  m.H = H;
  m.W = W;
  m.P = H * W;
  Passes ps;
  ps.num = num_passes;
  for (int p = 0; p < PCT_MERGE_MAX_PASSES; ++p) {
    ps.threshold[p] = p < num_passes ? passes[2 * p] : 0;
    ps.window[p] = p < num_passes ? passes[2 * p + 1] : 1;
  }
  const ChunkPlan plan = chunk_plan(m.P, MG_BLOCK, MG_MAX_CHUNKS);               // passes of MG_BLOCK pixels; workgroups per image
  init_kernel<<<dim3(16, N), MG_BLOCK, 0, stream>>>(workspace, areas_before, status);
  bitmap_kernel<<<dim3(plan.chunks, N), MG_BLOCK, 0, stream>>>(m, plan, workspace, status);
  rank_kernel<<<N, MG_BLOCK, 0, stream>>>(workspace, values, num, status);
  sums_kernel<<<dim3(plan.chunks, N), MG_BLOCK, 0, stream>>>(m, plan, workspace, areas_before);
  plan_kernel<<<N, MG_BLOCK, 0, stream>>>(m, ps, workspace, values, num, areas_before, final_, areas_after, merges, status);
  switch (dtype) {
    case 0: launch_apply<uint8_t>(m, N, out, workspace, final_, stream); break;
    case 1: launch_apply<int16_t>(m, N, out, workspace, final_, stream); break;
    case 2: launch_apply<int32_t>(m, N, out, workspace, final_, stream); break;
    case 3: launch_apply<int64_t>(m, N, out, workspace, final_, stream); break;
    default: launch_apply<float>(m, N, out, workspace, final_, stream); break;
  }
  return (int)hipGetLastError();
}

}  // namespace pct
