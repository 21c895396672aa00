// Validation metrics from label maps on the device (include/pctrans_hip_metrics.h: pct_label_overlap, pct_label_metrics): what
// the reference's trainer computes on the host after copying every label map back -- SymmetricBestDice / AbsDiffFGLabels for
// CVPPP, agg_jc_index / pixel_f1 / get_fast_pq for BBBC -- each a loop over all (label, label) pairs with full-image mask sums.
// All of them are functions of the contingency table of the two maps and its row and column totals.
//
// Overlap, five launches on one stream, nothing allocated, no host synchronisation, integer arithmetic only:
//   init_kernel      the workspace (bitmaps 0, value -> index tables "none"), the table 0, the status words 0
//   bitmap_kernel    presence of each of the 65 536 values of both maps: two 8 KB bitmaps per workgroup in LDS (a lane sets a
//                    bit only where its value differs from its neighbour's), the non-zero words OR-ed into the image's bitmaps.
//                    The prediction is read through the foreground map.  A value outside the covered ones sets a status bit
//   rank_kernel      one workgroup per (image, side): the set bits ranked in ascending order -> values, num, lowest / highest
//                    raw value, index table; COUNT and EMPTY status bits
//   table_kernel     a workgroup walks a contiguous run of pixels, 256 per pass, a lane per pixel; key = g * 512 + p of the
//                    compacted indices.  Every lane compares its key with the lane before (lane 0 always starts a run); the
//                    ballot of run heads gives each head its run length, and the head adds it to T[key] in one atomic
//   areas_kernel     row and column sums of the table: the pixel count of every value
// What a label value is, the merge of a workgroup's bitmaps and the rank step are label_census.hpp's, shared with
// instance_targets.hip.
// Metrics, one launch of one workgroup per image: see metrics_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "label_census.hpp"    // LC_MAX distinct values per map, LC_VALUES, LC_WORDS, LC_NONE; label_value, census_merge, census_rank
#include "launchers.hpp"
#include "wave_reduce.hpp"

namespace pct {

namespace {

constexpr int LM_BLOCK = 256;                   // threads of the map kernels = pixels of one workgroup pass
constexpr int LM_MAX_CHUNKS = 256;              // workgroups per image of the map kernels
constexpr unsigned LM_NO_KEY = 0xFFFFFFFFu;     // key of a pixel that is in no table cell
constexpr size_t LM_TABLE = (size_t)LC_MAX * LC_MAX;

// workspace of one image, in bytes: bitmap of side 0, of side 1, index table (16 bit per value) of side 0, of side 1
constexpr size_t LM_WS_BITMAP = 0;
constexpr size_t LM_WS_INDEX = LM_WS_BITMAP + 2 * (size_t)LC_WORDS * 4;
constexpr size_t LM_WS_IMAGE = LM_WS_INDEX + 2 * (size_t)LC_VALUES * 2;
static_assert(LC_MAX == PCT_METRICS_MAX_VALUES && LM_WS_IMAGE == PCT_METRICS_WORKSPACE_PER_IMAGE, "the header's limits");

__device__ __forceinline__ unsigned *ws_bitmap(void *ws, int n, int side)
{
  return (unsigned *)((char *)ws + n * LM_WS_IMAGE + LM_WS_BITMAP) + side * LC_WORDS;
}
__device__ __forceinline__ unsigned short *ws_index(const void *ws, int n, int side)
{
  return (unsigned short *)((char *)ws + n * LM_WS_IMAGE + LM_WS_INDEX) + side * LC_VALUES;
}

// label_value of element i of a map of `dtype`.  `dtype` is uniform over the launch: the switch costs a scalar branch
__device__ __forceinline__ int load_label(const void *__restrict__ base, const int dtype, const size_t i)
{
  switch (dtype) {
    case 0: return label_value(((const uint8_t *)base)[i]);
    case 1: return label_value(((const int16_t *)base)[i]);
    case 2: return label_value(((const int32_t *)base)[i]);
    case 3: return label_value(((const int64_t *)base)[i]);
    default: return label_value(((const float *)base)[i]);
  }
}

struct Maps {
  const void *pred, *gt;
  const uint8_t *fg;
  int pred_dtype, gt_dtype, P;
};

__global__ __launch_bounds__(LM_BLOCK) void init_kernel(void *__restrict__ ws, int *__restrict__ table, int *__restrict__ status)
{
  const int n = blockIdx.y;
  uint4 *zero = (uint4 *)((char *)ws + n * LM_WS_IMAGE + LM_WS_BITMAP);
  uint4 *none = (uint4 *)((char *)ws + n * LM_WS_IMAGE + LM_WS_INDEX);
  uint4 *tab = (uint4 *)(table + (size_t)n * LM_TABLE);
  const int step = gridDim.x * LM_BLOCK, t = blockIdx.x * LM_BLOCK + threadIdx.x;
  for (int i = t; i < (int)(2 * LC_WORDS * 4 / 16); i += step) zero[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int i = t; i < (int)(2 * LC_VALUES * 2 / 16); i += step) none[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  for (int i = t; i < (int)(LM_TABLE * 4 / 16); i += step) tab[i] = make_uint4(0u, 0u, 0u, 0u);
  if (t == 0) status[n] = 0;
}

__global__ __launch_bounds__(LM_BLOCK) void bitmap_kernel(const Maps m, const ChunkPlan plan, void *__restrict__ ws,
                                                          int *__restrict__ status)
{
  __shared__ unsigned bits[2][LC_WORDS];
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const size_t base = (size_t)n * m.P;
  for (int i = threadIdx.x; i < 2 * LC_WORDS; i += LM_BLOCK) (&bits[0][0])[i] = 0u;
  __syncthreads();
  int bad = 0;
  for (int pass = 0; pass < plan.passes; ++pass) {
    const int start = (blockIdx.x * plan.passes + pass) * LM_BLOCK;             // (uniform: the whole workgroup leaves together)
    if (start >= m.P) break;
    const int i = start + threadIdx.x;
    int vp = -2, vg = -2;                                                       // -2: no pixel
    if (i < m.P) {
      vp = (m.fg && m.fg[base + i] == 0) ? 0 : load_label(m.pred, m.pred_dtype, base + i);
      vg = load_label(m.gt, m.gt_dtype, base + i);
      if (vp < 0) bad |= PCT_METRICS_STATUS_PRED_VALUE;
      if (vg < 0) bad |= PCT_METRICS_STATUS_GT_VALUE;
    }
    const int bp = __shfl_up(vp, 1), bg = __shfl_up(vg, 1);
    if (vp >= 0 && (lane == 0 || vp != bp)) atomicOr(&bits[0][vp >> 5], 1u << (vp & 31));
    if (vg >= 0 && (lane == 0 || vg != bg)) atomicOr(&bits[1][vg >> 5], 1u << (vg & 31));
  }
  __syncthreads();
  census_merge<LM_BLOCK>(&bits[0][0], 2 * LC_WORDS, ws_bitmap(ws, n, 0));       // (side 1 follows side 0)
  if (bad) atomicOr(&status[n], bad);
}

__global__ __launch_bounds__(LM_BLOCK) void rank_kernel(void *__restrict__ ws, int *__restrict__ values, int *__restrict__ num,
                                                        int *__restrict__ range, int *__restrict__ status)
{
  __shared__ int first[LM_BLOCK + 1];
  __shared__ int lo, hi;
  const int n = blockIdx.x, side = blockIdx.y;
  const int total = census_rank<LM_BLOCK, true>(ws_bitmap(ws, n, side), -1, values + ((size_t)n * 2 + side) * LC_MAX, 0,
                                                ws_index(ws, n, side), first, &lo, &hi);
  if (threadIdx.x == 0) {
    num[n * 2 + side] = total;
    range[(n * 2 + side) * 2] = total ? lo : 0;                                 // (total = 0: every pixel of the map was uncovered)
    range[(n * 2 + side) * 2 + 1] = total ? hi : 0;
    int bitsout = 0;
    if (total > LC_MAX) bitsout |= side ? PCT_METRICS_STATUS_GT_COUNT : PCT_METRICS_STATUS_PRED_COUNT;
    if (hi <= 0) bitsout |= side ? PCT_METRICS_STATUS_EMPTY_GT : PCT_METRICS_STATUS_EMPTY_PRED;
    if (bitsout) atomicOr(&status[n], bitsout);
  }
}

__global__ __launch_bounds__(LM_BLOCK) void table_kernel(const Maps m, const ChunkPlan plan, const void *__restrict__ ws,
                                                         int *__restrict__ table)
{
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const size_t base = (size_t)n * m.P;
  const unsigned short *ip = ws_index(ws, n, 0), *ig = ws_index(ws, n, 1);
  int *T = table + (size_t)n * LM_TABLE;
  for (int pass = 0; pass < plan.passes; ++pass) {
    const int start = (blockIdx.x * plan.passes + pass) * LM_BLOCK;             // (uniform)
    if (start >= m.P) break;
    const int i = start + threadIdx.x;
    unsigned key = LM_NO_KEY;
    if (i < m.P) {
      const int vp = (m.fg && m.fg[base + i] == 0) ? 0 : load_label(m.pred, m.pred_dtype, base + i);
      const int vg = load_label(m.gt, m.gt_dtype, base + i);
      if (vp >= 0 && vg >= 0) {
        const unsigned a = ip[vp], b = ig[vg];
        if (a != LC_NONE && b != LC_NONE) key = b * LC_MAX + a;                 // a, b < LC_MAX: inside the image's table
      }
    }
    const unsigned before = __shfl_up(key, 1);
    const bool head = lane == 0 || key != before;
    const unsigned long long heads = __ballot(head);
    if (head && key != LM_NO_KEY) {
      const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = later ? __ffsll(later) : 64 - lane;                       // up to the next head, or to the wave's end
      atomicAdd(&T[key], len);
    }
  }
}

__global__ __launch_bounds__(LC_MAX) void areas_kernel(const int *__restrict__ table, const int *__restrict__ num,
                                                       int *__restrict__ areas)
{
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nP = min(num[n * 2], LC_MAX), nG = min(num[n * 2 + 1], LC_MAX);
  const int *T = table + (size_t)n * LM_TABLE;
  int *ap = areas + (size_t)n * 2 * LC_MAX, *ag = ap + LC_MAX;
  int col = 0;
  if (t < nP)
    for (int g = 0; g < nG; ++g) col += T[g * LC_MAX + t];
  ap[t] = col;
  if (t >= nG) ag[t] = 0;
  for (int g = wave; g < nG; g += LC_MAX / 64) {
    int row = 0;
    for (int p = lane; p < nP; p += 64) row += T[g * LC_MAX + p];
    row = wave_sum(row);
    if (lane == 0) ag[g] = row;
  }
}

// One workgroup of 512 threads per image.  nP, nG: distinct values of the two maps; compact index 0 is the lowest value present
// (the CVPPP background); p0, g0 = 1 where that value is 0 (the BBBC background is present), else 0.
//   column pass   thread a: max_b dice(a, b) over b >= 1 -> termP[a]                                   (BD(pred, gt))
//   row pass      wave per row b: max_a dice over a >= 1 -> termG[b] (BD(gt, pred)); the one a with IoU > 1/2 -> iouM[b] (PQ);
//                 foreground pixels of the row that meet predicted foreground (F1's TP)
//   wave 0        AJI: sequential over the instances, the predictions over the lanes, "taken" as a bit per lane and slot
//   thread 64     the ordered sums and the remaining columns
__global__ __launch_bounds__(LC_MAX) void metrics_kernel(const int *__restrict__ values, const int *__restrict__ areas,
                                                         const int *__restrict__ num, const int *__restrict__ range,
                                                         const int *__restrict__ table, double *__restrict__ metrics,
                                                         int *__restrict__ counts)
{
  __shared__ int aP[LC_MAX], aG[LC_MAX];
  __shared__ double termP[LC_MAX], termG[LC_MAX], iouM[LC_MAX];
  __shared__ unsigned long long tp_pixels;
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nP = min(num[n * 2], LC_MAX), nG = min(num[n * 2 + 1], LC_MAX);
  const int *T = table + (size_t)n * LM_TABLE;
  const int p0 = (nP > 0 && values[(size_t)n * 2 * LC_MAX] == 0) ? 1 : 0;
  const int g0 = (nG > 0 && values[((size_t)n * 2 + 1) * LC_MAX] == 0) ? 1 : 0;
  double *out = metrics + (size_t)n * PCT_METRICS_COLUMNS;
  aP[t] = t < nP ? areas[(size_t)n * 2 * LC_MAX + t] : 0;
  aG[t] = t < nG ? areas[((size_t)n * 2 + 1) * LC_MAX + t] : 0;
  termP[t] = termG[t] = iouM[t] = 0.0;
  if (t == 0) tp_pixels = 0ull;
  __syncthreads();

  if (t >= 1 && t < nP) {
    double best = 0.0;
    for (int b = 1; b < nG; ++b) {
      const int x = T[b * LC_MAX + t];
      if (x) best = fmax(best, (double)(2 * x) / (double)(aP[t] + aG[b]));
    }
    termP[t] = best;
  }
  for (int b = wave; b < nG; b += LC_MAX / 64) {
    double best = 0.0, match = 0.0;
    for (int a = lane; a < nP; a += 64) {
      const int x = T[b * LC_MAX + a];
      if (!x) continue;
      if (a >= 1 && b >= 1) best = fmax(best, (double)(2 * x) / (double)(aP[a] + aG[b]));
      if (a >= p0 && b >= g0) {
        const int u = aG[b] + aP[a] - x;
        if (2 * x > u) match = (double)x / (double)u;                           // IoU > 1/2, decided in integers; at most one a
      }
    }
    best = wave_max(best);
    match = wave_max(match);
    if (lane == 0) {
      termG[b] = best;
      iouM[b] = match;
      if (b >= g0) atomicAdd(&tp_pixels, (unsigned long long)(aG[b] - (p0 ? T[b * LC_MAX] : 0)));
    }
  }
  __syncthreads();

  if (wave == 0) {
    unsigned taken = 0u;                                                        // bit k: prediction p0 + lane + 64 k
    long long c = 0, u = 0;
    int used = 0;
    if (nP - p0 > 0) {
      for (int b = g0; b < nG; ++b) {
        double bq = -1.0;
        int bi = 0x7FFFFFFF;
        for (int k = 0, a = p0 + lane; a < nP; a += 64, ++k) {
          const int x = ((taken >> k) & 1u) ? 0 : T[b * LC_MAX + a];
          const double q = x ? (double)x / (double)(aG[b] + aP[a] - x) : 0.0;
          if (q > bq) {
            bq = q;
            bi = a;
          }
        }
        for (int off = 32; off; off >>= 1) {                                    // the largest quotient, the lowest index among equals
          const double oq = __shfl_xor(bq, off);
          const int oi = __shfl_xor(bi, off);
          if (oq > bq || (oq == bq && oi < bi)) {
            bq = oq;
            bi = oi;
          }
        }
        const int owner = (bi - p0) & 63, slot = (bi - p0) >> 6;
        const int was = __shfl((int)((taken >> slot) & 1u), owner);
        const int x = was ? 0 : T[b * LC_MAX + bi];
        c += x;
        u += was ? aG[b] : aG[b] + aP[bi] - x;
        if (lane == owner) taken |= 1u << slot;
      }
      long long rest = 0;
      for (int k = 0, a = p0 + lane; a < nP; a += 64, ++k) {
        if ((taken >> k) & 1u) ++used; else rest += aP[a];
      }
      u += wave_sum(rest);
      used = wave_sum(used);
    }
    if (lane == 0) {
      out[4] = u > 0 ? (double)c / (double)u : 0.0;
      counts[n * 4 + 3] = used;
    }
  }

  if (t == 64) {
    const int dP = range[n * 4 + 1] - range[n * 4], dG = range[n * 4 + 3] - range[n * 4 + 2];
    double sp = 0.0, sg = 0.0, si = 0.0;
    for (int a = 1; a < nP; ++a) sp += termP[a];
    for (int b = 1; b < nG; ++b) sg += termG[b];
    const double bdp = dP > 0 ? sp / (double)dP : 0.0, bdg = dG > 0 ? sg / (double)dG : 0.0;
    out[0] = bdp;
    out[1] = bdg;
    out[2] = fmin(bdp, bdg);
    out[3] = (double)abs(dP - dG);
    long long fgp = 0, fgg = 0;
    for (int a = p0; a < nP; ++a) fgp += aP[a];
    for (int b = g0; b < nG; ++b) fgg += aG[b];
    const long long den = fgp + fgg;                                            // 2 TP + FP + FN
    out[5] = den > 0 ? (double)(2 * (long long)tp_pixels) / (double)den : 0.0;
    int tp = 0;
    for (int b = g0; b < nG; ++b)
      if (iouM[b] > 0.0) {
        ++tp;
        si += iouM[b];
      }
    const int fp = nP - p0 - tp, fn = nG - g0 - tp;
    const double dd = (double)tp + 0.5 * (double)fp + 0.5 * (double)fn;
    const double dq = dd > 0.0 ? (double)tp / dd : 0.0, sq = si / ((double)tp + 1e-6);
    out[6] = dq;
    out[7] = sq;
    out[8] = dq * sq;
    counts[n * 4] = tp;
    counts[n * 4 + 1] = fp;
    counts[n * 4 + 2] = fn;
  }
  if (t >= 65 && t < 68) out[9 + t - 65] = 0.0;
}

}  // namespace

int label_metrics_geometry_status(int pred_dtype, int gt_dtype, int N, int H, int W)
{
  if (pred_dtype < 0 || pred_dtype > 4 || gt_dtype < 0 || gt_dtype > 4) return PCT_ERR_UNSUPPORTED;
  if (N <= 0 || N > 65535 || (long long)H * W >= (1ll << 24)) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

int launch_label_overlap(const void *pred, int pred_dtype, const void *gt, int gt_dtype, const uint8_t *fg, int N, int H, int W,
                         void *workspace, int *values, int *areas, int *num, int *range, int *table, int *status,
                         hipStream_t stream)
{
  const int rc = label_metrics_geometry_status(pred_dtype, gt_dtype, N, H, W);
  if (rc != PCT_OK) return rc;
  Maps m;
  m.pred = pred;
  m.gt = gt;
  m.fg = fg;
  m.pred_dtype = pred_dtype;
  m.gt_dtype = gt_dtype;
  m.P = H * W;
  const ChunkPlan plan = chunk_plan(m.P, LM_BLOCK, LM_MAX_CHUNKS);               // passes of LM_BLOCK pixels; workgroups per image
  init_kernel<<<dim3(64, N), LM_BLOCK, 0, stream>>>(workspace, table, status);
  bitmap_kernel<<<dim3(plan.chunks, N), LM_BLOCK, 0, stream>>>(m, plan, workspace, status);
  rank_kernel<<<dim3(N, 2), LM_BLOCK, 0, stream>>>(workspace, values, num, range, status);
  table_kernel<<<dim3(plan.chunks, N), LM_BLOCK, 0, stream>>>(m, plan, workspace, table);
  areas_kernel<<<N, LC_MAX, 0, stream>>>(table, num, areas);
  return (int)hipGetLastError();
}

int launch_label_metrics(const int *values, const int *areas, const int *num, const int *range, const int *table, int N,
                         double *metrics, int *counts, hipStream_t stream)
{
  if (N <= 0 || N > 65535) return PCT_ERR_UNSUPPORTED;
  metrics_kernel<<<N, LC_MAX, 0, stream>>>(values, areas, num, range, table, metrics, counts);
  return (int)hipGetLastError();
}

}  // namespace pct
