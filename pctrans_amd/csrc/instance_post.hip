// Instance post-processing on the device: query mask logits -> [N, H, W] int16 instance-id maps (include/pctrans_hip_post.h).
// Replaces instance_inference / mask_post / dice_for / mask_nms / comput_mmi of the reference's arch/maskformer.py:267-431 for
// a whole batch in one sequence of launches, with no host synchronisation and no [N, Q, H, W] tensor at input resolution.
//
//   ip_threshold   resize (bilinear, align_corners = False, fp32) + threshold on the logit + bit-pack + per-query area.
//                  One workgroup per (image, query) plane; a wavefront votes 64 pixels into a 64-bit ballot, 32 ballots make
//                  one 256-byte store.  Reads each logit from HBM once, writes 1 bit per output pixel.
//   ip_pair        intersections of all pairs of kept planes: popcount of the AND, 16 bytes per lane, 8 partners per wavefront.
//   ip_cluster     one workgroup per image: keep (area > 40), dice > thres1 as a [Q, Q] bit matrix in LDS, first-come clustering.
//   ip_merge       one workgroup per cluster: per-pixel member count in bit-sliced counters (32 pixels per register), compared
//                  with the count that count / size > thres2 needs (CVPPP: the new hard plane) or with 0 (BBBC: the cluster's
//                  support, which lets the label kernel skip the clusters that do not cover a pixel).
//   ip_nms         CVPPP, one workgroup per image: greedy NMS in descending area and the final ascending sort.
//   ip_label       one thread per pixel: first sorted plane that covers it (CVPPP), first maximum of count / size (BBBC).
//
// Every quantity after the threshold is an integer (areas, intersections, cluster sizes, member counts); the three places the
// reference rounds are reproduced as it rounds them: dice = (2 I + 1) / (a_i + a_j + 1) by IEEE fp32 division of integers
// below 2^24, the cluster mean count / size in fp32 against fp32(thres2), and the NMS ratio in double.  The BBBC argmax compares
// count / size of different clusters by cross-multiplication: two different fractions with denominators <= 512 are at least
// 2^-18 apart and at most 1, so their fp32 quotients are ordered as the fractions are, and equal fractions give equal quotients.
//
// Workspace (caller-owned, 16-byte aligned, 32-bit words; r4 rounds up to a multiple of 4; PW = 4 * ceil(H*W / 128) words per
// bit plane, QW = ceil(Q / 32)):
//   from_bits:  N*Q*PW  +  r4(N*Q*Q)  +  r4(N*Q*QW)  +  5 * r4(N*Q)  +  4*N
//   one call :  the above  +  N*Q*PW  +  r4(N*Q)         (the thresholded planes and their areas)
// Nothing is allocated, no atomic operation is used and no word of the workspace is read before this call has written it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "launchers.hpp"
#include "wave_reduce.hpp"

namespace pct {

namespace {

constexpr int IP_MAX_Q = 512;
constexpr int IP_MAX_QW = IP_MAX_Q / 32;
constexpr int IP_MAX_H_PLUS_W = 8000;
constexpr int IP_MIN_AREA = 40;          // a query is kept where its area is > 40 (:279, :311)

struct IpParams {
  double threshold;   // on the sigmoid
  float thres1;       // dice above which two queries are one cluster
  float thres2;       // hard merge: mean above which a pixel stays (CVPPP)
  int soft;           // BBBC: the merged mask is the mean itself
  double nms;         // CVPPP
};

bool ip_params(int dataset, IpParams *p)
{
  if (dataset == 0) { *p = {0.69, 0.5f, 0.6f, 0, 0.72}; return true; }      // CVPPP (:283-309)
  if (dataset == 1) { *p = {0.05, 0.15f, 0.25f, 1, 0.0}; return true; }     // BBBC  (:310-331)
  return false;
}

inline size_t r4(size_t x) { return (x + 3) & ~(size_t)3; }

__device__ inline float ip_load(const float *p, size_t i) { return p[i]; }
__device__ inline float ip_load(const unsigned short *p, size_t i) { return __uint_as_float((unsigned)p[i] << 16); }

__device__ inline int ip_block_sum(int v, int *scratch)     // 256 threads; the sum, in thread 0
{
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

// ---- resize + threshold + bit-pack + area ------------------------------------------------------------------------------------
// Source coordinate of output index d: (d + 0.5) * in / out - 0.5 = ((2 d + 1) * in - out) / (2 out), clamped at 0 as torch
// does.  Formed in integers, so the tap index is exact and the weight is one fp32 division of integers below 2^24.
template <typename T, bool COPY>
__global__ __launch_bounds__(256) void ip_threshold_kernel(const T *__restrict__ logits, int h, int w, int H, int W, int pw,
                                                           float thr, unsigned *__restrict__ bits, int *__restrict__ areas)
{
  extern __shared__ __align__(16) unsigned char ip_smem[];
  __shared__ int scratch[4];
  const size_t plane = blockIdx.x;
  const T *src = logits + plane * (size_t)h * w;
  unsigned *dst = bits + plane * (size_t)pw;
  const int HW = H * W;
  int *x0 = reinterpret_cast<int *>(ip_smem);
  float *xl = reinterpret_cast<float *>(x0 + W);
  int *y0 = reinterpret_cast<int *>(xl + W);
  float *yl = reinterpret_cast<float *>(y0 + H);
  if (!COPY) {
    for (int i = threadIdx.x; i < W + H; i += 256) {
      const bool isx = i < W;
      const int d = isx ? i : i - W, in = isx ? w : h, out = isx ? W : H;
      const long long num = (2LL * d + 1) * in - out;
      int i0 = 0;
      float l = 0.f;
      if (num > 0) {
        i0 = (int)(num / (2LL * out));
        l = __fdiv_rn((float)(int)(num - 2LL * out * i0), (float)(2 * out));
      }
      if (isx) { x0[d] = i0; xl[d] = l; } else { y0[d] = i0; yl[d] = l; }
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ngroups = (pw + 63) / 64;                 // a group: 64 words = 2048 pixels = 32 ballots of one wavefront
  int area = 0;
  for (int g = wave; g < ngroups; g += 4) {
    int p = g * 2048 + lane;
    int y = COPY ? 0 : p / W, x = COPY ? 0 : p - y * W;
    unsigned mine = 0;
    for (int j = 0; j < 32; ++j) {
      bool on = false;
      if (p < HW) {
        float v;
        if (COPY) {
          v = ip_load(src, (size_t)p);
        } else {
          const int xa = x0[x], xb = min(xa + 1, w - 1), ya = y0[y], yb = min(ya + 1, h - 1);
          const float lx = xl[x], ly = yl[y];
          const size_t ra = (size_t)ya * w, rb = (size_t)yb * w;
          const float v00 = ip_load(src, ra + xa), v01 = ip_load(src, ra + xb);
          const float v10 = ip_load(src, rb + xa), v11 = ip_load(src, rb + xb);
          v = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
        }
        on = v > thr;
      }
      const unsigned long long b = __ballot(on);
      area += __popcll(b);
      if ((lane >> 1) == j) mine = (lane & 1) ? (unsigned)(b >> 32) : (unsigned)b;
      p += 64;
      if (!COPY) {
        x += 64;
        while (x >= W) { x -= W; ++y; }
      }
    }
    const int word = g * 64 + lane;
    if (word < pw) dst[word] = mine;                  // the words past H*W (padding to PW) are written as zero
  }
  const int total = ip_block_sum(lane == 0 ? area : 0, scratch);
  if (threadIdx.x == 0) areas[plane] = total;
}

// ---- pairwise intersections ---------------------------------------------------------------------------------------------------
// grid (ceil(Q / 32), Q, N).  A wavefront takes plane i and eight partners j0 .. j0 + 7; only pairs with j >= i are computed and
// both inter[i][j] and inter[j][i] are written.  Pairs with a plane at or below min_area, or at or beyond the image's count, are
// left unwritten and never read.
__global__ __launch_bounds__(256) void ip_pair_kernel(const unsigned *__restrict__ planes, const int *__restrict__ areas,
                                                      const int *__restrict__ counts, int Q, int pw, int min_area,
                                                      int *__restrict__ inter)
{
  const int n = blockIdx.z, i = blockIdx.y, lane = threadIdx.x & 63;
  const int cnt = counts ? counts[4 * n] : Q;
  const int j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
  if (i >= cnt || j0 >= cnt || j0 + 7 < i) return;
  const int *a = areas + (size_t)n * Q;
  if (a[i] <= min_area) return;
  const unsigned *base = planes + (size_t)n * Q * pw;
  const uint4 *pi = reinterpret_cast<const uint4 *>(base + (size_t)i * pw);
  const uint4 *pj[8];
  int c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    pj[k] = reinterpret_cast<const uint4 *>(base + (size_t)min(j0 + k, cnt - 1) * pw);
    c[k] = 0;
  }
  for (int t = lane; t < pw / 4; t += 64) {
    const uint4 u = pi[t];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint4 v = pj[k][t];
      c[k] += __popc(u.x & v.x) + __popc(u.y & v.y) + __popc(u.z & v.z) + __popc(u.w & v.w);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = wave_sum(c[k]);
  if (lane == 0) {
    int *out = inter + (size_t)n * Q * Q;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = j0 + k;
      if (j < cnt && j >= i && a[j] > min_area) {
        out[(size_t)i * Q + j] = c[k];
        out[(size_t)j * Q + i] = c[k];
      }
    }
  }
}

// ---- keep, dice, first-come clustering (mask_post :403-431, dice_for :392-401) ------------------------------------------------
// counts[4 n] = number of clusters; cluster c: members[(n Q + c) QW ..] bit set of its queries, csize, csum = sum of their areas.
// soft (BBBC: no NMS follows): also the final order, ascending by csum / csize (compared exactly), stable by cluster index.
__global__ __launch_bounds__(256) void ip_cluster_kernel(const int *__restrict__ areas, const int *__restrict__ inter, int Q,
                                                         int soft, float thres1, unsigned *__restrict__ members,
                                                         int *__restrict__ csize, long long *__restrict__ csum,
                                                         int *__restrict__ order, int *__restrict__ counts)
{
  __shared__ int a[IP_MAX_Q];
  __shared__ unsigned M[IP_MAX_Q][IP_MAX_QW];
  __shared__ int reps[IP_MAX_Q];
  __shared__ int lsize[IP_MAX_Q];
  __shared__ long long lsum[IP_MAX_Q];
  __shared__ int nclus;
  const int n = blockIdx.x, QW = (Q + 31) / 32, tid = threadIdx.x;
  for (int q = tid; q < Q; q += 256) a[q] = areas[(size_t)n * Q + q];
  __syncthreads();
  for (int t = tid; t < Q * QW; t += 256) {
    const int i = t / QW, wd = t - i * QW;
    unsigned m = 0;
    if (a[i] > IP_MIN_AREA) {
      const int *row = inter + ((size_t)n * Q + i) * Q;
      for (int b = 0; b < 32; ++b) {
        const int j = wd * 32 + b;
        if (j < Q && a[j] > IP_MIN_AREA) {
          const float dice = __fdiv_rn((float)(2 * row[j] + 1), (float)(a[i] + a[j] + 1));
          if (dice > thres1) m |= 1u << b;
        }
      }
    }
    M[i][wd] = m;
  }
  __syncthreads();
  if (tid < 64) {                       // lane wd holds word wd of the set of queries already taken
    unsigned taken = 0;
    int C = 0;
    for (int i = 0; i < Q; ++i) {
      if (a[i] <= IP_MIN_AREA) continue;
      const unsigned t = __shfl(taken, i >> 5);
      if ((t >> (i & 31)) & 1u) continue;
      if (tid < QW) taken |= M[i][tid];   // not filtered against earlier clusters: a query can sit in two (:411-420)
      if (tid == 0) reps[C] = i;
      ++C;
    }
    if (tid == 0) nclus = C;
  }
  __syncthreads();
  const int C = nclus;
  for (int c = tid; c < C; c += 256) {
    const int r = reps[c];
    int size = 0;
    long long sum = 0;
    for (int wd = 0; wd < QW; ++wd) {
      unsigned m = M[r][wd];
      members[((size_t)n * Q + c) * QW + wd] = m;
      size += __popc(m);
      while (m) {
        sum += a[wd * 32 + __ffs(m) - 1];
        m &= m - 1;
      }
    }
    csize[(size_t)n * Q + c] = size;
    csum[(size_t)n * Q + c] = sum;
    lsize[c] = size;
    lsum[c] = sum;
  }
  __syncthreads();
  if (soft) {
    for (int c = tid; c < C; c += 256) {
      int rank = 0;
      for (int t = 0; t < C; ++t) {
        const long long lhs = lsum[t] * lsize[c], rhs = lsum[c] * lsize[t];     // area_t < area_c
        rank += (lhs < rhs || (lhs == rhs && t < c)) ? 1 : 0;
      }
      order[(size_t)n * Q + rank] = c;
    }
  }
  if (tid == 0) {
    counts[4 * n] = C;
    counts[4 * n + 1] = soft ? C : 0;
    counts[4 * n + 2] = 0;
    counts[4 * n + 3] = 0;
  }
}

// ---- merged planes ----------------------------------------------------------------------------------------------------------------
// grid N*Q: workgroup (n, c) does cluster c of image n, the others leave.  hard: pixel set where count / size > thres2 in fp32,
// i.e. count >= the smallest such count; soft: where count >= 1.  marea = popcount of the plane written.
__global__ __launch_bounds__(256) void ip_merge_kernel(const unsigned *__restrict__ bits, const unsigned *__restrict__ members,
                                                       const int *__restrict__ csize, const int *__restrict__ counts, int Q,
                                                       int pw, int soft, float thres2, unsigned *__restrict__ merged,
                                                       int *__restrict__ marea)
{
  __shared__ int mem[IP_MAX_Q];
  __shared__ int nmem, need;
  __shared__ int scratch[4];
  const int n = blockIdx.x / Q, c = blockIdx.x - n * Q, QW = (Q + 31) / 32;
  if (c >= counts[4 * n]) return;
  if (threadIdx.x == 0) {
    int k = 0;
    for (int wd = 0; wd < QW; ++wd) {
      unsigned m = members[((size_t)n * Q + c) * QW + wd];
      while (m) {
        mem[k++] = wd * 32 + __ffs(m) - 1;
        m &= m - 1;
      }
    }
    nmem = k;
    const int size = csize[(size_t)n * Q + c];
    int t = 1;
    if (!soft) {
      t = 0;
      while (t <= size && !(__fdiv_rn((float)t, (float)size) > thres2)) ++t;
    }
    need = t;
  }
  __syncthreads();
  const unsigned *base = bits + (size_t)n * Q * pw;
  unsigned *out = merged + ((size_t)n * Q + c) * pw;
  const int nm = nmem, below = need - 1;             // count >= need  <=>  count > below
  int area = 0;
  for (int wd = threadIdx.x; wd < pw; wd += 256) {
    unsigned cnt[10];                                // bit k of the 32 pixels' counts; a count is at most 512
#pragma unroll
    for (int k = 0; k < 10; ++k) cnt[k] = 0;
    for (int m = 0; m < nm; ++m) {
      unsigned x = base[(size_t)mem[m] * pw + wd];
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        const unsigned carry = cnt[k] & x;
        cnt[k] ^= x;
        x = carry;
      }
    }
    unsigned gt = 0, eq = ~0u;
#pragma unroll
    for (int k = 9; k >= 0; --k) {
      const unsigned tb = ((below >> k) & 1) ? ~0u : 0u;
      gt |= eq & cnt[k] & ~tb;
      eq &= ~(cnt[k] ^ tb);
    }
    out[wd] = gt;
    area += __popc(gt);
  }
  const int total = ip_block_sum(area, scratch);
  if (threadIdx.x == 0) marea[(size_t)n * Q + c] = total;
}

// ---- mask_nms (:357-390, comput_mmi :349-355) and the final sort (:333-335), CVPPP --------------------------------------------
__global__ __launch_bounds__(256) void ip_nms_kernel(const int *__restrict__ marea, const int *__restrict__ inter, int Q,
                                                     double thres, int *__restrict__ order, int *__restrict__ counts)
{
  __shared__ int a[IP_MAX_Q];
  __shared__ int ord[IP_MAX_Q];
  __shared__ int keep[IP_MAX_Q];
  __shared__ unsigned char sup[IP_MAX_Q];
  const int n = blockIdx.x, tid = threadIdx.x, C = counts[4 * n];
  for (int c = tid; c < C; c += 256) {
    a[c] = marea[(size_t)n * Q + c];
    sup[c] = 0;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {               // descending area; equal areas as a reversed stable ascending sort
    int rank = 0;
    for (int t = 0; t < C; ++t) rank += (a[t] > a[c] || (a[t] == a[c] && t > c)) ? 1 : 0;
    ord[rank] = c;
  }
  __syncthreads();
  int nk = 0;
  for (int i = 0; i < C; ++i) {
    const int idx = ord[i];
    // Uniform: sup[] is written only in the loop below, to entries later in the order than idx, and the barrier that ends an
    // iteration separates those writes from the next iteration's read.  The reference also compares idx with itself (its
    // inner loop starts at i) and suppresses it; that flag is never read again, so the self pair is left out here -- taking it
    // in would write sup[idx] while other wavefronts may still be reading it above.
    if (sup[idx]) continue;
    if (tid == 0) keep[nk] = idx;
    ++nk;
    const int *row = inter + ((size_t)n * Q + idx) * Q;
    for (int jj = i + 1 + tid; jj < C; jj += 256) {
      const int j = ord[jj];
      if (sup[j]) continue;
      double aa = a[idx], bb = a[j];
      const double I = row[j];
      if (aa == 0 || bb == 0) { aa += 0.00001; bb += 0.00001; }
      if (fmax(I / aa, I / bb) >= thres) sup[j] = 1;
    }
    __syncthreads();
  }
  __syncthreads();
  for (int s = tid; s < nk; s += 256) {              // ascending area, stable by position in the keep list
    const int as = a[keep[s]];
    int rank = 0;
    for (int t = 0; t < nk; ++t) {
      const int at = a[keep[t]];
      rank += (at < as || (at == as && t < s)) ? 1 : 0;
    }
    order[(size_t)n * Q + rank] = keep[s];
  }
  if (tid == 0) counts[4 * n + 1] = nk;
}

// ---- labels: argmax over [zeros, sorted masks] (:336-338) -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void ip_label_kernel(const unsigned *__restrict__ merged, const unsigned *__restrict__ bits,
                                                       const unsigned *__restrict__ members, const int *__restrict__ csize,
                                                       const int *__restrict__ order, const int *__restrict__ counts, int Q,
                                                       int HW, int pw, int soft, short *__restrict__ labels)
{
  __shared__ int ord[IP_MAX_Q];
  __shared__ int size[IP_MAX_Q];
  const int n = blockIdx.y, S = counts[4 * n + 1], QW = (Q + 31) / 32;
  for (int s = threadIdx.x; s < S; s += 256) {
    ord[s] = order[(size_t)n * Q + s];
    size[s] = csize[(size_t)n * Q + ord[s]];
  }
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int wd = p >> 5, bit = p & 31;
  const unsigned *mp = merged + (size_t)n * Q * pw + wd;
  int label = 0;
  if (!soft) {
    for (int s = 0; s < S; ++s)
      if ((mp[(size_t)ord[s] * pw] >> bit) & 1u) { label = s + 1; break; }
  } else {
    const unsigned *bp = bits + (size_t)n * Q * pw + wd;
    int bk = 0, bs = 1;
    for (int s = 0; s < S; ++s) {
      const int c = ord[s];
      if (!((mp[(size_t)c * pw] >> bit) & 1u)) continue;          // outside the cluster's support: its mean is 0 here
      int k = 0;
      for (int wq = 0; wq < QW; ++wq) {
        unsigned m = members[((size_t)n * Q + c) * QW + wq];
        while (m) {
          k += (bp[(size_t)(wq * 32 + __ffs(m) - 1) * pw] >> bit) & 1u;
          m &= m - 1;
        }
      }
      if (k * bs > bk * size[s]) { bk = k; bs = size[s]; label = s + 1; }     // strictly above: the first maximum stays
    }
  }
  labels[(size_t)n * HW + p] = (short)label;
}

template <typename T>
int threshold_launch(const void *logits, int N, int Q, int h, int w, int H, int W, int pw, float thr, unsigned *bits, int *areas,
                     hipStream_t stream)
{
  const dim3 grid((unsigned)((size_t)N * Q));
  if (h == H && w == W)
    hipLaunchKernelGGL((ip_threshold_kernel<T, true>), grid, dim3(256), 0, stream, static_cast<const T *>(logits), h, w, H, W, pw,
                       thr, bits, areas);
  else
    hipLaunchKernelGGL((ip_threshold_kernel<T, false>), grid, dim3(256), (size_t)(H + W) * 8, stream,
                       static_cast<const T *>(logits), h, w, H, W, pw, thr, bits, areas);
  return (int)hipGetLastError();
}

}  // namespace

int instance_geometry_status(int N, int Q, int H, int W)
{
  if (Q > IP_MAX_Q || N > 65535) return PCT_ERR_UNSUPPORTED;
  if (2LL * H * W + 1 >= (1LL << 24)) return PCT_ERR_UNSUPPORTED;      // areas and 2 I + 1 stay exact in fp32
  // the resize's tap tables: 8 (H + W) bytes of dynamic LDS beside 16 bytes of static, 64 016 bytes at the limit -- inside the
  // 64 KB a workgroup gets without asking for more
  if ((long long)H + W > IP_MAX_H_PLUS_W) return PCT_ERR_UNSUPPORTED;
  if ((long long)N * Q >= 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

int launch_instance_masks(const void *logits, int bf16, int N, int Q, int h, int w, int H, int W, int dataset, unsigned *bits,
                          int *areas, hipStream_t stream)
{
  IpParams prm;
  if (!ip_params(dataset, &prm)) return PCT_ERR_BAD_ARG;
  const int pw = 4 * ((H * W + 127) / 128);
  const float thr = (float)log(prm.threshold / (1.0 - prm.threshold));
  return bf16 ? threshold_launch<unsigned short>(logits, N, Q, h, w, H, W, pw, thr, bits, areas, stream)
              : threshold_launch<float>(logits, N, Q, h, w, H, W, pw, thr, bits, areas, stream);
}

int launch_instance_labels_from_bits(const unsigned *bits, const int *areas, int N, int Q, int H, int W, int dataset,
                                     void *workspace, short *labels, hipStream_t stream)
{
  IpParams prm;
  if (!ip_params(dataset, &prm)) return PCT_ERR_BAD_ARG;
  const int HW = H * W, pw = 4 * ((HW + 127) / 128), QW = (Q + 31) / 32;
  const size_t NQ = (size_t)N * Q;
  unsigned *merged = static_cast<unsigned *>(workspace);
  int *inter = reinterpret_cast<int *>(merged + NQ * pw);
  unsigned *members = reinterpret_cast<unsigned *>(inter + r4(NQ * Q));
  long long *csum = reinterpret_cast<long long *>(members + r4(NQ * QW));
  int *marea = reinterpret_cast<int *>(csum) + 2 * r4(NQ);
  int *csize = marea + r4(NQ);
  int *order = csize + r4(NQ);
  int *counts = order + r4(NQ);
  const dim3 pairs((Q + 31) / 32, Q, N);
  hipLaunchKernelGGL(ip_pair_kernel, pairs, dim3(256), 0, stream, bits, areas, (const int *)nullptr, Q, pw, IP_MIN_AREA, inter);
  hipLaunchKernelGGL(ip_cluster_kernel, dim3(N), dim3(256), 0, stream, areas, (const int *)inter, Q, prm.soft, prm.thres1,
                     members, csize, csum, order, counts);
  hipLaunchKernelGGL(ip_merge_kernel, dim3((unsigned)NQ), dim3(256), 0, stream, bits, (const unsigned *)members,
                     (const int *)csize, (const int *)counts, Q, pw, prm.soft, prm.thres2, merged, marea);
  if (!prm.soft) {
    hipLaunchKernelGGL(ip_pair_kernel, pairs, dim3(256), 0, stream, (const unsigned *)merged, (const int *)marea,
                       (const int *)counts, Q, pw, -1, inter);
    hipLaunchKernelGGL(ip_nms_kernel, dim3(N), dim3(256), 0, stream, (const int *)marea, (const int *)inter, Q, prm.nms, order,
                       counts);
  }
  hipLaunchKernelGGL(ip_label_kernel, dim3((HW + 255) / 256, N), dim3(256), 0, stream, (const unsigned *)merged, bits,
                     (const unsigned *)members, (const int *)csize, (const int *)order, (const int *)counts, Q, HW, pw, prm.soft,
                     labels);
  return (int)hipGetLastError();
}

int launch_instance_labels(const void *logits, int bf16, int N, int Q, int h, int w, int H, int W, int dataset, void *workspace,
                           short *labels, hipStream_t stream)
{
  const int pw = 4 * ((H * W + 127) / 128);
  const size_t NQ = (size_t)N * Q;
  unsigned *bits = static_cast<unsigned *>(workspace);
  int *areas = reinterpret_cast<int *>(bits + NQ * pw);
  const int rc = launch_instance_masks(logits, bf16, N, Q, h, w, H, W, dataset, bits, areas, stream);
  if (rc != 0) return rc;
  return launch_instance_labels_from_bits(bits, areas, N, Q, H, W, dataset, areas + r4(NQ), labels, stream);
}

}  // namespace pct
