// Pixel-embedding loss on the device (include/pctrans_hip_train.h: pct_instance_label_map_f32,
// pct_discriminative_loss_forward_f32, pct_discriminative_loss_backward_f32): SetCriterion.loss_embedding and
// discriminative_loss of pctrans_amd/loss/maskformer_criterion.py without the resized mask stack, torch.unique, the one-hot
// membership matrix and the chain of small launches.
//
// Forward, six launches on one stream, nothing allocated, no host synchronisation, no floating-point atomic:
//   A   sums_kernel<false>   per-label channel sums and counts of one (chunk of pixels, tile of 32 labels, image)
//       combine_kernel<0>    the chunks added in ascending order: count and centroid mu_g into the table
//   B   sums_kernel<true>    per-label sum (r_p - delta_v)^2 and S_g = sum 2 (r_p - delta_v)(e_p - mu_g) / r_p, same structure
//       combine_kernel<1>    the chunks added in ascending order into the table
//   C   centroid_kernel      32 labels per workgroup against all labels: the pairwise term and its gradient, the regulariser,
//                            c_g and T_g into the table, three partial sums per workgroup
//       finish_kernel        workgroups, then images, added in ascending order: the loss, and the status word
//
// The sums over pixels are emb[E, P] . onehot[P, L] on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation: bit for bit an
// fmaf chain in ascending k).  A workgroup is ONE wave.  It walks its chunk in passes of EL_SUB = 256 pixels: the labels of the
// pass go to LDS, a pass without a label of the tile is skipped, the A operand (channel i of pixel p: the embedding in pass A,
// w_p (e_p - mu_g) in pass B, 0 for a pixel whose label is outside the tile) is staged in LDS as es[channel][pixel] with a row
// stride of 258 words -- the staging writes (lanes along the pixels) and the operand reads (lane (i, kh) reads es[i][2 s + kh]:
// bank 2 i + kh + 2 s) both touch 64 different banks -- and the B operand (k = kh, column j) is label[2 s + kh] == 32 tile + j,
// formed in registers.  With a 0 / 1 operand every product is exact, so a label's sum is the fp32 sum of its pixels of the chunk
// in ascending pixel order; the chunks are added in ascending order.  The count is an integer sum of the B operands a lane forms
// anyway; sum (r - delta_v)^2 a lane's running sum over its pixels (even pixels in lanes kh = 0, odd in kh = 1, added at the end).
// Background (label 0) and labels outside [0, L] belong to no tile: row 0 of the table is zero.
//
// More than 32 channels (the model's pixel embedding has CONVS_DIM = 128): the channels go in tiles of 32, one workgroup of passes
// A and B per (chunk, channel tile, label tile, image), each staging its own 32 rows of es -- a channel's sum is the same fmaf chain
// as before, and pass B forms r_p over ALL channels (pixel_weight) in every channel tile.  The channel tiles are 1, 2 or 4 (nch =
// 32, 64, 128 channel slots): a slot of the workspace is nch + 2 floats, a row of the table 4 + 2 nch (mu_g at 4, T_g at 4 + nch).
// Up to 32 channels that is the layout and the arithmetic of the single-tile kernel, bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.hpp"
#include "wave_reduce.hpp"

namespace pct {

namespace {

constexpr int EL_SUB = 256;               // pixels of one pass
constexpr int EL_ES = EL_SUB + 2;         // row stride of es in words
constexpr int EL_MAX_CHUNKS = 64;         // of the pixels of an image: bounds the workspace
constexpr int EL_MAX_E = 128;             // four channel tiles
constexpr int EL_CT = 32;                 // channels of one tile: the rows of the MFMA
constexpr int EL_MAX_L = 1024;
constexpr int EL_SLOT = 34;               // floats of one label of one chunk at nch = 32: nch channel sums, the count (int), sum (r - dv)^2
constexpr int EL_ROW = 68;                // floats of one label of the table at nch = 32: 4 + 2 nch
constexpr int EL_N = 0, EL_C = 1, EL_Q = 2, EL_MU = 4;      // count, c_g, sum (r - dv)^2, mu_g[nch]; then T_g[nch] (S_g before C)
constexpr int EL_CBLOCK = 256;            // pass C: 32 labels x 8 slices of the other labels
static_assert(EL_SLOT == EL_CT + 2 && EL_ROW == 4 + 2 * EL_CT, "the single-tile layout");

typedef float el_f16 __attribute__((ext_vector_type(16)));

struct EmbLossPlan {
  int passes, chunks, tiles, lblocks;     // passes of EL_SUB pixels per chunk; tiles of 32 labels over 0 .. L; blocks of pass C
  int ctiles, nch, slot, row;             // channel tiles (1, 2, 4), channel slots 32 ctiles, floats of a workspace slot / table row
  long long partial, bad, part;           // offsets (floats) of the three regions of the workspace, `partial` = 0
};

inline EmbLossPlan emb_loss_plan(const int B, const long long P, const int L, const int E)
{
  EmbLossPlan m;
  const ChunkPlan cp = chunk_plan(P, EL_SUB, EL_MAX_CHUNKS);
  m.passes = cp.passes;
  m.chunks = cp.chunks;
  m.tiles = L / 32 + 1;
  m.lblocks = (L + 31) / 32;
  m.ctiles = E <= 32 ? 1 : E <= 64 ? 2 : 4;
  m.nch = EL_CT * m.ctiles;
  m.slot = m.nch + 2;
  m.row = 4 + 2 * m.nch;
  m.partial = 0;
  m.bad = (long long)B * m.chunks * m.tiles * 32 * m.slot;
  m.part = m.bad + (long long)B * m.chunks;
  return m;
}

// r_p = |e_p - mu_g| (an fmaf chain over the channels in ascending order) and w_p = 2 (r_p - delta_v) / r_p, 0 where r_p = 0 as
// torch's norm backward makes it.  Pass B and the backward both call this: the same bits.
__device__ __forceinline__ float pixel_weight(const float *__restrict__ e, const size_t stride, const float *__restrict__ mu,
                                              const int E, const float delta_v, float &r)
{
  float r2 = 0.f;
  for (int c = 0; c < E; ++c) {
    const float d = e[c * stride] - mu[c];
    r2 = fmaf(d, d, r2);
  }
  r = sqrtf(r2);
  return r > 0.f ? 2.f * (r - delta_v) / r : 0.f;
}

template <bool PASS_B>
__global__ __launch_bounds__(64) void sums_kernel(const float *__restrict__ emb, const int *__restrict__ labels,
                                                  const float *__restrict__ table, const int E, const int P, const int L,
                                                  const float delta_v, const EmbLossPlan plan, float *__restrict__ ws)
{
  __shared__ float es[EL_CT * EL_ES];
  __shared__ float qs[EL_SUB];
  __shared__ int ls[EL_SUB];
  const int chunk = blockIdx.x % plan.chunks, ct = blockIdx.x / plan.chunks, tile = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x, col = lane & 31, kh = lane >> 5;
  const int c0 = ct * EL_CT, ce = min(EL_CT, E - c0);                       // this workgroup's channels c0 .. c0 + ce (ce may be <= 0)
  const float *eb = emb + (size_t)b * E * P;
  const int *lb = labels + (size_t)b * P;
  const int g0 = tile * 32;

  el_f16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  int cnt = 0, bad = 0;
  float qsum = 0.f;

  for (int pass = 0; pass < plan.passes; ++pass) {
    const long long p0 = ((long long)chunk * plan.passes + pass) * EL_SUB;
    if (p0 >= P) break;                                                     // (uniform)
    __syncthreads();                                                        // the previous pass has read ls, es, qs
    int mine[EL_SUB / 64];
    bool any = false;
#pragma unroll
    for (int k = 0; k < EL_SUB / 64; ++k) {
      const long long p = p0 + k * 64 + lane;
      int g = -1;
      if (p < P) {
        g = lb[p];
        if (g < 0 || g > L) ++bad;
        if (g < 1 || g > L) g = -1;
      }
      mine[k] = g;
      ls[k * 64 + lane] = g;
      any |= (unsigned)(g - g0) < 32u;
    }
    if (!__any(any)) continue;                                              // (uniform: the workgroup is one wave)
#pragma unroll
    for (int k = 0; k < EL_SUB / 64; ++k) {
      const int pix = k * 64 + lane, g = mine[k];
      if ((unsigned)(g - g0) < 32u) {
        const float *e = eb + (p0 + pix);
        if (PASS_B) {
          const float *mu = table + ((size_t)b * (L + 1) + g) * plan.row + EL_MU;
          float r;
          const float w = pixel_weight(e, (size_t)P, mu, E, delta_v, r);
          for (int c = 0; c < ce; ++c) es[c * EL_ES + pix] = w * (e[(size_t)(c0 + c) * P] - mu[c0 + c]);
          qs[pix] = (r - delta_v) * (r - delta_v);
        } else {
          for (int c = 0; c < ce; ++c) es[c * EL_ES + pix] = e[(size_t)(c0 + c) * P];
        }
      } else {
        for (int c = 0; c < ce; ++c) es[c * EL_ES + pix] = 0.f;
        if (PASS_B) qs[pix] = 0.f;
      }
    }
    __syncthreads();
    const bool row_ok = col < ce;
#pragma unroll 4
    for (int s = 0; s < EL_SUB / 2; ++s) {
      const int pix = 2 * s + kh;
      const bool hit = ls[pix] == g0 + col;
      const float a = row_ok ? es[col * EL_ES + pix] : 0.f;
      cnt += hit ? 1 : 0;
      if (PASS_B) qsum += hit ? qs[pix] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, hit ? 1.f : 0.f, acc, 0, 0, 0);
    }
  }

  // acc[r] = D[row 8 (r / 4) + 4 kh + r % 4][column col]: row = channel, column = label of the tile
  float *slot = ws + (((size_t)b * plan.chunks + chunk) * plan.tiles * 32 + g0 + col) * plan.slot;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 8 * (r / 4) + 4 * kh + r % 4;
    if (row < ce) slot[c0 + row] = acc[r];
  }
  cnt += __shfl_xor(cnt, 32, 64);                                           // even pixels + odd pixels
  qsum += __shfl_xor(qsum, 32, 64);
  if (kh == 0 && ct == 0) {                                                 // (every channel tile counts the same: the first writes)
    slot[plan.nch] = __int_as_float(cnt);
    slot[plan.nch + 1] = qsum;
  }
  if (!PASS_B && tile == 0 && ct == 0) {
    bad = wave_sum(bad);
    if (lane == 0) reinterpret_cast<int *>(ws + plan.bad)[(size_t)b * plan.chunks + chunk] = bad;
  }
}

// One thread per (image, label 0 .. L, slot): the chunks in ascending order.  MODE 0 (after pass A) writes the whole row of the
// table: count, centroid (0 for an absent label and for the channels past E), zeros elsewhere.  MODE 1 (after pass B) writes
// S_g into the T slots and sum (r - delta_v)^2.
template <int MODE>
__global__ __launch_bounds__(256) void combine_kernel(const float *__restrict__ ws, const int E, const int L, const long long total,
                                                      const EmbLossPlan plan, float *__restrict__ table)
{
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int nch = plan.nch, EL_T = EL_MU + nch;
  const int k = (int)(i % plan.slot);
  const long long bg = i / plan.slot;
  const int g = (int)(bg % (L + 1)), b = (int)(bg / (L + 1));
  const size_t per_chunk = (size_t)plan.tiles * 32 * plan.slot;
  const float *w = ws + (size_t)b * plan.chunks * per_chunk + (size_t)g * plan.slot;
  float *row = table + (size_t)bg * plan.row;
  float sum = 0.f;
  int n = 0;
  const bool has_sum = g > 0 && (k < E || (MODE == 1 && k == nch + 1));
  for (int ch = 0; ch < plan.chunks; ++ch, w += per_chunk) {
    if (has_sum) sum += w[k];
    if (MODE == 0 && g > 0) n += __float_as_int(w[nch]);
  }
  if (MODE == 0) {
    if (k < nch) {
      row[EL_MU + k] = (has_sum && n > 0) ? sum / (float)n : 0.f;
      row[EL_T + k] = 0.f;
    } else if (k == nch) {
      row[EL_N] = (float)n;
      row[EL_C] = 0.f;
    } else {
      row[EL_Q] = 0.f;
      row[3] = 0.f;
    }
  } else {
    if (k < nch) row[EL_T + k] = has_sum ? sum : 0.f;
    else if (k == nch + 1) row[EL_Q] = has_sum ? sum : 0.f;
  }
}

// Pass C.  Thread (il, s) = (tid / 8, tid % 8): label i = 32 blockIdx.x + il + 1 against the labels j = 1 + s, 9 + s, ...; the
// eight slices are added by a butterfly over the lanes (the same sum in every lane).  Only present labels (count > 0) enter.
template <int NCH>
__global__ __launch_bounds__(EL_CBLOCK) void centroid_kernel(float *__restrict__ table, const int B, const int E, const int L,
                                                             const float delta_d, const float alpha, const float beta,
                                                             const float gama, const EmbLossPlan plan, float *__restrict__ ws)
{
  __shared__ int s_count[EL_CBLOCK / 64];
  __shared__ float s_part[EL_CBLOCK / 64][3];
  constexpr int EL_ROW = 4 + 2 * NCH, EL_T = EL_MU + NCH;                   // this instance's table row
  const int b = blockIdx.y, tid = threadIdx.x, il = tid >> 3, s = tid & 7, lane = tid & 63, wave = tid >> 6;
  float *tb = table + (size_t)b * (L + 1) * EL_ROW;

  int present = 0;
  for (int g = 1 + tid; g <= L; g += EL_CBLOCK) present += tb[(size_t)g * EL_ROW + EL_N] > 0.f ? 1 : 0;
  present = wave_sum(present);
  if (lane == 0) s_count[wave] = present;
  __syncthreads();
  int num_id = 0;
#pragma unroll
  for (int w = 0; w < EL_CBLOCK / 64; ++w) num_id += s_count[w];

  const int i = blockIdx.x * 32 + il + 1;
  const bool valid = i <= L;
  float *row = tb + (size_t)(valid ? i : 0) * EL_ROW;
  const float n_i = valid ? row[EL_N] : 0.f;
  const bool here = n_i > 0.f;

  float mu[NCH], acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    mu[c] = (c < E && here) ? row[EL_MU + c] : 0.f;
    acc[c] = 0.f;
  }
  float dist = 0.f;
  if (num_id > 1) {                                                         // (uniform)
    for (int j = 1 + s; j <= L; j += 8) {
      const float *rj = tb + (size_t)j * EL_ROW;
      if (!here || j == i || !(rj[EL_N] > 0.f)) continue;
      float d2 = 0.f, diff[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        diff[c] = 0.f;
        if (c < E) {
          diff[c] = mu[c] - rj[EL_MU + c];
          d2 = fmaf(diff[c], diff[c], d2);
        }
      }
      const float d = sqrtf(d2), h = fmaxf(delta_d - d, 0.f);
      dist = fmaf(h, h, dist);
      if (d > 0.f && h > 0.f) {
        const float k = h / d;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
          if (c < E) acc[c] = fmaf(k, diff[c], acc[c]);
      }
    }
#pragma unroll
    for (int m = 1; m <= 4; m <<= 1) {
      dist += __shfl_xor(dist, m, 64);
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (c < E) acc[c] += __shfl_xor(acc[c], m, 64);
    }
  }

  float var_i = 0.f, reg_i = 0.f, dist_i = 0.f;
  if (here && s == 0) {
    float m2 = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < E) m2 = fmaf(mu[c], mu[c], m2);
    const float norm = sqrtf(m2), fB = (float)B, fid = (float)num_id;
    var_i = row[EL_Q] / n_i;
    reg_i = norm;
    dist_i = dist;
    const float c_i = alpha / (fB * fid * n_i);
    const float kd = num_id > 1 ? -2.f * beta / (fid * (fid - 1.f)) : 0.f;  // beta d dist / d mu_i = kd * acc
    const float kr = norm > 0.f ? gama / (norm * fid) : 0.f;                // gama d reg / d mu_i = kr * mu_i
    const float inv = 1.f / (fB * n_i);
    row[EL_C] = c_i;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c < E) row[EL_T + c] = -c_i * row[EL_T + c] / n_i + (kd * acc[c] + kr * mu[c]) * inv;
  }
  // the workgroup's three sums: a butterfly inside each wave, the waves in ascending order
  var_i = wave_sum(var_i);
  dist_i = wave_sum(dist_i);
  reg_i = wave_sum(reg_i);
  if (lane == 0) {
    s_part[wave][0] = var_i;
    s_part[wave][1] = dist_i;
    s_part[wave][2] = reg_i;
  }
  __syncthreads();
  if (tid == 0) {
    float v = 0.f, d = 0.f, r = 0.f;
#pragma unroll
    for (int w = 0; w < EL_CBLOCK / 64; ++w) {
      v += s_part[w][0];
      d += s_part[w][1];
      r += s_part[w][2];
    }
    float *out = ws + plan.part + ((size_t)b * plan.lblocks + blockIdx.x) * 4;
    out[0] = v;
    out[1] = d;
    out[2] = r;
    out[3] = __int_as_float(num_id);
  }
}

// One wave.  Lane k holds the three sums of workgroup k of pass C (at most 32); lane 0 adds them in ascending order, then the
// images in ascending order.  The status word is an integer sum.
__global__ __launch_bounds__(64) void finish_kernel(const float *__restrict__ ws, const int B, const float alpha, const float beta,
                                                    const float gama, const EmbLossPlan plan, float *__restrict__ loss,
                                                    int *__restrict__ status)
{
  const int lane = threadIdx.x;
  float tv = 0.f, td = 0.f, tr = 0.f;
  for (int b = 0; b < B; ++b) {
    const float *p = ws + plan.part + ((size_t)b * plan.lblocks + (lane < plan.lblocks ? lane : 0)) * 4;
    const float pv = p[0], pd = p[1], pr = p[2];
    const int num_id = __float_as_int(p[3]);
    float v = 0.f, d = 0.f, r = 0.f;
    for (int k = 0; k < plan.lblocks; ++k) {
      v += __shfl(pv, k, 64);
      d += __shfl(pd, k, 64);
      r += __shfl(pr, k, 64);
    }
    if (num_id > 0) {
      const float fid = (float)num_id;
      tv += v / fid;
      if (num_id > 1) td += d / (fid * (fid - 1.f)) / 2.f;
      tr += r / fid;
    }
  }
  const int *badp = reinterpret_cast<const int *>(ws + plan.bad);
  int bad = 0;
  for (long long k = lane; k < (long long)B * plan.chunks; k += 64) bad += badp[k];
  bad = wave_sum(bad);
  if (lane == 0) {
    const float fB = (float)B;
    *loss = alpha * tv / fB + beta * td / fB + gama * tr / fB;
    *status = bad;
  }
}

__global__ __launch_bounds__(256) void emb_loss_backward_kernel(const float *__restrict__ emb, const int *__restrict__ labels,
                                                                const float *__restrict__ table,
                                                                const float *__restrict__ grad_out, const int E, const int P,
                                                                const int L, const int nch, const float delta_v,
                                                                float *__restrict__ grad)
{
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (p >= P) return;
  const int g = labels[(size_t)b * P + p];
  const size_t at = (size_t)b * E * P + p;
  if (g < 1 || g > L) {
    for (int c = 0; c < E; ++c) grad[at + (size_t)c * P] = 0.f;
    return;
  }
  const float *row = table + ((size_t)b * (L + 1) + g) * (4 + 2 * nch);
  const float *mu = row + EL_MU, *T = row + EL_MU + nch;
  const float go = *grad_out;
  float r;
  const float k = row[EL_C] * pixel_weight(emb + at, (size_t)P, mu, E, delta_v, r);
  for (int c = 0; c < E; ++c) grad[at + (size_t)c * P] = go * fmaf(k, emb[at + (size_t)c * P] - mu[c], T[c]);
}

// label = 1 + the lowest g with plane[g][sy][sx] > 0 (NaN is not), else 0; (sy, sx) torch's legacy nearest source index
__global__ __launch_bounds__(256) void label_map_kernel(const float *__restrict__ planes, const int num_planes, const int Ht,
                                                        const int Wt, const int *__restrict__ start, const int *__restrict__ count,
                                                        const int h, const int w, const float scale_y, const float scale_x,
                                                        int *__restrict__ labels)
{
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= (long long)h * w) return;
  const int y = (int)(i / w), x = (int)(i - (long long)y * w);
  const int sy = min((int)floorf((float)y * scale_y), Ht - 1), sx = min((int)floorf((float)x * scale_x), Wt - 1);
  const size_t plane = (size_t)Ht * Wt, off = (size_t)sy * Wt + sx;
  const int first = start[b], n = count[b];
  int label = 0;
  for (int g = 0; g < n; ++g) {
    const long long pl = (long long)first + g;
    if (pl < 0 || pl >= num_planes) continue;                               // outside the planes: nothing is read
    if (planes[(size_t)pl * plane + off] > 0.f) {
      label = g + 1;
      break;
    }
  }
  labels[(size_t)b * h * w + i] = label;
}

}  // namespace

int emb_loss_geometry_status(int B, int E, int h, int w, int L)
{
  if (E > EL_MAX_E || L > EL_MAX_L) return PCT_ERR_UNSUPPORTED;
  if ((long long)h * w >= 0x7fffffffLL || B > 65535) return PCT_ERR_UNSUPPORTED;
  return PCT_OK;
}

int launch_instance_label_map(const float *planes, int num_planes, int Ht, int Wt, const int *start, const int *count, int B, int h,
                              int w, int *labels, hipStream_t stream)
{
  if ((long long)h * w >= 0x7fffffffLL || (long long)Ht * Wt >= 0x7fffffffLL || B > 65535) return PCT_ERR_UNSUPPORTED;
  const long long P = (long long)h * w;
  label_map_kernel<<<dim3((unsigned)((P + 255) / 256), (unsigned)B), dim3(256), 0, stream>>>(
      planes, num_planes, Ht, Wt, start, count, h, w, (float)Ht / (float)h, (float)Wt / (float)w, labels);
  return (int)hipGetLastError();
}

int launch_emb_loss_forward(const float *emb, const int *labels, int B, int E, int h, int w, int L, float delta_v, float delta_d,
                            float alpha, float beta, float gama, void *workspace, float *table, float *loss, int *status,
                            hipStream_t stream)
{
  if (const int rc = emb_loss_geometry_status(B, E, h, w, L); rc != PCT_OK) return rc;
  const int P = h * w;
  const EmbLossPlan plan = emb_loss_plan(B, P, L, E);
  float *ws = static_cast<float *>(workspace);
  const dim3 grid((unsigned)(plan.chunks * plan.ctiles), (unsigned)plan.tiles, (unsigned)B);       // at most 64 x 4 in x
  const long long total = (long long)B * (L + 1) * plan.slot;
  const dim3 cgrid((unsigned)((total + 255) / 256));
  sums_kernel<false><<<grid, dim3(64), 0, stream>>>(emb, labels, table, E, P, L, delta_v, plan, ws);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  combine_kernel<0><<<cgrid, dim3(256), 0, stream>>>(ws, E, L, total, plan, table);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  sums_kernel<true><<<grid, dim3(64), 0, stream>>>(emb, labels, table, E, P, L, delta_v, plan, ws);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  combine_kernel<1><<<cgrid, dim3(256), 0, stream>>>(ws, E, L, total, plan, table);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  const dim3 pgrid((unsigned)plan.lblocks, (unsigned)B);
  if (plan.nch == 32) centroid_kernel<32><<<pgrid, dim3(EL_CBLOCK), 0, stream>>>(table, B, E, L, delta_d, alpha, beta, gama, plan, ws);
  else if (plan.nch == 64) centroid_kernel<64><<<pgrid, dim3(EL_CBLOCK), 0, stream>>>(table, B, E, L, delta_d, alpha, beta, gama, plan, ws);
  else centroid_kernel<128><<<pgrid, dim3(EL_CBLOCK), 0, stream>>>(table, B, E, L, delta_d, alpha, beta, gama, plan, ws);
  if (const int rc = (int)hipGetLastError(); rc != 0) return rc;
  finish_kernel<<<dim3(1), dim3(64), 0, stream>>>(ws, B, alpha, beta, gama, plan, loss, status);
  return (int)hipGetLastError();
}

int launch_emb_loss_backward(const float *emb, const int *labels, const float *table, const float *grad_out, int B, int E, int h,
                             int w, int L, float delta_v, float *grad_emb, hipStream_t stream)
{
  if (const int rc = emb_loss_geometry_status(B, E, h, w, L); rc != PCT_OK) return rc;
  const int P = h * w;
  const int nch = emb_loss_plan(B, P, L, E).nch;
  emb_loss_backward_kernel<<<dim3((unsigned)((P + 255) / 256), (unsigned)B), dim3(256), 0, stream>>>(emb, labels, table, grad_out, E,
                                                                                                    P, L, nch, delta_v, grad_emb);
  return (int)hipGetLastError();
}

}  // namespace pct
