// Backward of the fp32 per-query dynamic mask head for MI355X (gfx950, wave64): the training-path counterpart of
// dyn_mask_head.hip (out_dtype = 0), i.e. what autograd computes for the reference's dynamic_mask_with_coords +
// mask_heads_forward (transformer_decoder/mask2former_transformer_decoder.py:647-719) from the gradient of the
// x2-upsampled logits.  The attention mask is detached there and carries no gradient.
//
// Nothing is saved by the forward: per (image n, query q, pixel p), with in = [rel_x, rel_y, F(0..15)],
//     g      = adjoint of upsample_bilinear2d (x2, align_corners = False) applied to grad_up     (16 taps, in registers)
//     a0,x0,a1,x1 recomputed with the forward kernel's fmaf chains (so the ReLU gates are the forward's gates)
//     dx1 = g w2 [a1 > 0]      dx0 = W1^T dx1 [a0 > 0]      grad_feat[:, p] += W0[:, 2:]^T dx0      (summed over q)
//     db2 += g   dw2 += g x1   db1 += dx1   dW1 += dx1 (x) x0   db0 += dx0   dW0 += dx0 (x) in      (summed over p)
//     grad_ref[q] = (W stride, H stride) o sum_k w0[k, 0:2] db0[k]
//
// Decomposition.  One wave owns a tile of 128 consecutive pixels of one image (2 per lane) and walks a group of queries:
// the tile's features and its grad_feat accumulators stay in registers over the whole walk and are stored once.  The sums
// over pixels are ONE matrix product per (tile, query) on the matrix cores, K = pixel:
//     rows  A = [dx0 (8) | dx1 (8) | g | x1 (8)]          columns  B = [F (16) | rel (2) | x0 (8) | 1 | g]
// through LDS (lane = pixel on the way in, lane = matrix row / column on the way out), 64 v_mfma_f32_32x32x2_f32 per query;
// the 233 wanted entries of the 32 x 32 product (dW0, db0, dW1, db1, db2, dw2) go to a per-(tile, query) slot of the
// workspace.  Two small kernels finish: one adds the tiles in a fixed order and forms grad_ref, one adds the query groups
// of grad_feat.  No atomics anywhere and every sum has a fixed order: results are bit-identical from run to run.
// All global writes are plain vector stores; the generated parameters are read through scalar loads as in the forward.
#include "launchers.hpp"

namespace pct {

constexpr int DB_HID = 8;
constexpr int DB_C = 16;
constexpr int DB_PX = 2;                  // 64-pixel chunks per wave
constexpr int DB_TILE = 64 * DB_PX;       // pixels per wave
constexpr int DB_S = 65;                  // LDS row stride in floats (64 pixels + 1: the 32 rows of an operand read fall in 32
                                          // banks; the two K halves of a read still meet two-way, lane (i, 1) with (i + 1, 0))
constexpr int DB_AROWS = 25;              // dx0 0-7 | dx1 8-15 | g 16 | x1 17-24
constexpr int DB_BROWS = 10;              // rel_x, rel_y | x0 0-7      (columns 16-25; features are columns 0-15)
constexpr int DB_MAX_QSPLIT = 8;          // query groups per tile (grad_feat partials in the workspace)
constexpr int DB_COL_ONE = 26, DB_COL_G = 27;

typedef float db_f16 __attribute__((ext_vector_type(16)));
typedef float db_f2 __attribute__((ext_vector_type(2)));

template <bool REL>
__global__ __launch_bounds__(64) void dyn_mask_head_bwd_kernel(
    const float *__restrict__ feat,     // [N, 16, H, W]
    const float *__restrict__ ref,      // [N, Q, 2]
    const float *__restrict__ params,   // [N, Q, G]
    const float *__restrict__ gup,      // [N, Q, 2H, 2W]
    const int Q, const int H, const int W, const int stride, const int ntiles, const int qsplit, const int qper,
    float *__restrict__ ws_par,         // [N, ntiles, Q, G]   per-tile parameter-gradient partials
    float *__restrict__ gfeat)          // [N, qsplit, 16, H, W]   (grad_feat itself when qsplit == 1)
{
  constexpr int C = DB_C, CIN = REL ? C + 2 : C, FOFF = REL ? 2 : 0;
  constexpr int O1 = CIN * DB_HID, O2 = O1 + DB_HID * DB_HID, OB0 = O2 + DB_HID, OB1 = OB0 + DB_HID, OB2 = OB1 + DB_HID;
  constexpr int G = OB2 + 1;
  constexpr int SM_F = 0, SM_A = DB_PX * C * DB_S, SM_B = SM_A + DB_AROWS * DB_S;
  __shared__ float sm[SM_B + DB_BROWS * DB_S];

  const int lane = (int)threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)ntiles);
  const int grp = (int)((blockIdx.x / (unsigned)ntiles) % (unsigned)qsplit);
  const int n = (int)(blockIdx.x / ((unsigned)ntiles * (unsigned)qsplit));
  const int q0 = grp * qper, q1 = min(q0 + qper, Q);
  const int HW = H * W, OW = 2 * W;
  const float half = (float)(stride / 2);

  // ---- per-pixel constants: features, pixel centre, the 4 x 4 taps of the upsample's adjoint -----------------------
  float f[DB_PX][C], gf[DB_PX][C], cx[DB_PX], cy[DB_PX], wx[DB_PX][4], wy[DB_PX][4];
  int roff[DB_PX][4], c0[DB_PX], c1[DB_PX], c3[DB_PX];
#pragma unroll
  for (int j = 0; j < DB_PX; ++j) {
    const int p = tile * DB_TILE + j * 64 + lane;
    const bool valid = p < HW;
    const int pc = valid ? p : HW - 1;                         // tail lanes recompute the last pixel with zero taps
    const int y = pc / W, x = pc - y * W;
    const float *fp = feat + (size_t)n * C * HW + pc;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      f[j][c] = fp[(size_t)c * HW];
      gf[j][c] = 0.f;
      sm[SM_F + (j * C + c) * DB_S + lane] = f[j][c];
    }
    cx[j] = (float)(x * stride) + half;
    cy[j] = (float)(y * stride) + half;
    // out[o] = (1 - lam) in[i0] + lam in[i1] with src = o / 2 - 0.25 clamped at 0 and i1 clamped at the last element:
    // in[x] receives 0.25 out[2x-1] + 0.75 out[2x] + 0.75 out[2x+1] + 0.25 out[2x+2]; at a border the missing tap's
    // weight falls on its inner neighbour (0.75 -> 1)
    const bool xl = x > 0, xr = x < W - 1, yt = y > 0, yb = y < H - 1;
    wx[j][0] = xl ? 0.25f : 0.f;  wx[j][1] = xl ? 0.75f : 1.f;  wx[j][2] = xr ? 0.75f : 1.f;  wx[j][3] = xr ? 0.25f : 0.f;
    wy[j][0] = yt ? 0.25f : 0.f;  wy[j][1] = yt ? 0.75f : 1.f;  wy[j][2] = yb ? 0.75f : 1.f;  wy[j][3] = yb ? 0.25f : 0.f;
    if (!valid) wy[j][0] = wy[j][1] = wy[j][2] = wy[j][3] = 0.f;
    c0[j] = xl ? 2 * x - 1 : 0;
    c1[j] = 2 * x;
    c3[j] = xr ? 2 * x + 2 : 2 * x + 1;
    roff[j][0] = (yt ? 2 * y - 1 : 0) * OW;
    roff[j][1] = (2 * y) * OW;
    roff[j][2] = (2 * y + 1) * OW;
    roff[j][3] = (yb ? 2 * y + 2 : 2 * y + 1) * OW;
  }

  // ---- this lane's place in the matrix product: A row / B column lane & 31, K half lane >> 5 ----------------------
  const int mi = lane & 31, mh = lane >> 5;
  const int a_off = SM_A + (mi < DB_AROWS ? mi : DB_AROWS - 1) * DB_S + mh;      // rows past the 25th: unused results
  int b_off[DB_PX];
#pragma unroll
  for (int j = 0; j < DB_PX; ++j)
    b_off[j] = (mi < C ? SM_F + (j * C + mi) * DB_S                           // features
                : (mi < DB_COL_ONE && (REL || mi >= C + 2)) ? SM_B + (mi - C) * DB_S   // rel (written with REL only), x0
                : SM_A + 16 * DB_S) + mh;                                      // g; also every column whose result is unused
  const bool b_one = mi == DB_COL_ONE;

  for (int q = q0; q < q1; ++q) {
    const size_t nq = (size_t)n * Q + q;
    // the generated parameters are wave-uniform: scalar loads from the constant address space.  Kept live from the
    // forward recompute to their second use they exceed the SGPR file and spill to VGPR lanes, so the pointer is
    // laundered per stage and each stage fetches what it uses from the scalar cache
    typedef const __attribute__((address_space(4))) float *cfloat_p;
    unsigned long long praw = (unsigned long long)(params + nq * G);
    asm volatile("" : "+s"(praw));
    cfloat_p w0 = (cfloat_p)praw, w1 = w0 + O1, b0 = w0 + OB0, b1 = w0 + OB1;

    float g[DB_PX];
    {
      const float *gq = gup + nq * 4 * (size_t)HW;
#pragma unroll
      for (int j = 0; j < DB_PX; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float *row = gq + roff[j][r];
          const db_f2 m = *reinterpret_cast<const db_f2 *>(row + c1[j]);
          const float t = wx[j][0] * row[c0[j]] + wx[j][1] * m.x + wx[j][2] * m.y + wx[j][3] * row[c3[j]];
          acc += wy[j][r] * t;
        }
        g[j] = acc;
      }
    }

    float relx[DB_PX], rely[DB_PX];
    if constexpr (REL) {
      const float rx = ref[nq * 2] * (float)(W * stride), ry = ref[nq * 2 + 1] * (float)(H * stride);
#pragma unroll
      for (int j = 0; j < DB_PX; ++j) {
        relx[j] = rx - cx[j];
        rely[j] = ry - cy[j];
      }
    }

    // ---- forward recompute: the forward kernel's operation order ------------------------------------------------
    float x0[DB_PX][DB_HID], x1[DB_PX][DB_HID];
#pragma unroll
    for (int k = 0; k < DB_HID; ++k) {
      cfloat_p wk = w0 + k * CIN;
      const float bk = b0[k];
#pragma unroll
      for (int j = 0; j < DB_PX; ++j) {
        float a = bk;
        if constexpr (REL) {
          a = fmaf(wk[0], relx[j], a);
          a = fmaf(wk[1], rely[j], a);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) a = fmaf(wk[FOFF + c], f[j][c], a);
        x0[j][k] = fmaxf(a, 0.f);
      }
    }
#pragma unroll
    for (int k = 0; k < DB_HID; ++k) {
      cfloat_p wk = w1 + k * DB_HID;
      const float bk = b1[k];
#pragma unroll
      for (int j = 0; j < DB_PX; ++j) {
        float a = bk;
#pragma unroll
        for (int c = 0; c < DB_HID; ++c) a = fmaf(wk[c], x0[j][c], a);
        x1[j][k] = fmaxf(a, 0.f);
      }
    }

    // ---- backward through the MLP (x > 0 is a > 0: x = max(a, 0)) -----------------------------------------------
    float dx0[DB_PX][DB_HID], dx1[DB_PX][DB_HID];
    asm volatile("" : "+s"(praw));
    cfloat_p w2 = (cfloat_p)praw + O2;
    w1 = (cfloat_p)praw + O1;
#pragma unroll
    for (int k = 0; k < DB_HID; ++k) {
      const float wk = w2[k];
#pragma unroll
      for (int j = 0; j < DB_PX; ++j) dx1[j][k] = x1[j][k] > 0.f ? g[j] * wk : 0.f;
    }
#pragma unroll
    for (int j = 0; j < DB_PX; ++j)
#pragma unroll
      for (int c = 0; c < DB_HID; ++c) dx0[j][c] = 0.f;
#pragma unroll
    for (int k = 0; k < DB_HID; ++k) {
      cfloat_p wk = w1 + k * DB_HID;
#pragma unroll
      for (int c = 0; c < DB_HID; ++c) {
        const float w = wk[c];
#pragma unroll
        for (int j = 0; j < DB_PX; ++j) dx0[j][c] = fmaf(w, dx1[j][k], dx0[j][c]);
      }
    }
#pragma unroll
    for (int j = 0; j < DB_PX; ++j)
#pragma unroll
      for (int c = 0; c < DB_HID; ++c) dx0[j][c] = x0[j][c] > 0.f ? dx0[j][c] : 0.f;
    asm volatile("" : "+s"(praw));
    w0 = (cfloat_p)praw;
#pragma unroll
    for (int k = 0; k < DB_HID; ++k) {
      cfloat_p wk = w0 + k * CIN + FOFF;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float w = wk[c];
#pragma unroll
        for (int j = 0; j < DB_PX; ++j) gf[j][c] = fmaf(w, dx0[j][k], gf[j][c]);
      }
    }

    // ---- the sums over pixels: one 32 x 32 x 128 product on the matrix cores ------------------------------------
    db_f16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < DB_PX; ++j) {
#pragma unroll
      for (int k = 0; k < DB_HID; ++k) {
        sm[SM_A + k * DB_S + lane] = dx0[j][k];
        sm[SM_A + (8 + k) * DB_S + lane] = dx1[j][k];
        sm[SM_A + (17 + k) * DB_S + lane] = x1[j][k];
        sm[SM_B + (2 + k) * DB_S + lane] = x0[j][k];
      }
      sm[SM_A + 16 * DB_S + lane] = g[j];
      if constexpr (REL) {
        sm[SM_B + lane] = relx[j];
        sm[SM_B + DB_S + lane] = rely[j];
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const float a = sm[a_off + 2 * s];
        const float bl = sm[b_off[j] + 2 * s];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b_one ? 1.f : bl, acc, 0, 0, 0);
      }
      __syncthreads();
    }

    // acc[r] = D[row 8 (r / 4) + 4 mh + r % 4][column mi]
    float *dst = ws_par + (((size_t)n * ntiles + tile) * Q + q) * G;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 4 * mh + r;                                 // rows 0-7: dx0[k]
      const int idx = mi < C ? k * CIN + FOFF + mi : (REL && mi < C + 2) ? k * CIN + (mi - C) : b_one ? OB0 + k : -1;
      if (idx >= 0) dst[idx] = acc[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 4 * mh + r;                                 // rows 8-15: dx1[k]
      const int idx = (mi >= C + 2 && mi < DB_COL_ONE) ? O1 + k * DB_HID + (mi - C - 2) : b_one ? OB1 + k : -1;
      if (idx >= 0) dst[idx] = acc[4 + r];
    }
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int row = 16 + (r < 4 ? 4 * mh + r : 8 + 4 * mh);   // rows 16-24 (and 28, unused): g, x1[0..7]
      int idx = -1;
      if (row == 16 && b_one) idx = OB2;
      if (row > 16 && row < DB_AROWS && mi == DB_COL_G) idx = O2 + row - 17;
      if (idx >= 0) dst[idx] = acc[8 + r];
    }
  }

  // ---- grad_feat of the tile (this query group's share) -------------------------------------------------------------
#pragma unroll
  for (int j = 0; j < DB_PX; ++j) {
    const int p = tile * DB_TILE + j * 64 + lane;
    if (p < HW) {
      float *o = gfeat + ((size_t)n * qsplit + grp) * C * HW + p;
#pragma unroll
      for (int c = 0; c < C; ++c) o[(size_t)c * HW] = gf[j][c];
    }
  }
}

// grad_params[n, q, :] = sum over tiles (ascending), grad_ref[n, q] from the summed db0
template <bool REL>
__global__ __launch_bounds__(256) void dyn_mask_head_bwd_params_kernel(const float *__restrict__ ws_par,
                                                                       const float *__restrict__ params, const int Q,
                                                                       const int H, const int W, const int stride,
                                                                       const int ntiles, float *__restrict__ grad_params,
                                                                       float *__restrict__ grad_ref)
{
  constexpr int CIN = REL ? DB_C + 2 : DB_C;
  constexpr int OB0 = CIN * DB_HID + DB_HID * DB_HID + DB_HID, G = OB0 + 2 * DB_HID + 1;
  static_assert(G <= 256, "one thread per generated parameter");
  __shared__ float db0[DB_HID];
  const size_t nq = blockIdx.x;
  const int n = (int)(nq / (unsigned)Q), q = (int)(nq - (size_t)n * Q), t = (int)threadIdx.x;
  if (t < G) {
    const float *src = ws_par + ((size_t)n * ntiles * Q + q) * G + t;
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < ntiles; ++i) s += src[(size_t)i * Q * G];
    grad_params[nq * G + t] = s;
    if (t >= OB0 && t < OB0 + DB_HID) db0[t - OB0] = s;
  }
  __syncthreads();
  if (grad_ref != nullptr && t < 2) {
    float a = 0.f;
    if constexpr (REL) {
#pragma unroll
      for (int k = 0; k < DB_HID; ++k) a = fmaf(params[nq * G + k * CIN + t], db0[k], a);
      a *= (float)((t == 0 ? W : H) * stride);
    }
    grad_ref[nq * 2 + t] = a;
  }
}

// grad_feat[n] = sum over query groups (ascending)
__global__ __launch_bounds__(256) void dyn_mask_head_bwd_feat_kernel(const float *__restrict__ part, const int qsplit,
                                                                     const long long per_image,
                                                                     float *__restrict__ grad_feat)
{
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n = (int)blockIdx.y;
  if (i >= per_image) return;
  const float *src = part + (size_t)n * qsplit * per_image + i;
  float s = 0.f;
  for (int k = 0; k < qsplit; ++k) s += src[(size_t)k * per_image];
  grad_feat[(size_t)n * per_image + i] = s;
}

// The workspace: batch * ntiles * num_query * G parameter partials, then batch * qsplit * 16 * H * W grad_feat partials
// (the header documents the bound with qsplit = DB_MAX_QSPLIT).
int launch_dyn_mask_head_bwd(const float *feat, const float *ref, const float *params, const float *grad_up, int N, int C,
                             int Q, int H, int W, int stride, int rel_coord, void *workspace, float *grad_feat,
                             float *grad_ref, float *grad_params, hipStream_t stream)
{
  if (C != DB_C) return PCT_ERR_UNSUPPORTED;
  if (N > 65535) return PCT_ERR_UNSUPPORTED;
  if (Q == 0) {     // no query: grad_feat is zero, the other outputs are empty (a kernel, not a memset node: see the MSDA backward)
    const long long per_image = (long long)C * H * W;
    hipLaunchKernelGGL(dyn_mask_head_bwd_feat_kernel, dim3((unsigned)((per_image + 255) / 256), (unsigned)N), dim3(256), 0,
                       stream, grad_feat, 0, per_image, grad_feat);
    return (int)hipGetLastError();
  }
  const long long HW = (long long)H * W;
  const long long ntiles_ll = (HW + DB_TILE - 1) / DB_TILE;
  const int G = (C + (rel_coord ? 2 : 0)) * DB_HID + DB_HID * DB_HID + 3 * DB_HID + 1;
  // enough waves for two per SIMD of the chip (2048: reasoned from the register count, not tuned -- only the two training
  // geometries, where it gives 8 and 6 groups, have been timed); every group holds at least one query
  int qsplit = (int)((2048 + (long long)N * ntiles_ll - 1) / ((long long)N * ntiles_ll));
  if (qsplit > DB_MAX_QSPLIT) qsplit = DB_MAX_QSPLIT;
  if (qsplit > Q) qsplit = Q;
  const int qper = (Q + qsplit - 1) / qsplit;
  qsplit = (Q + qper - 1) / qper;
  const long long nblk = (long long)N * ntiles_ll * qsplit;
  if (nblk > 0x7fffffffLL || (long long)N * Q > 0x7fffffffLL || 4 * HW > 0x7fffffffLL) return PCT_ERR_UNSUPPORTED;
  const int ntiles = (int)ntiles_ll;
  float *ws_par = static_cast<float *>(workspace);
  float *ws_feat = ws_par + (size_t)N * ntiles * Q * G;
  float *gf = qsplit == 1 ? grad_feat : ws_feat;
  const dim3 grid((unsigned)nblk), gridp((unsigned)((long long)N * Q));
  if (rel_coord) {
    hipLaunchKernelGGL(dyn_mask_head_bwd_kernel<true>, grid, dim3(64), 0, stream, feat, ref, params, grad_up, Q, H, W, stride,
                       ntiles, qsplit, qper, ws_par, gf);
    hipLaunchKernelGGL(dyn_mask_head_bwd_params_kernel<true>, gridp, dim3(256), 0, stream, ws_par, params, Q, H, W, stride,
                       ntiles, grad_params, grad_ref);
  } else {
    hipLaunchKernelGGL(dyn_mask_head_bwd_kernel<false>, grid, dim3(64), 0, stream, feat, ref, params, grad_up, Q, H, W, stride,
                       ntiles, qsplit, qper, ws_par, gf);
    hipLaunchKernelGGL(dyn_mask_head_bwd_params_kernel<false>, gridp, dim3(256), 0, stream, ws_par, params, Q, H, W, stride,
                       ntiles, grad_params, grad_ref);
  }
  if (qsplit > 1) {
    const long long per_image = (long long)C * HW;
    hipLaunchKernelGGL(dyn_mask_head_bwd_feat_kernel, dim3((unsigned)((per_image + 255) / 256), (unsigned)N), dim3(256), 0,
                       stream, ws_feat, qsplit, per_image, grad_feat);
  }
  return (int)hipGetLastError();
}

}  // namespace pct
