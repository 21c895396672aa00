// Position-guided masked cross-attention core of the PCTrans decoder on CDNA4 MFMA (gfx950, wave64), bf16 operands / fp32
// accumulation -- the CrossAttentionLayer's own operand form (mask2former_transformer_decoder.py:130-183 -> attention.py:
// 271-387): per head the query and key are [content (16) | position (16)] halves coming from DIFFERENT projections, so the
// kernel takes the halves as separate tensors in the layout the projection GEMMs write ([tokens, N, heads * 16]) and the
// per-head concatenations (dec.py:160-172: two torch.cat passes over the keys per layer) never exist; the value tensor is
// read as the projection writes it too (no V^T GEMM).
//
// Same arithmetic, in the same order, as masked_attention.hip (S^T = K . Q^T with v_mfma_f32_16x16x32_bf16, online softmax
// over 32-key steps, P^T as the B operand of O^T += V^T . P^T with the k-slot permutation 8g+j <-> key 4g+j | 16+4g+(j-4)):
// outputs are bit-identical to that kernel on the concatenated operands (tests/test_cross_attention_gpu.py).  What changes
// is how the operands reach the matrix cores.  There one wave per (image, head, 16 queries) fetched its fragments straight
// from global memory: 64-byte head slices of a key 64 KB apart, value rows per channel, mask bytes per query row -- about
// 290 tag look-ups in the texture addresser per 32-key step and wave, the K / V bytes of an (image, head) fetched seven
// times over, 0.66 ms at 4 096 keys and batch 128 (2.4 % of the MFMA rate, 9 % of the HBM rate).  Here:
//   * workgroup = (image, 4 heads, up to 4 query tiles of 16): 4 waves = 4 heads, every wave walking all the keys for its
//     head and keeping up to four query tiles' softmax state and output accumulators in registers (four independent MFMA /
//     exp chains per wave to interleave);
//   * the keys arrive in chunks of 64: each thread fetches 16-byte pieces of whole 128-byte rows (4 heads x 16 dims: full
//     lines) of K-content, K-position and V, and of the 64 x 64 mask bytes, one chunk AHEAD into registers while the
//     current chunk is computed, then stores them into a double-buffered LDS image (one barrier per chunk);
//   * LDS image: [key][8 pieces of 16 B], piece c of key k stored at c ^ (k % 8): the ds_read_b128 of an A operand (16 keys x
//     one head's 32 bytes) and the ds_read_b64_tr_b16 of a V block (4 keys x 16 channels, delivered transposed: the
//     hardware does the V^T) are then bank-conflict free; mask rows as 16 dwords rotated by 2 * (query / 2);
//   * the two workgroups of an (image, head group) -- query tiles 0-3 and 4-6 at 100 queries -- sit next to each other in
//     the XCD-chunked block order, so the second one finds the K / V lines in L2.
#include "attn_common.hpp"
#include "launchers.hpp"

namespace pct {

constexpr int XA_HG = 4;      // heads per workgroup (one wave each)
constexpr int XA_T = 4;       // query tiles per wave
constexpr int XA_CH = 64;     // keys per chunk

typedef unsigned xa_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned xa_u32x2 __attribute__((ext_vector_type(2)));

// q_c, q_s [Q, N, heads*16]; k_c, k_p, v [S, N, heads*16] bf16; mask [N, Q, S] bytes (nonzero = may not attend) or NULL;
// row_open [N, Q] bytes or NULL: nonzero = this query's mask row is ignored (it attends everywhere) -- the decoder's "a query
// whose mask rules out every pixel attends everywhere instead" (dec.py:561) without re-writing the [N, Q, S] mask;
// out [Q, N, heads*16] bf16.  S % 64 == 0, heads % 4 == 0.
// RAGGED instantiations (pct_cross_attention_ragged_bf16): any S >= 1, mask rows mask_pitch bytes apart (mask_pitch % 16 == 0,
// mask_pitch >= S; bytes at positions >= S are never trusted).  The last chunk then holds 1 .. 64 keys.  Its rules:
//   * no load addresses a key past S - 1 or a mask byte past mask_pitch (see fetch);
//   * the LDS rows of keys >= S hold zeros, K and V alike: p = 0 times a finite value, never a NaN;
//   * keys >= S are dead whatever the mask bytes, row_open or HAS_MASK say: their dead bytes come from the key index and are ORed
//     in AFTER the AND with keep[t] (an opened row attends to every real key and to nothing else);
//   * a 32-key step without a live key (S % 64 in 1 .. 32: the chunk's second step) is skipped -- masked_attention.hip walks
//     ceil(S / 32) steps, and the bit identity with it on the concatenated operands holds for every S.
struct XaShared {
  xa_u32x4 sKc[2][XA_CH * 8], sKp[2][XA_CH * 8], sV[2][XA_CH * 8];
  unsigned sM[2][XA_T * 16][16];
};

// NT: the query tiles this workgroup's waves carry (1 .. XA_T; compile time, so that the tiles' chains are straight-line code
// the scheduler can interleave -- with a run-time count each tile became its own basic block)
// PARTIAL (RAGGED only; pct_cross_attention_split_keys_bf16): the grid holds `splits` workgroups for every workgroup of the plain
// grid, next to each other's tile groups (block order: image, head group, split, tile group -- the tile groups of one split are
// adjacent and share its K / V lines in L2).  Split j walks the chunks [xa_split_begin(j), xa_split_begin(j + 1)) with the same
// staging, steps and tail rules -- `ch` stays the call's absolute chunk index, so a ragged tail can only sit in the last split --
// and its epilogue does not divide: o (still relative to m_run), m_run and l_run of every live query row go to the workspace
//   o [splits][N][heads][Q][16] fp32 | m [splits][N][heads][Q] fp32 | l [splits][N][heads][Q] fp32
// for cross_attention_combine_kernel.  A wave's store of one tile's o is 1 KB contiguous; m and l come from the g == 0 lanes.
__host__ __device__ __forceinline__ int xa_split_begin(const int j, const int nch, const int splits)
{
  return (int)((long long)j * nch / splits);             // the one statement of the rule (split_key_attention.chunk_ranges)
}

template <bool HAS_MASK, bool RAGGED, int NT, bool PARTIAL = false>
__device__ __forceinline__ void cross_attention_body(XaShared &sh, const __bf16 *__restrict__ q_c, const __bf16 *__restrict__ q_s,
                                                     const __bf16 *__restrict__ k_c, const __bf16 *__restrict__ k_p,
                                                     const __bf16 *__restrict__ v, const unsigned char *__restrict__ mask,
                                                     const unsigned char *__restrict__ row_open, const int N, const int heads,
                                                     const int Q, const int S, const int mask_pitch, const float scale,
                                                     const int tgroups, __bf16 *__restrict__ out, const int splits = 1,
                                                     float *__restrict__ ws = nullptr)
{
  static_assert(RAGGED || !PARTIAL, "the partial kernel is built on the ragged rules");
  auto &sKc = sh.sKc;
  auto &sKp = sh.sKp;
  auto &sV = sh.sV;
  auto &sM = sh.sM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int C = heads * 16;
  const int hgroups = heads / XA_HG;
  const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
  const int tg = (int)(lb % (unsigned)tgroups);
  int hg, n, split = 0;
  if constexpr (PARTIAL) {
    split = (int)((lb / (unsigned)tgroups) % (unsigned)splits);
    hg = (int)((lb / (unsigned)(tgroups * splits)) % (unsigned)hgroups);
    n = (int)(lb / (unsigned)(tgroups * splits * hgroups));
  } else {
    hg = (int)((lb / (unsigned)tgroups) % (unsigned)hgroups);
    n = (int)(lb / (unsigned)(tgroups * hgroups));
  }
  const int h = hg * XA_HG + wave;
  const int tile0 = tg * XA_T;

  // ---- B operands of S^T = K . Q^T: Q[query][k-slot 8g .. 8g+7] = content dims 8g.. (g < 2) | position dims 8(g-2).. ------
  bf16x8 qb[NT];
  unsigned keep[NT];                                     // all ones, or 0 for a query whose mask is to be ignored (row_open)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int qi = min((tile0 + t) * 16 + col, Q - 1);
    keep[t] = (HAS_MASK && row_open && row_open[(size_t)n * Q + qi]) ? 0u : 0xFFFFFFFFu;
    const __bf16 *src = (g < 2 ? q_c : q_s) + ((size_t)qi * N + n) * C + h * 16 + 8 * (g & 1);
    qb[t] = *reinterpret_cast<const bf16x8 *>(src);
  }
  f32x4 o[NT];
  float m_run[NT], l_run[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    m_run[t] = -INFINITY;
    l_run[t] = 0.f;
  }

  // ---- staging: which 16-byte pieces of a chunk this thread moves ---------------------------------------------------------
  // K: 64 keys x {content, position} x 8 pieces = 1 024 pieces, 4 per thread; V: 512 pieces, 2 per thread; mask: 64 query rows
  // x 4 pieces of 16 keys, 1 per thread.  piece p of a tensor: key = p / 8, c = p % 8 -> the 128-byte row of the head group
  const size_t row_elems = (size_t)N * C;                                   // elements between two keys of one image
  const __bf16 *kc_img = k_c + (size_t)n * C + hg * (XA_HG * 16);
  const __bf16 *kp_img = k_p + (size_t)n * C + hg * (XA_HG * 16);
  const __bf16 *v_img = v + (size_t)n * C + hg * (XA_HG * 16);
  const int sk_key = tid >> 3, sk_c = tid & 7;                              // + 32 keys for the second piece
  const int sm_q = tid >> 2, sm_part = tid & 3;
  const unsigned char *m_row = nullptr;
  if constexpr (HAS_MASK)
    m_row = mask + ((size_t)n * Q + min(tile0 * 16 + sm_q, Q - 1)) * (RAGGED ? mask_pitch : S) + sm_part * 16;
  xa_u32x4 pkc[2], pkp[2], pv[2], pm;
  auto fetch = [&](const int key0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int key = key0 + sk_key + 32 * i;
      // RAGGED address bound: the row index is min(key, S - 1) <= S - 1 and the piece lies inside that row's N * C elements
      // (n * C + hg * 64 + sk_c * 8 + 8 <= N * C), so the last byte read is inside key S - 1's row of the tensor; what a
      // thread fetched for a key >= S is discarded for zeros
      const bool live = !RAGGED || key < S;
      if constexpr (RAGGED) key = min(key, S - 1);
      const size_t off = (size_t)key * row_elems + sk_c * 8;
      pkc[i] = *reinterpret_cast<const xa_u32x4 *>(kc_img + off);
      pkp[i] = *reinterpret_cast<const xa_u32x4 *>(kp_img + off);
      pv[i] = *reinterpret_cast<const xa_u32x4 *>(v_img + off);
      if constexpr (RAGGED) {
        const xa_u32x4 zero = {0u, 0u, 0u, 0u};
        pkc[i] = live ? pkc[i] : zero;
        pkp[i] = live ? pkp[i] : zero;
        pv[i] = live ? pv[i] : zero;
      }
    }
    if constexpr (HAS_MASK) {
      if constexpr (RAGGED) {
        // address bound: the piece covers the row's bytes [key0 + 16 sm_part, + 16); key0, 16 sm_part and mask_pitch are
        // multiples of 16, so start < mask_pitch implies end <= mask_pitch, and the address (16-byte aligned base + multiples
        // of 16) is aligned.  A piece at or past the pitch is not fetched: all its keys are >= S, dead by the key index
        pm = xa_u32x4{~0u, ~0u, ~0u, ~0u};
        if (key0 + sm_part * 16 < mask_pitch) pm = *reinterpret_cast<const xa_u32x4 *>(m_row + key0);
      } else {
        pm = *reinterpret_cast<const xa_u32x4 *>(m_row + key0);
      }
    }
  };
  auto stash = [&](const int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = sk_key + 32 * i;
      const int pos = key * 8 + (sk_c ^ (key & 7));
      sKc[buf][pos] = pkc[i];
      sKp[buf][pos] = pkp[i];
      sV[buf][pos] = pv[i];
    }
    if constexpr (HAS_MASK) {
      // row sm_q, dwords 4 part .. 4 part + 3, rotated by 2 * ((query % 16) / 2): two aligned dword pairs
      const int rot = 2 * ((sm_q & 15) >> 1);
      unsigned *row = sM[buf][sm_q];
      *reinterpret_cast<xa_u32x2 *>(row + ((4 * sm_part + rot) & 15)) = xa_u32x2{pm[0], pm[1]};
      *reinterpret_cast<xa_u32x2 *>(row + ((4 * sm_part + 2 + rot) & 15)) = xa_u32x2{pm[2], pm[3]};
    }
  };

  // per-lane LDS addresses of the fragments (fixed for the launch; + 16 keys / + 32 keys by immediate offsets)
  // A operand: key kb + col, piece 2 wave + (g & 1) of content (g < 2) or position
  const int a_c = 2 * wave + (g & 1);
  // V block of group g: rows kb + 4 g + (l / 4), pieces 2 wave + (l % 4) / 2, half (l % 2), l = lane % 16
  const int v_r = 4 * g + (col >> 2), v_c = 2 * wave + ((col & 3) >> 1), v_h = col & 1;
  const int m_rot = 2 * (col >> 1);

  const int nch = RAGGED ? (S + XA_CH - 1) / XA_CH : S / XA_CH;
  int c0 = 0, c1 = nch;                                  // this workgroup's chunks
  if constexpr (PARTIAL) {
    c0 = xa_split_begin(split, nch, splits);
    c1 = xa_split_begin(split + 1, nch, splits);
  }
  fetch(c0 * XA_CH);
  stash(0);
  __syncthreads();
  if (c0 + 1 < c1) fetch((c0 + 1) * XA_CH);
  for (int ch = c0; ch < c1; ++ch) {
    const int buf = (ch - c0) & 1;
    const unsigned char *kt = reinterpret_cast<const unsigned char *>(g < 2 ? sKc[buf] : sKp[buf]);
    const unsigned char *vt = reinterpret_cast<const unsigned char *>(sV[buf]);
#pragma unroll
    for (int j = 0; j < XA_CH / 32; ++j) {
      const int kb = 32 * j;
      // RAGGED: dead bytes of the keys >= S among this lane's kA .. kA + 3 and kB .. kB + 3 (0 .. 4 keys left in each group)
      unsigned tailA = 0, tailB = 0;
      if constexpr (RAGGED) {
        if (ch * XA_CH + kb >= S) break;                  // no live key in this step (uniform: S is a launch constant)
        const int leftA = S - (ch * XA_CH + kb + 4 * g), leftB = leftA - 16;
        tailA = leftA >= 4 ? 0u : (leftA <= 0 ? ~0u : ~0u << (8 * leftA));
        tailB = leftB >= 4 ? 0u : (leftB <= 0 ? ~0u : ~0u << (8 * leftB));
      }
      // ---- fragments of this 32-key step, shared by the wave's query tiles ------------------------------------------------
      const int ka = kb + col, kb2 = kb + 16 + col;
      const bf16x8 a0 = *reinterpret_cast<const bf16x8 *>(kt + (ka * 8 + (a_c ^ (ka & 7))) * 16);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8 *>(kt + (kb2 * 8 + (a_c ^ (kb2 & 7))) * 16);
      const int va_k = kb + v_r, vb_k = kb + 16 + v_r;
      const bf16x4 va0 = lds_read_tr16_b64(vt + (va_k * 8 + (v_c ^ (va_k & 7))) * 16 + v_h * 8);
      const bf16x4 va1 = lds_read_tr16_b64(vt + (vb_k * 8 + (v_c ^ (vb_k & 7))) * 16 + v_h * 8);
      const bf16x8 va = {va0[0], va0[1], va0[2], va0[3], va1[0], va1[1], va1[2], va1[3]};
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        unsigned mA = 0, mB = 0;
        if constexpr (HAS_MASK) {
          const unsigned *mr = sM[buf][t * 16 + col];
          mA = mr[(8 * j + g + m_rot) & 15] & keep[t];
          mB = mr[(8 * j + 4 + g + m_rot) & 15] & keep[t];
        }
        if constexpr (RAGGED) {
          mA |= tailA;                                      // after the AND with keep: an opened row's tail stays dead
          mB |= tailB;
        }
        attn_step(a0, a1, qb[t], va, mA, mB, scale, o[t], m_run[t], l_run[t]);
      }
    }
    if (ch + 1 < c1) {
      stash(buf ^ 1);               // (everyone left that buffer before the barrier that ended the previous chunk)
      __syncthreads();
      if (ch + 2 < c1) fetch((ch + 2) * XA_CH);
    }
  }

  if constexpr (PARTIAL) {
    // record of (split, image, head, query): every live query of every (split, image, head) is written by exactly one lane
    // group here, so the combine reads no word this call has not written
    const size_t rows = (size_t)splits * N * heads * Q;
    const size_t row0 = (((size_t)split * N + n) * heads + h) * Q;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int qo = (tile0 + t) * 16 + col;
      if (qo < Q) {
        *reinterpret_cast<f32x4 *>(ws + (row0 + qo) * 16 + 4 * g) = o[t];
        if (g == 0) {
          ws[rows * 16 + row0 + qo] = m_run[t];
          ws[rows * 17 + row0 + qo] = l_run[t];
        }
      }
    }
    return;
  }

#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int qo = (tile0 + t) * 16 + col;
    if (qo < Q) {
      const float inv = 1.0f / l_run[t];                             // l_run == 0 -> NaN, as softmax(all -inf)
      __bf16 *dst = out + ((size_t)qo * N + n) * C + h * 16 + 4 * g;
      bf16x4 r = {(__bf16)(o[t][0] * inv), (__bf16)(o[t][1] * inv), (__bf16)(o[t][2] * inv), (__bf16)(o[t][3] * inv)};
      *reinterpret_cast<bf16x4 *>(dst) = r;
    }
  }
}

template <bool HAS_MASK>
__global__ __launch_bounds__(256, 2) void cross_attention_kernel(const __bf16 *__restrict__ q_c, const __bf16 *__restrict__ q_s,
                                                                 const __bf16 *__restrict__ k_c, const __bf16 *__restrict__ k_p,
                                                                 const __bf16 *__restrict__ v,
                                                                 const unsigned char *__restrict__ mask,
                                                                 const unsigned char *__restrict__ row_open, const int N,
                                                                 const int heads, const int Q, const int S, const float scale,
                                                                 const int tgroups, __bf16 *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) XaShared sh;
  const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
  const int tg = (int)(lb % (unsigned)tgroups);
  const int ntile = min(XA_T, (Q + 15) / 16 - tg * XA_T);            // uniform over the workgroup
  static_assert(XA_T == 4, "dispatch below");
  if (ntile == 4) cross_attention_body<HAS_MASK, false, 4>(sh, q_c, q_s, k_c, k_p, v, mask, row_open, N, heads, Q, S, S, scale, tgroups, out);
  else if (ntile == 3) cross_attention_body<HAS_MASK, false, 3>(sh, q_c, q_s, k_c, k_p, v, mask, row_open, N, heads, Q, S, S, scale, tgroups, out);
  else if (ntile == 2) cross_attention_body<HAS_MASK, false, 2>(sh, q_c, q_s, k_c, k_p, v, mask, row_open, N, heads, Q, S, S, scale, tgroups, out);
  else cross_attention_body<HAS_MASK, false, 1>(sh, q_c, q_s, k_c, k_p, v, mask, row_open, N, heads, Q, S, S, scale, tgroups, out);
}

// any S >= 1 (the RAGGED rules above); the same workgroup shape, LDS image and dispatch
template <bool HAS_MASK>
__global__ __launch_bounds__(256, 2) void cross_attention_ragged_kernel(
    const __bf16 *__restrict__ q_c, const __bf16 *__restrict__ q_s, const __bf16 *__restrict__ k_c, const __bf16 *__restrict__ k_p,
    const __bf16 *__restrict__ v, const unsigned char *__restrict__ mask, const unsigned char *__restrict__ row_open, const int N,
    const int heads, const int Q, const int S, const int mask_pitch, const float scale, const int tgroups, __bf16 *__restrict__ out)
{
  __shared__ __attribute__((aligned(16))) XaShared sh;
  const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
  const int tg = (int)(lb % (unsigned)tgroups);
  const int ntile = min(XA_T, (Q + 15) / 16 - tg * XA_T);            // uniform over the workgroup
  static_assert(XA_T == 4, "dispatch below");
#define PCT_XA_RAGGED(NT_) \
  cross_attention_body<HAS_MASK, true, NT_>(sh, q_c, q_s, k_c, k_p, v, mask, row_open, N, heads, Q, S, mask_pitch, scale, tgroups, out)
  if (ntile == 4) PCT_XA_RAGGED(4);
  else if (ntile == 3) PCT_XA_RAGGED(3);
  else if (ntile == 2) PCT_XA_RAGGED(2);
  else PCT_XA_RAGGED(1);
#undef PCT_XA_RAGGED
}

// the PARTIAL form: the ragged kernel's workgroup, dispatch and LDS image on the chunks of one split
template <bool HAS_MASK>
__global__ __launch_bounds__(256, 2) void cross_attention_partial_kernel(
    const __bf16 *__restrict__ q_c, const __bf16 *__restrict__ q_s, const __bf16 *__restrict__ k_c, const __bf16 *__restrict__ k_p,
    const __bf16 *__restrict__ v, const unsigned char *__restrict__ mask, const unsigned char *__restrict__ row_open, const int N,
    const int heads, const int Q, const int S, const int mask_pitch, const float scale, const int tgroups, const int splits,
    float *__restrict__ ws)
{
  __shared__ __attribute__((aligned(16))) XaShared sh;
  const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
  const int tg = (int)(lb % (unsigned)tgroups);
  const int ntile = min(XA_T, (Q + 15) / 16 - tg * XA_T);            // uniform over the workgroup
  static_assert(XA_T == 4, "dispatch below");
#define PCT_XA_PARTIAL(NT_)                                                                                                      \
  cross_attention_body<HAS_MASK, true, NT_, true>(sh, q_c, q_s, k_c, k_p, v, mask, row_open, N, heads, Q, S, mask_pitch, scale, \
                                                  tgroups, nullptr, splits, ws)
  if (ntile == 4) PCT_XA_PARTIAL(4);
  else if (ntile == 3) PCT_XA_PARTIAL(3);
  else if (ntile == 2) PCT_XA_PARTIAL(2);
  else PCT_XA_PARTIAL(1);
#undef PCT_XA_PARTIAL
}

// One thread per (query, image, head, 4 channels), in the order of `out`.  M = max_j m_j; w_j = exp(m_j - M), 0 for a split
// that saw no live key (m_j = -inf: its o_j and l_j are 0); L = sum_j w_j l_j and O = sum_j w_j o_j in ascending j, starting
// from the j = 0 term; out = bf16(O * (1 / L)).  No live key in any split: L = 0 and 0 * inf = NaN, as the kernels above.
__global__ __launch_bounds__(256) void cross_attention_combine_kernel(const float *__restrict__ ws, const int N, const int heads,
                                                                      const int Q, const int splits, __bf16 *__restrict__ out)
{
  const size_t per_split = (size_t)N * heads * Q, rows = per_split * splits;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= per_split * 4) return;
  const int g = (int)(idx & 3);
  const int h = (int)((idx >> 2) % (unsigned)heads);
  const int n = (int)((idx / ((size_t)4 * heads)) % (unsigned)N);
  const int qo = (int)(idx / ((size_t)4 * heads * N));
  const size_t row0 = ((size_t)n * heads + h) * Q + qo;
  const float *ws_m = ws + rows * 16, *ws_l = ws + rows * 17;
  float M = -INFINITY;
  for (int j = 0; j < splits; ++j) M = fmaxf(M, ws_m[row0 + j * per_split]);
  f32x4 O = {0.f, 0.f, 0.f, 0.f};
  float L = 0.f;
  for (int j = 0; j < splits; ++j) {
    const size_t row = row0 + j * per_split;
    const float m = ws_m[row];
    const float w = m == -INFINITY ? 0.f : __expf(m - M);
    const f32x4 oj = *reinterpret_cast<const f32x4 *>(ws + row * 16 + 4 * g);
    const float lj = ws_l[row];
    if (j == 0) {
      L = w * lj;
#pragma unroll
      for (int r = 0; r < 4; ++r) O[r] = w * oj[r];
    } else {
      L += w * lj;
#pragma unroll
      for (int r = 0; r < 4; ++r) O[r] += w * oj[r];
    }
  }
  const float inv = 1.0f / L;
  const bf16x4 r = {(__bf16)(O[0] * inv), (__bf16)(O[1] * inv), (__bf16)(O[2] * inv), (__bf16)(O[3] * inv)};
  *reinterpret_cast<bf16x4 *>(out + idx * 4) = r;
}

// PCT_NOT_COVERED: geometry not covered (the caller concatenates the halves and uses pct_masked_attention_bf16)
int launch_cross_attention(const void *q_c, const void *q_s, const void *k_c, const void *k_p, const void *v,
                           const unsigned char *mask, const unsigned char *row_open, int N, int heads, int Q, int S,
                           float scale, void *out, hipStream_t stream)
{
  if (heads <= 0 || heads % XA_HG != 0 || S <= 0 || S % XA_CH != 0) return PCT_NOT_COVERED;
  if (N == 0 || Q == 0) return 0;
  if ((long long)S * N * heads * 16 >= 0x7fffffffLL) return PCT_NOT_COVERED;
  if ((((uintptr_t)q_c | (uintptr_t)q_s | (uintptr_t)k_c | (uintptr_t)k_p | (uintptr_t)v) & 15u) || ((uintptr_t)out & 7u)) return PCT_NOT_COVERED;
  if (mask && (((uintptr_t)mask & 15u) || (S & 15))) return PCT_NOT_COVERED;
  const int qtiles = (Q + 15) / 16, tgroups = (qtiles + XA_T - 1) / XA_T;
  const long long nblk = (long long)N * (heads / XA_HG) * tgroups;
  if (nblk > 0x7fffffffLL) return PCT_NOT_COVERED;
  const dim3 grid((unsigned)nblk), block(256);
  const __bf16 *qc = static_cast<const __bf16 *>(q_c), *qs = static_cast<const __bf16 *>(q_s);
  const __bf16 *kc = static_cast<const __bf16 *>(k_c), *kp = static_cast<const __bf16 *>(k_p);
  const __bf16 *vv = static_cast<const __bf16 *>(v);
  if (mask)
    hipLaunchKernelGGL(cross_attention_kernel<true>, grid, block, 0, stream, qc, qs, kc, kp, vv, mask, row_open, N, heads, Q, S,
                       scale, tgroups, static_cast<__bf16 *>(out));
  else
    hipLaunchKernelGGL(cross_attention_kernel<false>, grid, block, 0, stream, qc, qs, kc, kp, vv, mask, row_open, N, heads, Q, S,
                       scale, tgroups, static_cast<__bf16 *>(out));
  return (int)hipGetLastError();
}

// Any S >= 1, mask rows mask_pitch bytes apart (the caller has checked mask_pitch >= S and mask_pitch % 16 == 0).  A call the
// 64-key kernel covers in this very form goes to it: the same bits.  PCT_NOT_COVERED: heads % 4 != 0 or the 2^31 element limit
int launch_cross_attention_ragged(const void *q_c, const void *q_s, const void *k_c, const void *k_p, const void *v,
                                  const unsigned char *mask, int mask_pitch, const unsigned char *row_open, int N, int heads,
                                  int Q, int S, float scale, void *out, hipStream_t stream)
{
  if (heads <= 0 || heads % XA_HG != 0 || S <= 0) return PCT_NOT_COVERED;
  if (N == 0 || Q == 0) return 0;
  if ((long long)S * N * heads * 16 >= 0x7fffffffLL || (long long)Q * N * heads * 16 >= 0x7fffffffLL) return PCT_NOT_COVERED;
  if (S % XA_CH == 0 && (!mask || mask_pitch == S))
    return launch_cross_attention(q_c, q_s, k_c, k_p, v, mask, row_open, N, heads, Q, S, scale, out, stream);
  if ((((uintptr_t)q_c | (uintptr_t)q_s | (uintptr_t)k_c | (uintptr_t)k_p | (uintptr_t)v) & 15u) || ((uintptr_t)out & 7u)) return PCT_NOT_COVERED;
  if (mask && (((uintptr_t)mask & 15u) || (mask_pitch & 15) || mask_pitch < S)) return PCT_NOT_COVERED;
  const int qtiles = (Q + 15) / 16, tgroups = (qtiles + XA_T - 1) / XA_T;
  const long long nblk = (long long)N * (heads / XA_HG) * tgroups;
  if (nblk > 0x7fffffffLL) return PCT_NOT_COVERED;
  const dim3 grid((unsigned)nblk), block(256);
  const __bf16 *qc = static_cast<const __bf16 *>(q_c), *qs = static_cast<const __bf16 *>(q_s);
  const __bf16 *kc = static_cast<const __bf16 *>(k_c), *kp = static_cast<const __bf16 *>(k_p);
  const __bf16 *vv = static_cast<const __bf16 *>(v);
  if (mask)
    hipLaunchKernelGGL(cross_attention_ragged_kernel<true>, grid, block, 0, stream, qc, qs, kc, kp, vv, mask, row_open, N, heads, Q,
                       S, mask_pitch, scale, tgroups, static_cast<__bf16 *>(out));
  else
    hipLaunchKernelGGL(cross_attention_ragged_kernel<false>, grid, block, 0, stream, qc, qs, kc, kp, vv, mask, row_open, N, heads, Q,
                       S, 0, scale, tgroups, static_cast<__bf16 *>(out));
  return (int)hipGetLastError();
}

long long cross_attention_split_keys_workspace(int N, int heads, int Q, int splits)
{
  return splits <= 1 ? 0 : (long long)splits * N * heads * Q * 18 * (long long)sizeof(float);
}

int launch_cross_attention_split_keys(const void *q_c, const void *q_s, const void *k_c, const void *k_p, const void *v,
                                      const unsigned char *mask, int mask_pitch, const unsigned char *row_open, int N, int heads,
                                      int Q, int S, float scale, int splits, void *workspace, long long workspace_bytes, void *out,
                                      hipStream_t stream)
{
  // what launch_cross_attention_ragged answers first, in its order
  if (heads <= 0 || heads % XA_HG != 0 || S <= 0) return PCT_NOT_COVERED;
  if (N == 0 || Q == 0) return 0;
  if ((long long)S * N * heads * 16 >= 0x7fffffffLL || (long long)Q * N * heads * 16 >= 0x7fffffffLL) return PCT_NOT_COVERED;
  if ((((uintptr_t)q_c | (uintptr_t)q_s | (uintptr_t)k_c | (uintptr_t)k_p | (uintptr_t)v) & 15u) || ((uintptr_t)out & 7u)) return PCT_NOT_COVERED;
  if (mask && (((uintptr_t)mask & 15u) || (mask_pitch & 15) || mask_pitch < S)) return PCT_NOT_COVERED;
  const int nch = (S + XA_CH - 1) / XA_CH;
  if (splits < 1 || splits > 16 || splits > nch) return PCT_ERR_BAD_ARG;
  if (splits == 1)
    return launch_cross_attention_ragged(q_c, q_s, k_c, k_p, v, mask, mask_pitch, row_open, N, heads, Q, S, scale, out, stream);
  if (!workspace || workspace_bytes < cross_attention_split_keys_workspace(N, heads, Q, splits)) return PCT_ERR_BAD_ARG;
  if ((uintptr_t)workspace & 15u) return PCT_ERR_ALIGNMENT;
  const int qtiles = (Q + 15) / 16, tgroups = (qtiles + XA_T - 1) / XA_T;
  const long long nblk = (long long)N * (heads / XA_HG) * splits * tgroups;
  if (nblk > 0x7fffffffLL) return PCT_NOT_COVERED;
  const dim3 grid((unsigned)nblk), block(256);
  const __bf16 *qc = static_cast<const __bf16 *>(q_c), *qs = static_cast<const __bf16 *>(q_s);
  const __bf16 *kc = static_cast<const __bf16 *>(k_c), *kp = static_cast<const __bf16 *>(k_p);
  const __bf16 *vv = static_cast<const __bf16 *>(v);
  float *ws = static_cast<float *>(workspace);
  if (mask)
    hipLaunchKernelGGL(cross_attention_partial_kernel<true>, grid, block, 0, stream, qc, qs, kc, kp, vv, mask, row_open, N, heads, Q,
                       S, mask_pitch, scale, tgroups, splits, ws);
  else
    hipLaunchKernelGGL(cross_attention_partial_kernel<false>, grid, block, 0, stream, qc, qs, kc, kp, vv, mask, row_open, N, heads, Q,
                       S, 0, scale, tgroups, splits, ws);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  const long long threads = (long long)Q * N * heads * 4;             // < 2^29 by the element limit above
  hipLaunchKernelGGL(cross_attention_combine_kernel, dim3((unsigned)((threads + 255) / 256)), block, 0, stream, ws, N, heads, Q,
                     splits, static_cast<__bf16 *>(out));
  return (int)hipGetLastError();
}

}  // namespace pct
