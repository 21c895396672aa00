// MSDeformAttn forward, "pyramid-column" kernel for MI355X (gfx950, wave64): the default for PCTrans' encoder
// self-attention (Lq == S, fp32, D = 16, P = 4) once the problem fills the chip.
//
// Same semantics as msda_forward.hip (reference: ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304 + :38-89).
//
// What it changes against the windowed kernel of round 1 (msda_forward_win.hip: 16 x 16 tile of ONE level x one head per
// item, 4 lanes per (query, head), 0.33 of the HBM roofline with 1.87x the algorithmic bytes on the memory side and
// ~2 600 vector instructions per wave and item):
//   * work item = (image, pyramid COLUMN, head): the queries of ALL levels whose pixel centres fall into one cell of a
//     CX x CY grid over the image -- e.g. 32 x 22 pixels of the 128^2 level + 16 x 11 + 8 x 6 + 4 x 3 of the coarser
//     ones, <= 1024 queries.  Every query of the column samples, on each level, around the same spatial cell, so one
//     window per level serves the whole column: ~1.9 staged head-pixels per query instead of 3.3 (fine tiles re-staging
//     the coarse levels), and a coarse-level query looking at a fine level needs no window of its own;
//   * one lane = one (query, head): it loads its whole 128-byte sampling-location record and 64-byte weight record
//     (nothing is shared between lanes, so no DPP broadcasts and no owner/consumer split), derives each sample's
//     geometry once and accumulates all D = 16 channels -- ~45 % of the vector instructions per sample;
//   * a 64-byte head-pixel is read as four ds_read_b128 whose piece order is ROTATED per 8-lane block
//     (piece (j + lane/8) % 4 in instruction j): the 16 lanes the LDS serves together would otherwise meet on 4 of
//     the 16 bank groups (pixels are 64 B apart) -- 4-way conflicts; the rotation only permutes which accumulator
//     register holds which 4 channels, which the final store undoes with address arithmetic;
//   * three workgroups of 256 threads per CU, each with a pool of ~50 KB of LDS, windows = per-level bounding boxes of
//     the column's samples (packed-u16 min/max: DPP inside a wave, one LDS hop across the 4 waves) staged by LDS-DMA
//     with a zero apron; levels that do not fit the pool together are staged and gathered in successive PHASES
//     (accumulators stay in registers), a level whose box alone exceeds the pool is gathered from global memory
//     through a bounds-checked buffer descriptor;
//   * persistent grid, items handed out per XCD from self-resetting counters, two items ahead, the two heads that share
//     every 128-byte line of a column's windows adjacent.
// The launch-level structure -- column grid, a lane's slot, the cell tables, item order and decode, the queue, the
// quad-cooperative record fetch -- is shared with msda_forward_col16.hip and msda_backward_col.hip and lives, with its
// reasoning, in msda_col_common.hpp; this file keeps the windows and their phases, the staging and the gather.
#include <math.h>

#include <utility>

#include "msda_col_common.hpp"
#include "launchers.hpp"

namespace pct {

// 256 threads per workgroup, 3 workgroups per CU, a ~50 KB LDS pool each (168 registers): the memory phases of one
// workgroup (records, staging) overlap the gather of the others.
constexpr int COL_BLOCK = 256, COL_WG_PER_CU = 3, COL_POOL_KB = 50;

// PP ("piece planes", an MI355X-native operand layout for the callers that control the producers -- the encoder's own
// projection GEMM writes it, pct_ms_deform_attn_forward_planes_f32): value, locations / offsets and weights / logits are
// stored per image as [heads * pieces][queries][4 floats], piece = four consecutive floats of a (query, head) record.  A
// lane then loads piece i of ITS OWN record at (plane * S + query) * 16: the 64 lanes of a wave read the pieces of
// consecutive queries, i.e. whole 128-byte lines, 2 - 8 tag look-ups per instruction -- and the quad-cooperative access with
// its register transposes (176 vector instructions per wave and item), the half lines a record shares with its sibling
// head's and the 64-byte-in-512 pixel slices of the window staging are all gone.  Same arithmetic, bit-identical output.
template <int L, bool FUSED, bool PP = false>
__global__ __launch_bounds__(COL_BLOCK, COL_WG_PER_CU) void msda_forward_col_kernel(
    const float *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
    const float *__restrict__ loc, const float *__restrict__ attn, const int N, const int S, const int M,
    const int pool_px, float *__restrict__ out, const float *__restrict__ ref, const long long ref_batch_stride,
    unsigned *__restrict__ queue)
{
  constexpr int P = 4, D = 16, PXB = 64, BLOCK = COL_BLOCK, NW = BLOCK / 64;
  static_assert(L >= 1 && L <= 5 && NW <= 16, "unsupported geometry");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned char *pool = smem_raw;                                              // level windows, 64 B per head-pixel
  unsigned *bb = reinterpret_cast<unsigned *>(smem_raw + (size_t)pool_px * PXB);   // [L][NW][2] per-wave boxes {min lo, ~max hi}
  unsigned *next_idx = bb + NW * L * 2;                                        // the workgroup's next item

  int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int MD = M * D;

  // ---- level geometry (uniform) -------------------------------------------------------------------------------------
  ColLevels<L> lv;
  col_f32x2 fWH[L], invWH[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    lv.H[l] = (int)shapes[2 * l];
    lv.W[l] = (int)shapes[2 * l + 1];
    lv.St[l] = (int)starts[l];
    fWH[l] = uni_pair((float)lv.W[l], (float)lv.H[l]);
    invWH[l] = uni_pair(1.0f / (float)lv.W[l], 1.0f / (float)lv.H[l]);           // FUSED: offset / (W, H) as offset * (1 / W, 1 / H)
  }

  // ---- column grid, this lane's slot in a column, the cell tables and the launch's items (msda_col_common.hpp) --------
  const ColGrid grid = col_grid<L, BLOCK>(lv, S);
  ColSlot slot = col_lane_slot<L>(lv, grid, tid);
  // the tables are carved off the end of the pool; a grid whose tables would take more than half of it is not used (flat columns)
  const int tab_px = (col_table_bytes<L>(grid) + PXB - 1) / PXB;
  const int pool_eff = pool_px - tab_px;
  unsigned *tab = reinterpret_cast<unsigned *>(pool + (size_t)max(pool_eff, 0) * PXB);
  const bool use_tab = pool_eff * 2 >= pool_px;
  if (use_tab) col_fill_tables<L, BLOCK>(tab, lv, grid, tid);
  const int pool_use = use_tab ? pool_eff : pool_px;                           // pixels the windows may take
  const ColItems ci = col_items<L, BLOCK>(lv, grid, use_tab, N, M);

  // this lane's place in its quad (quad-cooperative record access, msda_col_common.hpp)
  int qi = lane & 3;
  const bool qi0 = qi & 1, qi1 = qi & 2;
  const bool qn1 = ((4 - qi) & 3) & 2;                                         // bit 1 of (-qi) % 4 (bit 0 is qi0)

  // per-lane rotation of the four 16-byte pieces of a head-pixel (see the header)
  const unsigned rho = (unsigned)(lane >> 3) & 3u;
  unsigned rot[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) rot[j] = ((j + rho) & 3u) << 4;

  // ---- persistent, XCD-chunked walk over the items, software-pipelined across items.  The queue runs TWO items ahead
  // (msda_col_common.hpp): right behind barrier (A) of item i every lane knows its next query and ISSUES THE NEXT ITEM'S
  // SAMPLING-LOCATION LOADS; they stay in flight through staging and gather of item i (32 registers) and item i + 1 starts
  // on data that has already landed.  (Measured before this change: a workgroup spent a third of an item waiting for them.)
  const ColChunk ch = col_chunk(ci.items);

  constexpr int NPL = L * 2, NGL = (NPL + 3) / 4;                              // locations: 16-byte pieces, 64-byte groups
  constexpr int NGW = (L + 3) / 4;                                             // weights: one 16-byte piece per level

  auto decode = [&](const int it, int &b_, int &m_, int &qv_) {               // col_decode for this launch and lane
    const ColItem i = col_decode<L, BLOCK>(it, ci, grid, lv, tab, slot, tid);
    b_ = i.b;
    m_ = i.m;
    qv_ = i.qv;
  };
  typedef unsigned col_u32x4 __attribute__((ext_vector_type(4)));
  constexpr int RSRC_FLAGS = 0x00020000;
  // the location records of the quad's four queries (quad-cooperative, msda_col_common.hpp)
  auto issue_loc = [&](const int b_, const int m_, const int qv_, col_f32x4 (&raw)[NGL][4]) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(loc + (long long)b_ * S * M * (L * P * 2)), 0,
                                                      (int)((unsigned)S * (unsigned)M * (unsigned)(L * P * 8)), RSRC_FLAGS);
    if constexpr (PP) {                           // piece i of (query, head m_): plane m_ * NPL + i, the plane in the scalar offset
      const unsigned qo = (unsigned)(qv_ ^ (qv_ >> 31)) << 4;
      const unsigned s16 = (unsigned)__builtin_amdgcn_readfirstlane(S) * 16u;
      const unsigned p0 = (unsigned)__builtin_amdgcn_readfirstlane(m_) * (unsigned)NPL * s16;       // (scalar unit, not 12 vector multiplies)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int g = 0; g < NGL; ++g)
          raw[g][s4] = g * 4 + s4 < NPL
                           ? __builtin_bit_cast(col_f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                 rs, (int)qo, (int)(p0 + (unsigned)(g * 4 + s4) * s16), 0))
                           : col_f32x4{0.f, 0.f, 0.f, 0.f};
      return;
    }
    col_quad_load<NGL>(rs, col_rec_index(qv_, m_, M) * (unsigned)(L * P * 8), qi, raw);
  };
  // FUSED: the query's reference points (one (x, y) per level), fetched with the record
  auto issue_ref = [&](const int b_, const int qv_, col_f32x2 (&rr)[L]) {
    if constexpr (FUSED) {
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(ref + b_ * ref_batch_stride), 0,
                                                        (int)((unsigned)S * (unsigned)(L * 8)), RSRC_FLAGS);
      const unsigned o = (unsigned)(qv_ ^ (qv_ >> 31)) * (unsigned)(L * 8);
      if constexpr (L % 2 == 0) {                   // 16-byte loads (launcher: ref is 16-byte aligned when L is even)
#pragma unroll
        for (int l = 0; l < L; l += 2) {
          const col_f32x4 r4 = __builtin_bit_cast(col_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(o + 8u * l), 0, 0));
          rr[l] = col_f32x2{r4[0], r4[1]};
          rr[l + 1] = col_f32x2{r4[2], r4[3]};
        }
      } else {
#pragma unroll
        for (int l = 0; l < L; ++l)
          rr[l] = __builtin_bit_cast(col_f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(o + 8u * l), 0, 0));
      }
    }
  };

  int item = ch.xcd * ch.chunk + ch.slot0;
  bool have = item < ch.item_end;
  int b = 0, m = 0, qv = 0;
  col_f32x4 raw[NGL][4];
  if (have) {
    decode(item, b, m, qv);
    issue_loc(b, m, qv, raw);
    col_queue_first_fetch(queue, next_idx, ch, tid);
  }

  while (have) {
    // (opaque per iteration: the compiler otherwise hoists every per-lane expression of tid / qi out of the item loop --
    // a dozen 64-bit piece offsets, float copies of tid, ... -- and spills them)
    asm volatile("" : "+v"(tid), "+v"(qi), "+v"(slot.slot), "+v"(slot.c0));
    const unsigned own = col_rec_index(qv, m, M);                             // this lane's record: query * M + head

    // FUSED: the reference points sit in L2 (shared by the heads and the batch): fetched here, not a whole item ahead
    // (eight more registers alive across the gather spilled); the transposition below runs while they arrive
    col_f32x2 rr[L];
    issue_ref(b, qv, rr);
    // ---- the record: sampling locations (FUSED: reference point + offset / (W, H)), loaded one item ago ----------------
    col_f32x2 lxy[L][P];
    {
      if constexpr (!PP) {
#pragma unroll
        for (int g = 0; g < NGL; ++g) quad_transpose_in(raw[g], qi0, qi1);
      }
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int k = 0; k < P; ++k) {
          const col_f32x4 pc = raw[(l * 2 + k / 2) / 4][(l * 2 + k / 2) & 3];
          col_f32x2 v = {pc[(k & 1) * 2], pc[(k & 1) * 2 + 1]};
          if constexpr (FUSED) v = __builtin_elementwise_fma(v, invWH[l], rr[l]);
          // from here on the PIXEL coordinates (w_im, h_im) = loc * (W, H) - 0.5 (cuh:283-288), formed once for the
          // boxes and the gather (packed FMAs: x and y in one instruction)
          const col_f32x2 px = __builtin_elementwise_fma(v, fWH[l], col_f32x2{-0.5f, -0.5f});
          // The reference gates a sample on -1 < w_im < W and -1 < h_im < H (cuh:290-296).  Here the gate is folded into
          // the coordinate itself: a coordinate that fails its test (NaN included: the comparison is false) moves to -2,
          // one that passes W moves to W.  The staged window carries a ZERO APRON of two pixels on each side (columns
          // -2, -1 and W, W + 1), so a sample moved there reads four apron pixels -- its contribution is exactly 0 and no
          // map pixel is touched, which is what the reference's `if` gives -- and every other sample keeps its own
          // coordinates.  No per-sample gate, select or predicate is left in the gather (it cost 13 vector instructions
          // per sample).
          lxy[l][k][0] = fminf(px[0] > -1.f ? px[0] : -2.f, fWH[l][0]);
          lxy[l][k][1] = fminf(px[1] > -1.f ? px[1] : -2.f, fWH[l][1]);
        }
    }

    // (everything that waits for the reference-point loads must be complete before the atomic below is issued)
    if constexpr (FUSED) {
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int k = 0; k < P; ++k) asm volatile("" : "+v"(lxy[l][k]));
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- publish the next item's index, fetch the one after it (its value is parked in LDS behind the staging barrier).
    // Issued behind the loads the pre-pass waits for: the memory counter is in-order, a wait for those would include it. ---
    const ColFetch fetch = col_queue_publish(queue, next_idx, ch, item, tid);

    // ---- pre-pass: per-level bounding box (first corners, biased by +1; the box covers x0 .. x0 + 1) ----------------
#pragma unroll
    for (int l = 0; l < L; ++l) {
      // min / max over the lane's four samples (already inside [-2, W] x [-2, H], see above); the gather floors the very
      // same registers.  Packed as u16 pairs biased by +2 (low corner) / +3 (high corner + 1: the box covers x0 .. x0 + 1).
      const float mnx = fminf(fminf(lxy[l][0][0], lxy[l][1][0]), fminf(lxy[l][2][0], lxy[l][3][0]));
      const float mxx = fmaxf(fmaxf(lxy[l][0][0], lxy[l][1][0]), fmaxf(lxy[l][2][0], lxy[l][3][0]));
      const float mny = fminf(fminf(lxy[l][0][1], lxy[l][1][1]), fminf(lxy[l][2][1], lxy[l][3][1]));
      const float mxy = fmaxf(fmaxf(lxy[l][0][1], lxy[l][1][1]), fmaxf(lxy[l][2][1], lxy[l][3][1]));
      const unsigned lo = (unsigned)(cvt_flr(mnx) + 2) | ((unsigned)(cvt_flr(mny) + 2) << 16);
      const unsigned hi = (unsigned)(cvt_flr(mxx) + 3) | ((unsigned)(cvt_flr(mxy) + 3) << 16);
      const unsigned red = wave_reduce_box(lo, hi);                 // lane 31: min lo, lane 63: ~max hi
      if ((lane & 31) == 31) bb[(l * NW + wave) * 2 + (lane >> 5)] = red;
    }
    // ---- this item's weights (FUSED: logits): fetched now, looked at after the staging barrier.  (Behind the pre-pass:
    // anything that waits on the memory counter there -- it is in-order -- would otherwise wait for these loads too.) ---------
    col_f32x4 wraw[NGW][4];
    auto load_weights = [&]() {
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(attn + (long long)b * S * M * (L * P)), 0,
                                                        (int)((unsigned)S * (unsigned)M * (unsigned)(L * P * 4)), RSRC_FLAGS);
      if constexpr (PP) {                         // piece = level: the level's P = 4 weights of (query, head)
        const unsigned qo = (unsigned)(qv ^ (qv >> 31)) << 4;
        const unsigned s16 = (unsigned)__builtin_amdgcn_readfirstlane(S) * 16u;
        const unsigned p0 = (unsigned)__builtin_amdgcn_readfirstlane(m) * (unsigned)L * s16;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
          for (int g = 0; g < NGW; ++g)
            wraw[g][s4] = g * 4 + s4 < L
                              ? __builtin_bit_cast(col_f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                    rs, (int)qo, (int)(p0 + (unsigned)(g * 4 + s4) * s16), 0))
                              : col_f32x4{0.f, 0.f, 0.f, 0.f};
        return;
      }
      col_quad_load<NGW>(rs, own * (unsigned)(L * P * 4), qi, wraw);
    };
    load_weights();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                       // boxes in LDS before the barrier
    __syncthreads();                                                          // (A) boxes visible; pool free
    // Wave priorities (s_setprio) by part of an item: records, pre-pass, planning, staging and decode 0, the first gathered
    // level 3, the other levels 2.  A wave in its gather is served before the waves of the other workgroups that are
    // decoding, planning or staging -- the gather is the LDS-latency chain of an item, everything else fills its gaps --
    // and the first (finest, largest) level before the later ones.  Same-box A/B, P2 batch 128: I 1.70 -> 1.65 ms, M 2.24
    // -> 2.16 ms against no priorities; other splits (gather 3 / 3, 1 / 1, planning raised) were within 1 % of each other
    // on I and 2 % worse on M.
    __builtin_amdgcn_s_setprio(0);

    // ---- the next item: its query per lane, its location loads issued (in flight until the next iteration) --------------
    const int item_n = col_next_item(next_idx, ch);
    int b_n = 0, m_n = 0, qv_n = 0;
    const bool have_n = item_n < ch.item_end;             // (decoded once this item's first staging is issued, below)

    // ---- windows and phases (uniform) --------------------------------------------------------------------------------
    int wx0[L], wy0[L], wwid[L], whgt[L], wsize[L], wbase[L], phase_of[L];
    bool latin[L];
    bool starts_phase[L];
    {
#pragma unroll
      for (int l = 0; l < L; ++l) {
        unsigned lo, hi;
        block_box<NW>(bb + l * NW * 2, lo, hi);
        // un-bias (the origin may be -2: apron).  hi >= lo + 1 in both halves -- a box always holds a sample's two
        // columns and two rows -- so there is no empty case
        const unsigned lx = lo & 0xFFFFu, ly = lo >> 16;
        wx0[l] = (int)lx - 2;
        wy0[l] = (int)ly - 2;
        wwid[l] = (int)((hi & 0xFFFFu) - lx) + 1;
        // (conflict-free corner order, below: the four corners of a sample must fall into four different bank classes --
        // pool index mod 4 -- which they do when the window is 2 mod 4 pixels wide; the extra columns are staged like any other)
        // Taken only where the box is much larger than the column's cell on this level, i.e. where the lanes' offsets
        // differ by several pixels and their pixel classes collide (model-like offsets: halo ~14 + 14 pixels; the init-like
        // ones, whose classes are consecutive by construction, stay at 4 - 10 and keep the cheaper fixed order).  Same-box
        // A/B, P2 batch 128 (profiles/r04_forward_structural_ab.txt), against the fixed order everywhere: M 2.168 -> 2.085 ms
        // as an op, 2.290 -> 2.209 ms in the bench step; I 1.649 -> 1.700 (the two code paths cost the init-like case 3
        // spilled registers).  The conflict-free order on every level: M 2.038, I 1.779.
        latin[l] = (wwid[l] - col_max_cell(lv.W[l], grid.CX)) + ((int)((hi >> 16) - ly) + 1 - col_max_cell(lv.H[l], grid.CY)) >= 16;
        if (latin[l]) wwid[l] += (2 - wwid[l]) & 3;
        whgt[l] = (int)((hi >> 16) - ly) + 1;
        wsize[l] = wwid[l] * whgt[l];
      }
      // levels are gathered in a fixed order (col_level_of_step); a level that does not fit beside the ones already
      // planned opens a new PHASE: the pool is re-staged right before it (two barriers)
      int ph = 0, used = 0;
      bool fresh = true;
#pragma unroll
      for (int ll = 0; ll < L; ++ll) {
        const int l = col_level_of_step<L>(ll);
        starts_phase[l] = false;
        // (never fits -- or a map too large for the 16-bit box corners --: gathered from global memory, which does not look at the box)
        if (wsize[l] > pool_use || ci.big_map) {
          phase_of[l] = -1;
          wbase[l] = 0;
          continue;
        }
        if (used + wsize[l] > pool_use) {
          ++ph;
          used = 0;
          fresh = true;
        }
        phase_of[l] = ph;
        starts_phase[l] = fresh;
        fresh = false;
        wbase[l] = used;
        used += wsize[l];
      }
    }

    // EARLY second phase.  With model-like offsets the four windows of a column need two phases ({finest, coarsest} and the
    // two middle levels).  The finest level is gathered first and sits at the bottom of the pool, the second phase's windows
    // are planned from the bottom too: when they fit inside the finest window's region, they are staged right behind the
    // finest level's gather (one barrier: every wave is done with that region) and FLY while the coarsest level is gathered
    // from its own region above -- instead of the workgroup sitting through that flight between two barriers later.
    bool early_ok = false;
    if constexpr (L >= 3) {
      int used1 = 0;
      bool has1 = false;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        used1 += phase_of[l] == 1 ? wsize[l] : 0;
        has1 = has1 || phase_of[l] == 1;
      }
      early_ok = has1 && phase_of[L - 1] == 0 && phase_of[col_level_of_step<L>(1)] == 0 && wbase[L - 1] == 0 &&
                 used1 <= wsize[L - 1];
    }

    int woff[L];
#pragma unroll
    for (int l = 0; l < L; ++l) woff[l] = wbase[l] - wy0[l] * wwid[l] - wx0[l];
    float wts[L][P];
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(value + (long long)b * S * MD), 0,
                                                        (int)((unsigned)S * (unsigned)MD * 4u), 0x00020000);

    col_f32x2 acc[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = col_f32x2{0.f, 0.f};

    // (the empty asm pins the accumulators: without it the compiler sinks a level's 128 packed FMAs below the LDS reads of
    // all four samples and spills the 256 data registers in between)
    auto pin_acc = [&]() {
      asm volatile("" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[2][0]),
                        "+v"(acc[2][1]), "+v"(acc[3][0]), "+v"(acc[3][1]));
    };
    // two corners of one pixel row: corner-major, so consecutive packed FMAs go to different accumulators (8 chains)
    auto fma_row = [&](const col_f32x4 (&va)[4], const col_f32x4 (&vb)[4], const float wa, const float wb) {
      const col_f32x2 wwa = {wa, wa}, wwb = {wb, wb};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e)
          acc[j][e] = __builtin_elementwise_fma(wwa, col_f32x2{va[j][2 * e], va[j][2 * e + 1]}, acc[j][e]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e)
          acc[j][e] = __builtin_elementwise_fma(wwb, col_f32x2{vb[j][2 * e], vb[j][2 * e + 1]}, acc[j][e]);
    };
    // a sample's geometry: first corner and the four bilinear * attention weights (the gate of cuh:290-296 is already in
    // the coordinates, see where lxy is formed)
    struct Geo {
      col_f32x2 g12, g34;                 // (hh * hw, hh * lw) * w and (lh * hw, lh * lw) * w
      int x0, y0;
    };
    auto geometry = [&](auto lc, auto kc) {
      constexpr int l = decltype(lc)::value;
      constexpr int k = decltype(kc)::value;
      // (opaque: without it the compiler hoists every sample's geometry to the top of the item and keeps it alive)
      asm volatile("" : "+v"(lxy[l][k]));                                      // (in place: the coordinates are not needed again)
      const col_f32x2 pix = lxy[l][k];
      Geo g;
      g.x0 = cvt_flr(pix[0]);
      g.y0 = cvt_flr(pix[1]);
      const float lw = __builtin_amdgcn_fractf(pix[0]), lh = __builtin_amdgcn_fractf(pix[1]);
      const col_f32x2 ax = {1.f - lw, lw}, ay = {1.f - lh, lh};                // (hw, lw), (hh, lh): pairs as the packed ops take them
      const col_f32x2 t = ax * col_f32x2{wts[l][k], wts[l][k]};                // (hw, lw) * w
      g.g12 = t * col_f32x2{ay[0], ay[0]};
      g.g34 = t * col_f32x2{ay[1], ay[1]};
      return g;
    };

    // One level from its LDS window, one pixel ROW of a sample at a time (two corners = 8 x 16 B per lane in flight): the
    // other waves of the SIMD cover the LDS latency.  (A rolling pipeline with the next row's reads in flight during the
    // FMAs needs 32 more data registers than the 168 of three workgroups per CU leave: it spilled and was slower.)
    // All four corners lie inside the staged window (out-of-map ones are apron zeros).
    auto gather_level_lds = [&](auto lc) {
      constexpr int l = decltype(lc)::value;
      [&]<int... Ks>(std::integer_sequence<int, Ks...>) {
        ([&] {
          const Geo g = geometry(lc, std::integral_constant<int, Ks>{});
          // pixel (x0, y0) sits at pool index woff + y0 * width + x0 (woff folds the window origin and base: one scalar)
          const unsigned a = (unsigned)(__mul24(g.y0, wwid[l]) + g.x0 + woff[l]) << 6;
          const unsigned rowb = (unsigned)wwid[l] << 6;
          {
            col_f32x4 va[4], vb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const unsigned char *pa = pool + (a + rot[j]);
              va[j] = *reinterpret_cast<const col_f32x4 *>(pa);
              vb[j] = *reinterpret_cast<const col_f32x4 *>(pa + PXB);
            }
            fma_row(va, vb, g.g12[0], g.g12[1]);
          }
          pin_acc();
          __builtin_amdgcn_sched_barrier(0);
          {
            col_f32x4 va[4], vb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const unsigned char *pb = pool + (a + rowb + rot[j]);
              va[j] = *reinterpret_cast<const col_f32x4 *>(pb);
              vb[j] = *reinterpret_cast<const col_f32x4 *>(pb + PXB);
            }
            fma_row(va, vb, g.g34[0], g.g34[1]);
          }
          pin_acc();
          __builtin_amdgcn_sched_barrier(0);
        }(), ...);
      }(std::make_integer_sequence<int, P>{});
    };
    // The same level with a CONFLICT-FREE corner order.  The LDS serves a ds_read_b128 in groups of 16 lanes, four lanes of
    // each 8-lane block (one QUAD) per group; the piece rotation above keeps the quads of a group on different bank
    // quarters, so what is left to collide are the four lanes of a quad whose pixels fall into the same class (pool index
    // mod 4: pixels are 64 B = 16 banks apart) -- with model-like offsets 59 % of all LDS cycles of the kernel.  A sample's
    // four corners are the pool indices i, i + 1, i + width, i + width + 1: with the window width = 2 (mod 4) they are one
    // pixel of EACH class.  So lane q of the quad starts with the corner of class q and walks the classes upwards: at every
    // corner step the quad's four lanes read four different classes, whatever the locations.  Price: the corner order
    // differs per lane and sample -- offsets and weights are selected by two bits of (q - i) -- ~27 vector instructions
    // per sample more than the fixed order.  The sums are accumulated in a different order per lane than with the fixed
    // order (results agree to rounding, not bit for bit).
    auto gather_level_lds_latin = [&](auto lc) {
      constexpr int l = decltype(lc)::value;
      [&]<int... Ks>(std::integer_sequence<int, Ks...>) {
        ([&] {
          asm volatile("" : "+v"(lxy[l][Ks]));
          const col_f32x2 pix = lxy[l][Ks];
          const int x0 = cvt_flr(pix[0]), y0 = cvt_flr(pix[1]);
          const float lw = __builtin_amdgcn_fractf(pix[0]), lh = __builtin_amdgcn_fractf(pix[1]);
          const float hw = 1.f - lw, hh = 1.f - lh;
          const col_f32x2 tw = col_f32x2{hw, lw} * col_f32x2{wts[l][Ks], wts[l][Ks]};      // (hw, lw) * w, as the fixed order
          const unsigned pi = (unsigned)(__mul24(y0, wwid[l]) + x0 + woff[l]);
          const unsigned e = ((unsigned)qi - pi) & 3u;          // first corner d = dx + 2 dy of this lane; then d + 1, d + 2, d + 3 (mod 4)
          const bool e0 = e & 1u, e1 = e & 2u, f1 = (e + 1u) & 2u;                          // dy of the steps: e1, f1, !e1, !f1
          const float wa = e0 ? tw[1] : tw[0], wb = e0 ? tw[0] : tw[1];                    // dx of the steps: e0, !e0, e0, !e0
          const unsigned rowb = (unsigned)wwid[l] << 6;
          const unsigned base = pi << 6;
          const unsigned xa = e0 ? 64u : 0u, xb = xa ^ 64u;
          const unsigned a0 = base + xa + (e1 ? rowb : 0u), a1 = base + xb + (f1 ? rowb : 0u);
          const unsigned a2 = base + xa + (e1 ? 0u : rowb), a3 = base + xb + (f1 ? 0u : rowb);
          const float w0 = wa * (e1 ? lh : hh), w1 = wb * (f1 ? lh : hh), w2 = wa * (e1 ? hh : lh), w3 = wb * (f1 ? hh : lh);
          {
            col_f32x4 va[4], vb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              va[j] = *reinterpret_cast<const col_f32x4 *>(pool + (a0 + rot[j]));
              vb[j] = *reinterpret_cast<const col_f32x4 *>(pool + (a1 + rot[j]));
            }
            fma_row(va, vb, w0, w1);
          }
          pin_acc();
          __builtin_amdgcn_sched_barrier(0);
          {
            col_f32x4 va[4], vb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              va[j] = *reinterpret_cast<const col_f32x4 *>(pool + (a2 + rot[j]));
              vb[j] = *reinterpret_cast<const col_f32x4 *>(pool + (a3 + rot[j]));
            }
            fma_row(va, vb, w2, w3);
          }
          pin_acc();
          __builtin_amdgcn_sched_barrier(0);
        }(), ...);
      }(std::make_integer_sequence<int, P>{});
    };
    // ... or from global memory (a level whose box exceeds the pool), through the buffer descriptor: out-of-map corners
    // get an out-of-range offset and read zeros.  A head-pixel is 64 contiguous bytes; fetched lane by lane, every
    // 16-byte access of a wave instruction touches a different 128-byte line and the texture addresser serialises the 64
    // tag look-ups (measured: uniformly random locations ran at 0.064 of the roofline, half the windowed kernel's rate).
    // So the QUAD works on one member's sample at a time: the member's four corner offsets and weights are broadcast
    // (DPP), lane c fetches piece (s - c) % 4 of every corner of member s's sample -- the quad reads whole 64-byte
    // pixels, 16 look-ups per instruction -- and accumulates "its piece of member s's sum".  After the level the 4 x 4
    // block of pieces is transposed back (as the record loads are) and added to the lane's own accumulators.
    // Measured at the north-star shape, uniformly random locations: 13.9 -> 5.3 ms; distributions I / M pay < 1 % (same
    // box A/B).  (As a real, non-inlined function the kernel ran at half speed on EVERY input: scratch set-up and
    // call-clobbered registers.  With two or four members' fetches in flight the hot path picked up spills whose reloads
    // wait on the memory counter behind the prefetched records: +5 % on I / M, and 6.1 ms on U.  One member at a time is
    // spill-free at 4 levels and the fastest on U.)
    auto gather_level_global = [&](auto lc) {
      constexpr int l = decltype(lc)::value;
      const int H = lv.H[l], W = lv.W[l];
      constexpr unsigned OOB = 0x80000000u;                                    // S * M * D * 4 < 2^31 (C ABI check)
      const unsigned MDb = (unsigned)MD * 4u;
      col_f32x2 part[4][2];                                                    // [member s]: piece (s - qi) % 4 of s's sum
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) part[s4][0] = part[s4][1] = col_f32x2{0.f, 0.f};
      [&]<int... Ks>(std::integer_sequence<int, Ks...>) {
        ([&] {
          const Geo g = geometry(lc, std::integral_constant<int, Ks>{});
          const bool top = (unsigned)g.y0 < (unsigned)H, bot = (unsigned)(g.y0 + 1) < (unsigned)H;   // (y0, x0 in [-2, H] x [-2, W])
          const bool lft = (unsigned)g.x0 < (unsigned)W, rgt = (unsigned)(g.x0 + 1) < (unsigned)W;
          // (PP: piece c of pixel p of head m at ((m * 4 + c) * S + p) * 16: the pixel stride is 16 bytes, the piece a plane)
          const unsigned pxs = PP ? 16u : MDb;
          const unsigned a = PP ? (unsigned)(m * (D / 4) * S + lv.St[l] + g.y0 * W + g.x0) * 16u
                                : (unsigned)(lv.St[l] + g.y0 * W + g.x0) * MDb + (unsigned)(m * D) * 4u;
          const unsigned o1 = (top && lft) ? a : OOB, o2 = (top && rgt) ? a + pxs : OOB;
          const unsigned o3 = (bot && lft) ? a + (unsigned)W * pxs : OOB, o4 = (bot && rgt) ? a + (unsigned)W * pxs + pxs : OOB;
          [&]<int... Ss>(std::integer_sequence<int, Ss...>) {                    // one member at a time (16 registers of data)
            ([&] {
              constexpr int CT = BcastCtrl<4, Ss>::value;
              const unsigned pc = PP ? (unsigned)((Ss - qi) & 3) * ((unsigned)S * 16u)     // (an out-of-range offset stays out of range)
                                     : (unsigned)((Ss - qi) & 3) << 4;
              col_f32x4 v[4];
              v[0] = __builtin_bit_cast(col_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(dpp_u<CT>(o1) + pc), 0, 0));
              v[1] = __builtin_bit_cast(col_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(dpp_u<CT>(o2) + pc), 0, 0));
              v[2] = __builtin_bit_cast(col_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(dpp_u<CT>(o3) + pc), 0, 0));
              v[3] = __builtin_bit_cast(col_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(dpp_u<CT>(o4) + pc), 0, 0));
              const float w[4] = {dpp_f<CT>(g.g12[0]), dpp_f<CT>(g.g12[1]), dpp_f<CT>(g.g34[0]), dpp_f<CT>(g.g34[1])};
#pragma unroll
              for (int c4 = 0; c4 < 4; ++c4)
#pragma unroll
                for (int e = 0; e < 2; ++e)
                  part[Ss][e] = __builtin_elementwise_fma(col_f32x2{w[c4], w[c4]},
                                                          col_f32x2{v[c4][2 * e], v[c4][2 * e + 1]}, part[Ss][e]);
              asm volatile("" : "+v"(part[0][0]), "+v"(part[0][1]), "+v"(part[1][0]), "+v"(part[1][1]), "+v"(part[2][0]),
                                "+v"(part[2][1]), "+v"(part[3][0]), "+v"(part[3][1]));
              __builtin_amdgcn_sched_barrier(0);
            }(), ...);
          }(std::make_integer_sequence<int, 4>{});
        }(), ...);
      }(std::make_integer_sequence<int, P>{});
      col_f32x4 x[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) x[s4] = col_f32x4{part[s4][0][0], part[s4][0][1], part[s4][1][0], part[s4][1][1]};
      quad_transpose_in(x, qi0, qi1);                                          // x[k] = piece k of this lane's own sum
      rot_regs(x, rho & 1u, rho & 2u);                                         // x[j] = piece (j + rho) % 4: the slot order
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4) {
        acc[j4][0] += col_f32x2{x[j4][0], x[j4][1]};
        acc[j4][1] += col_f32x2{x[j4][2], x[j4][3]};
      }
      pin_acc();
      __builtin_amdgcn_sched_barrier(0);
    };

    // stage the windows of one phase: LDS-DMA (buffer_load_dwordx4 ... lds), no VGPR round trip, every piece in flight at
    // once; LDS address of a piece = wave-uniform base + lane * 16; the global source is a per-lane 32-bit offset into this
    // image's buffer descriptor
    auto stage_phase = [&](const int phx) {
      // One wave instruction copies 64 consecutive 16-byte pieces = CPX pixels of ONE window row; the waves take the rows
      // in turn.  A lane's source offset splits into a per-lane part that depends on its column only (computed once per
      // level and 64-piece column block) and a per-row part that is uniform and travels in the instruction's scalar
      // offset: no vector arithmetic per copy.  (Piece-linear indexing cost ~18 vector instructions per copy: a third of
      // the kernel's vector work when the windows are wide.)  Columns outside the map keep an out-of-range offset, rows
      // outside the map use it for every lane: the descriptor's bounds check then delivers zeros -- the apron.
      constexpr int PPX = PXB / 16, CPX = 64 / PPX;
      constexpr unsigned OOB = 0x80000000u;
      const int ln = tid & 63;
      const int dx = ln / PPX, cc = ln & (PPX - 1);
      const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
      const unsigned MDb = (unsigned)MD * 4u;                                 // bytes per pixel, all heads
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if (phase_of[l] == phx && wsize[l] > 0) {
          // (PP: piece cc of a pixel lives in plane m * 4 + cc, pixels 16 bytes apart: a copy instruction reads four runs of
          // 256 consecutive bytes instead of sixteen 64-byte slices 512 bytes apart)
          const unsigned lvl_off = PP ? ((unsigned)(m * (D / 4)) * (unsigned)S + (unsigned)lv.St[l]) * 16u
                                      : (unsigned)lv.St[l] * MDb + (unsigned)(m * D) * 4u;   // bytes, this level and head
          const unsigned row_bytes = (unsigned)lv.W[l] * (PP ? 16u : MDb);
          unsigned char *dst = pool + (size_t)wbase[l] * PXB;
          for (int c0 = 0; c0 < wwid[l]; c0 += CPX) {
            const int xw = c0 + dx, x = wx0[l] + xw;
            const unsigned voff = (unsigned)x < (unsigned)lv.W[l]
                                      ? (PP ? (unsigned)x * 16u + (unsigned)cc * ((unsigned)S * 16u) : (unsigned)x * MDb + (unsigned)(cc * 16))
                                      : OOB;
            if (xw < wwid[l]) {
              for (int r = wv; r < whgt[l]; r += NW) {
                const int y = wy0[l] + r;
                const bool in_y = (unsigned)y < (unsigned)lv.H[l];
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsrc, (__attribute__((address_space(3))) void *)(dst + (size_t)(r * wwid[l] + c0) * PXB), 16,
                    (int)(in_y ? voff : OOB), (int)(in_y ? lvl_off + (unsigned)y * row_bytes : 0u), 0, 0);
              }
            }
          }
        }
      }
    };
    auto front_end = [&]() {                                                  // the weights, once they are needed
      if constexpr (!PP) {
#pragma unroll
        for (int g = 0; g < NGW; ++g) quad_transpose_in(wraw[g], qi0, qi1);
      }
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int k = 0; k < P; ++k) wts[l][k] = wraw[l / 4][l & 3][k];
      if constexpr (FUSED) {                                                  // softmax over the record's L * P logits
        // exp(x - mx) as exp2(x * log2(e) - mx * log2(e)): one packed FMA per logit pair instead of a subtraction and a
        // multiplication per logit; sums and the final scaling packed as well; 1 / sum as v_rcp_f32 (1 ulp) instead of
        // the ten-instruction IEEE division -- 50 vector instructions instead of 98 per (query, head)
        static_assert(P % 2 == 0, "logit pairs");
        float mx = -INFINITY;
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
          for (int k = 0; k < P; ++k) mx = fmaxf(mx, wts[l][k]);
        constexpr float LOG2E = 1.44269504088896340736f;
        const float nm = -mx * LOG2E;
        col_f32x2 sum2 = {0.f, 0.f};
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
          for (int k = 0; k < P; k += 2) {
            const col_f32x2 a = __builtin_elementwise_fma(col_f32x2{wts[l][k], wts[l][k + 1]}, col_f32x2{LOG2E, LOG2E},
                                                          col_f32x2{nm, nm});
            wts[l][k] = __builtin_amdgcn_exp2f(a[0]);
            wts[l][k + 1] = __builtin_amdgcn_exp2f(a[1]);
            sum2 += col_f32x2{wts[l][k], wts[l][k + 1]};
          }
        const float inv = __builtin_amdgcn_rcpf(sum2[0] + sum2[1]);
#pragma unroll
        for (int l = 0; l < L; ++l)
#pragma unroll
          for (int k = 0; k < P; k += 2) {
            const col_f32x2 w2 = col_f32x2{wts[l][k], wts[l][k + 1]} * col_f32x2{inv, inv};
            wts[l][k] = w2[0];
            wts[l][k + 1] = w2[1];
          }
      }
    };

    auto level_step = [&](auto llc) {
      constexpr int ll = decltype(llc)::value;
      constexpr int l = col_level_of_step<L>(ll);
      if (starts_phase[l]) {
        if (ll > 0 && early_ok && phase_of[l] == 1) {
          // staged early (below): landed + visible.  The memory counter is in order and the NEXT item's location record
          // was requested behind that staging: wait for everything BUT those youngest loads -- a plain barrier's
          // vmcnt(0) made every two-phase item sit through the best part of an HBM round trip here
          if (have_n) {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NGL * 4) : "memory");
          } else
            __syncthreads();
        } else {
          if (ll > 0) __syncthreads();                                        // every wave is done with the pool
          stage_phase(phase_of[l]);
          if constexpr (ll == 0) {
            if (have_n) decode(item_n, b_n, m_n, qv_n);                        // while the LDS-DMA pieces are in flight
            // (an unevaluated use: level_step keeps load_weights among its captures, and with that closure layout the
            // compiler allocates this kernel's registers exactly as in the build the recorded timings were taken with)
            (void)load_weights;
          }
          __syncthreads();                                                    // windows staged (vmcnt(0) + barrier)
        }
      }
      if constexpr (ll == 0) {
        // (thread 0) park the counter value fetched at the top of the item: the weights below need the memory counter at
        // zero anyway, so this wait is free -- anywhere earlier it would stall on the loads issued since
        col_queue_park(next_idx, fetch);
        front_end();
      }
      __builtin_amdgcn_s_setprio(ll == 0 ? 3 : 2);                            // (wave priorities: see the planning above)
      if (phase_of[l] >= 0) {
        if (latin[l]) gather_level_lds_latin(std::integral_constant<int, l>{});
        else gather_level_lds(std::integral_constant<int, l>{});
      }
      else gather_level_global(std::integral_constant<int, l>{});             // box larger than the pool: global memory
      // (marking the global-memory path unlikely makes hipcc outline it behind a real call: 544 bytes of scratch per lane, 10x slower)
      if constexpr (ll == 0 && L >= 3) {
        if (early_ok) {
          __syncthreads();                                                    // every wave is done with the finest window
          stage_phase(1);
        }
      }
      // the next item's location record (32 registers: the ones this level's points and the weights freed), all groups at
      // once behind the first gathered level: the two 64-byte halves of a 128-byte line back to back (-2 % on I and M
      // against one group per gathered level, same-box A/B)
      if constexpr (ll == 0) {
        if (have_n) issue_loc(b_n, m_n, qv_n, raw);
      }

    };
    if (!starts_phase[L - 1]) {                                               // (the finest level is gathered from global)
      if (have_n) decode(item_n, b_n, m_n, qv_n);
    }
    [&]<int... LLs>(std::integer_sequence<int, LLs...>) {
      (level_step(std::integral_constant<int, LLs>{}), ...);
    }(std::make_integer_sequence<int, L>{});
    __builtin_amdgcn_s_setprio(0);
    static_assert(NGL <= L, "one location group per level");

    {
      // store, quad-cooperatively: register j of lane c holds piece (j + rho) % 4 of ITS record (rho is the same in the
      // whole quad).  A quad_perm rotation by k hands lane i the register k of lane (i - k) % 4; rotating the four received
      // registers by -i puts the one that came from lane s into slot s: piece (i - s + rho) % 4 of record s.  Store
      // instruction s then writes the 64 consecutive bytes of record s from the quad's four lanes.
      col_f32x4 u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = col_f32x4{acc[j][0][0], acc[j][0][1], acc[j][1][0], acc[j][1][1]};
      u[1] = quad_rot<1>(u[1]);
      u[2] = quad_rot<2>(u[2]);
      u[3] = quad_rot<3>(u[3]);
      // slot s <- received register (i - s) % 4: reverse the order (compile time), then rotate by (-i) % 4
      col_f32x4 w4[4] = {u[0], u[3], u[2], u[1]};
      rot_regs(w4, qi0, qn1);
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(out + (long long)b * S * MD, 0,
                                                        (int)((unsigned)S * (unsigned)MD * 4u), RSRC_FLAGS);
      // an idle lane's record goes out of range (the descriptor's bounds check drops the store)
      // (the record index is formed again rather than kept alive through the gather)
      const unsigned own_o = (col_rec_index(qv, m, M) * (unsigned)(D * 4)) | ((unsigned)(qv >> 31) & 0x80000000u);
      const unsigned oo[4] = {dpp_u<0x00>(own_o), dpp_u<0x55>(own_o), dpp_u<0xAA>(own_o), dpp_u<0xFF>(own_o)};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
        // (non-temporal: the outputs are written once and must not push the value lines, which neighbouring columns and the
        // sibling head re-use, out of the XCD's L2.  The records are loaded with default caching: nt there re-fetches the
        // half lines two heads / two load groups share -- I: 7.9 -> 9.7 GB read per launch, 1.95 -> 2.14 ms.)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(col_u32x4, w4[s4]), rs,
                                               (int)(oo[s4] + ((unsigned)(((qi - s4) + (int)rho) & 3) << 4)), 0, 2);
    }

    item = item_n;
    have = have_n;
    b = b_n;
    m = m_n;
    qv = qv_n;
  }
}

// ---- launcher: returns PCT_NOT_COVERED when this geometry is not covered (caller uses another kernel) ----------------------------
// ref == nullptr: plain op; ref != nullptr: fused front-end (loc = raw offsets, attn = raw logits).
int launch_msda_forward_col(const MsdaFwdCall &c, bool planes)
{
  const int N = c.N, S = c.S, M = c.M, L = c.L;
  const float *ref = c.ref;
  if ((((uintptr_t)c.value | (uintptr_t)c.out | (uintptr_t)c.loc | (uintptr_t)c.attn) & 15u)) return PCT_NOT_COVERED;
  if (ref && (((uintptr_t)ref) & ((L % 2 == 0) ? 15u : 7u))) return PCT_NOT_COVERED;
  if (ref && (L % 2 == 0) && (c.ref_batch_stride & 3)) return PCT_NOT_COVERED;
  if (!msda_col_covers(c)) return PCT_NOT_COVERED;
  const int pool_px = COL_POOL_KB * 1024 / 64;
  const size_t lds = (size_t)pool_px * 64 + ((size_t)(COL_BLOCK / 64) * L * 2 + 4) * sizeof(unsigned);   // pool, boxes, queue words
  const dim3 grid(256 * COL_WG_PER_CU), block(COL_BLOCK);
  unsigned *queue = win_queue_slot(c.stream);                                  // nullptr: static item stride
  const float *v = static_cast<const float *>(c.value);
  const float *lc = static_cast<const float *>(c.loc), *at = static_cast<const float *>(c.attn);
  float *o = static_cast<float *>(c.out);
#define PCT_COL(L_, FU_, PP_)                                                                                           \
  do {                                                                                                                  \
    const hipError_t attr_rc = func_attr_per_device(reinterpret_cast<const void *>(&msda_forward_col_kernel<L_, FU_, PP_>)); \
    if (attr_rc != hipSuccess) return (int)attr_rc;                                                                     \
    hipLaunchKernelGGL((msda_forward_col_kernel<L_, FU_, PP_>), grid, block, lds, c.stream, v, c.shapes, c.starts, lc,  \
                       at, N, S, M, pool_px, o, ref, c.ref_batch_stride, queue);                                        \
  } while (0)
#define PCT_COL_L(FU_, PP_)               \
  do {                                    \
    if (L == 3) PCT_COL(3, FU_, PP_);     \
    else if (L == 4) PCT_COL(4, FU_, PP_); \
    else PCT_COL(5, FU_, PP_);            \
  } while (0)
  if (planes) {                         // piece-plane operands (see the kernel)
    if (ref) PCT_COL_L(true, true);
    else PCT_COL_L(false, true);
  } else {
    if (ref) PCT_COL_L(true, false);
    else PCT_COL_L(false, false);
  }
#undef PCT_COL_L
#undef PCT_COL
  return (int)hipGetLastError();
}

}  // namespace pct
