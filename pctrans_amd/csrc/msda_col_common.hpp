// Shared by the pyramid-column MSDeformAttn kernels (msda_forward_col.hip: fp32 values, 4 points; msda_forward_col16.hip:
// 16-bit values, 4 or 8 points; msda_backward_col.hip: the fp32 backward): the leaf helpers, and the launch-level structure
// of a column kernel -- column grid, lane slots, cell tables, item decode, XCD chunking, work queue, the quad-cooperative
// record fetch -- each stated once.  A kernel keeps what is its own: how it derives its windows from the boxes and plans
// them into phases, staging, gather / scatter, and its asm pins and scheduling barriers.
#pragma once
#include "msda_win_common.hpp"

namespace pct {

typedef int col_i32x4 __attribute__((ext_vector_type(4)));
typedef float col_f32x2 __attribute__((ext_vector_type(2)));
typedef float col_f32x4 __attribute__((ext_vector_type(4)));

// Gather order of the levels (step ll -> level).  The finest level (the last one in PCTrans' pyramids) comes first; its
// window is the largest, and the level that most often still fits beside it in the pool is the COARSEST one, so that
// one goes second and the two middle levels share the next phase: with model-like offsets at the north-star shape
// {finest, coarsest} + {the two middle levels} is two phases where finest-to-coarsest order needed three for every
// fifth item (each phase costs a re-staging of the pool and two barriers).
template <int L>
__host__ __device__ constexpr int col_level_of_step(const int ll)
{
  return ll == 0 ? L - 1 : (ll == 1 ? 0 : L - ll);
}

// first pixel x of column c (of C) on a level W pixels wide: the pixels whose centre (x + 0.5) / W lies in
// [c / C, (c + 1) / C); every pixel belongs to exactly one column, col_lo(C) == W
__device__ __forceinline__ int col_lo(const int c, const int W, const int C) { return (2 * c * W + C - 1) / (2 * C); }
// the widest column: col_lo(c) = floor(c * s + d) with s = W / C and d = (C - 1) / (2 C) < 1/2, so consecutive columns
// differ by floor(s) or floor(s) + 1, and as the C widths add up to W the larger one occurs whenever s is not an integer:
// max_c (col_lo(c + 1) - col_lo(c)) = ceil(W / C).  (The kernels used to walk all columns of all levels with two integer
// divisions each, in every workgroup, several times over: tens of microseconds before the first item of a launch.)
__device__ __forceinline__ int col_max_cell(const int W, const int C) { return (W + C - 1) / C; }

// a wave-uniform float, pinned to a scalar register: gfx950 has no scalar float unit, so a uniform float expression is
// evaluated on the vector unit and -- hoisted out of the item loop -- would otherwise occupy a vector register for the
// whole kernel (dozens of them here: per-level sizes, reciprocals, clamps)
__device__ __forceinline__ float uni(const float v)
{
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

__device__ __forceinline__ double uni_d(const double v)
{
  // (explicit v_readfirstlane: the builtin is folded away on a value the compiler already knows to be uniform, and the
  // vector copy then stays alive across the item loop -- five of these were spilled)
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned ul = (unsigned)u, uh = (unsigned)(u >> 32);
  unsigned lo, hi;
  asm volatile("v_readfirstlane_b32 %0, %2\n\tv_readfirstlane_b32 %1, %3" : "=s"(lo), "=s"(hi) : "v"(ul), "v"(uh));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// a uniform (x, y) pair in an aligned scalar register pair: a packed FMA takes it as an operand directly (built in vector
// registers instead, the per-level constant pairs were hoisted out of the item loop and spilled)
__device__ __forceinline__ col_f32x2 uni_pair(const float a, const float b)
{
  const unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
  unsigned lo, hi;
  asm volatile("v_readfirstlane_b32 %0, %2\n\tv_readfirstlane_b32 %1, %3" : "=s"(lo), "=s"(hi) : "v"(ua), "v"(ub));
  return __builtin_bit_cast(col_f32x2, ((unsigned long long)hi << 32) | lo);
}

// floor(n / d) for uniform 0 <= n < 2^31 given inv = 1.0 / d: (n + 0.5) / d is at least 0.5 / d away from an integer and
// the double product is off by less than 2^-20 of that margin.  An integer division by a run-time divisor costs ~35
// dependent instructions here (no hardware divide); the item decode had twenty of them per item.
__device__ __forceinline__ int udiv_by(const int n, const double inv)
{
  return __builtin_amdgcn_readfirstlane((int)(((double)n + 0.5) * inv));
}

// floor(n / d) for uniform 0 <= n < 2^31, 1 <= d < 2^31, entirely on the scalar unit (s_mul_hi_u32): with
// m = floor((2^32 - 1) / d) the estimate q' = floor(n * m / 2^32) falls short of n / d by less than n / 2^32 < 1/2, so it
// is the quotient or one below it, and one comparison of the remainder settles which.  (The double-precision form
// above costs four vector instructions and a readfirstlane; an item decode holds some twenty divisions.)
struct UDiv {
  unsigned d, m;
};
__device__ __forceinline__ UDiv make_udiv(const int d)
{
  const unsigned du = (unsigned)__builtin_amdgcn_readfirstlane(d);
  return UDiv{du, (unsigned)__builtin_amdgcn_readfirstlane((int)(0xFFFFFFFFu / du))};
}
__device__ __forceinline__ int udiv_s(const int n, const UDiv u)
{
  const unsigned q = __umulhi((unsigned)n, u.m);
  const unsigned r = (unsigned)n - q * u.d;
  return (int)(q + (r >= u.d ? 1u : 0u));
}

// floor to int in one instruction (the compiler emits v_floor_f32 + v_cvt_i32_f32)
__device__ __forceinline__ int cvt_flr(const float x)
{
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// A wave's bounding box in ONE reduction.  lo = packed (u16, u16) low corner, hi = packed high corner: the maximum is
// taken as the minimum of complements, and after a half-wave swap lanes 0-31 reduce the low corners of all 64 lanes
// while lanes 32-63 reduce the complemented high corners.  Returns, in lane 31, min(lo) and, in lane 63, ~max(hi)
// (other lanes: partial results).  12 vector instructions against 30 for two separate reductions.
__device__ __forceinline__ unsigned wave_reduce_box(const unsigned lo, const unsigned hi)
{
  const auto s = __builtin_amdgcn_permlane32_swap(lo, ~hi, false, false);
  unsigned v = pk_min(s[0], s[1]);
  v = pk_min(v, dpp_u<0xB1>(v));    // quad_perm [1,0,3,2]
  v = pk_min(v, dpp_u<0x4E>(v));    // quad_perm [2,3,0,1]
  v = pk_min(v, dpp_u<0x141>(v));   // row_half_mirror
  v = pk_min(v, dpp_u<0x140>(v));   // row_mirror
  v = pk_min(v, dpp_u<0x142>(v));   // row_bcast:15 -- rows 1 and 3 take in lane 15 of rows 0 and 2
  return v;
}

// The workgroup's box from the NW per-wave records {min lo, ~max hi} (8 bytes each, contiguous, 16-byte aligned): every
// lane reads all of them (LDS broadcast) and reduces in registers; the result is uniform.
template <int NW>
__device__ __forceinline__ void block_box(const unsigned *rec, unsigned &lo, unsigned &hi)
{
  unsigned a = 0xFFFFFFFFu, b = 0xFFFFFFFFu;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    a = pk_min(a, rec[2 * w]);
    b = pk_min(b, rec[2 * w + 1]);
  }
  lo = (unsigned)__builtin_amdgcn_readfirstlane((int)a);
  hi = ~(unsigned)__builtin_amdgcn_readfirstlane((int)b);
}

// ---- the launch-level structure of a column kernel: grid, slots, tables, items, queue ----------------------------------
// Stated once for the three kernels.  They differ in two figures: the queries a work item holds (QPI: the workgroup's
// threads, or half of them where two lanes share a (query, head) pair) and a lane's rank among them (its thread index, or
// half of it).  Everything uniform travels BY VALUE in small structs: a kernel-local array handed over by reference stays
// in scratch memory and its elements stop being wave-uniform -- dozens of spilled registers in every instantiation.

template <int L>
struct ColLevels {                                                             // the pyramid: sizes and first query of every level
  int H[L], W[L], St[L];
};

// The column grid (every workgroup derives the same one): CX x CY cells such that no column holds more than QPI queries,
// cells about square on the finest level with a width near a multiple of 8 lanes.
struct ColGrid {
  int CX, CY;
};
template <int L, int QPI>
__device__ __forceinline__ ColGrid col_grid(const ColLevels<L> lv, const int S)
{
  int Hf = lv.H[0], Wf = lv.W[0];
#pragma unroll
  for (int l = 1; l < L; ++l)
    if (lv.H[l] * lv.W[l] > Hf * Wf) { Hf = lv.H[l]; Wf = lv.W[l]; }
  const float area = (float)QPI * (float)(Hf * Wf) / (float)S;               // finest-level pixels per full column
  const int side = (int)sqrtf(area);
  const int nxt = min(Wf, max(8, (side + 4) & ~7));
  int CX = (Wf + nxt - 1) / nxt;
  const int nx0 = (Wf + CX - 1) / CX;
  const int nyt = max(1, (int)(area / (float)nx0));
  int CY = min(Hf, (Hf + nyt - 1) / nyt);
  for (int guard = 0; guard < 4096; ++guard) {
    int maxq = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) maxq += col_max_cell(lv.W[l], CX) * col_max_cell(lv.H[l], CY);
    if (maxq <= QPI) break;
    if (CY < Hf) ++CY;
    else if (CX < Wf) ++CX;
    else break;                                                                // (L pixels per column: cannot exceed QPI)
  }
  return ColGrid{CX, CY};
}

// A lane's SLOT in a column (fixed for the whole launch).  A column's queries are dealt to the ranks level by level,
// finest (last) first, each level taking a block of mx * my ranks where mx x my is its LARGEST cell over the grid -- the
// grid search made these blocks fit the item -- so a lane's (level, x, y inside the cell) never changes from item to item
// and the per-item decode is two table look-ups and a multiply-add (it used to walk the levels: ~100 vector and ~250
// scalar instructions per item).  A lane whose slot lies outside a smaller border cell idles for that item.
struct ColSlot {
  int c0;                                                                      // level start + (y * W + x) inside the cell
  unsigned slot;                                                               // x | y << 10 | level << 20; x = y = 1023: no slot
};
template <int L>
__device__ __forceinline__ ColSlot col_lane_slot(const ColLevels<L> lv, const ColGrid g, const int rank)
{
  ColSlot s{0, 0x000FFFFFu};
  int r = rank;
  bool placed = false;
#pragma unroll
  for (int ll = 0; ll < L; ++ll) {
    const int l = L - 1 - ll;
    const int mx = col_max_cell(lv.W[l], g.CX), my = col_max_cell(lv.H[l], g.CY);
    const int cnt = mx * my;                                                   // (<= QPI <= 1024: x, y fit 10 bits)
    if (!placed && r < cnt) {
      const int ly = r / max(mx, 1), lx = r - ly * max(mx, 1);
      s.slot = (unsigned)lx | ((unsigned)ly << 10) | ((unsigned)l << 20);
      s.c0 = lv.St[l] + ly * lv.W[l] + lx;
      placed = true;
    }
    r -= placed ? 0 : cnt;
  }
  return s;
}

// The cell tables in LDS: xtab[l][cx] = first x | width << 16, ytab[l][cy] likewise, then the level widths.  A kernel whose
// LDS cannot hold them (absurdly elongated maps: thousands of columns along one axis) does not use the grid at all: the
// launch then runs on FLAT columns, see col_decode.
template <int L>
__device__ __forceinline__ int col_table_bytes(const ColGrid g)
{
  return (L * (g.CX + g.CY) + L) * 4;
}
template <int L, int BLOCK>
__device__ __forceinline__ void col_fill_tables(unsigned *tab, const ColLevels<L> lv, const ColGrid g, const int tid)
{
  const int CX = g.CX, CY = g.CY;
  // (the levels are indexed per lane here: from arrays of their own, which the compiler turns into selects -- indexed
  // inside the struct, the whole struct would live in scratch memory)
  int H[L], W[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    H[l] = lv.H[l];
    W[l] = lv.W[l];
  }
  for (int t = tid; t < L * CX; t += BLOCK) {
    const int l = t / CX, c = t - l * CX;
    const int a = col_lo(c, W[l], CX);
    tab[t] = (unsigned)a | ((unsigned)(col_lo(c + 1, W[l], CX) - a) << 16);
  }
  for (int t = tid; t < L * CY; t += BLOCK) {
    const int l = t / CY, c = t - l * CY;
    const int a = col_lo(c, H[l], CY);
    tab[L * CX + t] = (unsigned)a | ((unsigned)(col_lo(c + 1, H[l], CY) - a) << 16);
  }
  if (tid < L) tab[L * (CX + CY) + tid] = (unsigned)W[tid];
  __syncthreads();
}

// The launch's work items: (image, column, head), with flat columns -- QPI consecutive queries of one level -- when there
// are no tables.  big_map: a level too large for the 16-bit box corners (every level is then gathered from global memory).
struct ColItems {
  int M, ncol, items;
  bool use_tab, big_map;
  UDiv dv_ncolM, dv_2ncol, dv_CX;
};
template <int L, int QPI>
__device__ __forceinline__ ColItems col_items(const ColLevels<L> lv, const ColGrid g, const bool use_tab, const int N, const int M)
{
  bool big_map = false;
#pragma unroll
  for (int l = 0; l < L; ++l) big_map = big_map || lv.W[l] > 65531 || lv.H[l] > 65531;
  int ncol = g.CX * g.CY;
  if (!use_tab) {
    ncol = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) ncol += (lv.H[l] * lv.W[l] + QPI - 1) / QPI;
  }
  return ColItems{M, ncol, N * ncol * M, use_tab, big_map, make_udiv(ncol * M), make_udiv(2 * ncol), make_udiv(g.CX)};
}

// item -> (image, head) [uniform] and this lane's query (qv = q, or ~q of the query an idle lane shadows).
// Item order inside an image: head PAIR outermost, then column, then the head inside the pair.  The two heads of a pair
// share every 128-byte line of the value tensor (64 B each) and run in adjacent workgroups; the columns of one pair follow
// each other, so an XCD works through one head pair's value maps (2.8 MB of lines at the north-star shape, inside its 4 MB
// L2) with all the neighbouring columns -- whose windows overlap -- in flight together.  (With the 8 heads of a column
// adjacent instead, an XCD held 12 columns x 8 heads of windows at once, more than its L2: measured 1.41x / 1.92x the
// algorithmic bytes on the memory side for distributions I / M.)
struct ColItem {
  int b, m, qv;
};
template <int L, int QPI>
__device__ __forceinline__ ColItem col_decode(const int it, const ColItems ci, const ColGrid g, const ColLevels<L> lv,
                                              const unsigned *tab, const ColSlot s, const int rank)
{
  const int CX = g.CX, CY = g.CY, ncol = ci.ncol, M = ci.M;
  ColItem r;
  r.b = udiv_s(it, ci.dv_ncolM);
  const int r_img = it - r.b * (ncol * M);
  int col;
  if (r_img < 2 * ncol * (M >> 1)) {
    const int pr = udiv_s(r_img, ci.dv_2ncol);
    const int rr = r_img - pr * 2 * ncol;
    col = rr >> 1;
    r.m = 2 * pr + (rr & 1);
  } else {                                                                     // odd head count: the last head alone
    col = r_img - 2 * ncol * (M >> 1);
    r.m = M - 1;
  }
  const int cy = udiv_s(col, ci.dv_CX), cx = col - cy * CX;
  int q;
  bool valid;
  if (ci.use_tab) {
    const unsigned lx = s.slot & 0x3FFu, ly = (s.slot >> 10) & 0x3FFu, lv_ = s.slot >> 20;
    const unsigned char *tb = reinterpret_cast<const unsigned char *>(tab);
    const unsigned xt = *reinterpret_cast<const unsigned *>(tb + (__umul24(lv_, (unsigned)(CX * 4)) + (unsigned)(cx * 4)));
    const unsigned yt = *reinterpret_cast<const unsigned *>(tb + (__umul24(lv_, (unsigned)(CY * 4)) + (unsigned)((L * CX + cy) * 4)));
    const unsigned lw = *reinterpret_cast<const unsigned *>(tb + (lv_ * 4u + (unsigned)(L * (CX + CY) * 4)));
    valid = lx < (xt >> 16) && ly < (yt >> 16);
    q = s.c0 + (int)__umul24(yt & 0xFFFFu, lw) + (int)(xt & 0xFFFFu);
  } else {
    // flat columns: QPI consecutive queries of one level (no tables, no divisions; the boxes of such a strip are wide, so
    // its levels mostly take the global-memory path -- correct, not fast)
    int c = col;
    q = 0;
    valid = false;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const int cnt = lv.H[l] * lv.W[l], nch = (cnt + QPI - 1) / QPI;
      if (c >= 0 && c < nch) {
        q = lv.St[l] + c * QPI + rank;
        valid = c * QPI + rank < cnt;
      }
      c = c >= nch ? c - nch : -1;
    }
  }
  // idle lanes shadow a query of the column (they cannot move its boxes): the wave's first busy lane's; a wave without
  // any busy lane shadows query 0 (correct, merely wide boxes; it takes a pyramid whose levels shrink the wrong way)
  const unsigned long long vm = __ballot(valid);
  const int q_sh = vm ? __builtin_amdgcn_readlane(q, (int)__builtin_ctzll(vm)) : 0;
  r.qv = valid ? q : ~q_sh;
  return r;
}

// The persistent grid's walk over the items, chunked by XCD: workgroup slot `slot0` of the XCD's `nslots` starts on item
// xcd * chunk + slot0 of its XCD's n_x items [xcd * chunk, item_end).
struct ColChunk {
  int xcd, slot0, nslots, chunk, item_end;
  unsigned n_x;
};
__device__ __forceinline__ ColChunk col_chunk(const int items)
{
  ColChunk c;
  c.xcd = blockIdx.x & 7;
  c.slot0 = blockIdx.x >> 3;
  c.nslots = gridDim.x >> 3;
  c.chunk = (items + 7) / 8;
  c.item_end = min((c.xcd + 1) * c.chunk, items);
  c.n_x = (unsigned)max(c.item_end - c.xcd * c.chunk, 0);                      // items of this XCD
  return c;
}
// the item the workgroup takes next, from the index thread 0 published in next_idx[0] (behind a barrier)
__device__ __forceinline__ int col_next_item(const unsigned *next_idx, const ColChunk c)
{
  const unsigned nxt = __builtin_amdgcn_readfirstlane(next_idx[0]);
  return nxt < c.n_x ? c.xcd * c.chunk + (int)nxt : c.item_end;               // never out of the chunk
}

// Queue protocol of the forward kernels: as in msda_win_common.hpp (first item static, every further one nslots + the XCD's
// counter, the fetch that returns n_x - 1 resets the counter), run TWO items ahead: the index of item i + 1 is published
// before the boxes' barrier of item i, so right behind that barrier every lane knows its next query and issues the next
// item's sampling-location loads.  A fetch is made only while the next item is valid, so fetches == items processed still
// holds.  (thread 0) the counter value fetched last lives in LDS word next_idx[1], not in a register: a register alive
// across the whole item was spilled by the compiler, and spilling an atomic's result means waiting for it on the spot.
__device__ __forceinline__ void col_queue_first_fetch(unsigned *queue, unsigned *next_idx, const ColChunk c, const int tid)
{
  if (queue && tid == 0) next_idx[1] = atomicAdd(queue + c.xcd * WIN_QUEUE_STRIDE, 1u);
}
// publish the next item's index, fetch the one after it; the fetched value is parked by col_queue_park once the kernel
// waits for its memory counter anyway
struct ColFetch {
  unsigned f_new;
  bool fetched;
};
__device__ __forceinline__ ColFetch col_queue_publish(unsigned *queue, unsigned *next_idx, const ColChunk c, const int item,
                                                      const int tid)
{
  ColFetch f{0u, false};
  if (tid == 0) {
    unsigned nxt = (unsigned)(item - c.xcd * c.chunk + c.nslots);             // static stride when there is no queue
    if (queue) {
      const unsigned f_next = next_idx[1];
      if (f_next + 1u >= c.n_x)                                               // that was the launch's last fetch
        __hip_atomic_store(queue + c.xcd * WIN_QUEUE_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      nxt = (unsigned)c.nslots + f_next;
      if (nxt < c.n_x) {
        // (inline asm: the compiler waits for a returning atomic at the end of this divergent block -- a full round trip
        // to L2 in front of the pre-pass; the wait now sits where the value is parked, behind the pre-pass)
        const unsigned one = 1u, zero = 0u;
        const unsigned *qp = queue + c.xcd * WIN_QUEUE_STRIDE;
        // (s_nop: the base may just have been restored by v_readlane; a vector-memory instruction reading a scalar
        // register a vector instruction wrote needs 5 wait states, and the hazard recogniser does not see into inline asm)
        asm volatile("s_nop 4\n\tglobal_atomic_add %0, %1, %2, %3 sc0"
                     : "=v"(f.f_new) : "v"(zero), "v"(one), "s"(qp) : "memory");
        f.fetched = true;
      }
    }
    next_idx[0] = nxt;
  }
  return f;
}
__device__ __forceinline__ void col_queue_park(unsigned *next_idx, ColFetch f)
{
  if (f.fetched) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(f.f_new)::"memory");
    next_idx[1] = f.f_new;
  }
}

// ---- quad-cooperative record access ------------------------------------------------------------------------------------
// A lane's records (128 B of sampling locations, 64 B of weights, 64 B of output per (query, head)) are 512 B - 1 KB apart
// from its neighbours': loaded lane by lane, every 16-byte access of a wave instruction touches a different 128-byte line
// and the texture-addresser serialises them (64 tag look-ups per instruction; measured: 16 K of the 77 K cycles an
// item took, and everything behind it in the queue waits).  So the 4 lanes of a quad fetch 64 CONSECUTIVE bytes of ONE
// record per instruction (16 look-ups), taking the quad's four records in turn, and the 4 x 4 block of 16-byte pieces is
// transposed in registers: instruction s gives lane i piece (s - i) % 4 of record s; the lane rotates its four registers
// by its own index (two layers of v_cndmask) and a quad_perm rotation by k delivers piece k of its own record.
template <int K>
__device__ __forceinline__ col_f32x4 quad_rot(const col_f32x4 v)      // lane c receives lane (c - K) % 4's value
{
  constexpr int ctrl = ((0 - K) & 3) | (((1 - K) & 3) << 2) | (((2 - K) & 3) << 4) | (((3 - K) & 3) << 6);
  if constexpr (K == 0) return v;
  return col_f32x4{dpp_f<ctrl>(v[0]), dpp_f<ctrl>(v[1]), dpp_f<ctrl>(v[2]), dpp_f<ctrl>(v[3])};
}
// x[k] <- x[(a + k) % 4] with the per-lane amount a = a0 + 2 * a1
__device__ __forceinline__ void rot_regs(col_f32x4 (&x)[4], const bool a0, const bool a1)
{
  col_f32x4 t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) t[k][e] = a0 ? x[(k + 1) & 3][e] : x[k][e];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) x[k][e] = a1 ? t[(k + 2) & 3][e] : t[k][e];
}
// in: x[s] = what this lane loaded for record s of its quad (piece (s - i) % 4); out: x[k] = piece k of its own record
__device__ __forceinline__ void quad_transpose_in(col_f32x4 (&x)[4], const bool i0, const bool i1)
{
  rot_regs(x, i0, i1);
  x[1] = quad_rot<1>(x[1]);
  x[2] = quad_rot<2>(x[2]);
  x[3] = quad_rot<3>(x[3]);
}
// The fetch goes through per-image buffer descriptors: a scalar base, one 32-bit vector offset per record and the piece as
// an immediate -- no 64-bit vector address arithmetic.  A lane forms the byte offset of ITS OWN record once; the quad's
// other three get it by DPP (record s of the quad belongs to lane 4 * (lane / 4) + s).  Offsets past the end of a
// descriptor read zeros / drop the store: an idle lane's record is simply moved out of range for the store.
// (launchers: S < 2^24, per-image tensors below 2 GiB)
__device__ __forceinline__ unsigned col_rec_index(const int qv, const int m, const int M)   // query * M + head of the lane's own record
{
  return __umul24((unsigned)(qv ^ (qv >> 31)), (unsigned)M) + (unsigned)m;
}
struct ColQuadOff {
  unsigned o[4];                                                               // record s of the quad + the piece this lane fetches of it
};
__device__ __forceinline__ ColQuadOff col_quad_offsets(const unsigned own_bytes, const int qi)
{
  ColQuadOff q;
  q.o[0] = dpp_u<0x00>(own_bytes) + ((unsigned)((0 - qi) & 3) << 4);
  q.o[1] = dpp_u<0x55>(own_bytes) + ((unsigned)((1 - qi) & 3) << 4);
  q.o[2] = dpp_u<0xAA>(own_bytes) + ((unsigned)((2 - qi) & 3) << 4);
  q.o[3] = dpp_u<0xFF>(own_bytes) + ((unsigned)((3 - qi) & 3) << 4);
  return q;
}
// the records of the quad's four (query, head) pairs, all NG groups (64 bytes each) at once: the two halves of a 128-byte
// line are requested back to back (a partial last group reads into the next record: never looked at)
template <int NG>
__device__ __forceinline__ void col_quad_load(const __amdgpu_buffer_rsrc_t rs, const unsigned own_bytes, const int qi,
                                              col_f32x4 (&raw)[NG][4])
{
  const ColQuadOff q = col_quad_offsets(own_bytes, qi);
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
    for (int g = 0; g < NG; ++g)
      raw[g][s4] = __builtin_bit_cast(col_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(q.o[s4] + g * 64), 0, 0));
}

}  // namespace pct
