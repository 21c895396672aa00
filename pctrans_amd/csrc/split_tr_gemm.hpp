// What the split-bf16 GEMMs with 16-channel steps share beyond split_bf16.hpp (conv1x1_split.hip, fpn_stage.hip): the stream
// of per-step weight images through registers into LDS, and the pipelined step loop of the kernels whose B operand lies
// k-major in LDS and is read through ds_read_b64_tr_b16.  The LDS layouts of the weight image stay with the kernels.
#pragma once
#include "attn_common.hpp"    // lds_read_tr16_b64; split_bf16.hpp

namespace pct {

// A step's weight image [3 planes][128 rows][16 k] bf16 = 3 x BLOCK chunks of 16 bytes: thread tid carries chunk tid of every
// plane from memory (images STEP bf16 apart) to byte `loff` of the plane in LDS (planes LDS_PLANE bytes apart).
template <int LDS_PLANE, int STEP, int BLOCK = 256>
struct WeightStepStream {
  i32x4 g[3];
  int loff;
  __device__ __forceinline__ void fetch(const unsigned short *img, const int step, const int tid)
  {
    const i32x4 *p = reinterpret_cast<const i32x4 *>(img + (size_t)step * STEP) + tid;
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = p[i * BLOCK];
  }
  __device__ __forceinline__ void stash(unsigned char *buf) const
  {
#pragma unroll
    for (int i = 0; i < 3; ++i) *reinterpret_cast<i32x4 *>(buf + i * LDS_PLANE + loff) = g[i];
  }
};

// -> sum over nsteps steps of W(step) . x(step) for a wave's 64 channels x 64 pixels (from pixel px0 of the 128 staged ones).
// xs, wsm: two buffers each of three planes, x as [16 k][XROW bytes: 128 pixels bf16 + pad], W with planes WPLANE bytes
// apart and the lane's fragment of row block rb at a_off[rb].  fetch(step) loads a step's x and W into registers, stash(buf)
// splits / writes them into buffer `buf`: the operands of step s + 1 are fetched while step s is multiplied, one barrier per step.
template <int XROW, int WPLANE, typename Fetch, typename Stash>
__device__ __forceinline__ SplitTile2x2 split_tr_gemm(const unsigned char *xs, const unsigned char *wsm, const int (&a_off)[2],
                                                      const int lane, const int px0, const int nsteps, const Fetch &fetch,
                                                      const Stash &stash)
{
  constexpr int XPLANE = 16 * XROW;
  // B operand through the transposing read: 16-lane group g16 = lane / 16 covers pixels 16 (g16 % 2) .. + 15 and k = 8 (g16 / 2) ..;
  // lane 4 q + pp of the group supplies row q (+ 4 for the second read), columns 4 pp .. 4 pp + 3
  const int g16 = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3;
  int b_off[2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) b_off[cb] = (8 * (g16 >> 1) + q4) * XROW + (px0 + cb * 32 + 16 * (g16 & 1) + 4 * pp) * 2;

  SplitTile2x2 acc;
  acc.zero();
  fetch(0);
  stash(0);
  __syncthreads();
  for (int step = 0; step < nsteps; ++step) {
    const int buf = step & 1;
    if (step + 1 < nsteps) fetch(step + 1);
    __builtin_amdgcn_sched_barrier(0);                            // the fetches ahead of the MFMAs
    const unsigned char *xbuf = xs + buf * 3 * XPLANE, *wbuf = wsm + buf * 3 * WPLANE;
    bf16x8 wa[2][3], xb[2][3];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) wa[rb][pl] = *reinterpret_cast<const bf16x8 *>(wbuf + pl * WPLANE + a_off[rb]);
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const unsigned char *p = xbuf + pl * XPLANE + b_off[cb];
        const bf16x4 lo = lds_read_tr16_b64(p), hi = lds_read_tr16_b64(p + 4 * XROW);
        xb[cb][pl] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
    }
    acc.mac(wa, xb);
    if (step + 1 < nsteps) stash(buf ^ 1);                       // (everyone left that buffer before the previous barrier)
    __syncthreads();
  }
  return acc;
}

}  // namespace pct
