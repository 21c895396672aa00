// Micro-benchmark (diagnostic, not part of the library): how long a wave's fresh non-temporal stores stay counted in vmcnt
// while every CU streams stores, i.e. what an `s_waitcnt vmcnt(0)` (or a counted wait for a load issued behind the stores)
// costs right after them.  512 workgroups of 4 waves (2 per CU, the occupancy of dmh_fused_kernel and
// linear_k128_split_kernel); per iteration a wave writes 4 x dwordx4 per lane = 4 KB of new lines, then either
//   drain:   stamps s_memtime, waits vmcnt(0), stamps again           -> cycles from the last store's issue to the last ack
//   no wait: goes on
// and idles `pad` x 64 cycles (s_sleep) as the stand-in for the kernel's work between two bursts of stores.
// The host prints the mean drain in shader cycles and the wall time of both forms.
//   hipcc -O3 --offload-arch=gfx950 tools/micro/store_ack.hip -o tools/micro/store_ack && tools/micro/store_ack
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int WGS = 512, WAVES = 4, ITERS = 200;
constexpr size_t PER_WAVE = (size_t)ITERS * 256;             // u32x4 elements: 64 lanes x 4 stores per iteration

template <bool DRAIN>
__global__ __launch_bounds__(256, 2) void ack_kernel(u32x4 *out, const int pad, unsigned long long *cyc)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4 *p = out + ((size_t)blockIdx.x * WAVES + wave) * PER_WAVE + lane;     // < WGS * WAVES * PER_WAVE: the allocation
  const u32x4 v = {(unsigned)lane, (unsigned)wave, blockIdx.x, 7u};
  unsigned long long sum = 0;
  for (int it = 0; it < ITERS; ++it, p += 256) {
#pragma unroll
    for (int k = 0; k < 4; ++k) __builtin_nontemporal_store(v, p + 64 * k);
    if constexpr (DRAIN) {
      unsigned long long t0, t1;
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
      sum += t1 - t0;
    }
    for (int s = 0; s < pad; ++s) __builtin_amdgcn_s_sleep(1);               // 64 cycles each
  }
  if (lane == 0) cyc[blockIdx.x * WAVES + wave] = sum;
}

int main()
{
  u32x4 *out;
  unsigned long long *cyc;
  const size_t n = (size_t)WGS * WAVES * PER_WAVE;
  if (hipMalloc(&out, n * sizeof(u32x4)) != hipSuccess || hipMalloc(&cyc, WGS * WAVES * 8) != hipSuccess) return 1;
  std::vector<unsigned long long> h(WGS * WAVES);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  for (int pad : {0, 16, 48, 96}) {
    float ms[2] = {0.f, 0.f};
    double drain = 0;
    for (int form = 0; form < 2; ++form)
      for (int rep = 0; rep < 3; ++rep) {                      // the last repetition counts
        hipEventRecord(e0);
        if (form == 0) hipLaunchKernelGGL(ack_kernel<true>, dim3(WGS), dim3(256), 0, 0, out, pad, cyc);
        else hipLaunchKernelGGL(ack_kernel<false>, dim3(WGS), dim3(256), 0, 0, out, pad, cyc);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms[form], e0, e1);
        if (form == 0) {
          hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost);
          drain = 0;
          for (auto c : h) drain += (double)c;
          drain /= (double)h.size() * ITERS;
        }
      }
    printf("pad %4d cycles between bursts: drain after 4 nt stores %7.0f cycles (mean);  kernel %.3f ms with the drain, %.3f ms "
           "without  (%.0f GB/s with, %.0f without)\n",
           pad * 64, drain, ms[0], ms[1], n * 16 / ms[0] / 1e6, n * 16 / ms[1] / 1e6);
  }
  if (hipGetLastError() != hipSuccess) { printf("HIP error\n"); return 1; }
  return 0;
}
