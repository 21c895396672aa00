// MSDeformAttn routing: which kernel a call runs on.  Host code only -- the kernels and their own launchers are in
// msda_forward*.hip and msda_backward*.hip; a specialised launcher returns PCT_NOT_COVERED for a call it does not cover and
// the route goes on to the next one.
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "msda_common.hpp"
#include "launchers.hpp"

namespace pct {

// ---- kernel choice (diagnostics and development A/B; see include/pctrans_hip.h), one for the forward and one for the
// backward: the override of pct_msda_set_*kernel_choice, else the environment variable (read once, at the first call); and
// what the last call launched ------------------------------------------------------------------------------------------------------
struct KernelChoice {
  int (*read_env)();                                 // the environment variable's kernel id
  int max_id;
  std::atomic<int> override_id{-1};                  // -1: follow the environment
  std::atomic<int> last{0};
  std::once_flag env_once;
  int env_id = 0;

  void set(int v) { override_id.store((v >= 0 && v <= max_id) ? v : -1, std::memory_order_relaxed); }
  int get()
  {
    const int ov = override_id.load(std::memory_order_relaxed);
    if (ov >= 0) return ov;
    std::call_once(env_once, [this] { env_id = read_env(); });
    return env_id;
  }
  void note(int k) { last.store(k, std::memory_order_relaxed); }
};

// PCT_MSDA_KERNEL = auto | win | dpp | generic | col (development A/B), told apart by the first letter
static KernelChoice g_fwd{[] {
                            const char *e = getenv("PCT_MSDA_KERNEL");
                            if (!e) return (int)MSDA_FWD_AUTO;
                            if (e[0] == 'w') return (int)MSDA_FWD_WIN;
                            if (e[0] == 'd') return (int)MSDA_FWD_QUAD;
                            if (e[0] == 'g') return (int)MSDA_FWD_GENERIC;
                            if (e[0] == 'c') return (int)MSDA_FWD_COL;
                            return (int)MSDA_FWD_AUTO;
                          },
                          MSDA_FWD_COL};
// PCT_MSDA_BWD_KERNEL = auto | col | win | generic, spelled out
static KernelChoice g_bwd{[] {
                            const char *e = getenv("PCT_MSDA_BWD_KERNEL");
                            if (!e) return (int)MSDA_BWD_AUTO;
                            if (!strcmp(e, "win")) return (int)MSDA_BWD_WIN;
                            if (!strcmp(e, "generic")) return (int)MSDA_BWD_GENERIC;
                            if (!strcmp(e, "col")) return (int)MSDA_BWD_COL;
                            return (int)MSDA_BWD_AUTO;
                          },
                          MSDA_BWD_COL};

void set_msda_kernel_choice(int v) { g_fwd.set(v); }
int msda_last_kernel() { return g_fwd.last.load(std::memory_order_relaxed); }
void set_msda_bwd_kernel_choice(int c) { g_bwd.set(c); }
int msda_bwd_last_kernel() { return g_bwd.last.load(std::memory_order_relaxed); }

// ---- forward ------------------------------------------------------------------------------------------------------------
// Kernel choice for PCTrans' geometry.  Default "auto": the windowed-LDS kernel when the queries are the pyramid's
// own pixels (Lq == S: neighbouring queries sample neighbouring texels, the case it is built for) and the problem fills
// its persistent grid (except where it was measured slower, see below), else the quad-owner kernel.
//
// shared by the plain and the fused entry points: PCT_NOT_COVERED = geometry not covered by the specialised kernels
template <typename T>
int launch_msda_forward_special(const MsdaFwdCall &c)
{
  const int N = c.N, S = c.S, M = c.M, L = c.L, Lq = c.Lq, P = c.P;
  const int choice = g_fwd.get();
  if (choice == MSDA_FWD_GENERIC) return PCT_NOT_COVERED;
  int rc = PCT_NOT_COVERED;
  // 16-bit values with 8 points per level (SURVEY config 5): the windowed variant (2 lanes per head-pixel, 4 points per
  // lane and level, 20-40 spilled VGPRs) loses to the quad-owner kernel (P3, N = 1: 0.49 vs 0.34 ms) -- measured, so
  // "auto" skips it there; fp32 with 8 points and 16-bit with 4 points stay on the windowed kernel (faster)
  const bool win_loses = sizeof(typename Traits<T>::store_t) == 2 && P == 8;
  // ... and a persistent grid of 768 workgroups needs about three work items each to beat the quad-owner kernel
  // (P2: N = 1 0.046 vs 0.040 ms, N = 2 equal, N = 4 0.089 vs 0.113 ms; P4, N = 1: 0.024 vs 0.014 ms)
  const long long per_item = P == 8 ? 128 : (sizeof(typename Traits<T>::store_t) == 2 ? 512 : 256);   // queries per item
  const bool win_small = (long long)N * ((Lq + per_item - 1) / per_item) * M < 3 * 768;
  // the pyramid-column kernel (fp32, 4 points): persistent grid of 768 workgroups with items of <= 256 queries.  Measured
  // crossover against the windowed / quad-owner kernels (model-like locations, profiles/r02_small_batch.txt): with 4
  // levels it wins from one 512^2 image on (N * S * M = 174 k); with 3 levels from about 450 k (quad-owner before that)
  if constexpr (sizeof(typename Traits<T>::store_t) == 4) {
    const bool col_big = (long long)N * S * M >= (L >= 4 ? 160000LL : 450000LL);
    if (choice == MSDA_FWD_COL || (choice == MSDA_FWD_AUTO && Lq == S && P == 4 && col_big)) {
      rc = launch_msda_forward_col(c, false);
      if (rc != PCT_NOT_COVERED) g_fwd.note(MSDA_FWD_COL);
    }
  }
  if constexpr (sizeof(typename Traits<T>::store_t) == 2) {
    // 16-bit values: the column kernel's 16-bit variant (4 or 8 points; two lanes per (query, head) with 8 points)
    const bool col_big = (long long)N * S * M * (P / 4) >= (L >= 4 ? 160000LL : 450000LL);
    if (choice == MSDA_FWD_COL || (choice == MSDA_FWD_AUTO && Lq == S && (P == 4 || P == 8) && col_big)) {
      rc = launch_msda_forward_col16<T>(c);
      if (rc != PCT_NOT_COVERED) g_fwd.note(MSDA_FWD_COL);
    }
  }
  if (rc == PCT_NOT_COVERED && (choice == MSDA_FWD_WIN || (choice == MSDA_FWD_AUTO && Lq == S && !win_loses && !win_small))) {
    rc = launch_msda_forward_win<T>(c);
    if (rc != PCT_NOT_COVERED) g_fwd.note(MSDA_FWD_WIN);
  }
  if (rc == PCT_NOT_COVERED) {
    rc = launch_msda_forward_dpp<T>(c);
    if (rc != PCT_NOT_COVERED) g_fwd.note(MSDA_FWD_QUAD);
  }
  return rc;
}
// piece-plane operands (pct_ms_deform_attn_forward_planes_f32): the pyramid-column kernel or nothing (PCT_NOT_COVERED)
int launch_msda_forward_planes(const MsdaFwdCall &c)
{
  const int rc = launch_msda_forward_col(c, true);
  if (rc != PCT_NOT_COVERED) g_fwd.note(MSDA_FWD_COL);
  return rc;
}

// the plain entry points: a specialised kernel (sampling locations and weights in fp32), else the generic one
template <typename T>
int launch_msda_forward(const MsdaFwdCall &c)
{
  if constexpr (sizeof(typename Traits<T>::acc_t) == 4) {
    const int rc = launch_msda_forward_special<T>(c);
    if (rc != PCT_NOT_COVERED) return rc;
  }
  g_fwd.note(MSDA_FWD_GENERIC);
  return launch_msda_forward_generic<T>(c);
}

template int launch_msda_forward_special<float>(const MsdaFwdCall &);
template int launch_msda_forward<float>(const MsdaFwdCall &);
template int launch_msda_forward<double>(const MsdaFwdCall &);
template int launch_msda_forward<half_bits>(const MsdaFwdCall &);
template int launch_msda_forward<bf16_bits>(const MsdaFwdCall &);

// ---- backward -------------------------------------------------------------------------------------------------------------
// Zeroes the gradients the kernels add into -- grad_value always, grad_loc and grad_attn unless every kernel the call can
// reach stores them plainly (msda_backward_shuffles) -- before any launch, then column -> windowed -> generic.
template <typename A>
int launch_msda_backward(const MsdaBwdCall &c)
{
  const int N = c.N, S = c.S, M = c.M, D = c.D, Lq = c.Lq;
  const bool shfl = msda_backward_shuffles(D, sizeof(A));
  const size_t recs = (size_t)N * Lq * M, LP = (size_t)c.L * c.P;

  hipError_t e = zero_fill(c.grad_value, sizeof(A) * (size_t)N * S * M * D, c.stream);
  if (e != hipSuccess) return (int)e;
  if (!shfl) {
    e = zero_fill(c.grad_loc, sizeof(A) * recs * LP * 2, c.stream);
    if (e != hipSuccess) return (int)e;
    e = zero_fill(c.grad_attn, sizeof(A) * recs * LP, c.stream);
    if (e != hipSuccess) return (int)e;
  }
  if (recs == 0) return 0;
  if constexpr (sizeof(A) == 4) {
    // PCT_MSDA_BWD_KERNEL = auto (pyramid-column when the queries are the pyramid's own pixels and the problem fills the
    // chip, else windowed, else generic) | col | win | generic; pct_msda_set_bwd_kernel_choice overrides the environment
    const int mode = g_bwd.get();
    if (shfl && (mode == MSDA_BWD_AUTO || mode == MSDA_BWD_COL) && Lq == S) {
      const int rc = launch_msda_backward_col(c, mode == MSDA_BWD_COL);
      if (rc != PCT_NOT_COVERED) {
        g_bwd.note(MSDA_BWD_COL);
        return rc;
      }
    }
    if (shfl && mode != MSDA_BWD_GENERIC && (mode == MSDA_BWD_WIN || Lq == S)) {
      const int rc = launch_msda_backward_win(c);
      if (rc != PCT_NOT_COVERED) {
        g_bwd.note(MSDA_BWD_WIN);
        return rc;
      }
    }
  }
  g_bwd.note(MSDA_BWD_GENERIC);
  return launch_msda_backward_generic<A>(c);
}

template int launch_msda_backward<float>(const MsdaBwdCall &);
template int launch_msda_backward<double>(const MsdaBwdCall &);

}  // namespace pct
