// Instantiations and launcher of the two-role chained full-column pass (k_colfull_dual,
// fft_colfull_kernels.h): the sizes whose single-role chained pass is alone on its CU (state
// column + exchange buffer beyond half of the LDS) and whose doubled workgroup still fits 12
// waves; a translation unit of its own so that it compiles next to the others.
#include "fft_colfull_kernels.h"
#include "rs_cfg.h"
#include "rs_launch.h"

template <int A, int B>
struct DualCfg {
  using D = RsDual<16, A, B>;
  using C = RsCfg<A, B>;
  // worth it only where one chained workgroup fills the CU's LDS (two of them do not fit)
  static constexpr bool on = D::ok && C::CHAIN && C::LDSC > (size_t)80 * 1024;
  // the state-fused instance (k_colfull_dual<..., true>): every size whose instance compiles without scratch,
  // i.e. all but the two radix-20 sizes (20 x 14 and 20 x 16 spill 1 and 5 registers, as their plain instances do)
  static constexpr bool sf = on && D::S::RMAX <= 18;
};

bool rs_dual_ok(int r2, int r3) {
#define X(A, B) \
  if (r2 == A && r3 == B) return DualCfg<A, B>::on;
  PS_RS_SIZES(X)
#undef X
  return false;
}

bool rs_dual_state_ok(int r2, int r3) {
#define X(A, B) \
  if (r2 == A && r3 == B) return DualCfg<A, B>::sf;
  PS_RS_SIZES(X)
#undef X
  return false;
}

static int dual_set_attr(const void* kern, size_t bytes) {
  return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess ? 0 : -1;
}

int rs_coldual_set_attrs() {
#define X(A, B)                                                                                         \
  if constexpr (DualCfg<A, B>::on) {                                                                    \
    using DD = RsDual<16, A, B>;                                                                        \
    auto kern = k_colfull_dual<16, A, B>;                                                               \
    if (dual_set_attr((const void*)kern, DD::bytes) != 0) return -1;                                    \
    if constexpr (DualCfg<A, B>::sf) {                                                                  \
      auto kern_sf = k_colfull_dual<16, A, B, true>;                                                    \
      if (dual_set_attr((const void*)kern_sf, DD::bytes) != 0) return -1;                               \
    }                                                                                                   \
  }
  PS_RS_SIZES(X)
#undef X
  return 0;
}

// a.alt_src set: the state-fused instance (the state column from the row-pass output a.alt_src)
int rs_launch_coldual(int r2, int r3, const ColFullArgs& a, int lines8, int batch, hipStream_t st) {
  const dim3 grid((unsigned)(lines8 * 64), batch);
#define X(A, B)                                                                                         \
  if (r2 == A && r3 == B) {                                                                             \
    if constexpr (DualCfg<A, B>::on) {                                                                  \
      using DD = RsDual<16, A, B>;                                                                      \
      if (a.alt_src) {                                                                                  \
        if constexpr (DualCfg<A, B>::sf) {                                                              \
          if (batch != 1 || a.pred) return 0;                                                           \
          auto kern_sf = k_colfull_dual<16, A, B, true>;                                                \
          hipLaunchKernelGGL(kern_sf, grid, dim3(2 * DD::S::NTHR), DD::bytes, st, a);                   \
          return 1;                                                                                     \
        }                                                                                               \
        return 0;                                                                                       \
      }                                                                                                 \
      auto kern = k_colfull_dual<16, A, B>;                                                             \
      hipLaunchKernelGGL(kern, grid, dim3(2 * DD::S::NTHR), DD::bytes, st, a);                          \
      return 1;                                                                                         \
    }                                                                                                   \
    return 0;                                                                                           \
  }
  PS_RS_SIZES(X)
#undef X
  return 0;
}
