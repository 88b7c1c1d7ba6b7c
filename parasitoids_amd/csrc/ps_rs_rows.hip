// Instantiations and launchers of the register-resident row kernels (fft_rs_kernels.h), one
// translation unit so that they compile in parallel with the rest of the library.
#include "rs_cfg.h"
#include "rs_launch.h"
#include <algorithm>
#include <cstdlib>

bool rs_lookup(int L, int* r2, int* r3) {
#define X(A, B) if (L == 16 * A * B) { *r2 = A; *r3 = B; return true; }
  PS_RS_SIZES(X)
#undef X
  return false;
}

int rs_next_size(int n) {
  int best = 0;
#define X(A, B) if (16 * A * B >= n && (best == 0 || 16 * A * B < best)) best = 16 * A * B;
  PS_RS_SIZES(X)
#undef X
  return best;
}

bool rs_info(int r2, int r3, RsInfo* out) {
#define X(A, B)                                                                       \
  if (r2 == A && r3 == B) {                                                           \
    using C = RsCfg<A, B>;                                                            \
    *out = RsInfo{C::NP, C::S::NTHR, C::LDS, C::LDSC1, C::LDSC, C::CHAIN, RsPLds<16, A, B>::fits};            \
    return true;                                                                      \
  }
  PS_RS_SIZES(X)
#undef X
  return false;
}

// k_row_fwd_rsp serves the sizes that put two or more row pairs into a workgroup (NP >= 2: up to six waves per
// pair).  The NP = 1 sizes (seven waves and more per pair; 5600, 6912 and 8400 among them) keep
// k_row_fwd_rs: measured on the Carnarvon 10 km chain at 5600 points, whose kernels are 1650-2780 rows wide, the
// batch launch was 10 % slower with the persistent kernel and the chain 2 %.  Neither instance
// spills there (149 against 142 VGPRs at 16 x 25 x 14, NP = 1); the cause is not known.
template <int R2, int R3>
constexpr bool rs_fwd_live_ok() { return RsCfg<R2, R3>::NP >= 2; }

// The sizes with TWO pairs per workgroup (five or six waves per pair; the headline's 5184 and 4608 among them)
// run the persistent kernel with ONE pair per workgroup, two workgroups resident per CU: the two
// halves of a two-pair workgroup pass the same barriers, so both issue their column-major stores at the same
// time and both wait while they are taken; two workgroups drift into anti-phase.  Measured at 5184 only; the
// three- and four-pair sizes keep their workgroups.
template <int R2, int R3>
constexpr bool rs_fwd_solo() { return RsCfg<R2, R3>::NP == 2; }

bool rs_row_fwd_info(int r2, int r3, int* np, int* persistent) {
#define X(A, B) if (r2 == A && r3 == B) { *np = RsCfg<A, B>::NP; *persistent = rs_fwd_live_ok<A, B>() ? 1 : 0; return true; }
  PS_RS_SIZES(X)
#undef X
  return false;
}

// The staged kernel (k_row_fwd_rsps) needs the exchange buffers and 2 NP source rows of src_ld doubles in
// whole 1 KB chunks side by side in LDS (row_fwd_stage.h): a question of the kernel box, not of the size alone.
// 0 when (r2, r3) is not served or keeps the one-shot kernel.
static const size_t kRsMaxLds = (size_t)160 * 1024;
size_t rs_row_fwd_stage_lds(int r2, int r3, int src_ld) {
#define X(A, B) if (r2 == A && r3 == B) return rs_fwd_live_ok<A, B>() && src_ld > 0 ? RsCfg<A, B>::LDS + fstage_bytes(RsCfg<A, B>::NP, src_ld) : 0;
  PS_RS_SIZES(X)
#undef X
  return 0;
}
bool rs_row_fwd_staged(int r2, int r3, int src_ld) {
  const size_t b = rs_row_fwd_stage_lds(r2, r3, src_ld);
  return b > 0 && b <= kRsMaxLds;
}

int rs_rows_set_attrs() {
#define X(A, B)                                                                                              \
  {                                                                                                          \
    using C = RsCfg<A, B>;                                                                                   \
    constexpr int np = C::NP;                                                                                \
    using Z = RsPLds<16, A, B>;                                                                              \
    if constexpr (Z::fits) {                                                                                 \
      auto kp = k_row_inv_rsp<16, A, B>;                                                                     \
      if (hipFuncSetAttribute((const void*)kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Z::bytes) != hipSuccess) return -1; \
    }                                                                                                        \
    using Z2 = Rs2Lds<16, A, B>;                                                                             \
    if constexpr (Z2::ok) {                                                                                  \
      auto k2 = k_row_inv_rs2<16, A, B>;                                                                     \
      if (Z2::bytes > 48 * 1024 &&                                                                           \
          hipFuncSetAttribute((const void*)k2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Z2::bytes) != hipSuccess) return -1; \
    }                                                                                                        \
    if (C::LDSC1 > 48 * 1024) {                                                                              \
      auto kr = k_row_inv_fold<16, A, B>;                                                                    \
      if (hipFuncSetAttribute((const void*)kr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDSC1) != hipSuccess) return -1; \
    }                                                                                                        \
    if (C::LDS > 48 * 1024) {                                                                                \
      auto ki = k_row_inv_rs<16, A, B, np>;                                                                  \
      auto kf = k_row_fwd_rs<16, A, B, np>;                                                                  \
      if (hipFuncSetAttribute((const void*)ki, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS) != hipSuccess) return -1; \
      if (hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS) != hipSuccess) return -1; \
      if constexpr (rs_fwd_live_ok<A, B>()) {                                                                \
        auto kl = k_row_fwd_rsp<16, A, B, np>;                                                               \
        if (hipFuncSetAttribute((const void*)kl, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS) != hipSuccess) return -1; \
      }                                                                                                      \
    }                                                                                                        \
    if constexpr (rs_fwd_live_ok<A, B>()) {   /* exchange buffers + staged rows: up to the whole CU */       \
      auto ks = k_row_fwd_rsps<16, A, B, np>;                                                                \
      if (hipFuncSetAttribute((const void*)ks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRsMaxLds) != hipSuccess) return -1; \
    }                                                                                                        \
    if constexpr (rs_fwd_solo<A, B>()) {                                                                     \
      auto k1 = k_row_fwd_rsp<16, A, B, 1>;                                                                  \
      if (C::LDSC1 > 48 * 1024 &&                                                                            \
          hipFuncSetAttribute((const void*)k1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDSC1) != hipSuccess) return -1; \
    }                                                                                                        \
  }
  PS_RS_SIZES(X)
#undef X
  return 0;
}

static int device_cus();
static int grid_x(int npairs, int np, int tstride) {
  int gx = (npairs + np - 1) / np;
  if (tstride) {   // column-major side: the workgroups sharing a 128-byte line sit on one XCD
    const int m = 8 * (np >= 4 ? 1 : 4 / np);
    gx = (gx + m - 1) / m * m;
  }
  return gx;
}

int rs_launch_row_fwd(int r2, int r3, const RowFwdArgs& a, int npairs, int batch, hipStream_t st) {
#define X(A, B)                                                                                              \
  if (r2 == A && r3 == B) {                                                                                  \
    using C = RsCfg<A, B>;                                                                                   \
    constexpr int np = C::NP;                                                                                \
    /* small transforms pack 2-4 row pairs into a 12-wave workgroup; a single field with few live rows   \
       (the 1201-row torus of the R = 400 fold child on 1920 points: 151 workgroups for 256 CUs) then     \
       leaves CUs idle -- half the pairs per workgroup there */                                             \
    constexpr int np2 = (np >= 2 && C::S::L <= 2560) ? np / 2 : np;                                          \
    if constexpr (np2 != np) {                                                                               \
      const int live = a.rmap.n1 + (a.P > a.rmap.lo2 ? a.P - a.rmap.lo2 : 0);                                \
      if ((((live + 1) / 2 + np - 1) / np) * batch < device_cus()) {                                         \
        auto k2 = k_row_fwd_rs<16, A, B, np2>;                                                               \
        using Y2 = RsInvLds<16, A, B>;                                                                       \
        constexpr size_t lds2 = Y2::bytes(np2);                                                              \
        hipLaunchKernelGGL(k2, dim3(grid_x(npairs, np2, a.tstride), batch), dim3(C::S::NTHR * np2), lds2, st, a); \
        return 1;                                                                                            \
      }                                                                                                      \
    }                                                                                                        \
    auto kern = k_row_fwd_rs<16, A, B, np>;                                                                  \
    hipLaunchKernelGGL(kern, dim3(grid_x(npairs, np, a.tstride), batch), dim3(C::S::NTHR * np), C::LDS, st, a); \
    return 1;                                                                                                \
  }
  PS_RS_SIZES(X)
#undef X
  return 0;
}

// Kernel batches of the full-column pipeline: one persistent workgroup per CU slot over the live units
// (k_row_fwd_rsp).  hranges: host copy of a.rowrange, [batch][2].
// stage: take k_row_fwd_rsps where its staging area fits (rs_row_fwd_staged) and every source column of the
// column map lies inside a staged row.
int rs_launch_row_fwd_live(int r2, int r3, const RowFwdArgs& a, const int* hranges, int batch, hipStream_t st,
                           bool stage, bool solo) {
#define X(A, B)                                                                                              \
  if (r2 == A && r3 == B) {                                                                                  \
    using C = RsCfg<A, B>;                                                                                   \
    constexpr int np = C::NP;                                                                                \
    if constexpr (!rs_fwd_live_ok<A, B>()) return rs_launch_row_fwd(r2, r3, a, (a.P + 1) / 2, batch, st);    \
    else {                                                                                                   \
    constexpr int kl = np >= 4 ? 1 : 4 / np;                                                                 \
    const int total = kl * live_total(a.rmap.n1, a.rmap.off1, a.rmap.lo2, a.rmap.off2, a.P, hranges, batch, 2 * np * kl); \
    if (total == 0) return 1;   /* every kernel of the batch is empty */                                     \
    /* resident workgroups per CU: 12 wave slots at the kernel's <= 168 registers, 160 KB of LDS */          \
    constexpr int W = C::S::NTHR / 64 * np;                                                                  \
    constexpr int kw = 12 / W < 1 ? 1 : 12 / W, kld = (int)((size_t)160 * 1024 / C::LDS);                    \
    constexpr int per_cu = kw < kld ? kw : (kld < 1 ? 1 : kld);                                              \
    const int m = 8 * kl;                                                                                    \
    const int cmax = std::max(a.cmap.n1 - 1 + a.cmap.off1, a.P - 1 - a.cmap.lo2 + a.cmap.off2);             \
    if (stage && rs_row_fwd_staged(r2, r3, a.src_ld) && cmax < a.src_ld && a.cmap.off1 >= 0 && a.cmap.off2 >= 0) { \
      const size_t lds = C::LDS + fstage_bytes(np, a.src_ld);                                                \
      const int kls = (int)(kRsMaxLds / lds), per_cu_s = kw < kls ? kw : kls;                                \
      const int wgs = (std::min(total, device_cus() * per_cu_s) + m - 1) / m * m;                            \
      auto ks = k_row_fwd_rsps<16, A, B, np>;                                                                \
      hipLaunchKernelGGL(ks, dim3(wgs), dim3(C::S::NTHR * np), lds, st, a, batch, total,                     \
                         a.src + (int64_t)batch * a.src_bstride);                                            \
      return 1;                                                                                              \
    }                                                                                                        \
    if constexpr (rs_fwd_solo<A, B>()) {                                                                     \
      if (solo) {   /* one pair per workgroup: four units per output line, two workgroups per CU */          \
        const int total1 = 4 * live_total(a.rmap.n1, a.rmap.off1, a.rmap.lo2, a.rmap.off2, a.P, hranges, batch, 8); \
        const int wgs1 = (std::min(total1, device_cus() * 2) + 31) / 32 * 32;                                \
        auto k1 = k_row_fwd_rsp<16, A, B, 1>;                                                                \
        hipLaunchKernelGGL(k1, dim3(wgs1), dim3(C::S::NTHR), C::LDSC1, st, a, batch, total1);                \
        return 1;                                                                                            \
      }                                                                                                      \
    }                                                                                                        \
    const int wgs = (std::min(total, device_cus() * per_cu) + m - 1) / m * m;                                \
    auto kern = k_row_fwd_rsp<16, A, B, np>;                                                                 \
    hipLaunchKernelGGL(kern, dim3(wgs), dim3(C::S::NTHR * np), C::LDS, st, a, batch, total);                 \
    return 1;                                                                                                \
    }                                                                                                        \
  }
  PS_RS_SIZES(X)
#undef X
  return 0;
}

int rs_row_live_units(int P, int M, int np, int nd, const int* ranges, int* day, int* unit, int cap) {
  if (P < 1 || M < 0 || np < 1 || nd < 0 || 2 * M + 1 > P) return -1;
  const int n1 = M + 1, off1 = M, lo2 = P - M, off2 = 0, g = 2 * np;   // map_wrap(M, P)
  const int total = live_total(n1, off1, lo2, off2, P, ranges, nd, g);
  LiveCursor cur = live_cursor(n1, off1, lo2, off2, P, ranges, nd, g);
  for (int k = 0; k < total && k < cap; ++k) {
    if (!live_advance(cur, k, n1, off1, lo2, off2, P, ranges, nd, g)) return -1;
    day[k] = cur.day;
    unit[k] = live_unit(cur.runs, k - cur.base);
  }
  return total;
}

int rs_launch_row_fold(int r2, int r3, const RowFoldArgs& a, int units, hipStream_t st) {
#define X(A, B)                                                                                              \
  if (r2 == A && r3 == B) {                                                                                  \
    using C = RsCfg<A, B>;                                                                                   \
    auto kern = k_row_inv_fold<16, A, B>;                                                                    \
    hipLaunchKernelGGL(kern, dim3(units), dim3(C::S::NTHR), C::LDSC1, st, a);                                \
    return 1;                                                                                                \
  }
  PS_RS_SIZES(X)
#undef X
  return 0;
}

// workgroups of the persistent kernel: one per CU
static int device_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return n;
}

int rs_launch_row_inv(int r2, int r3, const RowInvArgs& a, int npairs, int batch, hipStream_t st) {
#define X(A, B)                                                                                              \
  if (r2 == A && r3 == B) {                                                                                  \
    using C = RsCfg<A, B>;                                                                                   \
    using Z = RsPLds<16, A, B>;                                                                              \
    using Z2 = Rs2Lds<16, A, B>;                                                                             \
    if constexpr (Z2::ok) {                                                                                  \
      if (a.persistent == 2 && a.tstride == 0) {   /* two roles in anti-phase, one workgroup per CU */      \
        const int units = npairs * batch;                                                                    \
        const int wgs = std::min(device_cus(), (units + 1) / 2);                                             \
        auto k2 = k_row_inv_rs2<16, A, B>;                                                                   \
        hipLaunchKernelGGL(k2, dim3(wgs), dim3(2 * C::S::NTHR), Z2::bytes, st, a, npairs, units);            \
        return 1;                                                                                            \
      }                                                                                                      \
    }                                                                                                        \
    if constexpr (Z::fits) {                                                                                 \
      if (a.persistent && a.tstride == 0) {                                                                  \
        const int units = npairs * batch;                                                                    \
        /* resident workgroups per CU: 8 wave slots at the kernel's ~210 registers, 160 KB of LDS */         \
        constexpr int W = C::S::NTHR / 64;                                                                   \
        constexpr int kw = 8 / W < 1 ? 1 : 8 / W, kl = (int)((size_t)160 * 1024 / Z::bytes);                 \
        constexpr int per_cu = kw < kl ? kw : kl;                                                            \
        const int slots = device_cus() * per_cu;                                                             \
        const int wgs = units < slots ? units : slots;                                                       \
        auto kp = k_row_inv_rsp<16, A, B>;                                                                   \
        hipLaunchKernelGGL(kp, dim3(wgs), dim3(C::S::NTHR), Z::bytes, st, a, npairs, units); \
        return 1;                                                                                            \
      }                                                                                                      \
    }                                                                                                        \
    constexpr int np = C::NP;                                                                                \
    auto kern = k_row_inv_rs<16, A, B, np>;                                                                  \
    hipLaunchKernelGGL(kern, dim3(grid_x(npairs, np, a.tstride), batch), dim3(C::S::NTHR * np), C::LDS, st, a); \
    return 1;                                                                                                \
  }
  PS_RS_SIZES(X)
#undef X
  return 0;
}
