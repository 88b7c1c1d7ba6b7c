// Reweighted posterior histograms (include/parasitoid_hip.h, ps_whist_*): ps_hist.hip's per-cell histograms on
// fixed bin edges under up to 4 reweighting scenarios at once, every weight a real number on the log scale the
// caller keeps (as ps_wsum.hip: a rescale r of what is held so far and a weight omega on the new scale per member
// and scenario).  Bin b = searchsorted(edges, v, side='right'), bin 0 not stored.  Layout (pitch = N*N rounded up
// to 64 cells, every plane 16-byte aligned):
//   H[j][slot][b - 1][pitch]   fp64, b = 1 .. B+1: the weight of the members of scenario j with bin b, on exp(ref_j)
//   rng[slot][pitch]           uint32, the cell's touched bins as ps_hist.hip's, shared by the scenarios
// An add reads 8 B of record per cell once for all scenarios and, only where v >= e_0, 4 B of range and per
// scenario that takes the member 8 B of the bin's plane (read and written).  A rescale (r != 1) is a launch of
// its own, before the add, over each cell's planes lo .. hi only: untouched planes hold +0.0 and 0 r = +0.0.
// One writer per cell, no atomics: the same calls in the same order give the same bits; another order of adds or
// merges moves a plane within the rounding of its sums.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"
#include "ps_hist_core.h"   // hist_bin, hist_range_add

#define PS_WHIST_MAX_EDGES 1024
#define PS_WHIST_MAX_SCEN 4
#define PS_WHIST_MAX_SLOT 32   // one launch: 32 descriptors = 1.3 kB of kernel arguments

namespace {

struct WhSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct WhSlots {
  WhSlot s[PS_WHIST_MAX_SLOT];
};
// per scenario the rescale r and the member's weight omega (0: the scenario is left untouched); the same for
// every lane, so they stay in scalar registers
struct WhScen {
  double r[PS_WHIST_MAX_SCEN], om[PS_WHIST_MAX_SCEN];
};

// blockIdx.y = slot; thread j of the slot owns the pair of cells 2j, 2j + 1 (j == npair: the tail cell of an odd
// N*N alone).  The record is read once for all NJ scenarios; a block with no value >= e_0 returns before it
// stages the edge table in LDS.  jstride = nslot * nedge * pitch: the distance between two scenarios.
template <int NJ>
__global__ void __launch_bounds__(256) k_whist_add(WhSlots desc, const double* __restrict__ edges, int nedge,
                                                   double* __restrict__ H, uint32_t* __restrict__ rng, int64_t ncell,
                                                   int64_t pitch, int64_t jstride, double negval, WhScen sc) {
  __shared__ double se[PS_WHIST_MAX_EDGES];
  const WhSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pair = j < npair, tail = j == npair && (ncell & 1);
  double v0 = 0.0, v1 = 0.0;
  if (pair) {
    const double2 r = *reinterpret_cast<const double2*>(sd.rec + 2 * j);
    v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
    v1 = ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval);
  } else if (tail) {
    v0 = ps_record_value(sd.rec[ncell - 1], sd.stat_scale, sd.post_scale, delta, negval);
  }
  const double e0 = edges[0];
  const bool h0 = v0 >= e0, h1 = v1 >= e0;   // v1 stays 0 for the tail cell
  if (!__syncthreads_or(h0 || h1)) return;   // every value of the block in bin 0: nothing is stored
  for (int t = threadIdx.x; t < nedge; t += blockDim.x) se[t] = edges[t];
  __syncthreads();
  if (!(h0 || h1)) return;
  double* hs = H + (int64_t)sd.slot * nedge * pitch;   // plane b - 1 of bin b, scenario 0
  uint32_t* rs = rng + (int64_t)sd.slot * pitch;
  const int b0 = h0 ? hist_bin(se, nedge, v0) : 0;
  const int b1 = h1 ? hist_bin(se, nedge, v1) : 0;
  const int64_t i = 2 * j;
  if (tail) {
    const int64_t c = ncell - 1;
    rs[c] = hist_range_add(rs[c], b0);
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      if (!(sc.om[q] > 0.0)) continue;   // uniform: the member leaves this scenario untouched
      double* p = hs + q * jstride + (int64_t)(b0 - 1) * pitch + c;
      *p = *p + sc.om[q];
    }
    return;
  }
  const uint2 rr = *reinterpret_cast<const uint2*>(rs + i);
  const uint2 rn = make_uint2(h0 ? hist_range_add(rr.x, b0) : rr.x, h1 ? hist_range_add(rr.y, b1) : rr.y);
  if (rn.x != rr.x || rn.y != rr.y) *reinterpret_cast<uint2*>(rs + i) = rn;
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    if (!(sc.om[q] > 0.0)) continue;
    double* hq = hs + q * jstride + i;
    if (b0 == b1) {   // both >= 1 here: one 16-byte update
      double2* p = reinterpret_cast<double2*>(hq + (int64_t)(b0 - 1) * pitch);
      double2 c = *p;
      c.x = c.x + sc.om[q];
      c.y = c.y + sc.om[q];
      *p = c;
    } else {
      if (h0) {
        double* p = hq + (int64_t)(b0 - 1) * pitch;
        *p = *p + sc.om[q];
      }
      if (h1) {
        double* p = hq + (int64_t)(b1 - 1) * pitch + 1;
        *p = *p + sc.om[q];
      }
    }
  }
}

using WhAddKernel = void (*)(WhSlots, const double*, int, double*, uint32_t*, int64_t, int64_t, int64_t, double, WhScen);
const WhAddKernel wh_add_kernels[PS_WHIST_MAX_SCEN] = {k_whist_add<1>, k_whist_add<2>, k_whist_add<3>, k_whist_add<4>};

// blockIdx.y = slot, one thread per cell: H = H * r on the planes lo .. hi of the cell's range word, for every
// scenario with r != 1.  Outside the range the planes hold +0.0, which r >= 0 leaves as it is.
__global__ void __launch_bounds__(256) k_whist_rescale(double* __restrict__ H, const uint32_t* __restrict__ rng,
                                                       int nscen, int nedge, int64_t ncell, int64_t pitch,
                                                       int64_t jstride, WhScen sc) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  const int slot = blockIdx.y;
  const uint32_t r = rng[(int64_t)slot * pitch + i];
  const int hi = (int)(r >> 16), lo = (int)(0xffffu - (r & 0xffffu));
  if (hi < lo) return;   // untouched
  double* hs = H + (int64_t)slot * nedge * pitch + i;
  for (int q = 0; q < nscen; ++q) {
    const double rq = sc.r[q];
    if (rq == 1.0) continue;   // uniform
    double* hq = hs + q * jstride;
    for (int b = lo; b <= hi; ++b) {
      double* p = hq + (int64_t)(b - 1) * pitch;
      *p = *p * rq;
    }
  }
}

// one scenario, flat over n doubles: both sides brought to the common scale, every step a statement of its own
__global__ void __launch_bounds__(256) k_whist_merge(double* __restrict__ ha, const double* __restrict__ hb, int64_t n,
                                                     double ra, double rb) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const double x = ha[i] * ra;
    const double y = hb[i] * rb;
    ha[i] = x + y;
  }
}

// flat over nslot * pitch range words: the per-half maximum
__global__ void __launch_bounds__(256) k_whist_merge_range(uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb,
                                                           int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t a = ra[i], b = rb[i];
    ra[i] = (max(a >> 16, b >> 16) << 16) | max(a & 0xffffu, b & 0xffffu);
  }
}

// one scenario and slot, one thread per cell.  T_b = T_{b+1} + H_b from the cell's highest touched bin down
// (T above it is 0), C_b = W - T_{b+1}; b* = the smallest b with C_b >= p W.  T only grows on the way down, so the
// walk stops at b* and reads the planes b* .. hi only; below the lowest touched bin every C equals W - T_lo.  With
// integer weights every T and C is exact and the walk, the fraction and the value are those of k_hist_quantile.
__global__ void k_whist_quantile(const double* __restrict__ hs, const uint32_t* __restrict__ rs,
                                 const double* __restrict__ edges, int nedge, int64_t ncell, int64_t pitch, double p,
                                 double W, double* __restrict__ value, int32_t* __restrict__ bstar) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  const double pW = p * W;
  const uint32_t r = rs[i];
  const int hi = (int)(r >> 16), lo = (int)(0xffffu - (r & 0xffffu));
  int b = 0;
  double v = 0.0;
  if (hi >= lo) {   // touched; else all the weight is in bin 0 and b* = 0
    b = hi;
    double c = hs[(int64_t)(b - 1) * pitch + i];
    double T = 0.0 + c;    // T_b
    double Cm = W - T;     // C_{b-1}
    // invariant: C_b >= pW (C_hi = W); c = H_b, T = T_b, Cm = C_{b-1}
    while (b > lo && Cm >= pW) {
      --b;
      c = hs[(int64_t)(b - 1) * pitch + i];
      T = T + c;
      Cm = W - T;
    }
    if (b == lo && Cm >= pW) {
      b = 0;
    } else if (b == nedge) {
      v = edges[nedge - 1];
    } else {
      const double el = edges[b - 1], eh = edges[b];
      double f = (pW - Cm) / c;
      f = f < 0.0 ? 0.0 : f;
      f = f > 1.0 ? 1.0 : f;
      v = el * pow(eh / el, f);
    }
  }
  value[i] = v;
  bstar[i] = b;
}

// one scenario and slot, one thread per cell: T_{b0} = the sum of H_b over b >= b0 (b0 >= 1), added from the
// cell's highest touched bin down, inside its range only
__global__ void k_whist_tail(const double* __restrict__ hs, const uint32_t* __restrict__ rs, int b0, int64_t ncell,
                             int64_t pitch, double* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  const uint32_t r = rs[i];
  const int hi = (int)(r >> 16), lo = max((int)(0xffffu - (r & 0xffffu)), b0);
  double T = 0.0;
  for (int b = hi; b >= lo; --b) T = T + hs[(int64_t)(b - 1) * pitch + i];
  out[i] = T;
}

}  // namespace

struct ps_whist {
  int device = 0, N = 0, nscen = 0, nslot = 0, nedge = 0;   // nedge = B + 1 edges = stored planes (bins 1 .. B+1)
  std::vector<double> edges;
  int64_t ncell = 0, pitch = 0;
  double* d_edges = nullptr;
  double* H = nullptr;         // [scen][slot][nedge][pitch]
  uint32_t* rng = nullptr;     // [slot][pitch]
  double* qval = nullptr;      // [pitch] quantile / tail scratch
  int32_t* qbin = nullptr;     // [pitch]
  double W[PS_WHIST_MAX_SCEN] = {0, 0, 0, 0};
  int64_t members[PS_WHIST_MAX_SCEN] = {0, 0, 0, 0};
  int64_t skipped[PS_WHIST_MAX_SCEN] = {0, 0, 0, 0};
  hipStream_t stream = nullptr;   // reset / merge / quantile / fetch, and the adds from fields
  PsLastOp last;                  // the last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds, 1: the quantile and tail calls, 2: the rescales
};

static int64_t wh_scen_cells(const ps_whist* a) { return (int64_t)a->nslot * a->nedge * a->pitch; }
static size_t wh_h_bytes(const ps_whist* a) { return (size_t)a->nscen * (size_t)wh_scen_cells(a) * sizeof(double); }
static size_t wh_rng_bytes(const ps_whist* a) { return (size_t)a->nslot * a->pitch * sizeof(uint32_t); }
static bool wh_finite(double v) { return v == v && !isinf(v); }

extern "C" void ps_whist_destroy(ps_whist* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->H, (void*)a->rng, (void*)a->qval, (void*)a->qbin, (void*)a->d_edges})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_whist_reset(ps_whist* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "whist_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->H, 0, wh_h_bytes(a), a->stream));
  PS_HIP(hipMemsetAsync(a->rng, 0, wh_rng_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  for (int j = 0; j < PS_WHIST_MAX_SCEN; ++j) {
    a->W[j] = 0.0;
    a->members[j] = 0;
    a->skipped[j] = 0;
  }
  return PS_OK;
}

extern "C" int ps_whist_create(int device, int N, int nscen, int nslot, int nedge, const double* edges,
                               ps_whist** out) {
  if (!out || N < 1 || nscen < 1 || nscen > PS_WHIST_MAX_SCEN || nslot < 1 || nslot > PS_WHIST_MAX_SLOT || nedge < 2 ||
      nedge > PS_WHIST_MAX_EDGES || !edges)
    return ps_fail(PS_ERR_BAD_ARG, "whist_create: N %d, %d scenarios (1..%d), %d slots (1..%d), %d edges (2..%d)", N,
                   nscen, PS_WHIST_MAX_SCEN, nslot, PS_WHIST_MAX_SLOT, nedge, PS_WHIST_MAX_EDGES);
  for (int k = 0; k < nedge; ++k) {
    if (!(edges[k] > 0.0) || !isfinite(edges[k]))
      return ps_fail(PS_ERR_BAD_ARG, "whist_create: edge %d = %g is not finite and > 0", k, edges[k]);
    if (k > 0 && !(edges[k] > edges[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "whist_create: edges not strictly increasing at %d", k);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // everything, checked before anything is allocated: planes, ranges, quantile scratch, edges
  const double need = (double)nscen * nslot * pitch * nedge * 8.0 + (double)nslot * pitch * 4.0 + (double)pitch * 12.0 +
                      nedge * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "whist_create: %d scenarios x %d edges x %d slots x %lld cells x 8 B = %.3g GB, %.3g GB free",
                   nscen, nedge, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_whist* a = new ps_whist();
  a->device = device;
  a->N = N;
  a->nscen = nscen;
  a->nslot = nslot;
  a->nedge = nedge;
  a->edges.assign(edges, edges + nedge);
  a->ncell = ncell;
  a->pitch = pitch;
  auto fail = [&](int rc) {
    ps_whist_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->H, wh_h_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->rng, wh_rng_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->qval, (size_t)pitch * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&a->qbin, (size_t)pitch * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&a->d_edges, (size_t)nedge * sizeof(double));
  if (e == hipSuccess)
    e = hipMemcpyAsync(a->d_edges, a->edges.data(), (size_t)nedge * sizeof(double), hipMemcpyHostToDevice, a->stream);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "whist_create: %s", hipGetErrorString(e)));
  int rc = ps_whist_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// what every add checks before it resolves a descriptor (who: the entry point)
static int wh_check_add(ps_whist* a, const char* who, int nscen, const double* rescale, const double* omega) {
  if (!a || !rescale || !omega) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (nscen != a->nscen) return ps_fail(PS_ERR_BAD_ARG, "%s: %d scenarios given, the handle has %d", who, nscen, a->nscen);
  for (int j = 0; j < nscen; ++j) {
    if (!(rescale[j] >= 0.0 && rescale[j] <= 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "%s: rescale[%d] = %g is not in [0, 1]", who, j, rescale[j]);
    if (!wh_finite(omega[j]) || omega[j] < 0.0)
      return ps_fail(PS_ERR_BAD_ARG, "%s: omega[%d] = %g is not finite and >= 0", who, j, omega[j]);
  }
  return PS_OK;
}

// one member from the slot descriptors d (one per slot of the handle), enqueued on `stream`: the rescale of the
// scenarios with r != 1 first, where there is one, then the add
static int wh_launch(ps_whist* a, const std::vector<PsSrc>& d, hipStream_t stream, double negval, const double* rescale,
                     const double* omega) {
  WhScen sc;
  double Wn[PS_WHIST_MAX_SCEN] = {0, 0, 0, 0};
  bool any = false, scaled = false;
  for (int j = 0; j < PS_WHIST_MAX_SCEN; ++j) {
    sc.r[j] = 1.0;
    sc.om[j] = 0.0;
    if (j < a->nscen && omega[j] > 0.0) {
      double W = a->W[j];
      W = W * rescale[j];
      W = W + omega[j];
      Wn[j] = W;
      sc.r[j] = rescale[j];
      sc.om[j] = omega[j];
      any = true;
      if (rescale[j] != 1.0 && a->W[j] != 0.0) scaled = true;   // an empty scenario holds zeros
    }
  }
  if (any) {
    PS_TRY(a->last.wait(stream));
    const int threads = 256;
    if (scaled) {
      hipEvent_t e2 = nullptr;
      PS_TRY(a->prof.begin(2, stream, &e2));
      hipLaunchKernelGGL(k_whist_rescale, dim3((unsigned)((a->ncell + threads - 1) / threads), a->nslot), dim3(threads),
                         0, stream, a->H, a->rng, a->nscen, a->nedge, a->ncell, a->pitch, wh_scen_cells(a), sc);
      PS_HIP(hipGetLastError());
      PS_TRY(a->prof.end(stream, e2));
    }
    hipEvent_t e1 = nullptr;
    PS_TRY(a->prof.begin(0, stream, &e1));
    WhSlots desc;
    for (int i = 0; i < PS_WHIST_MAX_SLOT; ++i) {   // the unused tail repeats the last slot
      const int q = std::min(i, a->nslot - 1);
      desc.s[i] = ps_slotted<WhSlot>(d[(size_t)q], q);
    }
    const int64_t npair = a->ncell / 2 + 1;   // the pairs and the tail cell's thread
    const int bx = (int)((npair + threads - 1) / threads);
    hipLaunchKernelGGL(wh_add_kernels[a->nscen - 1], dim3(bx, a->nslot), dim3(threads), 0, stream, desc, a->d_edges,
                       a->nedge, a->H, a->rng, a->ncell, a->pitch, wh_scen_cells(a), negval, sc);
    PS_HIP(hipGetLastError());
    PS_TRY(a->prof.end(stream, e1));
    PS_TRY(a->last.mark(stream));
  }
  for (int j = 0; j < a->nscen; ++j) {
    if (omega[j] > 0.0) {
      a->W[j] = Wn[j];
      a->members[j] += 1;
    } else {
      a->skipped[j] += 1;
    }
  }
  return PS_OK;
}

extern "C" int ps_whist_add(ps_whist* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                            const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                            int nscen, const double* rescale, const double* omega) {
  if (!s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "whist_add: bad arguments");
  PS_TRY(wh_check_add(a, "whist_add", nscen, rescale, omega));
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "whist_add: %d slots given, the handle has %d", nslot, a->nslot);
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("whist_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, d.data(), &stream));
  return wh_launch(a, d, stream, negval, rescale, omega);
}

// one member whose values are the current fields of a projection or a release plan (who: the entry point)
static int wh_add_fields(ps_whist* a, void* h, const PsFieldsOps& src, const char* who, int nscen, const double* rescale,
                         const double* omega) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(wh_check_add(a, who, nscen, rescale, omega));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  std::vector<PsSrc> d((size_t)a->nslot);
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, d.data()));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(wh_launch(a, d, a->stream, 0.0, rescale, omega));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_whist_add_project(ps_whist* a, ps_project* p, int nscen, const double* rescale, const double* omega) {
  return wh_add_fields(a, p, ps_project_fields(), "whist_add_project", nscen, rescale, omega);
}

extern "C" int ps_whist_add_sites(ps_whist* a, ps_sites* p, int nscen, const double* rescale, const double* omega) {
  return wh_add_fields(a, p, ps_sites_fields(), "whist_add_sites", nscen, rescale, omega);
}

extern "C" int ps_whist_merge(ps_whist* dst, ps_whist* src, const double* ra, const double* rb) {
  if (!dst || !src || !ra || !rb) return ps_fail(PS_ERR_BAD_ARG, "whist_merge: bad arguments");
  if (dst == src) return ps_fail(PS_ERR_BAD_ARG, "whist_merge: dst and src are the same handle");
  if (dst->device != src->device || dst->N != src->N || dst->nscen != src->nscen || dst->nslot != src->nslot ||
      dst->edges != src->edges)
    return ps_fail(PS_ERR_BAD_ARG, "whist_merge: handles differ in device, domain, scenarios, slots or edges");
  for (int j = 0; j < dst->nscen; ++j)
    if (!(ra[j] >= 0.0 && ra[j] <= 1.0) || !(rb[j] >= 0.0 && rb[j] <= 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "whist_merge: scale (%g, %g) of scenario %d is not in [0, 1]", ra[j], rb[j], j);
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  const int64_t n = wh_scen_cells(dst);
  bool any = false;
  for (int j = 0; j < dst->nscen; ++j) {
    if (src->W[j] == 0.0) {
      dst->skipped[j] += src->skipped[j];
      continue;
    }
    any = true;
    if (dst->W[j] == 0.0) {   // a copy: the merged scenario is src's bit for bit
      PS_HIP(hipMemcpyAsync(dst->H + j * n, src->H + j * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice,
                            dst->stream));
      dst->W[j] = src->W[j];
    } else {
      double Wa = dst->W[j];
      Wa = Wa * ra[j];
      double Wb = src->W[j];
      Wb = Wb * rb[j];
      hipLaunchKernelGGL(k_whist_merge, dim3(2048), dim3(256), 0, dst->stream, dst->H + j * n, src->H + j * n, n, ra[j],
                         rb[j]);
      PS_HIP(hipGetLastError());
      dst->W[j] = Wa + Wb;
    }
    dst->members[j] += src->members[j];
    dst->skipped[j] += src->skipped[j];
  }
  if (any) {
    hipLaunchKernelGGL(k_whist_merge_range, dim3(1024), dim3(256), 0, dst->stream, dst->rng, src->rng,
                       (int64_t)dst->nslot * dst->pitch);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  return PS_OK;
}

extern "C" int ps_whist_info(ps_whist* a, double* total_weight, int64_t* members, int64_t* skipped) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "whist_info: null handle");
  for (int j = 0; j < a->nscen; ++j) {
    if (total_weight) total_weight[j] = a->W[j];
    if (members) members[j] = a->members[j];
    if (skipped) skipped[j] = a->skipped[j];
  }
  return PS_OK;
}

static int wh_check(ps_whist* a, int scen, int slot, const char* who) {
  if (scen < 0 || scen >= a->nscen) return ps_fail(PS_ERR_BAD_ARG, "%s: scenario %d of %d", who, scen, a->nscen);
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: slot %d of %d", who, slot, a->nslot);
  if (a->W[scen] == 0.0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated in scenario %d (W = 0)", who, scen);
  return PS_OK;
}

static const double* wh_planes(const ps_whist* a, int scen, int slot) {
  return a->H + scen * wh_scen_cells(a) + (int64_t)slot * a->nedge * a->pitch;
}

extern "C" int ps_whist_quantile(ps_whist* a, int scen, int slot, double p, double* value, double* lower, double* upper,
                                 int32_t* bin) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "whist_quantile: null handle");
  if (!(p > 0.0 && p <= 1.0)) return ps_fail(PS_ERR_BAD_ARG, "whist_quantile: p = %g is not in (0, 1]", p);
  PS_TRY(wh_check(a, scen, slot, "whist_quantile"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  hipLaunchKernelGGL(k_whist_quantile, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream,
                     wh_planes(a, scen, slot), a->rng + (int64_t)slot * a->pitch, a->d_edges, a->nedge, a->ncell,
                     a->pitch, p, a->W[scen], a->qval, a->qbin);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  const size_t n = (size_t)a->ncell;
  if (value) PS_HIP(hipMemcpyAsync(value, a->qval, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  std::vector<int32_t> own;
  int32_t* b = bin;
  if (!b && (lower || upper)) {
    own.resize(n);
    b = own.data();
  }
  if (b) PS_HIP(hipMemcpyAsync(b, a->qbin, n * sizeof(int32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  const int B1 = a->nedge;   // B + 1
  const double* e = a->edges.data();
  if (lower || upper)
    for (size_t i = 0; i < n; ++i) {
      const int k = b[i];
      if (lower) lower[i] = k == 0 ? 0.0 : e[k - 1];
      if (upper) upper[i] = k == B1 ? INFINITY : e[k];
    }
  return PS_OK;
}

extern "C" int ps_whist_exceed(ps_whist* a, int scen, int slot, int k, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "whist_exceed: bad arguments");
  if (k < 0 || k >= a->nedge) return ps_fail(PS_ERR_BAD_ARG, "whist_exceed: edge %d of %d", k, a->nedge);
  PS_TRY(wh_check(a, scen, slot, "whist_exceed"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  // v >= e_k  <=>  bin >= k + 1
  hipLaunchKernelGGL(k_whist_tail, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream,
                     wh_planes(a, scen, slot), a->rng + (int64_t)slot * a->pitch, k + 1, a->ncell, a->pitch, a->qval);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  const size_t n = (size_t)a->ncell;
  PS_HIP(hipMemcpyAsync(out, a->qval, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  const double W = a->W[scen];
  for (size_t i = 0; i < n; ++i) {
    const double q = out[i] / W;
    out[i] = q < 1.0 ? q : 1.0;
  }
  return PS_OK;
}

extern "C" int ps_whist_fetch(ps_whist* a, int scen, int slot, int b, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "whist_fetch: bad arguments");
  if (scen < 0 || scen >= a->nscen) return ps_fail(PS_ERR_BAD_ARG, "whist_fetch: scenario %d of %d", scen, a->nscen);
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "whist_fetch: slot %d of %d", slot, a->nslot);
  if (b < 1 || b > a->nedge) return ps_fail(PS_ERR_BAD_ARG, "whist_fetch: bin %d of 1..%d", b, a->nedge);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const double* src = wh_planes(a, scen, slot) + (int64_t)(b - 1) * a->pitch;
  PS_HIP(hipMemcpyAsync(out, src, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_whist_prof(ps_whist* a, int enable, double* add_ms, int64_t* adds, double* q_ms, int64_t* q_launches,
                             double* rescale_ms, int64_t* rescales) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "whist_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  double* ms_out[3] = {add_ms, q_ms, rescale_ms};
  int64_t* n_out[3] = {adds, q_launches, rescales};
  for (int k = 0; k < 3; ++k)
    if (ms_out[k] || n_out[k]) PS_TRY(a->prof.totals(k, ms_out[k], n_out[k]));
  return PS_OK;
}
