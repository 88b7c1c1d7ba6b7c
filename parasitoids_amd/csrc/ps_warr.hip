// Reweighted posterior arrival maps (include/parasitoid_hip.h, ps_warr_*): ps_arrival.hip's per-cell distribution
// of the first day slot on which a member's value reaches t_k, under up to 4 reweighting scenarios at once, every
// weight a real number on the log scale the caller keeps (as ps_wsum.hip: a rescale r of what is held so far and
// a weight omega on the new scale per member and scenario).  a_k(c) = min{s : v_s(c) >= t_k}, nslot = never (not
// stored: W - the rest).  Layout (pitch = N*N rounded up to 64 cells, every plane 16-byte aligned):
//   A[j][k][slot][pitch]   fp64, the weight of the members of scenario j with a_k(c) = slot, on exp(ref_j)
// One thread owns a pair of cells and walks the slots in order: the records are read once for all scenarios, and
// every plane has a single writer.  No atomics: the same calls in the same order give the same bits; another
// order of adds or merges moves a plane within the rounding of its sums.  The members' reached-cell rows are
// ps_arrival's, not recomputed here.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_WARR_MAX_SLOT 32   // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_WARR_MAX_THR 4
#define PS_WARR_MAX_SCEN 4
#define PS_WARR_THREADS 256

namespace {

struct WaSlots {
  PsSrc s[PS_WARR_MAX_SLOT];
};
struct WaThr {
  double t[PS_WARR_MAX_THR];
};
// per scenario the rescale r and the member's weight omega (0: the scenario is left untouched)
struct WaScen {
  double r[PS_WARR_MAX_SCEN], om[PS_WARR_MAX_SCEN];
};

__device__ inline void wa_load(const double* __restrict__ rec, bool pair, int64_t i, double2& r) {
  if (pair)
    r = *reinterpret_cast<const double2*>(rec + i);
  else
    r = make_double2(rec[i], 0.0);
}

// thread j owns the cells 2j, 2j + 1 (j == npair: the tail cell of an odd N*N alone).  The record of slot s + 1
// is loaded while slot s is tested; a wave stops once every lane's cells reached the top threshold.  Then the
// NJ x K weighted updates; jstride = K * nslot * pitch: the distance between two scenarios.
template <int NJ, int K>
__global__ void __launch_bounds__(PS_WARR_THREADS) k_warr_add(WaSlots desc, WaThr thr, int nslot, double* __restrict__ A,
                                                              int64_t ncell, int64_t pitch, int64_t jstride,
                                                              double negval, WaScen sc) {
  __shared__ double sdelta[PS_WARR_MAX_SLOT];
  for (int t = threadIdx.x; t < nslot; t += blockDim.x) sdelta[t] = desc.s[t].stats ? desc.s[t].stats->delta : 0.0;
  __syncthreads();
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pair = j < npair, tail = j == npair && (ncell & 1);
  const int64_t i = 2 * j;
  int a0[K], a1[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a0[k] = a1[k] = nslot;
  const double top = thr.t[K - 1];
  bool top0 = false, top1 = !pair;   // the tail thread has no second cell
  bool live = pair || tail;
  double2 r = make_double2(0.0, 0.0);
  if (live) wa_load(desc.s[0].rec, pair, i, r);
  for (int s = 0; s < nslot; ++s) {
    if (!__any(live)) break;
    double2 rn = make_double2(0.0, 0.0);
    if (live && s + 1 < nslot) wa_load(desc.s[s + 1].rec, pair, i, rn);
    if (live) {
      const PsSrc& sd = desc.s[s];
      const double delta = sdelta[s];
      const double v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
      const double v1 = pair ? ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval) : 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (a0[k] == nslot && v0 >= thr.t[k]) a0[k] = s;
        if (pair && a1[k] == nslot && v1 >= thr.t[k]) a1[k] = s;
      }
      top0 = top0 || v0 >= top;
      top1 = top1 || v1 >= top;
      live = !(top0 && top1);
    }
    r = rn;
  }
  if (!(pair || tail)) return;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int s0 = a0[k], s1 = a1[k];   // s1 == nslot for the tail cell
    if (s0 == nslot && s1 == nslot) continue;
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      if (!(sc.om[q] > 0.0)) continue;   // uniform: the member leaves this scenario untouched
      double* ak = A + q * jstride + (int64_t)k * nslot * pitch + i;
      if (s0 == s1) {   // a pair arriving together: one 16-byte update
        double2* p = reinterpret_cast<double2*>(ak + (int64_t)s0 * pitch);
        double2 c = *p;
        c.x = c.x + sc.om[q];
        c.y = c.y + sc.om[q];
        *p = c;
      } else {
        if (s0 < nslot) {
          double* p = ak + (int64_t)s0 * pitch;
          *p = *p + sc.om[q];
        }
        if (s1 < nslot) {
          double* p = ak + (int64_t)s1 * pitch + 1;
          *p = *p + sc.om[q];
        }
      }
    }
  }
}

using WaAddKernel = void (*)(WaSlots, WaThr, int, double*, int64_t, int64_t, int64_t, double, WaScen);
#define WA_ROW(J) {k_warr_add<J, 1>, k_warr_add<J, 2>, k_warr_add<J, 3>, k_warr_add<J, 4>}
// k_warr_add<nscen, nthr>, nscen = 1 .. 4, nthr = 1 .. 4
const WaAddKernel wa_add_kernels[PS_WARR_MAX_SCEN][PS_WARR_MAX_THR] = {WA_ROW(1), WA_ROW(2), WA_ROW(3), WA_ROW(4)};

// one scenario, flat over n doubles: A = A * r
__global__ void __launch_bounds__(256) k_warr_rescale(double* __restrict__ a, int64_t n, double r) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) a[i] = a[i] * r;
}

// one scenario, flat over n doubles: both sides brought to the common scale, every step a statement of its own
__global__ void __launch_bounds__(256) k_warr_merge(double* __restrict__ aa, const double* __restrict__ ab, int64_t n,
                                                    double ra, double rb) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    const double x = aa[i] * ra;
    const double y = ab[i] * rb;
    aa[i] = x + y;
  }
}

// one scenario and threshold, one thread per cell: C = C + A_s over the planes 0 .. nplane - 1, ascending
__global__ void k_warr_prob(const double* __restrict__ ak, int nplane, int64_t ncell, int64_t pitch,
                            double* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  double c = 0.0;
  for (int s = 0; s < nplane; ++s) c = c + ak[(int64_t)s * pitch + i];
  out[i] = c;
}

// one scenario and threshold, one thread per cell: the smallest s with C_s >= p W, -1 if none; reads planes 0 .. s
__global__ void k_warr_quantile(const double* __restrict__ ak, int nslot, int64_t ncell, int64_t pitch, double pW,
                                int32_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  double c = 0.0;
  int q = -1;
  for (int s = 0; s < nslot; ++s) {
    c = c + ak[(int64_t)s * pitch + i];
    if (c >= pW) {
      q = s;
      break;
    }
  }
  out[i] = q;
}

}  // namespace

struct ps_warr {
  int device = 0, N = 0, nscen = 0, nslot = 0, nthr = 0;
  std::vector<double> thr;
  int64_t ncell = 0, pitch = 0;
  int nblk = 0;                // blocks of one add launch
  double* A = nullptr;         // [scen][k][slot][pitch]
  double* map = nullptr;       // [pitch] map scratch (running sums / quantile slots)
  double W[PS_WARR_MAX_SCEN] = {0, 0, 0, 0};
  int64_t members[PS_WARR_MAX_SCEN] = {0, 0, 0, 0};
  int64_t skipped[PS_WARR_MAX_SCEN] = {0, 0, 0, 0};
  hipStream_t stream = nullptr;    // reset / merge / maps / fetch, and the adds from fields
  PsLastOp last;                   // the last operation, on whatever stream it ran
  PsProf prof;                     // channel 0: the adds, 1: the maps, 2: the rescales
};

static int64_t wa_scen_cells(const ps_warr* a) { return (int64_t)a->nthr * a->nslot * a->pitch; }
static size_t wa_bytes(const ps_warr* a) { return (size_t)a->nscen * (size_t)wa_scen_cells(a) * sizeof(double); }
static bool wa_finite(double v) { return v == v && !isinf(v); }

extern "C" void ps_warr_destroy(ps_warr* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->A, (void*)a->map})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_warr_reset(ps_warr* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "warr_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->A, 0, wa_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  for (int j = 0; j < PS_WARR_MAX_SCEN; ++j) {
    a->W[j] = 0.0;
    a->members[j] = 0;
    a->skipped[j] = 0;
  }
  return PS_OK;
}

extern "C" int ps_warr_create(int device, int N, int nscen, int nslot, int nthr, const double* thr, ps_warr** out) {
  if (!out || N < 1 || nscen < 1 || nscen > PS_WARR_MAX_SCEN || nslot < 1 || nslot > PS_WARR_MAX_SLOT || nthr < 1 ||
      nthr > PS_WARR_MAX_THR || !thr)
    return ps_fail(PS_ERR_BAD_ARG, "warr_create: N %d, %d scenarios (1..%d), %d slots (1..%d), %d thresholds (1..%d)", N,
                   nscen, PS_WARR_MAX_SCEN, nslot, PS_WARR_MAX_SLOT, nthr, PS_WARR_MAX_THR);
  for (int k = 0; k < nthr; ++k) {
    if (!(thr[k] > 0.0) || !isfinite(thr[k]))
      return ps_fail(PS_ERR_BAD_ARG, "warr_create: threshold %d = %g is not finite and > 0", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "warr_create: thresholds not strictly increasing at %d", k);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  const int64_t nblk = (ncell / 2 + 1 + PS_WARR_THREADS - 1) / PS_WARR_THREADS;   // the pairs and the tail thread
  if (nblk > 0x7fffffffLL) return ps_fail(PS_ERR_BAD_ARG, "warr_create: N %d is too large for one launch", N);
  // everything, checked before anything is allocated: the planes and the map scratch
  const double need = (double)nscen * nthr * nslot * pitch * 8.0 + (double)pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM,
                   "warr_create: %d scenarios x %d thresholds x %d slots x %lld cells x 8 B = %.3g GB, %.3g GB free", nscen,
                   nthr, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_warr* a = new ps_warr();
  a->device = device;
  a->N = N;
  a->nscen = nscen;
  a->nslot = nslot;
  a->nthr = nthr;
  a->thr.assign(thr, thr + nthr);
  a->ncell = ncell;
  a->pitch = pitch;
  a->nblk = (int)nblk;
  auto fail = [&](int rc) {
    ps_warr_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->A, wa_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->map, (size_t)pitch * sizeof(double));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "warr_create: %s", hipGetErrorString(e)));
  int rc = ps_warr_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// what every add checks before it resolves a descriptor (who: the entry point)
static int wa_check_add(ps_warr* a, const char* who, int nscen, const double* rescale, const double* omega) {
  if (!a || !rescale || !omega) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (nscen != a->nscen) return ps_fail(PS_ERR_BAD_ARG, "%s: %d scenarios given, the handle has %d", who, nscen, a->nscen);
  for (int j = 0; j < nscen; ++j) {
    if (!(rescale[j] >= 0.0 && rescale[j] <= 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "%s: rescale[%d] = %g is not in [0, 1]", who, j, rescale[j]);
    if (!wa_finite(omega[j]) || omega[j] < 0.0)
      return ps_fail(PS_ERR_BAD_ARG, "%s: omega[%d] = %g is not finite and >= 0", who, j, omega[j]);
  }
  return PS_OK;
}

// one member from the slot descriptors (one per slot of the handle, the rest null), enqueued on `stream`: the
// rescale of every scenario with r != 1 first, then the add
static int wa_launch(ps_warr* a, const WaSlots& desc, hipStream_t stream, double negval, const double* rescale,
                     const double* omega) {
  WaScen sc;
  double Wn[PS_WARR_MAX_SCEN] = {0, 0, 0, 0};
  bool any = false;
  for (int j = 0; j < PS_WARR_MAX_SCEN; ++j) {
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
    }
  }
  if (any) {
    WaThr thr;
    for (int k = 0; k < PS_WARR_MAX_THR; ++k) thr.t[k] = k < a->nthr ? a->thr[(size_t)k] : 0.0;
    PS_TRY(a->last.wait(stream));
    const int64_t n = wa_scen_cells(a);
    for (int j = 0; j < a->nscen; ++j) {
      if (sc.r[j] == 1.0 || a->W[j] == 0.0) continue;   // an empty scenario holds zeros
      hipEvent_t e2 = nullptr;
      PS_TRY(a->prof.begin(2, stream, &e2));
      hipLaunchKernelGGL(k_warr_rescale, dim3(2048), dim3(256), 0, stream, a->A + j * n, n, sc.r[j]);
      PS_HIP(hipGetLastError());
      PS_TRY(a->prof.end(stream, e2));
    }
    hipEvent_t e1 = nullptr;
    PS_TRY(a->prof.begin(0, stream, &e1));
    hipLaunchKernelGGL(wa_add_kernels[a->nscen - 1][a->nthr - 1], dim3(a->nblk), dim3(PS_WARR_THREADS), 0, stream, desc,
                       thr, a->nslot, a->A, a->ncell, a->pitch, n, negval, sc);
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

extern "C" int ps_warr_add(ps_warr* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                           const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                           int nscen, const double* rescale, const double* omega) {
  if (!s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "warr_add: bad arguments");
  PS_TRY(wa_check_add(a, "warr_add", nscen, rescale, omega));
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "warr_add: %d slots given, the handle has %d", nslot, a->nslot);
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  WaSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("warr_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nslot; i < PS_WARR_MAX_SLOT; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return wa_launch(a, desc, stream, negval, rescale, omega);
}

// one member whose slots are the current fields of a projection or a release plan, in ascending output order
// (who: the entry point)
static int wa_add_fields(ps_warr* a, void* h, const PsFieldsOps& src, const char* who, int nscen, const double* rescale,
                         const double* omega) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(wa_check_add(a, who, nscen, rescale, omega));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  WaSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, desc.s));
  for (int e = a->nslot; e < PS_WARR_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(wa_launch(a, desc, a->stream, 0.0, rescale, omega));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_warr_add_project(ps_warr* a, ps_project* p, int nscen, const double* rescale, const double* omega) {
  return wa_add_fields(a, p, ps_project_fields(), "warr_add_project", nscen, rescale, omega);
}

extern "C" int ps_warr_add_sites(ps_warr* a, ps_sites* p, int nscen, const double* rescale, const double* omega) {
  return wa_add_fields(a, p, ps_sites_fields(), "warr_add_sites", nscen, rescale, omega);
}

extern "C" int ps_warr_merge(ps_warr* dst, ps_warr* src, const double* ra, const double* rb) {
  if (!dst || !src || !ra || !rb) return ps_fail(PS_ERR_BAD_ARG, "warr_merge: bad arguments");
  if (dst == src) return ps_fail(PS_ERR_BAD_ARG, "warr_merge: dst and src are the same handle");
  if (dst->device != src->device || dst->N != src->N || dst->nscen != src->nscen || dst->nslot != src->nslot ||
      dst->thr != src->thr)
    return ps_fail(PS_ERR_BAD_ARG, "warr_merge: handles differ in device, domain, scenarios, slots or thresholds");
  for (int j = 0; j < dst->nscen; ++j)
    if (!(ra[j] >= 0.0 && ra[j] <= 1.0) || !(rb[j] >= 0.0 && rb[j] <= 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "warr_merge: scale (%g, %g) of scenario %d is not in [0, 1]", ra[j], rb[j], j);
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  const int64_t n = wa_scen_cells(dst);
  for (int j = 0; j < dst->nscen; ++j) {
    if (src->W[j] == 0.0) {
      dst->skipped[j] += src->skipped[j];
      continue;
    }
    if (dst->W[j] == 0.0) {   // a copy: the merged scenario is src's bit for bit
      PS_HIP(hipMemcpyAsync(dst->A + j * n, src->A + j * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice,
                            dst->stream));
      dst->W[j] = src->W[j];
    } else {
      double Wa = dst->W[j];
      Wa = Wa * ra[j];
      double Wb = src->W[j];
      Wb = Wb * rb[j];
      hipLaunchKernelGGL(k_warr_merge, dim3(2048), dim3(256), 0, dst->stream, dst->A + j * n, src->A + j * n, n, ra[j],
                         rb[j]);
      PS_HIP(hipGetLastError());
      dst->W[j] = Wa + Wb;
    }
    dst->members[j] += src->members[j];
    dst->skipped[j] += src->skipped[j];
  }
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  return PS_OK;
}

extern "C" int ps_warr_info(ps_warr* a, double* total_weight, int64_t* members, int64_t* skipped) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "warr_info: null handle");
  for (int j = 0; j < a->nscen; ++j) {
    if (total_weight) total_weight[j] = a->W[j];
    if (members) members[j] = a->members[j];
    if (skipped) skipped[j] = a->skipped[j];
  }
  return PS_OK;
}

static int wa_check(ps_warr* a, int scen, int k, const char* who) {
  if (scen < 0 || scen >= a->nscen) return ps_fail(PS_ERR_BAD_ARG, "%s: scenario %d of %d", who, scen, a->nscen);
  if (k < 0 || k >= a->nthr) return ps_fail(PS_ERR_BAD_ARG, "%s: threshold %d of %d", who, k, a->nthr);
  if (a->W[scen] == 0.0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated in scenario %d (W = 0)", who, scen);
  return PS_OK;
}

static const double* wa_planes(const ps_warr* a, int scen, int k) {
  return a->A + scen * wa_scen_cells(a) + (int64_t)k * a->nslot * a->pitch;
}

extern "C" int ps_warr_prob(ps_warr* a, int scen, int k, int slot, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "warr_prob: bad arguments");
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "warr_prob: slot %d of %d", slot, a->nslot);
  PS_TRY(wa_check(a, scen, k, "warr_prob"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  hipLaunchKernelGGL(k_warr_prob, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream, wa_planes(a, scen, k),
                     slot + 1, a->ncell, a->pitch, a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  const size_t n = (size_t)a->ncell;
  PS_HIP(hipMemcpyAsync(out, a->map, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  const double W = a->W[scen];
  for (size_t i = 0; i < n; ++i) {
    const double q = out[i] / W;
    out[i] = q < 1.0 ? q : 1.0;
  }
  return PS_OK;
}

extern "C" int ps_warr_quantile(ps_warr* a, int scen, int k, double p, int32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "warr_quantile: bad arguments");
  if (!(p > 0.0 && p <= 1.0)) return ps_fail(PS_ERR_BAD_ARG, "warr_quantile: p = %g is not in (0, 1]", p);
  PS_TRY(wa_check(a, scen, k, "warr_quantile"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  hipLaunchKernelGGL(k_warr_quantile, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream,
                     wa_planes(a, scen, k), a->nslot, a->ncell, a->pitch, p * a->W[scen], (int32_t*)a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->map, (size_t)a->ncell * sizeof(int32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_warr_fetch(ps_warr* a, int scen, int k, int slot, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "warr_fetch: bad arguments");
  if (scen < 0 || scen >= a->nscen) return ps_fail(PS_ERR_BAD_ARG, "warr_fetch: scenario %d of %d", scen, a->nscen);
  if (k < 0 || k >= a->nthr) return ps_fail(PS_ERR_BAD_ARG, "warr_fetch: threshold %d of %d", k, a->nthr);
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "warr_fetch: slot %d of %d", slot, a->nslot);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const double* src = wa_planes(a, scen, k) + (int64_t)slot * a->pitch;
  PS_HIP(hipMemcpyAsync(out, src, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_warr_prof(ps_warr* a, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps,
                            double* rescale_ms, int64_t* rescales) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "warr_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  double* ms_out[3] = {add_ms, map_ms, rescale_ms};
  int64_t* n_out[3] = {adds, maps, rescales};
  for (int k = 0; k < 3; ++k)
    if (ms_out[k] || n_out[k]) PS_TRY(a->prof.totals(k, ms_out[k], n_out[k]));
  return PS_OK;
}
