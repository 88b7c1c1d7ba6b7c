// Linearised (delta-method) spread of the population around one model evaluation (include/parasitoid_hip.h,
// ps_linspread_*): the centre field, the per-cell sensitivities J_i = dU/dtheta_i accumulated from a
// finite-difference stencil, and after finalisation var = J' Sigma J and threshold exceedances under the
// normal approximation.  Layout as ps_summary.hip (pitch = N*N rounded up to 64 cells, every slot
// 16-byte aligned), one device block carved into
//   center[slot][pitch], J[param][slot][pitch], var[slot][pitch], exc[k][slot][pitch]   (fp64)
// so a flat index slot*pitch + cell addresses the same cell in every array.  Pad cells stay 0.
// An add reads 8 B of record and reads + writes 16 B of J per cell and slot; a finalize reads
// (nparam + 1) * 8 B and writes (1 + nthr) * 8 B per cell and slot.  Both are HBM-bound streams.
#include <math.h>

#include <vector>

#include "ps_common.h"

#define PS_LIN_MAX_PARAM 16
#define PS_LIN_MAX_THR 4
#define PS_LIN_CHUNK 32   // slots per launch: 32 descriptors = 1.3 kB of kernel arguments

namespace {

struct LinSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct LinSlots {
  LinSlot s[PS_LIN_CHUNK];
};
// Sigma = F F', F row-major [param][rank]: 2 kB of kernel arguments at 16 x 16
struct LinFactor {
  double f[PS_LIN_MAX_PARAM * PS_LIN_MAX_PARAM];
};
struct LinThr {
  double t[PS_LIN_MAX_THR];
};

// blockIdx.y = slot of the chunk; a thread owns a pair of cells (the tail cell of an odd N*N alone).
// set: dst = value (the centre); else dst += coef * value, no store where both values are 0.
__global__ void k_linspread_add(LinSlots desc, double* __restrict__ dst, int64_t ncell, int64_t pitch,
                                double negval, double coef, int set) {
  const LinSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double* __restrict__ rec = sd.rec;
  double* js = dst + (int64_t)sd.slot * pitch;
  const int64_t npair = ncell >> 1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j <= npair; j += (int64_t)gridDim.x * blockDim.x) {
    if (j < npair) {
      const double2 r = *reinterpret_cast<const double2*>(rec + 2 * j);
      const double v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
      const double v1 = ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval);
      if (set) {
        *reinterpret_cast<double2*>(js + 2 * j) = make_double2(v0, v1);
      } else if (v0 != 0.0 || v1 != 0.0) {
        double2 a = *reinterpret_cast<const double2*>(js + 2 * j);
        a.x += coef * v0;
        a.y += coef * v1;
        *reinterpret_cast<double2*>(js + 2 * j) = a;
      }
    } else if (ncell & 1) {
      const int64_t i = ncell - 1;
      const double v = ps_record_value(rec[i], sd.stat_scale, sd.post_scale, delta, negval);
      if (set)
        js[i] = v;
      else if (v != 0.0)
        js[i] += coef * v;
    }
  }
}

// exc_t = P(N(c, var) >= t); the 0/1 indicator where var == 0
__device__ inline double lin_exceed(double c, double var, double t) {
  const double sd = sqrt(var);
  if (sd == 0.0) return c >= t ? 1.0 : 0.0;
  return 0.5 * erfc((t - c) / (sd * 1.4142135623730951));
}

// flat over nslot * pitch cells (pitch is a multiple of 64: pairs never straddle a slot).  F goes from the
// kernel arguments to LDS once per workgroup (2 kB; every lane reads the same word: a broadcast).
__global__ void __launch_bounds__(256) k_linspread_finalize(const double* __restrict__ center,
                                                            const double* __restrict__ J, double* __restrict__ var,
                                                            double* __restrict__ exc, int64_t total, int nparam,
                                                            int rank, LinFactor F, int nthr, LinThr thr) {
  __shared__ double sF[PS_LIN_MAX_PARAM * PS_LIN_MAX_PARAM];
  for (int t = threadIdx.x; t < PS_LIN_MAX_PARAM * PS_LIN_MAX_PARAM; t += blockDim.x) sF[t] = F.f[t];
  __syncthreads();
  const int64_t npair = total >> 1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < npair; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = 2 * j;
    double jv0[PS_LIN_MAX_PARAM], jv1[PS_LIN_MAX_PARAM];
#pragma unroll
    for (int p = 0; p < PS_LIN_MAX_PARAM; ++p) {
      double2 a = make_double2(0.0, 0.0);
      if (p < nparam) a = *reinterpret_cast<const double2*>(J + (int64_t)p * total + i);
      jv0[p] = a.x;
      jv1[p] = a.y;
    }
    // var = sum_k (sum_i F_ik J_i)^2: a sum of squares, never negative
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < rank; ++k) {
      double u0 = 0.0, u1 = 0.0;
#pragma unroll
      for (int p = 0; p < PS_LIN_MAX_PARAM; ++p)
        if (p < nparam) {
          const double f = sF[p * PS_LIN_MAX_PARAM + k];
          u0 += f * jv0[p];
          u1 += f * jv1[p];
        }
      s0 += u0 * u0;
      s1 += u1 * u1;
    }
    *reinterpret_cast<double2*>(var + i) = make_double2(s0, s1);
    const double2 c = *reinterpret_cast<const double2*>(center + i);
#pragma unroll
    for (int k = 0; k < PS_LIN_MAX_THR; ++k)
      if (k < nthr)
        *reinterpret_cast<double2*>(exc + (int64_t)k * total + i) =
            make_double2(lin_exceed(c.x, s0, thr.t[k]), lin_exceed(c.y, s1, thr.t[k]));
  }
}

}  // namespace

struct ps_linspread {
  int device = 0, N = 0, nslot = 0, nparam = 0, nthr = 0;
  double thr[PS_LIN_MAX_THR] = {0, 0, 0, 0};
  int64_t ncell = 0, pitch = 0;
  double* block = nullptr;   // center | J | var | exc
  double* center = nullptr;
  double* J = nullptr;
  double* var = nullptr;
  double* exc = nullptr;
  bool centered = false, finalized = false;
  std::vector<int64_t> adds;   // per parameter
  hipStream_t stream = nullptr;   // reset / finalize / fetch
  PsLastOp last;                  // the last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds, 1: the finalizes
};

static int64_t lin_total(const ps_linspread* a) { return (int64_t)a->nslot * a->pitch; }

extern "C" void ps_linspread_destroy(ps_linspread* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  if (a->block) (void)hipFree(a->block);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_linspread_reset(ps_linspread* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "linspread_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->block, 0, (size_t)(a->nparam + 2 + a->nthr) * lin_total(a) * sizeof(double), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->centered = a->finalized = false;
  a->adds.assign((size_t)a->nparam, 0);
  return PS_OK;
}

extern "C" int ps_linspread_create(int device, int N, int nslot, int nparam, int nthr, const double* thr,
                                   ps_linspread** out) {
  if (!out || N < 1 || nslot < 1 || nparam < 1 || nparam > PS_LIN_MAX_PARAM || nthr < 0 || nthr > PS_LIN_MAX_THR ||
      (nthr > 0 && !thr))
    return ps_fail(PS_ERR_BAD_ARG, "linspread_create: N %d, %d slots, %d parameters (1..%d), %d thresholds (at most %d)",
                   N, nslot, nparam, PS_LIN_MAX_PARAM, nthr, PS_LIN_MAX_THR);
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // the whole block, checked before anything is allocated
  const double need = (double)(nparam + 2 + nthr) * (double)nslot * (double)pitch * sizeof(double);
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "linspread_create: (%d + 2 + %d) x %d slots x %lld cells x 8 B = %.3g GB, %.3g GB free",
                   nparam, nthr, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_linspread* a = new ps_linspread();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nparam = nparam;
  a->nthr = nthr;
  for (int k = 0; k < nthr; ++k) a->thr[k] = thr[k];
  a->ncell = ncell;
  a->pitch = pitch;
  auto fail = [&](int rc) {
    ps_linspread_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->block, (size_t)need);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "linspread_create: %s",
                        hipGetErrorString(e)));
  const int64_t t = lin_total(a);
  a->center = a->block;
  a->J = a->center + t;
  a->var = a->J + (int64_t)nparam * t;
  a->exc = a->var + t;
  int rc = ps_linspread_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// one record pass over every slot into dst (set: copy, else dst += coef * value)
static int lin_record_pass(ps_linspread* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                           const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                           double negval, double* dst, double coef, int set, const char* who) {
  if (!s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: %d slots given, the handle has %d", who, nslot, a->nslot);
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: a call with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records(who, "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta, false,
                         d.data(), &stream));
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  if (!set) PS_TRY(a->prof.begin(0, stream, &e1));
  const int64_t npair = a->ncell / 2 + 1;
  const int threads = 256;
  const int bx = (int)std::min<int64_t>((npair + threads - 1) / threads, 4096);
  for (int c0 = 0; c0 < nslot; c0 += PS_LIN_CHUNK) {
    const int n = std::min(PS_LIN_CHUNK, nslot - c0);
    LinSlots desc;
    for (int i = 0; i < n; ++i) desc.s[i] = ps_slotted<LinSlot>(d[(size_t)(c0 + i)], c0 + i);
    hipLaunchKernelGGL(k_linspread_add, dim3(bx, n), dim3(threads), 0, stream, desc, dst, a->ncell, a->pitch, negval,
                       coef, set);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  return PS_OK;
}

extern "C" int ps_linspread_set_center(ps_linspread* a, ps_solver* s, int nslot, const int32_t* kind,
                                       const int32_t* idx, const double* stat_scale, const double* post_scale,
                                       const int32_t* use_delta, double negval) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "linspread_set_center: null handle");
  PS_TRY(lin_record_pass(a, s, nslot, kind, idx, stat_scale, post_scale, use_delta, negval, a->center, 0.0, 1,
                         "linspread_set_center"));
  a->centered = true;
  a->finalized = false;
  return PS_OK;
}

extern "C" int ps_linspread_add(ps_linspread* a, ps_solver* s, int param, double coef, int nslot, const int32_t* kind,
                                const int32_t* idx, const double* stat_scale, const double* post_scale,
                                const int32_t* use_delta, double negval) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "linspread_add: null handle");
  if (param < 0 || param >= a->nparam)
    return ps_fail(PS_ERR_BAD_ARG, "linspread_add: parameter %d of %d", param, a->nparam);
  if (!(coef == coef) || coef == 0.0 || isinf(coef))
    return ps_fail(PS_ERR_BAD_ARG, "linspread_add: coefficient must be finite and non-zero");
  PS_TRY(lin_record_pass(a, s, nslot, kind, idx, stat_scale, post_scale, use_delta, negval,
                         a->J + (int64_t)param * lin_total(a), coef, 0, "linspread_add"));
  a->adds[(size_t)param] += 1;
  a->finalized = false;
  return PS_OK;
}

extern "C" int ps_linspread_finalize(ps_linspread* a, int nparam, int rank, const double* F) {
  if (!a || !F) return ps_fail(PS_ERR_BAD_ARG, "linspread_finalize: bad arguments");
  if (nparam != a->nparam || rank < 1 || rank > PS_LIN_MAX_PARAM)
    return ps_fail(PS_ERR_BAD_ARG, "linspread_finalize: factor %d x %d, the handle has %d parameters (rank 1..%d)",
                   nparam, rank, a->nparam, PS_LIN_MAX_PARAM);
  if (!a->centered) return ps_fail(PS_ERR_STATE, "linspread_finalize: no centre set");
  LinFactor f;
  for (int i = 0; i < PS_LIN_MAX_PARAM * PS_LIN_MAX_PARAM; ++i) f.f[i] = 0.0;
  for (int p = 0; p < nparam; ++p)
    for (int k = 0; k < rank; ++k) {
      const double v = F[(size_t)p * rank + k];
      if (!(v == v) || isinf(v)) return ps_fail(PS_ERR_BAD_ARG, "linspread_finalize: F[%d][%d] is not finite", p, k);
      f.f[p * PS_LIN_MAX_PARAM + k] = v;
    }
  LinThr thr;
  for (int k = 0; k < PS_LIN_MAX_THR; ++k) thr.t[k] = a->thr[k];
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  const int64_t total = lin_total(a);
  const int threads = 256;
  const int bx = (int)std::min<int64_t>((total / 2 + threads - 1) / threads, 8192);
  hipLaunchKernelGGL(k_linspread_finalize, dim3(bx), dim3(threads), 0, a->stream, a->center, a->J, a->var, a->exc,
                     total, a->nparam, rank, f, a->nthr, thr);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  a->finalized = true;
  return PS_OK;
}

extern "C" int ps_linspread_fetch(ps_linspread* a, int slot, int what, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "linspread_fetch: bad arguments");
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "linspread_fetch: slot %d of %d", slot, a->nslot);
  const int64_t t = lin_total(a);
  const double* src = nullptr;
  if (what == 0) {
    if (!a->centered) return ps_fail(PS_ERR_STATE, "linspread_fetch: no centre set");
    src = a->center;
  } else if (what >= 1 && what < 2 + a->nthr) {
    if (!a->finalized) return ps_fail(PS_ERR_STATE, "linspread_fetch: not finalized since the last change");
    src = what == 1 ? a->var : a->exc + (int64_t)(what - 2) * t;
  } else if (what >= 16 && what < 16 + a->nparam) {
    src = a->J + (int64_t)(what - 16) * t;
  } else {
    return ps_fail(PS_ERR_BAD_ARG, "linspread_fetch: quantity %d (0 centre, 1 variance, 2..%d exceedance, 16..%d sensitivity)",
                   what, 1 + a->nthr, 15 + a->nparam);
  }
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(out, src + (int64_t)slot * a->pitch, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost,
                        a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_linspread_info(ps_linspread* a, int* centered, int* finalized, int64_t* adds /* nparam */) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "linspread_info: null handle");
  if (centered) *centered = a->centered;
  if (finalized) *finalized = a->finalized;
  if (adds)
    for (int p = 0; p < a->nparam; ++p) adds[p] = a->adds[(size_t)p];
  return PS_OK;
}

extern "C" int ps_linspread_prof(ps_linspread* a, int enable, double* add_ms, int64_t* add_launches, double* fin_ms,
                                 int64_t* fin_launches) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "linspread_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  if (add_ms || add_launches) PS_TRY(a->prof.totals(0, add_ms, add_launches));
  if (fin_ms || fin_launches) PS_TRY(a->prof.totals(1, fin_ms, fin_launches));
  return PS_OK;
}
