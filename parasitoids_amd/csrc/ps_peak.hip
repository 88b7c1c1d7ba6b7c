// Posterior peak maps (include/parasitoid_hip.h, ps_peak_*): per member and cell the reductions along time of
// the records the chain has just written -- the peak value m(c) = max(+0.0, max_s v_s(c)), the first slot p(c)
// that attains it ("none" where m == 0), and per threshold t_k the number of listed slots with v_s(c) >= t_k --
// accumulated on the device as weighted integer counts.  The value of a slot is the one ps_summary_add adds
// (ps_record_value).  Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   Y[pitch]                 fp64, the peak field of the last member added (a PsFieldsOps source, nout = 1)
//   pk[slot][pitch]          uint32, the weight of the members whose peak falls on that slot
//   du[k][n - 1][pitch]      uint32, n = 1..nslot: the weight of the members with dur_k = n (n = 0: W - the rest)
// pk and du are one block, pk first.  One thread owns a pair of cells and walks every slot, so every count has
// a single writer and takes a plain read-modify-write.  No floating-point atomics and no global atomics:
// neither the order of adds nor that of merges nor the grid changes a bit.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_PEAK_MAX_SLOT 32   // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_PEAK_MAX_THR 4
#define PS_PEAK_THREADS 256

namespace {

struct PeakSlots {
  PsSrc s[PS_PEAK_MAX_SLOT];
};
struct PeakThr {
  double t[PS_PEAK_MAX_THR];
};

__device__ inline void peak_load(const double* __restrict__ rec, bool pair, int64_t i, double2& r) {
  if (pair)
    r = *reinterpret_cast<const double2*>(rec + i);
  else
    r = make_double2(rec[i], 0.0);
}

// w added to the count of both cells of a pair in one plane (one 8-byte update), or to either cell alone
__device__ inline void peak_count(uint32_t* __restrict__ plane0, int64_t pitch, int64_t i, int a0, int a1, bool on0,
                                  bool on1, uint32_t w) {
  if (on0 && on1 && a0 == a1) {
    uint2* p = reinterpret_cast<uint2*>(plane0 + (int64_t)a0 * pitch + i);
    uint2 c = *p;
    c.x += w;
    c.y += w;
    *p = c;
  } else {
    if (on0) plane0[(int64_t)a0 * pitch + i] += w;
    if (on1) plane0[(int64_t)a1 * pitch + i + 1] += w;
  }
}

// thread j owns the cells 2j, 2j + 1 (j == npair: the tail cell of an odd N*N alone).  The record of slot
// s + 1 is loaded while slot s is tested.  Unlike k_arrival_add there is no early exit: the maximum and the
// durations need every slot of every cell, so each launch reads all nslot records once.  m, p and the nthr
// duration counters of both cells stay in registers; a cell that is zero throughout writes only Y = 0.
__global__ void __launch_bounds__(PS_PEAK_THREADS) k_peak_add(PeakSlots desc, PeakThr thr, int nslot, int nthr,
                                                              double* __restrict__ Y, uint32_t* __restrict__ pk,
                                                              uint32_t* __restrict__ du, int64_t ncell, int64_t pitch,
                                                              double negval, uint32_t w) {
  __shared__ double sdelta[PS_PEAK_MAX_SLOT];
  for (int t = threadIdx.x; t < nslot; t += blockDim.x) sdelta[t] = desc.s[t].stats ? desc.s[t].stats->delta : 0.0;
  __syncthreads();
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pair = j < npair, tail = j == npair && (ncell & 1);
  if (!pair && !tail) return;
  const int64_t i = 2 * j;
  double m0 = 0.0, m1 = 0.0;
  int p0 = nslot, p1 = nslot;   // nslot: none
  int d0[PS_PEAK_MAX_THR], d1[PS_PEAK_MAX_THR];
#pragma unroll
  for (int k = 0; k < PS_PEAK_MAX_THR; ++k) d0[k] = d1[k] = 0;
  double2 r;
  peak_load(desc.s[0].rec, pair, i, r);
  for (int s = 0; s < nslot; ++s) {
    double2 rn = make_double2(0.0, 0.0);
    if (s + 1 < nslot) peak_load(desc.s[s + 1].rec, pair, i, rn);
    const PsSrc& sd = desc.s[s];
    const double delta = sdelta[s];
    const double v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
    const double v1 = pair ? ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval) : 0.0;
    if (v0 > m0) {   // strict: the first slot that attains the maximum keeps it
      m0 = v0;
      p0 = s;
    }
    if (v1 > m1) {
      m1 = v1;
      p1 = s;
    }
#pragma unroll
    for (int k = 0; k < PS_PEAK_MAX_THR; ++k) {
      if (k < nthr) {
        d0[k] += v0 >= thr.t[k] ? 1 : 0;
        d1[k] += v1 >= thr.t[k] ? 1 : 0;
      }
    }
    r = rn;
  }
  if (pair)
    *reinterpret_cast<double2*>(Y + i) = make_double2(m0, m1);
  else
    Y[i] = m0;
  if (p0 == nslot && p1 == nslot) return;   // zero throughout (every threshold is > 0): nothing to count
  peak_count(pk, pitch, i, p0, p1, p0 < nslot, p1 < nslot, w);
#pragma unroll
  for (int k = 0; k < PS_PEAK_MAX_THR; ++k) {
    if (k >= nthr) break;
    peak_count(du + (int64_t)k * nslot * pitch, pitch, i, d0[k] - 1, d1[k] - 1, d0[k] > 0, d1[k] > 0, w);
  }
}

// flat over (1 + nthr) * nslot * pitch words
__global__ void k_peak_merge(uint32_t* __restrict__ ca, const uint32_t* __restrict__ cb, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) ca[i] += cb[i];
}

// one thread per cell: C = the counts of nplane planes from `planes` on; prob = C / W, else cum = C
__global__ void k_peak_cum(const uint32_t* __restrict__ planes, int nplane, int64_t ncell, int64_t pitch, double W,
                           double* __restrict__ prob, uint32_t* __restrict__ cum) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  uint32_t c = 0;
  for (int s = 0; s < nplane; ++s) c += planes[(int64_t)s * pitch + i];
  if (prob)
    prob[i] = (double)c / W;
  else
    cum[i] = c;
}

// one thread per cell over nplane planes.  implied0 = 0: the smallest plane s with (double)C_s >= p W, -1 if
// none (the peak day).  implied0 = 1: the planes are n = 1..nplane behind an implied plane n = 0 that holds
// W - the rest; the smallest n in 0..nplane (the duration; the last one always qualifies as C = W and p <= 1).
__global__ void k_peak_quantile(const uint32_t* __restrict__ planes, int nplane, int implied0, int64_t ncell,
                                int64_t pitch, uint32_t W, double pW, int32_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  uint32_t c = 0;
  int q = -1;
  if (implied0) {
    uint32_t tot = 0;
    for (int s = 0; s < nplane; ++s) tot += planes[(int64_t)s * pitch + i];
    c = W - tot;
    if ((double)c >= pW) q = 0;
  }
  for (int s = 0; s < nplane && q < 0; ++s) {
    c += planes[(int64_t)s * pitch + i];
    if ((double)c >= pW) q = s + implied0;
  }
  out[i] = q;
}

// one thread per cell: (sum over n of n * du[n - 1]) / W, the sum exact in 64-bit integers
__global__ void k_peak_dur_mean(const uint32_t* __restrict__ planes, int nslot, int64_t ncell, int64_t pitch, double W,
                                double* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  uint64_t c = 0;
  for (int n = 1; n <= nslot; ++n) c += (uint64_t)n * planes[(int64_t)(n - 1) * pitch + i];
  out[i] = (double)c / W;
}

}  // namespace

struct ps_peak {
  int device = 0, N = 0, nslot = 0, nthr = 0;
  std::vector<double> thr;
  int64_t ncell = 0, pitch = 0;
  int nblk = 0;                // blocks of one add launch
  double* Y = nullptr;         // [pitch] the last member's peak field
  uint32_t* cnt = nullptr;     // pk[slot][pitch], then du[k][n - 1][pitch]
  double* map = nullptr;       // [pitch] map scratch (prob / quantile / cumulative counts / mean)
  uint64_t W = 0;
  int64_t members = 0;
  bool y_live = false;         // an add since create / reset wrote Y
  hipStream_t stream = nullptr;    // reset / merge / maps / fetch, and the adds of fields sources
  PsLastOp last;                   // the last operation, on whatever stream it ran
  PsProf prof;                     // channel 0: the adds, 1: the maps
};

static int64_t peak_planes(const ps_peak* a) { return (int64_t)(1 + a->nthr) * a->nslot; }
static size_t peak_cnt_bytes(const ps_peak* a) { return (size_t)peak_planes(a) * a->pitch * sizeof(uint32_t); }
static uint32_t* peak_du(const ps_peak* a, int k) { return a->cnt + (int64_t)(1 + k) * a->nslot * a->pitch; }

extern "C" void ps_peak_destroy(ps_peak* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->Y, (void*)a->cnt, (void*)a->map})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_peak_reset(ps_peak* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "peak_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->cnt, 0, peak_cnt_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  a->y_live = false;
  return PS_OK;
}

extern "C" int ps_peak_create(int device, int N, int nslot, int nthr, const double* thr, ps_peak** out) {
  if (!out || N < 1 || nslot < 1 || nslot > PS_PEAK_MAX_SLOT || nthr < 0 || nthr > PS_PEAK_MAX_THR || (nthr > 0 && !thr))
    return ps_fail(PS_ERR_BAD_ARG, "peak_create: N %d, %d slots (1..%d), %d thresholds (0..%d)", N, nslot,
                   PS_PEAK_MAX_SLOT, nthr, PS_PEAK_MAX_THR);
  *out = nullptr;
  for (int k = 0; k < nthr; ++k) {
    if (!(thr[k] > 0.0) || !isfinite(thr[k]))
      return ps_fail(PS_ERR_BAD_ARG, "peak_create: threshold %d = %g is not finite and > 0", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "peak_create: thresholds not strictly increasing at %d", k);
  }
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  const int64_t nblk = (ncell / 2 + 1 + PS_PEAK_THREADS - 1) / PS_PEAK_THREADS;   // the pairs and the tail thread
  if (nblk > 0x7fffffffLL) return ps_fail(PS_ERR_BAD_ARG, "peak_create: N %d is too large for one launch", N);
  // everything, checked before anything is allocated: the count planes, the peak field, the map scratch
  const double planes = (double)(1 + nthr) * nslot;
  const double need = planes * pitch * 4.0 + 2.0 * (double)pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "peak_create: (1 + %d thresholds) x %d slots x %lld cells x 4 B = %.3g GB, %.3g GB free",
                   nthr, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_peak* a = new ps_peak();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nthr = nthr;
  a->thr.assign(thr, thr + nthr);
  a->ncell = ncell;
  a->pitch = pitch;
  a->nblk = (int)nblk;
  auto fail = [&](int rc) {
    ps_peak_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->cnt, peak_cnt_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->Y, (size_t)pitch * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&a->map, (size_t)pitch * sizeof(double));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "peak_create: %s", hipGetErrorString(e)));
  int rc = ps_peak_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

static int peak_check_weight(const ps_peak* a, const char* who, uint32_t weight) {
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(a->W + weight));
  return PS_OK;
}

// one member from the slot descriptors (one per slot of the handle, the rest null), enqueued on `stream`
static int peak_launch(ps_peak* a, const PeakSlots& desc, hipStream_t stream, double negval, uint32_t weight) {
  PeakThr thr;
  for (int k = 0; k < PS_PEAK_MAX_THR; ++k) thr.t[k] = k < a->nthr ? a->thr[(size_t)k] : 0.0;
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  hipLaunchKernelGGL(k_peak_add, dim3(a->nblk), dim3(PS_PEAK_THREADS), 0, stream, desc, thr, a->nslot, a->nthr, a->Y,
                     a->cnt, peak_du(a, 0), a->ncell, a->pitch, negval, weight);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  a->y_live = true;
  return PS_OK;
}

extern "C" int ps_peak_add(ps_peak* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                           const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                           double negval, uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "peak_add: bad arguments");
  if (nslot != a->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "peak_add: %d slots given, the handle has %d", nslot, a->nslot);
  PS_TRY(peak_check_weight(a, "peak_add", weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  PeakSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("peak_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nslot; i < PS_PEAK_MAX_SLOT; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return peak_launch(a, desc, stream, negval, weight);
}

// one member whose slots are the current fields of a projection or a release plan, in ascending output order
// (who: the entry point)
static int peak_add_fields(ps_peak* a, void* h, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(peak_check_weight(a, who, weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  PeakSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, desc.s));
  for (int e = a->nslot; e < PS_PEAK_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(peak_launch(a, desc, a->stream, 0.0, weight));
  return src.mark(h, a->stream);   // the next apply overwrites the source's fields only after this read
}

extern "C" int ps_peak_add_project(ps_peak* a, ps_project* p, uint32_t weight) {
  return peak_add_fields(a, p, ps_project_fields(), "peak_add_project", weight);
}

extern "C" int ps_peak_add_sites(ps_peak* a, ps_sites* p, uint32_t weight) {
  return peak_add_fields(a, p, ps_sites_fields(), "peak_add_sites", weight);
}

extern "C" int ps_peak_merge(ps_peak* dst, ps_peak* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "peak_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->thr != src->thr)
    return ps_fail(PS_ERR_BAD_ARG, "peak_merge: handles differ in device, domain, slots or thresholds");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "peak_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  hipLaunchKernelGGL(k_peak_merge, dim3(2048), dim3(256), 0, dst->stream, dst->cnt, src->cnt,
                     peak_planes(dst) * dst->pitch);
  PS_HIP(hipGetLastError());
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  return PS_OK;
}

extern "C" int ps_peak_info(ps_peak* a, double* total_weight, int64_t* members) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "peak_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  return PS_OK;
}

extern "C" int ps_peak_fetch_field(ps_peak* a, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak_fetch_field: bad arguments");
  if (!a->y_live) return ps_fail(PS_ERR_STATE, "peak_fetch_field: no member added yet");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->Y, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

static int peak_check_k(ps_peak* a, int k, const char* who) {
  if (k < 0 || k >= a->nthr) return ps_fail(PS_ERR_BAD_ARG, "%s: threshold %d of %d", who, k, a->nthr);
  return PS_OK;
}
static int peak_check_w(ps_peak* a, const char* who) {
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated (W = 0)", who);
  return PS_OK;
}

// the map scratch to the host once the stream has drained
static int peak_map_out(ps_peak* a, void* out, size_t elem) {
  PS_HIP(hipMemcpyAsync(out, a->map, (size_t)a->ncell * elem, hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

// nplane planes from `planes` on summed into the map scratch (as prob = C / W, or as uint32 C)
static int peak_cum(ps_peak* a, const uint32_t* planes, int nplane, bool prob) {
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  hipLaunchKernelGGL(k_peak_cum, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream, planes, nplane,
                     a->ncell, a->pitch, (double)a->W, prob ? a->map : nullptr, prob ? nullptr : (uint32_t*)a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  return a->last.mark(a->stream);
}

static int peak_quantile(ps_peak* a, const uint32_t* planes, int implied0, double p, int32_t* out) {
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  hipLaunchKernelGGL(k_peak_quantile, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream, planes,
                     a->nslot, implied0, a->ncell, a->pitch, (uint32_t)a->W, p * (double)a->W, (int32_t*)a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  return peak_map_out(a, out, sizeof(int32_t));
}

extern "C" int ps_peak_fetch_day_counts(ps_peak* a, int slot, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak_fetch_day_counts: bad arguments");
  if (slot < 0 || slot >= a->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "peak_fetch_day_counts: slot %d of %d", slot, a->nslot);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->cnt + (int64_t)slot * a->pitch, (size_t)a->ncell * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_peak_fetch_duration_counts(ps_peak* a, int k, int n, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak_fetch_duration_counts: bad arguments");
  PS_TRY(peak_check_k(a, k, "peak_fetch_duration_counts"));
  if (n < 0 || n > a->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "peak_fetch_duration_counts: duration %d of 0..%d", n, a->nslot);
  const size_t nc = (size_t)a->ncell;
  if (n == 0) {   // W - the stored planes
    PS_TRY(peak_cum(a, peak_du(a, k), a->nslot, false));
    PS_TRY(peak_map_out(a, out, sizeof(uint32_t)));
    const uint32_t W = (uint32_t)a->W;
    for (size_t i = 0; i < nc; ++i) out[i] = W - out[i];
    return PS_OK;
  }
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(out, peak_du(a, k) + (int64_t)(n - 1) * a->pitch, nc * sizeof(uint32_t), hipMemcpyDeviceToHost,
                        a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_peak_day_prob(ps_peak* a, int slot, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak_day_prob: bad arguments");
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "peak_day_prob: slot %d of %d", slot, a->nslot);
  PS_TRY(peak_check_w(a, "peak_day_prob"));
  PS_TRY(peak_cum(a, a->cnt, slot + 1, true));
  return peak_map_out(a, out, sizeof(double));
}

extern "C" int ps_peak_day_quantile(ps_peak* a, double p, int32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak_day_quantile: bad arguments");
  if (!(p > 0.0 && p <= 1.0)) return ps_fail(PS_ERR_BAD_ARG, "peak_day_quantile: p = %g is not in (0, 1]", p);
  PS_TRY(peak_check_w(a, "peak_day_quantile"));
  return peak_quantile(a, a->cnt, 0, p, out);
}

extern "C" int ps_peak_duration_prob(ps_peak* a, int k, int n, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak_duration_prob: bad arguments");
  PS_TRY(peak_check_k(a, k, "peak_duration_prob"));
  if (n < 1 || n > a->nslot) return ps_fail(PS_ERR_BAD_ARG, "peak_duration_prob: duration %d of 1..%d", n, a->nslot);
  PS_TRY(peak_check_w(a, "peak_duration_prob"));
  PS_TRY(peak_cum(a, peak_du(a, k) + (int64_t)(n - 1) * a->pitch, a->nslot - n + 1, true));
  return peak_map_out(a, out, sizeof(double));
}

extern "C" int ps_peak_duration_quantile(ps_peak* a, int k, double p, int32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak_duration_quantile: bad arguments");
  PS_TRY(peak_check_k(a, k, "peak_duration_quantile"));
  if (!(p > 0.0 && p <= 1.0)) return ps_fail(PS_ERR_BAD_ARG, "peak_duration_quantile: p = %g is not in (0, 1]", p);
  PS_TRY(peak_check_w(a, "peak_duration_quantile"));
  return peak_quantile(a, peak_du(a, k), 1, p, out);
}

extern "C" int ps_peak_duration_mean(ps_peak* a, int k, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak_duration_mean: bad arguments");
  PS_TRY(peak_check_k(a, k, "peak_duration_mean"));
  PS_TRY(peak_check_w(a, "peak_duration_mean"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  hipLaunchKernelGGL(k_peak_dur_mean, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream, peak_du(a, k),
                     a->nslot, a->ncell, a->pitch, (double)a->W, a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  return peak_map_out(a, out, sizeof(double));
}

extern "C" int ps_peak_prof(ps_peak* a, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "peak_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  double* ms_out[2] = {add_ms, map_ms};
  int64_t* n_out[2] = {adds, maps};
  for (int k = 0; k < 2; ++k)
    if (ms_out[k] || n_out[k]) PS_TRY(a->prof.totals(k, ms_out[k], n_out[k]));
  return PS_OK;
}

// the peak field as a fields source of ps_summary.hip and ps_hist.hip: one output, the last member's Y
static int peak_view(void* h, PsProjectView* out) {
  ps_peak* a = static_cast<ps_peak*>(h);
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "peak view: null handle");
  if (!a->y_live) return ps_fail(PS_ERR_STATE, "no peak field yet: add a member to the peak maps first");
  out->Y = a->Y;
  out->pitch = a->pitch;
  out->N = a->N;
  out->nout = 1;
  out->device = a->device;
  return PS_OK;
}
static int peak_wait(void* h, hipStream_t stream) { return static_cast<ps_peak*>(h)->last.wait(stream); }
static int peak_mark(void* h, hipStream_t stream) { return static_cast<ps_peak*>(h)->last.mark(stream); }
PsFieldsOps ps_peak_fields() { return PsFieldsOps{"peak maps", peak_view, peak_wait, peak_mark}; }
