// Posterior predictive spread (include/parasitoid_hip.h, ps_summary_*): per-cell weighted mean, M2
// and threshold counts of many model evaluations, accumulated on the device from the solver's
// records.  Layout per slot (pitch = N*N rounded up to 64 cells, so every slot starts 16-byte
// aligned): mean[slot][pitch], m2[slot][pitch] (fp64), cnt[slot][k][pitch] (uint32).  An add reads
// 8 B of record and reads + writes 16 B of mean, 16 B of M2 and 8 B per threshold of every cell of
// every slot -- less where a pair of cells is unchanged (value == mean: nothing is stored).
#include <vector>

#include "ps_common.h"

#define PS_SUM_MAX_THR 4
#define PS_SUM_CHUNK 32   // slots per launch: 32 descriptors = 1.3 kB of kernel arguments

namespace {

struct SumSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct SumSlots {
  SumSlot s[PS_SUM_CHUNK];
};
struct SumThr {
  double t[PS_SUM_MAX_THR];
};

// blockIdx.y = slot of the chunk; a thread owns a pair of cells (the tail cell of an odd N*N alone)
__global__ void k_summary_add(SumSlots desc, double* __restrict__ mean, double* __restrict__ m2,
                              uint32_t* __restrict__ cnt, int64_t ncell, int64_t pitch, int nthr, SumThr thr,
                              double negval, double w, double Wn, uint32_t wi) {
  const SumSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double* __restrict__ rec = sd.rec;
  double* ms = mean + (int64_t)sd.slot * pitch;
  double* qs = m2 + (int64_t)sd.slot * pitch;
  uint32_t* cs = cnt + (int64_t)sd.slot * nthr * pitch;
  const int64_t npair = ncell >> 1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j <= npair; j += (int64_t)gridDim.x * blockDim.x) {
    if (j < npair) {
      const double2 r = *reinterpret_cast<const double2*>(rec + 2 * j);
      double2 m = *reinterpret_cast<const double2*>(ms + 2 * j);
      double2 q = *reinterpret_cast<const double2*>(qs + 2 * j);
      const double v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
      const double v1 = ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval);
      const bool c0 = sum_update(v0, w, Wn, m.x, q.x);
      const bool c1 = sum_update(v1, w, Wn, m.y, q.y);
      if (c0 || c1) {
        *reinterpret_cast<double2*>(ms + 2 * j) = m;
        *reinterpret_cast<double2*>(qs + 2 * j) = q;
      }
      for (int k = 0; k < nthr; ++k) {
        const bool e0 = v0 >= thr.t[k], e1 = v1 >= thr.t[k];
        if (e0 || e1) {
          uint2* p = reinterpret_cast<uint2*>(cs + (int64_t)k * pitch + 2 * j);
          uint2 c = *p;
          c.x += e0 ? wi : 0u;
          c.y += e1 ? wi : 0u;
          *p = c;
        }
      }
    } else if (ncell & 1) {
      const int64_t i = ncell - 1;
      const double v = ps_record_value(rec[i], sd.stat_scale, sd.post_scale, delta, negval);
      double m = ms[i], q = qs[i];
      if (sum_update(v, w, Wn, m, q)) {
        ms[i] = m;
        qs[i] = q;
      }
      for (int k = 0; k < nthr; ++k)
        if (v >= thr.t[k]) cs[(int64_t)k * pitch + i] += wi;
    }
  }
}

// Chan, Golub & LeVeque: (Wa, mean_a, M2a) + (Wb, mean_b, M2b) over every slot's cells
__global__ void k_summary_merge(double* __restrict__ ma, double* __restrict__ qa, uint32_t* __restrict__ ca,
                                const double* __restrict__ mb, const double* __restrict__ qb,
                                const uint32_t* __restrict__ cb, int64_t nval, int64_t ncnt, double Wa,
                                double Wb) {
  const double W = Wa + Wb;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nval; i += stride) {
    const double d = mb[i] - ma[i];
    ma[i] = ma[i] + d * (Wb / W);
    qa[i] = qa[i] + qb[i] + d * d * (Wa * Wb / W);
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ncnt; i += stride) ca[i] += cb[i];
}

}  // namespace

struct ps_summary {
  int device = 0, N = 0, nslot = 0, nthr = 0;
  double thr[PS_SUM_MAX_THR] = {0, 0, 0, 0};
  int64_t ncell = 0, pitch = 0;
  double* mean = nullptr;
  double* m2 = nullptr;
  uint32_t* cnt = nullptr;
  uint64_t W = 0;
  int64_t members = 0;
  hipStream_t stream = nullptr;   // reset / merge / fetch
  PsLastOp last;                  // the summary's last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds
};

static size_t val_bytes(const ps_summary* a) { return (size_t)a->nslot * a->pitch * sizeof(double); }
static size_t cnt_bytes(const ps_summary* a) { return (size_t)a->nslot * a->nthr * a->pitch * sizeof(uint32_t); }

extern "C" void ps_summary_destroy(ps_summary* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  if (a->mean) (void)hipFree(a->mean);
  if (a->m2) (void)hipFree(a->m2);
  if (a->cnt) (void)hipFree(a->cnt);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_summary_reset(ps_summary* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "summary_reset: null summary");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->mean, 0, val_bytes(a), a->stream));
  PS_HIP(hipMemsetAsync(a->m2, 0, val_bytes(a), a->stream));
  if (a->nthr) PS_HIP(hipMemsetAsync(a->cnt, 0, cnt_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  return PS_OK;
}

extern "C" int ps_summary_create(int device, int N, int nslot, int nthr, const double* thr, ps_summary** out) {
  if (!out || N < 1 || nslot < 1 || nthr < 0 || nthr > PS_SUM_MAX_THR || (nthr > 0 && !thr))
    return ps_fail(PS_ERR_BAD_ARG, "summary_create: N %d, %d slots, %d thresholds (at most %d)", N, nslot, nthr,
                   PS_SUM_MAX_THR);
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  ps_summary* a = new ps_summary();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nthr = nthr;
  for (int k = 0; k < nthr; ++k) a->thr[k] = thr[k];
  a->ncell = (int64_t)N * N;
  a->pitch = (a->ncell + 63) / 64 * 64;
  auto fail = [&](int rc) {
    ps_summary_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->mean, val_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->m2, val_bytes(a));
  if (e == hipSuccess && nthr) e = hipMalloc((void**)&a->cnt, cnt_bytes(a));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "summary_create: %s", hipGetErrorString(e)));
  int rc = ps_summary_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// one member from the slot descriptors d (one per slot of the summary), enqueued on `stream`
static int sum_launch(ps_summary* a, const std::vector<PsSrc>& d, hipStream_t stream, double negval,
                      uint32_t weight) {
  const int nslot = a->nslot;
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1;
  PS_TRY(a->prof.begin(0, stream, &e1));
  SumThr thr;
  for (int k = 0; k < PS_SUM_MAX_THR; ++k) thr.t[k] = a->thr[k];
  const double Wn = (double)(a->W + weight);
  const int64_t npair = a->ncell / 2 + 1;
  const int threads = 256;
  const int bx = (int)std::min<int64_t>((npair + threads - 1) / threads, 4096);
  for (int c0 = 0; c0 < nslot; c0 += PS_SUM_CHUNK) {
    const int n = std::min(PS_SUM_CHUNK, nslot - c0);
    SumSlots desc;
    for (int i = 0; i < n; ++i) desc.s[i] = ps_slotted<SumSlot>(d[(size_t)(c0 + i)], c0 + i);
    hipLaunchKernelGGL(k_summary_add, dim3(bx, n), dim3(threads), 0, stream, desc, a->mean, a->m2, a->cnt, a->ncell,
                       a->pitch, a->nthr, thr, negval, (double)weight, Wn, weight);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  return PS_OK;
}

extern "C" int ps_summary_add(ps_summary* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                              const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                              double negval, uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "summary_add: bad arguments");
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "summary_add: %d slots given, the summary has %d", nslot, a->nslot);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "summary_add: weight must be >= 1");
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "summary_add: total weight %llu would overflow the uint32 counts",
                   (unsigned long long)(a->W + weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("summary_add", "summary", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale,
                          use_delta, false, d.data(), &stream));
  return sum_launch(a, d, stream, negval, weight);
}

// one member whose values are the current fields of a projection or a release plan (who: the entry point)
static int sum_add_fields(ps_summary* a, void* h, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(a->W + weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  std::vector<PsSrc> d((size_t)a->nslot);
  PS_TRY(ps_read_fields(who, "summary", "slots", a->device, a->N, a->nslot, h, src, d.data()));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(sum_launch(a, d, a->stream, 0.0, weight));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_summary_add_project(ps_summary* a, ps_project* p, uint32_t weight) {
  return sum_add_fields(a, p, ps_project_fields(), "summary_add_project", weight);
}

extern "C" int ps_summary_add_sites(ps_summary* a, ps_sites* p, uint32_t weight) {
  return sum_add_fields(a, p, ps_sites_fields(), "summary_add_sites", weight);
}

extern "C" int ps_summary_add_peak(ps_summary* a, ps_peak* p, uint32_t weight) {
  return sum_add_fields(a, p, ps_peak_fields(), "summary_add_peak", weight);
}

extern "C" int ps_summary_add_catch(ps_summary* a, ps_catch* p, uint32_t weight) {
  return sum_add_fields(a, p, ps_catch_fields(), "summary_add_catch", weight);
}

extern "C" int ps_summary_add_gain(ps_summary* a, ps_gain* p, uint32_t weight) {
  return sum_add_fields(a, p, ps_gain_fields(), "summary_add_gain", weight);
}

extern "C" int ps_summary_add_nbhd(ps_summary* a, ps_nbhd* p, uint32_t weight) {
  return sum_add_fields(a, p, ps_nbhd_fields(), "summary_add_nbhd", weight);
}

extern "C" int ps_summary_add_prox(ps_summary* a, ps_prox* p, uint32_t weight) {
  return sum_add_fields(a, p, ps_prox_fields(), "summary_add_prox", weight);
}

// the mean planes for ps_gain.hip's finish: nothing is computed or changed here
int ps_summary_mean_internal(ps_summary* a, PsMeanView* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "summary mean view: null handle");
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "nothing accumulated (W = 0): add members to the summary first");
  *out = PsMeanView{a->mean, a->pitch, a->N, a->nslot, a->device};
  return PS_OK;
}
int ps_summary_mean_wait_internal(ps_summary* a, hipStream_t stream) { return a->last.wait(stream); }
int ps_summary_mean_done_internal(ps_summary* a, hipStream_t stream) { return a->last.mark(stream); }

extern "C" int ps_summary_merge(ps_summary* dst, ps_summary* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "summary_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->nthr != src->nthr)
    return ps_fail(PS_ERR_BAD_ARG, "summary_merge: summaries differ in device, domain, slots or thresholds");
  for (int k = 0; k < dst->nthr; ++k)
    if (dst->thr[k] != src->thr[k]) return ps_fail(PS_ERR_BAD_ARG, "summary_merge: threshold %d differs", k);
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "summary_merge: total weight would overflow");
  if (src->W == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  if (dst->W == 0) {   // a copy: the merged summary is src bit for bit
    PS_HIP(hipMemcpyAsync(dst->mean, src->mean, val_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
    PS_HIP(hipMemcpyAsync(dst->m2, src->m2, val_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
    if (dst->nthr) PS_HIP(hipMemcpyAsync(dst->cnt, src->cnt, cnt_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
  } else {
    const int64_t nval = (int64_t)dst->nslot * dst->pitch;
    hipLaunchKernelGGL(k_summary_merge, dim3(2048), dim3(256), 0, dst->stream, dst->mean, dst->m2, dst->cnt, src->mean,
                       src->m2, src->cnt, nval, nval * dst->nthr, (double)dst->W, (double)src->W);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  return PS_OK;
}

extern "C" int ps_summary_info(ps_summary* a, double* total_weight, int64_t* members) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "summary_info: null summary");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  return PS_OK;
}

extern "C" int ps_summary_fetch(ps_summary* a, int slot, int what, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "summary_fetch: bad arguments");
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "summary_fetch: slot %d of %d", slot, a->nslot);
  if (what < 0 || what >= 2 + a->nthr)
    return ps_fail(PS_ERR_BAD_ARG, "summary_fetch: quantity %d (0 mean, 1 variance, 2..%d exceedance)", what, 1 + a->nthr);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "summary_fetch: nothing accumulated (W = 0)");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const double W = (double)a->W;
  const size_t n = (size_t)a->ncell;
  if (what == 0) {
    PS_HIP(hipMemcpyAsync(out, a->mean + (int64_t)slot * a->pitch, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
    PS_HIP(hipStreamSynchronize(a->stream));
  } else if (what == 1) {
    PS_HIP(hipMemcpyAsync(out, a->m2 + (int64_t)slot * a->pitch, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
    PS_HIP(hipStreamSynchronize(a->stream));
    for (size_t i = 0; i < n; ++i) out[i] /= W;
  } else {
    std::vector<uint32_t> c(n);
    const uint32_t* src = a->cnt + ((int64_t)slot * a->nthr + (what - 2)) * a->pitch;
    PS_HIP(hipMemcpyAsync(c.data(), src, n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
    PS_HIP(hipStreamSynchronize(a->stream));
    for (size_t i = 0; i < n; ++i) out[i] = (double)c[i] / W;
  }
  return PS_OK;
}

extern "C" int ps_summary_prof(ps_summary* a, int enable, double* total_ms, int64_t* launches) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "summary_prof: null summary");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  if (total_ms || launches) PS_TRY(a->prof.totals(0, total_ms, launches));
  return PS_OK;
}
