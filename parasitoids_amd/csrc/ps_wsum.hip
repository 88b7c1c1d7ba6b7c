// Reweighted posterior summaries (include/parasitoid_hip.h, ps_wsum_*): per-cell weighted mean, M2 and weighted
// exceedance sums of many model evaluations under up to 4 reweighting scenarios at once, every weight a real
// number the caller supplies per member and scenario (importance weights: run length x likelihood of new
// observations), accumulated on the device from the solver's records, a projection's, a release plan's or a peak
// field.  Layout (pitch = N*N rounded up to 64 cells, every plane 16-byte aligned), one device block, per
// scenario j
//   mean[j][slot][pitch], m2[j][slot][pitch], S[j][slot][k][pitch]       (all fp64)
// An add reads 8 B of record once and, per scenario that takes the member, 8 B of mean of every cell; M2 and the K
// sums (8 + 8 K B) only where a statement can change a bit -- the scenario is rescaled (r != 1), the value differs
// from the mean or reaches the lowest threshold -- which outside the plume, most of the domain, is nowhere.  A pair
// of cells is written back only where a bit changed.
#include <math.h>

#include <vector>

#include "ps_common.h"

#define PS_WSUM_MAX_SCEN 4
#define PS_WSUM_MAX_THR 4
#define PS_WSUM_MAX_SLOT 32   // one launch: 32 descriptors = 1.3 kB of kernel arguments

namespace {

struct WsSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct WsSlots {
  WsSlot s[PS_WSUM_MAX_SLOT];
};
struct WsThr {
  double t[PS_WSUM_MAX_THR];
};
// per scenario: the rescale r, the member's weight omega (0: the scenario is left untouched) and the total
// weight W after this member; the same for every lane, so they stay in scalar registers
struct WsScen {
  double r[PS_WSUM_MAX_SCEN], om[PS_WSUM_MAX_SCEN], W[PS_WSUM_MAX_SCEN];
};

__device__ inline bool ws_differ(double a, double b) { return __double_as_longlong(a) != __double_as_longlong(b); }

// one cell of one scenario; every arithmetic step is a statement of its own (-ffp-contract=on fuses only within
// an expression), sum_update is the statement pair of ps_summary_add
template <int K>
__device__ inline void ws_cell(double v, double r, double om, double W, const WsThr& thr, double& m, double& q,
                               double* s) {
  q = q * r;
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = s[k] * r;
  sum_update(v, om, W, m, q);   // d = v - m; nothing where d == 0
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (v >= thr.t[k]) s[k] = s[k] + om;
}

// blockIdx.y = slot; a thread owns a pair of cells (the tail cell of an odd N*N alone), reads the record once
// and walks the NJ scenarios.  plane = nslot * pitch, jstride = (2 + K) * plane: the distance between two
// scenarios.  NJ and K are template arguments so that the scenario walk and the threshold loops are straight code.
template <int NJ, int K>
__global__ void __launch_bounds__(256) k_wsum_add(WsSlots desc, double* __restrict__ block, int64_t ncell,
                                                  int64_t pitch, int64_t plane, WsThr thr, double negval, WsScen sc) {
  const WsSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double* __restrict__ rec = sd.rec;
  const int64_t jstride = (int64_t)(2 + K) * plane;
  double* ms = block + (int64_t)sd.slot * pitch;
  double* qs = ms + plane;
  double* ss = block + 2 * plane + (int64_t)sd.slot * K * pitch;
  const int64_t npair = ncell >> 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= npair; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < npair) {
      const double2 rr = *reinterpret_cast<const double2*>(rec + 2 * i);
      const double v0 = ps_record_value(rr.x, sd.stat_scale, sd.post_scale, delta, negval);
      const double v1 = ps_record_value(rr.y, sd.stat_scale, sd.post_scale, delta, negval);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (!(sc.om[j] > 0.0)) continue;   // uniform: the member leaves this scenario untouched
        double* mp = ms + j * jstride + 2 * i;
        double* qp = qs + j * jstride + 2 * i;
        double* sp = ss + j * jstride + 2 * i;
        const double2 m0 = *reinterpret_cast<const double2*>(mp);
        // r == 1, v == m and v below every threshold: no statement changes a bit, so M2 and the sums are not read
        if (sc.r[j] == 1.0 && v0 == m0.x && v1 == m0.y && !(K > 0 && (v0 >= thr.t[0] || v1 >= thr.t[0]))) continue;
        const double2 q0 = *reinterpret_cast<const double2*>(qp);
        double2 s0[K ? K : 1];
#pragma unroll
        for (int k = 0; k < K; ++k) s0[k] = *reinterpret_cast<const double2*>(sp + (int64_t)k * pitch);
        double2 m = m0, q = q0;
        double sx[K ? K : 1], sy[K ? K : 1];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          sx[k] = s0[k].x;
          sy[k] = s0[k].y;
        }
        ws_cell<K>(v0, sc.r[j], sc.om[j], sc.W[j], thr, m.x, q.x, sx);
        ws_cell<K>(v1, sc.r[j], sc.om[j], sc.W[j], thr, m.y, q.y, sy);
        if (ws_differ(m.x, m0.x) || ws_differ(m.y, m0.y)) *reinterpret_cast<double2*>(mp) = m;
        if (ws_differ(q.x, q0.x) || ws_differ(q.y, q0.y)) *reinterpret_cast<double2*>(qp) = q;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (ws_differ(sx[k], s0[k].x) || ws_differ(sy[k], s0[k].y))
            *reinterpret_cast<double2*>(sp + (int64_t)k * pitch) = make_double2(sx[k], sy[k]);
      }
    } else if (ncell & 1) {
      const int64_t c = ncell - 1;
      const double v = ps_record_value(rec[c], sd.stat_scale, sd.post_scale, delta, negval);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (!(sc.om[j] > 0.0)) continue;
        double* mp = ms + j * jstride + c;
        double* qp = qs + j * jstride + c;
        double* sp = ss + j * jstride + c;
        const double m0 = *mp;
        if (sc.r[j] == 1.0 && v == m0 && !(K > 0 && v >= thr.t[0])) continue;
        const double q0 = *qp;
        double m = m0, q = q0;
        double s0[K ? K : 1], s[K ? K : 1];
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = s0[k] = sp[(int64_t)k * pitch];
        ws_cell<K>(v, sc.r[j], sc.om[j], sc.W[j], thr, m, q, s);
        if (ws_differ(m, m0)) *mp = m;
        if (ws_differ(q, q0)) *qp = q;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (ws_differ(s[k], s0[k])) sp[(int64_t)k * pitch] = s[k];
      }
    }
  }
}

using WsAddKernel = void (*)(WsSlots, double*, int64_t, int64_t, int64_t, WsThr, double, WsScen);
#define WS_ROW(J) {k_wsum_add<J, 0>, k_wsum_add<J, 1>, k_wsum_add<J, 2>, k_wsum_add<J, 3>, k_wsum_add<J, 4>}
// k_wsum_add<nscen, nthr>, nscen = 1 .. 4, nthr = 0 .. 4
const WsAddKernel ws_add_kernels[PS_WSUM_MAX_SCEN][PS_WSUM_MAX_THR + 1] = {WS_ROW(1), WS_ROW(2), WS_ROW(3), WS_ROW(4)};

// Chan, Golub & LeVeque on one scenario, both sides brought to a common scale by ra and rb:
// Wa = Wa0 ra, Wb = Wb0 rb (from the host).  nval cells of mean and M2, nsum of the exceedance sums.
__global__ void __launch_bounds__(256) k_wsum_merge(double* __restrict__ ma, double* __restrict__ qa,
                                                    double* __restrict__ sa, const double* __restrict__ mb,
                                                    const double* __restrict__ qb, const double* __restrict__ sb,
                                                    int64_t nval, int64_t nsum, double ra, double rb, double Wa,
                                                    double Wb) {
  const double W = Wa + Wb;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nval; i += stride) {
    const double d = mb[i] - ma[i];
    ma[i] = ma[i] + d * (Wb / W);
    qa[i] = qa[i] * ra + qb[i] * rb + d * d * (Wa * Wb / W);
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nsum; i += stride)
    sa[i] = sa[i] * ra + sb[i] * rb;
}

}  // namespace

struct ps_wsum {
  int device = 0, N = 0, nscen = 0, nslot = 0, nthr = 0;
  double thr[PS_WSUM_MAX_THR] = {0, 0, 0, 0};
  int64_t ncell = 0, pitch = 0;
  double* block = nullptr;   // per scenario: mean | M2 | S
  double W[PS_WSUM_MAX_SCEN] = {0, 0, 0, 0};
  int64_t members[PS_WSUM_MAX_SCEN] = {0, 0, 0, 0};
  int64_t skipped[PS_WSUM_MAX_SCEN] = {0, 0, 0, 0};
  hipStream_t stream = nullptr;   // reset / merge / fetch, and the adds from fields
  PsLastOp last;                  // the last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds
};

static int64_t ws_plane(const ps_wsum* a) { return (int64_t)a->nslot * a->pitch; }
static int64_t ws_scen_cells(const ps_wsum* a) { return (int64_t)(2 + a->nthr) * ws_plane(a); }
static double ws_block_bytes(int nscen, int nslot, int nthr, int64_t pitch) {
  return (double)nscen * (double)(2 + nthr) * (double)nslot * (double)pitch * sizeof(double);
}
static double* ws_mean(const ps_wsum* a, int j) { return a->block + (int64_t)j * ws_scen_cells(a); }
static double* ws_m2(const ps_wsum* a, int j) { return ws_mean(a, j) + ws_plane(a); }
static double* ws_S(const ps_wsum* a, int j) { return ws_mean(a, j) + 2 * ws_plane(a); }

static bool ws_finite(double v) { return v == v && !isinf(v); }

extern "C" void ps_wsum_destroy(ps_wsum* a) {
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

extern "C" int ps_wsum_reset(ps_wsum* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "wsum_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->block, 0, (size_t)ws_block_bytes(a->nscen, a->nslot, a->nthr, a->pitch), a->stream));
  PS_TRY(a->last.mark(a->stream));
  for (int j = 0; j < PS_WSUM_MAX_SCEN; ++j) {
    a->W[j] = 0.0;
    a->members[j] = 0;
    a->skipped[j] = 0;
  }
  return PS_OK;
}

extern "C" int ps_wsum_create(int device, int N, int nscen, int nslot, int nthr, const double* thr, ps_wsum** out) {
  if (!out || N < 1 || nscen < 1 || nscen > PS_WSUM_MAX_SCEN || nslot < 1 || nslot > PS_WSUM_MAX_SLOT || nthr < 0 ||
      nthr > PS_WSUM_MAX_THR || (nthr > 0 && !thr))
    return ps_fail(PS_ERR_BAD_ARG, "wsum_create: N %d, %d scenarios (1..%d), %d slots (1..%d), %d thresholds (0..%d)", N,
                   nscen, PS_WSUM_MAX_SCEN, nslot, PS_WSUM_MAX_SLOT, nthr, PS_WSUM_MAX_THR);
  *out = nullptr;
  for (int k = 0; k < nthr; ++k) {
    if (!ws_finite(thr[k]) || !(thr[k] > 0.0))
      return ps_fail(PS_ERR_BAD_ARG, "wsum_create: threshold %d is not finite and > 0", k);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "wsum_create: the thresholds are not strictly increasing at %d", k);
  }
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // the whole block, checked before anything is allocated
  const double need = ws_block_bytes(nscen, nslot, nthr, pitch);
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "wsum_create: %d scenarios x (2 + %d) x 8 B x %d slots x %lld cells = %.3g GB, %.3g GB free",
                   nscen, nthr, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_wsum* a = new ps_wsum();
  a->device = device;
  a->N = N;
  a->nscen = nscen;
  a->nslot = nslot;
  a->nthr = nthr;
  for (int k = 0; k < nthr; ++k) a->thr[k] = thr[k];
  a->ncell = ncell;
  a->pitch = pitch;
  auto fail = [&](int rc) {
    ps_wsum_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->block, (size_t)need);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "wsum_create: %s", hipGetErrorString(e)));
  int rc = ps_wsum_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// what every add checks before it resolves a descriptor (who: the entry point)
static int ws_check_add(ps_wsum* a, const char* who, int nscen, const double* rescale, const double* omega) {
  if (!a || !rescale || !omega) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (nscen != a->nscen) return ps_fail(PS_ERR_BAD_ARG, "%s: %d scenarios given, the handle has %d", who, nscen, a->nscen);
  for (int j = 0; j < nscen; ++j) {
    if (!(rescale[j] >= 0.0 && rescale[j] <= 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "%s: rescale[%d] = %g is not in [0, 1]", who, j, rescale[j]);
    if (!ws_finite(omega[j]) || omega[j] < 0.0)
      return ps_fail(PS_ERR_BAD_ARG, "%s: omega[%d] = %g is not finite and >= 0", who, j, omega[j]);
  }
  return PS_OK;
}

// one member from the slot descriptors d (one per slot of the handle), enqueued on `stream`
static int ws_launch(ps_wsum* a, const std::vector<PsSrc>& d, hipStream_t stream, double negval, const double* rescale,
                     const double* omega) {
  WsScen sc;
  bool any = false;
  for (int j = 0; j < PS_WSUM_MAX_SCEN; ++j) {
    sc.r[j] = 1.0;
    sc.om[j] = 0.0;
    sc.W[j] = 0.0;
    if (j < a->nscen && omega[j] > 0.0) {
      double W = a->W[j];
      W = W * rescale[j];
      W = W + omega[j];
      sc.r[j] = rescale[j];
      sc.om[j] = omega[j];
      sc.W[j] = W;
      any = true;
    }
  }
  if (any) {
    PS_TRY(a->last.wait(stream));
    hipEvent_t e1 = nullptr;
    PS_TRY(a->prof.begin(0, stream, &e1));
    WsThr thr;
    for (int k = 0; k < PS_WSUM_MAX_THR; ++k) thr.t[k] = a->thr[k];
    WsSlots desc;
    for (int i = 0; i < PS_WSUM_MAX_SLOT; ++i) {   // the unused tail repeats the last slot
      const int q = std::min(i, a->nslot - 1);
      desc.s[i] = ps_slotted<WsSlot>(d[(size_t)q], q);
    }
    const int64_t npair = a->ncell / 2 + 1;
    const int threads = 256;
    const int bx = (int)std::min<int64_t>((npair + threads - 1) / threads, 4096);
    hipLaunchKernelGGL(ws_add_kernels[a->nscen - 1][a->nthr], dim3(bx, a->nslot), dim3(threads), 0, stream, desc,
                       a->block, a->ncell, a->pitch, ws_plane(a), thr, negval, sc);
    PS_HIP(hipGetLastError());
    PS_TRY(a->prof.end(stream, e1));
    PS_TRY(a->last.mark(stream));
  }
  for (int j = 0; j < a->nscen; ++j) {
    if (omega[j] > 0.0) {
      a->W[j] = sc.W[j];
      a->members[j] += 1;
    } else {
      a->skipped[j] += 1;
    }
  }
  return PS_OK;
}

extern "C" int ps_wsum_add(ps_wsum* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                           const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                           int nscen, const double* rescale, const double* omega) {
  if (!s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "wsum_add: bad arguments");
  PS_TRY(ws_check_add(a, "wsum_add", nscen, rescale, omega));
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "wsum_add: %d slots given, the handle has %d", nslot, a->nslot);
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("wsum_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, d.data(), &stream));
  return ws_launch(a, d, stream, negval, rescale, omega);
}

// one member whose values are the current fields of a projection, a release plan or a peak (who: the entry point)
static int ws_add_fields(ps_wsum* a, void* h, const PsFieldsOps& src, const char* who, int nscen, const double* rescale,
                         const double* omega) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(ws_check_add(a, who, nscen, rescale, omega));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  std::vector<PsSrc> d((size_t)a->nslot);
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, d.data()));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(ws_launch(a, d, a->stream, 0.0, rescale, omega));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_wsum_add_project(ps_wsum* a, ps_project* p, int nscen, const double* rescale, const double* omega) {
  return ws_add_fields(a, p, ps_project_fields(), "wsum_add_project", nscen, rescale, omega);
}

extern "C" int ps_wsum_add_sites(ps_wsum* a, ps_sites* p, int nscen, const double* rescale, const double* omega) {
  return ws_add_fields(a, p, ps_sites_fields(), "wsum_add_sites", nscen, rescale, omega);
}

extern "C" int ps_wsum_add_peak(ps_wsum* a, ps_peak* p, int nscen, const double* rescale, const double* omega) {
  return ws_add_fields(a, p, ps_peak_fields(), "wsum_add_peak", nscen, rescale, omega);
}

extern "C" int ps_wsum_add_catch(ps_wsum* a, ps_catch* p, int nscen, const double* rescale, const double* omega) {
  return ws_add_fields(a, p, ps_catch_fields(), "wsum_add_catch", nscen, rescale, omega);
}

extern "C" int ps_wsum_add_gain(ps_wsum* a, ps_gain* p, int nscen, const double* rescale, const double* omega) {
  return ws_add_fields(a, p, ps_gain_fields(), "wsum_add_gain", nscen, rescale, omega);
}

extern "C" int ps_wsum_add_nbhd(ps_wsum* a, ps_nbhd* p, int nscen, const double* rescale, const double* omega) {
  return ws_add_fields(a, p, ps_nbhd_fields(), "wsum_add_nbhd", nscen, rescale, omega);
}

extern "C" int ps_wsum_add_prox(ps_wsum* a, ps_prox* p, int nscen, const double* rescale, const double* omega) {
  return ws_add_fields(a, p, ps_prox_fields(), "wsum_add_prox", nscen, rescale, omega);
}

// one scenario's mean planes for ps_gain.hip's finish: nothing is computed or changed here
int ps_wsum_mean_internal(ps_wsum* a, int scenario, PsMeanView* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "wsum mean view: null handle");
  if (scenario < 0 || scenario >= a->nscen)
    return ps_fail(PS_ERR_BAD_ARG, "wsum mean view: scenario %d of %d", scenario, a->nscen);
  if (a->W[scenario] == 0.0)
    return ps_fail(PS_ERR_STATE, "nothing accumulated in scenario %d (W = 0): add members first", scenario);
  *out = PsMeanView{ws_mean(a, scenario), a->pitch, a->N, a->nslot, a->device};
  return PS_OK;
}
int ps_wsum_mean_wait_internal(ps_wsum* a, hipStream_t stream) { return a->last.wait(stream); }
int ps_wsum_mean_done_internal(ps_wsum* a, hipStream_t stream) { return a->last.mark(stream); }

extern "C" int ps_wsum_merge(ps_wsum* dst, ps_wsum* src, const double* ra, const double* rb) {
  if (!dst || !src || !ra || !rb) return ps_fail(PS_ERR_BAD_ARG, "wsum_merge: bad arguments");
  if (dst == src) return ps_fail(PS_ERR_BAD_ARG, "wsum_merge: dst and src are the same handle");
  if (dst->device != src->device || dst->N != src->N || dst->nscen != src->nscen || dst->nslot != src->nslot ||
      dst->nthr != src->nthr)
    return ps_fail(PS_ERR_BAD_ARG, "wsum_merge: handles differ in device, domain, scenarios, slots or thresholds");
  for (int k = 0; k < dst->nthr; ++k)
    if (dst->thr[k] != src->thr[k]) return ps_fail(PS_ERR_BAD_ARG, "wsum_merge: threshold %d differs", k);
  for (int j = 0; j < dst->nscen; ++j)
    if (!(ra[j] >= 0.0 && ra[j] <= 1.0) || !(rb[j] >= 0.0 && rb[j] <= 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "wsum_merge: scale (%g, %g) of scenario %d is not in [0, 1]", ra[j], rb[j], j);
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  const int64_t nval = ws_plane(dst);
  const size_t scen_bytes = (size_t)ws_scen_cells(dst) * sizeof(double);
  for (int j = 0; j < dst->nscen; ++j) {
    if (src->W[j] == 0.0) {
      dst->skipped[j] += src->skipped[j];
      continue;
    }
    if (dst->W[j] == 0.0) {   // a copy: the merged scenario is src's bit for bit
      PS_HIP(hipMemcpyAsync(ws_mean(dst, j), ws_mean(src, j), scen_bytes, hipMemcpyDeviceToDevice, dst->stream));
      dst->W[j] = src->W[j];
    } else {
      double Wa = dst->W[j];
      Wa = Wa * ra[j];
      double Wb = src->W[j];
      Wb = Wb * rb[j];
      hipLaunchKernelGGL(k_wsum_merge, dim3(2048), dim3(256), 0, dst->stream, ws_mean(dst, j), ws_m2(dst, j),
                         ws_S(dst, j), ws_mean(src, j), ws_m2(src, j), ws_S(src, j), nval, nval * dst->nthr, ra[j],
                         rb[j], Wa, Wb);
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

extern "C" int ps_wsum_info(ps_wsum* a, double* total_weight, int64_t* members, int64_t* skipped) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "wsum_info: null handle");
  for (int j = 0; j < a->nscen; ++j) {
    if (total_weight) total_weight[j] = a->W[j];
    if (members) members[j] = a->members[j];
    if (skipped) skipped[j] = a->skipped[j];
  }
  return PS_OK;
}

extern "C" int ps_wsum_fetch(ps_wsum* a, int scen, int slot, int what, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "wsum_fetch: bad arguments");
  if (scen < 0 || scen >= a->nscen) return ps_fail(PS_ERR_BAD_ARG, "wsum_fetch: scenario %d of %d", scen, a->nscen);
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "wsum_fetch: slot %d of %d", slot, a->nslot);
  if (what < 0 || what >= 2 + a->nthr)
    return ps_fail(PS_ERR_BAD_ARG, "wsum_fetch: quantity %d (0 mean, 1 variance, 2..%d exceedance)", what, 1 + a->nthr);
  if (a->W[scen] == 0.0) return ps_fail(PS_ERR_STATE, "wsum_fetch: nothing accumulated in scenario %d (W = 0)", scen);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const double W = a->W[scen];
  const size_t n = (size_t)a->ncell;
  const double* src = what == 0   ? ws_mean(a, scen) + (int64_t)slot * a->pitch
                      : what == 1 ? ws_m2(a, scen) + (int64_t)slot * a->pitch
                                  : ws_S(a, scen) + ((int64_t)slot * a->nthr + (what - 2)) * a->pitch;
  PS_HIP(hipMemcpyAsync(out, src, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  if (what == 1) {
    for (size_t i = 0; i < n; ++i) out[i] /= W;
  } else if (what >= 2) {
    for (size_t i = 0; i < n; ++i) {
      const double p = out[i] / W;
      out[i] = p < 1.0 ? p : 1.0;
    }
  }
  return PS_OK;
}

extern "C" int ps_wsum_prof(ps_wsum* a, int enable, double* total_ms, int64_t* launches) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "wsum_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  if (total_ms || launches) PS_TRY(a->prof.totals(0, total_ms, launches));
  return PS_OK;
}
