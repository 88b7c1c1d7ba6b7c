// Trap information fields (include/parasitoid_hip.h, ps_gain_*): one member's whole count distribution at every
// cell for traps the user describes, and from the accumulated means the mutual information between a trap's count
// and the identity of the member.  Trap e = (input[e], rate[e], ymax[e]) observes the classes 0, 1, .., ymax and
// ">= ymax + 1" of Poisson(rate_e * v), v the value of input record input[e] at the cell -- the one ps_summary_add
// adds (ps_record_value) -- or output input[e] of another fields source.  Layout (pitch = N*N rounded up to 64
// cells, as ps_summary.hip):
//   Y[plane][pitch]    fp64, trap e owns the ymax[e] + 3 planes from base[e] on: d0 = 1 - P(0), p_1 .. p_ymax, the
//                      tail P(>= ymax + 1) and h, the entropy of the member's class distribution in nats;
//                      overwritten by every apply, zeros included
//   R[3 e + k][pitch]  fp64, the maps of the last finish: k = 0 gain, 1 entropy, 2 conditional
// The traps are grouped by input at create (GainTab, a kernel argument): one thread owns a pair of cells, reads each
// used record once and walks the group's traps.  A pair whose two values are zero -- most of the domain -- stores
// the group's zeros and never enters the transcendental path.  The value of a cell depends on its own (mu, ymax)
// alone (the statements are in the header): no atomics, no LDS, one writer per cell, the same call gives the same
// bits whatever the launch shape.
#include <math.h>

#include <utility>
#include <vector>

#include "ps_catch_value.h"   // catch_value: the tail class, the bits of ps_catch.hip
#include "ps_common.h"

#define PS_GAIN_MAX_IN 32      // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_GAIN_MAX_PLANE 32   // the slots of one accumulator
#define PS_GAIN_MAX_TRAP 10    // every trap owns at least 3 planes
#define PS_GAIN_MAX_YMAX 15    // the tail class is catch_value(mu, ymax + 1), stated for counts up to 16
#define PS_GAIN_THREADS 256

namespace {

struct GainSlots {
  PsSrc s[PS_GAIN_MAX_IN];
};
// the traps in group order: group g reads input gin[g] and owns the entries gstart[g] .. gstart[g + 1] - 1
struct GainTab {
  double rate[PS_GAIN_MAX_TRAP];
  int ymax[PS_GAIN_MAX_TRAP];
  int base[PS_GAIN_MAX_TRAP];     // the first plane an entry writes
  int gin[PS_GAIN_MAX_TRAP];
  int gstart[PS_GAIN_MAX_TRAP + 1];
  int ngroup;
};
// the traps in the caller's order, for the finish
struct GainPlan {
  int ymax[PS_GAIN_MAX_TRAP];
  int base[PS_GAIN_MAX_TRAP];
  int ntrap, pad_;
};

// the running state of one cell of one trap; every arithmetic step below is a statement of its own (one rounding
// each), as the header states them and tests/gain_ref.py repeats them
struct GainCell {
  double mu, t, h;
  bool live;   // 0 < mu < 800: the transcendental path
  bool sure;   // mu >= 800: the count is in the tail class with probability 1
};

// d0 of the cell, and the state the classes 1 .. ymax continue from
__device__ inline double gain_first(double mu, GainCell& c) {
  c.mu = mu;
  c.t = 0.0;
  c.h = 0.0;
  c.live = false;
  c.sure = false;
  if (!(mu > 0.0)) return 0.0;
  if (mu >= PS_CATCH_SURE) {
    c.sure = true;
    return 1.0;
  }
  c.live = true;
  const double nm = -mu;
  const double x = expm1(nm);
  const double e = exp(nm);
  c.h = e * mu;
  c.t = e;
  return -x;
}

// p_y, y = 1 .. ymax in turn
__device__ inline double gain_class(GainCell& c, int y) {
  if (!c.live) return 0.0;
  c.t = c.t * c.mu;
  c.t = c.t / (double)y;
  if (c.t > 0.0) {
    const double l = log(c.t);
    const double x = c.t * l;
    c.h = c.h - x;
  }
  return c.t;
}

// the tail class; c.h is complete after it
__device__ inline double gain_tail(GainCell& c, int ymax) {
  if (c.sure) return 1.0;
  if (!c.live) return 0.0;
  const double q = catch_value(c.mu, ymax + 1);
  if (q > 0.0) {
    const double l = log(q);
    const double x = q * l;
    c.h = c.h - x;
  }
  return q;
}

// thread j owns the cells 2j, 2j + 1 (j == npair: the tail cell of an odd N*N alone)
__global__ void __launch_bounds__(PS_GAIN_THREADS) k_gain_apply(GainSlots desc, GainTab tab, double* __restrict__ Y,
                                                                int64_t ncell, int64_t pitch, double negval) {
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pair = j < npair, tail = j == npair && (ncell & 1);
  if (!(pair || tail)) return;
  const int64_t i = pair ? 2 * j : ncell - 1;
  for (int g = 0; g < tab.ngroup; ++g) {
    const int d = tab.gin[g];
    const double* __restrict__ rec = desc.s[d].rec;
    const ps_day_stats* st = desc.s[d].stats;
    const double ss = desc.s[d].stat_scale, ps = desc.s[d].post_scale;
    const double delta = st ? st->delta : 0.0;
    double2 r;
    if (pair)
      r = *reinterpret_cast<const double2*>(rec + i);
    else
      r = make_double2(rec[i], 0.0);
    const double v0 = ps_record_value(r.x, ss, ps, delta, negval);
    const double v1 = pair ? ps_record_value(r.y, ss, ps, delta, negval) : 0.0;
    const int q0 = tab.gstart[g], q1 = tab.gstart[g + 1];
    const bool live = v0 != 0.0 || v1 != 0.0;
    for (int q = q0; q < q1; ++q) {
      const int ymax = tab.ymax[q];
      double* y = Y + (int64_t)tab.base[q] * pitch + i;
      if (!live) {   // the trap's ymax + 3 planes of zeros
        for (int k = 0; k < ymax + 3; ++k, y += pitch) {
          if (pair)
            *reinterpret_cast<double2*>(y) = make_double2(0.0, 0.0);
          else
            *y = 0.0;
        }
        continue;
      }
      const double rate = tab.rate[q];
      const double mu0 = rate * v0;
      const double mu1 = rate * v1;
      GainCell c0, c1;
      double a0 = gain_first(mu0, c0);
      double a1 = gain_first(mu1, c1);
      for (int k = 0;; ++k, y += pitch) {   // plane k: d0, p_1 .. p_ymax, the tail, h
        if (pair)
          *reinterpret_cast<double2*>(y) = make_double2(a0, a1);
        else
          *y = a0;
        if (k == ymax + 2) break;
        if (k < ymax) {
          a0 = gain_class(c0, k + 1);
          a1 = gain_class(c1, k + 1);
        } else if (k == ymax) {
          a0 = gain_tail(c0, ymax);
          a1 = gain_tail(c1, ymax);
        } else {
          a0 = c0.h;
          a1 = c1.h;
        }
      }
    }
  }
}

// one cell of one trap from the accumulator's mean planes m (stride pitch): gain, entropy, conditional
__global__ void __launch_bounds__(PS_GAIN_THREADS) k_gain_finish(GainPlan plan, const double* __restrict__ m,
                                                                 int64_t mpitch, double* __restrict__ R, int64_t ncell,
                                                                 int64_t pitch) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  for (int e = 0; e < plan.ntrap; ++e) {
    const int ymax = plan.ymax[e];
    const double* me = m + (int64_t)plan.base[e] * mpitch + i;
    const double m0 = me[0];
    double P = 1.0 - m0;
    double HY = 0.0;
    for (int k = 0;; ++k) {   // P0, m_1 .. m_{ymax + 1}
      if (P > 0.0) {
        const double l = log(P);
        const double x = P * l;
        HY = HY - x;
      }
      if (k == ymax + 1) break;
      P = me[(int64_t)(k + 1) * mpitch];
    }
    const double HYM = me[(int64_t)(ymax + 2) * mpitch];
    double G = HY - HYM;
    if (!(G > 0.0)) G = 0.0;
    double* re = R + (int64_t)(3 * e) * pitch + i;
    re[0] = G;
    re[pitch] = HY;
    re[2 * pitch] = HYM;
  }
}

// out[p][k] = Y_p(cell[k]); flat over nplane * n
__global__ void k_gain_gather(const double* __restrict__ Y, int64_t pitch, int nplane, int64_t n,
                              const int64_t* __restrict__ cell, double* __restrict__ out) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * nplane) return;
  const int64_t e = t / n, k = t - e * n;
  out[t] = Y[e * pitch + cell[k]];
}

}  // namespace

struct ps_gain {
  int device = 0, N = 0, nin = 0, ntrap = 0, nplane = 0;
  int64_t ncell = 0, pitch = 0;
  int nblk = 0;                    // blocks of one apply launch
  GainTab tab;
  GainPlan plan;
  double* Y = nullptr;             // [nplane][pitch]
  double* R = nullptr;             // [3 ntrap][pitch]
  int64_t* g_cell = nullptr;       // gather scratch, grown on demand
  double* g_out = nullptr;
  int64_t g_cap = 0;
  int64_t applies = 0, finishes = 0;
  hipStream_t stream = nullptr;    // fetch / gather / finish / apply of another fields source
  PsLastOp last;                   // the last operation on Y or R, on whatever stream it ran
  PsProf prof;                     // channel 0: the applies
};

extern "C" void ps_gain_destroy(ps_gain* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->last.sync();
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->prof.release();
  for (void* q : {(void*)c->Y, (void*)c->R, (void*)c->g_cell, (void*)c->g_out})
    if (q) (void)hipFree(q);
  c->last.destroy();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int ps_gain_create(int device, int N, int nin, int ntrap, const int32_t* input, const double* rate,
                              const int32_t* ymax, ps_gain** out) {
  if (!out || N < 1 || nin < 1 || nin > PS_GAIN_MAX_IN || ntrap < 1 || !input || !rate || !ymax)
    return ps_fail(PS_ERR_BAD_ARG, "gain_create: N %d, %d inputs (1..%d), %d traps (at least 1)", N, nin, PS_GAIN_MAX_IN,
                   ntrap);
  int64_t nplane = 0;
  for (int e = 0; e < ntrap; ++e) {
    if (input[e] < 0 || input[e] >= nin)
      return ps_fail(PS_ERR_BAD_ARG, "gain_create: trap %d reads input %d of %d", e, input[e], nin);
    if (!isfinite(rate[e]) || !(rate[e] > 0.0))
      return ps_fail(PS_ERR_BAD_ARG, "gain_create: rate [%d] = %g is not finite and > 0", e, rate[e]);
    if (ymax[e] < 0 || ymax[e] > PS_GAIN_MAX_YMAX)
      return ps_fail(PS_ERR_BAD_ARG, "gain_create: ymax [%d] = %d is not in 0..%d", e, ymax[e], PS_GAIN_MAX_YMAX);
    nplane += ymax[e] + 3;
    if (nplane > PS_GAIN_MAX_PLANE)
      return ps_fail(PS_ERR_BAD_ARG, "gain_create: the traps up to %d own %lld planes (ymax + 3 each), at most %d", e,
                     (long long)nplane, PS_GAIN_MAX_PLANE);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  const int64_t nblk = (ncell / 2 + 1 + PS_GAIN_THREADS - 1) / PS_GAIN_THREADS;   // the pairs and the tail thread
  if (2 * nblk > 0x7fffffffLL) return ps_fail(PS_ERR_BAD_ARG, "gain_create: N %d is too large for one launch", N);
  // the planes and the three maps per trap, checked before anything is allocated
  const double need = (double)(nplane + 3 * ntrap) * pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "gain_create: (%lld planes + 3 x %d maps) x %lld cells x 8 B = %.3g GB, %.3g GB free",
                   (long long)nplane, ntrap, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_gain* c = new ps_gain();
  c->device = device;
  c->N = N;
  c->nin = nin;
  c->ntrap = ntrap;
  c->nplane = (int)nplane;
  c->ncell = ncell;
  c->pitch = pitch;
  c->nblk = (int)nblk;
  GainPlan& plan = c->plan;
  plan = GainPlan();
  plan.ntrap = ntrap;
  int base = 0;
  for (int e = 0; e < ntrap; ++e) {
    plan.ymax[e] = ymax[e];
    plan.base[e] = base;
    base += ymax[e] + 3;
  }
  GainTab& tab = c->tab;
  tab = GainTab();
  int q = 0;
  for (int d = 0; d < nin; ++d) {   // ascending input, the traps of one input in ascending e
    const int q0 = q;
    for (int e = 0; e < ntrap; ++e) {
      if (input[e] != d) continue;
      tab.rate[q] = rate[e];
      tab.ymax[q] = ymax[e];
      tab.base[q] = plan.base[e];
      ++q;
    }
    if (q == q0) continue;
    tab.gin[tab.ngroup] = d;
    tab.gstart[tab.ngroup] = q0;
    tab.gstart[++tab.ngroup] = q;
  }
  auto fail = [&](int rc) {
    ps_gain_destroy(c);
    return rc;
  };
  const size_t y_b = (size_t)nplane * pitch * sizeof(double);
  const size_t r_b = (size_t)3 * ntrap * pitch * sizeof(double);
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = c->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&c->Y, y_b);
  if (e == hipSuccess) e = hipMalloc((void**)&c->R, r_b);
  if (e == hipSuccess) e = hipMemsetAsync(c->Y, 0, y_b, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->R, 0, r_b, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "gain_create: %s", hipGetErrorString(e)));
  *out = c;
  return PS_OK;
}

// one launch over the resolved descriptors on `stream`, behind the handle's last operation
static int gain_launch(ps_gain* c, const GainSlots& desc, hipStream_t stream, double negval) {
  PS_TRY(c->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(c->prof.begin(0, stream, &e1));
  hipLaunchKernelGGL(k_gain_apply, dim3(c->nblk), dim3(PS_GAIN_THREADS), 0, stream, desc, c->tab, c->Y, c->ncell,
                     c->pitch, negval);
  PS_HIP(hipGetLastError());
  PS_TRY(c->prof.end(stream, e1));
  PS_TRY(c->last.mark(stream));
  c->applies += 1;
  return PS_OK;
}

extern "C" int ps_gain_apply(ps_gain* c, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                             const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                             double negval) {
  if (!c || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "gain_apply: bad arguments");
  if (nin != c->nin) return ps_fail(PS_ERR_BAD_ARG, "gain_apply: %d inputs given, the handle has %d", nin, c->nin);
  PS_HIP(hipSetDevice(c->device));
  // every descriptor first: an apply with a bad record enqueues nothing
  GainSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("gain_apply", "handle", c->device, c->N, s, nin, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nin; i < PS_GAIN_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return gain_launch(c, desc, stream, negval);
}

// the inputs are the current fields of a projection or a release plan (who: the entry point): input i is the
// source's output i, on the handle's stream behind the source's last operation
static int gain_apply_fields(ps_gain* c, void* h, const PsFieldsOps& src, const char* who) {
  if (!c || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  // input i takes Y_i: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  GainSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "inputs", c->device, c->N, c->nin, h, src, desc.s));
  for (int i = c->nin; i < PS_GAIN_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(src.wait(h, c->stream));
  PS_TRY(gain_launch(c, desc, c->stream, 0.0));
  return src.mark(h, c->stream);   // the source's next apply overwrites its fields only after this read
}

extern "C" int ps_gain_apply_project(ps_gain* c, ps_project* p) {
  return gain_apply_fields(c, p, ps_project_fields(), "gain_apply_project");
}

extern "C" int ps_gain_apply_sites(ps_gain* c, ps_sites* p) {
  return gain_apply_fields(c, p, ps_sites_fields(), "gain_apply_sites");
}

// the three maps of every trap from an accumulator's mean planes: the view is checked before anything is ordered,
// the launch runs on the handle's stream
static int gain_finish_check(ps_gain* c, const PsMeanView& v, const char* who) {
  if (v.nslot != c->nplane)
    return ps_fail(PS_ERR_BAD_ARG, "%s: the accumulator has %d slots, the handle %d planes", who, v.nslot, c->nplane);
  if (v.device != c->device)
    return ps_fail(PS_ERR_BAD_ARG, "%s: accumulator on device %d, handle on device %d", who, v.device, c->device);
  if (v.N != c->N) return ps_fail(PS_ERR_BAD_ARG, "%s: accumulator domain %d, handle domain %d", who, v.N, c->N);
  return PS_OK;
}
static int gain_finish_launch(ps_gain* c, const PsMeanView& v) {
  PS_TRY(c->last.wait(c->stream));
  const unsigned nb = (unsigned)((c->ncell + PS_GAIN_THREADS - 1) / PS_GAIN_THREADS);
  hipLaunchKernelGGL(k_gain_finish, dim3(nb), dim3(PS_GAIN_THREADS), 0, c->stream, c->plan, v.mean, v.pitch, c->R,
                     c->ncell, c->pitch);
  PS_HIP(hipGetLastError());
  PS_TRY(c->last.mark(c->stream));
  c->finishes += 1;
  return PS_OK;
}

// behind the accumulator's last operation; its next operation waits for the read
extern "C" int ps_gain_finish_summary(ps_gain* c, ps_summary* a) {
  if (!c || !a) return ps_fail(PS_ERR_BAD_ARG, "gain_finish_summary: bad arguments");
  PsMeanView v;
  PS_TRY(ps_summary_mean_internal(a, &v));
  PS_TRY(gain_finish_check(c, v, "gain_finish_summary"));
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(ps_summary_mean_wait_internal(a, c->stream));
  PS_TRY(gain_finish_launch(c, v));
  return ps_summary_mean_done_internal(a, c->stream);
}

extern "C" int ps_gain_finish_wsum(ps_gain* c, ps_wsum* a, int scenario) {
  if (!c || !a) return ps_fail(PS_ERR_BAD_ARG, "gain_finish_wsum: bad arguments");
  PsMeanView v;
  PS_TRY(ps_wsum_mean_internal(a, scenario, &v));
  PS_TRY(gain_finish_check(c, v, "gain_finish_wsum"));
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(ps_wsum_mean_wait_internal(a, c->stream));
  PS_TRY(gain_finish_launch(c, v));
  return ps_wsum_mean_done_internal(a, c->stream);
}

static int gain_copy_out(ps_gain* c, const double* src, double* out) {
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(c->last.wait(c->stream));
  PS_HIP(hipMemcpyAsync(out, src, (size_t)c->ncell * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PS_HIP(hipStreamSynchronize(c->stream));
  return PS_OK;
}

extern "C" int ps_gain_fetch(ps_gain* c, int plane, double* out) {
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "gain_fetch: bad arguments");
  if (plane < 0 || plane >= c->nplane) return ps_fail(PS_ERR_BAD_ARG, "gain_fetch: plane %d of %d", plane, c->nplane);
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "gain_fetch: nothing applied yet");
  return gain_copy_out(c, c->Y + (int64_t)plane * c->pitch, out);
}

extern "C" int ps_gain_fetch_result(ps_gain* c, int trap, int what, double* out) {
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "gain_fetch_result: bad arguments");
  if (trap < 0 || trap >= c->ntrap) return ps_fail(PS_ERR_BAD_ARG, "gain_fetch_result: trap %d of %d", trap, c->ntrap);
  if (what < 0 || what > 2)
    return ps_fail(PS_ERR_BAD_ARG, "gain_fetch_result: quantity %d (0 gain, 1 entropy, 2 conditional)", what);
  if (c->finishes == 0) return ps_fail(PS_ERR_STATE, "gain_fetch_result: nothing finished yet");
  return gain_copy_out(c, c->R + (int64_t)(3 * trap + what) * c->pitch, out);
}

extern "C" int ps_gain_gather(ps_gain* c, int64_t n, const int32_t* rows, const int32_t* cols, double* out) {
  if (!c || n < 0 || (n > 0 && (!rows || !cols || !out))) return ps_fail(PS_ERR_BAD_ARG, "gain_gather: bad arguments");
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "gain_gather: nothing applied yet");
  if (n == 0) return PS_OK;
  std::vector<int64_t> cell((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    if (rows[k] < 0 || rows[k] >= c->N || cols[k] < 0 || cols[k] >= c->N)
      return ps_fail(PS_ERR_BAD_ARG, "gain_gather: cell %lld = (%d, %d) is outside the %d x %d domain", (long long)k,
                     rows[k], cols[k], c->N, c->N);
    cell[(size_t)k] = (int64_t)rows[k] * c->N + cols[k];
  }
  PS_HIP(hipSetDevice(c->device));
  if (n > c->g_cap) {   // nothing in flight uses the scratch: gather synchronises before it returns
    if (c->g_cell) PS_HIP(hipFree(c->g_cell));
    if (c->g_out) PS_HIP(hipFree(c->g_out));
    c->g_cell = nullptr;
    c->g_out = nullptr;
    c->g_cap = 0;
    PS_HIP(hipMalloc((void**)&c->g_cell, (size_t)n * sizeof(int64_t)));
    PS_HIP(hipMalloc((void**)&c->g_out, (size_t)n * c->nplane * sizeof(double)));
    c->g_cap = n;
  }
  PS_TRY(c->last.wait(c->stream));
  PS_HIP(hipMemcpyAsync(c->g_cell, cell.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  const int64_t total = n * c->nplane;
  hipLaunchKernelGGL(k_gain_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->Y, c->pitch,
                     c->nplane, n, c->g_cell, c->g_out);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(out, c->g_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PS_HIP(hipStreamSynchronize(c->stream));
  return PS_OK;
}

extern "C" int ps_gain_info(ps_gain* c, int* N, int* nin, int* ntrap, int* nplane, int64_t* applies) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "gain_info: null handle");
  if (N) *N = c->N;
  if (nin) *nin = c->nin;
  if (ntrap) *ntrap = c->ntrap;
  if (nplane) *nplane = c->nplane;
  if (applies) *applies = c->applies;
  return PS_OK;
}

extern "C" int ps_gain_prof(ps_gain* c, int enable, double* total_ms, int64_t* launches) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "gain_prof: null handle");
  PS_HIP(hipSetDevice(c->device));
  c->prof.set(enable);
  if (total_ms || launches) PS_TRY(c->prof.totals(0, total_ms, launches));
  return PS_OK;
}

static int gain_view(void* h, PsProjectView* out) {
  ps_gain* c = static_cast<ps_gain*>(h);
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "gain view: null handle");
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "nothing applied yet: apply the information fields first");
  out->Y = c->Y;
  out->pitch = c->pitch;
  out->N = c->N;
  out->nout = c->nplane;
  out->device = c->device;
  return PS_OK;
}
static int gain_wait(void* h, hipStream_t stream) { return static_cast<ps_gain*>(h)->last.wait(stream); }
static int gain_mark(void* h, hipStream_t stream) { return static_cast<ps_gain*>(h)->last.mark(stream); }
PsFieldsOps ps_gain_fields() { return PsFieldsOps{"information fields", gain_view, gain_wait, gain_mark}; }
