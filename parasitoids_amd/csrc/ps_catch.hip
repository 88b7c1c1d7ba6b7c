// Catch-probability fields (include/parasitoid_hip.h, ps_catch_*): what a trap of effort `rate` would find in
// one member's field, Y_e(c) = P(Poisson(rate_e * v(c)) >= count_e), v the value of input record input[e] at the
// cell -- the one ps_summary_add adds (ps_record_value) -- or output input[e] of another fields source.  Layout
// (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   Y[e][pitch]        fp64, overwritten by every apply, zeros included
// The outputs are grouped by input at create (CatchTab, a kernel argument): one thread owns a pair of cells, reads
// each used record once and walks the group's outputs.  A pair whose two values are zero -- most of the domain --
// stores the group's zeros and never enters the exponential path; where a whole wave lies outside the plume the
// branch is uniform and the wave skips it.  The value of a cell depends on its own (mu, count) alone
// (catch_value, stated step by step in the header): no atomics, no LDS, one writer per cell, the same call gives
// the same bits whatever the launch shape.
#include <math.h>

#include <utility>
#include <vector>

#include "ps_catch_value.h"   // catch_value: P(Poisson(mu) >= n), shared with ps_gain.hip
#include "ps_common.h"

#define PS_CATCH_MAX_IN 32     // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_CATCH_MAX_OUT 32
#define PS_CATCH_THREADS 256

namespace {

struct CatchSlots {
  PsSrc s[PS_CATCH_MAX_IN];
};
// the outputs in group order: group g reads input gin[g] and owns the entries gstart[g] .. gstart[g + 1] - 1
struct CatchTab {
  double rate[PS_CATCH_MAX_OUT];
  int count[PS_CATCH_MAX_OUT];
  int out[PS_CATCH_MAX_OUT];      // the output an entry writes
  int gin[PS_CATCH_MAX_OUT];
  int gstart[PS_CATCH_MAX_OUT + 1];
  int ngroup, pad_;
};

// thread j owns the cells 2j, 2j + 1 (j == npair: the tail cell of an odd N*N alone)
__global__ void __launch_bounds__(PS_CATCH_THREADS) k_catch_apply(CatchSlots desc, CatchTab tab, double* __restrict__ Y,
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
      double y0 = 0.0, y1 = 0.0;
      if (live) {
        const double rate = tab.rate[q];
        const int n = tab.count[q];
        const double mu0 = rate * v0;
        const double mu1 = rate * v1;
        y0 = catch_value(mu0, n);
        y1 = catch_value(mu1, n);
      }
      double* y = Y + (int64_t)tab.out[q] * pitch + i;
      if (pair)
        *reinterpret_cast<double2*>(y) = make_double2(y0, y1);
      else
        *y = y0;
    }
  }
}

// out[e][k] = Y_e(cell[k]); flat over nout * n
__global__ void k_catch_gather(const double* __restrict__ Y, int64_t pitch, int nout, int64_t n,
                               const int64_t* __restrict__ cell, double* __restrict__ out) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * nout) return;
  const int64_t e = t / n, k = t - e * n;
  out[t] = Y[e * pitch + cell[k]];
}

}  // namespace

struct ps_catch {
  int device = 0, N = 0, nin = 0, nout = 0;
  int64_t ncell = 0, pitch = 0;
  int nblk = 0;                    // blocks of one apply launch
  CatchTab tab;
  double* Y = nullptr;             // [nout][pitch]
  int64_t* g_cell = nullptr;       // gather scratch, grown on demand
  double* g_out = nullptr;
  int64_t g_cap = 0;
  int64_t applies = 0;
  hipStream_t stream = nullptr;    // fetch / gather / apply of another fields source
  PsLastOp last;                   // the last operation on Y, on whatever stream it ran
  PsProf prof;                     // channel 0: the applies
};

extern "C" void ps_catch_destroy(ps_catch* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->last.sync();
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->prof.release();
  for (void* q : {(void*)c->Y, (void*)c->g_cell, (void*)c->g_out})
    if (q) (void)hipFree(q);
  c->last.destroy();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int ps_catch_create(int device, int N, int nin, int nout, const int32_t* input, const double* rate,
                               const int32_t* count, ps_catch** out) {
  if (!out || N < 1 || nin < 1 || nin > PS_CATCH_MAX_IN || nout < 1 || nout > PS_CATCH_MAX_OUT || !input || !rate ||
      !count)
    return ps_fail(PS_ERR_BAD_ARG, "catch_create: N %d, %d inputs (1..%d), %d outputs (1..%d)", N, nin,
                   PS_CATCH_MAX_IN, nout, PS_CATCH_MAX_OUT);
  for (int e = 0; e < nout; ++e) {
    if (input[e] < 0 || input[e] >= nin)
      return ps_fail(PS_ERR_BAD_ARG, "catch_create: output %d reads input %d of %d", e, input[e], nin);
    if (!isfinite(rate[e]) || !(rate[e] > 0.0))
      return ps_fail(PS_ERR_BAD_ARG, "catch_create: rate [%d] = %g is not finite and > 0", e, rate[e]);
    if (count[e] < 1 || count[e] > PS_CATCH_MAX_COUNT)
      return ps_fail(PS_ERR_BAD_ARG, "catch_create: count [%d] = %d is not in 1..%d", e, count[e], PS_CATCH_MAX_COUNT);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  const int64_t nblk = (ncell / 2 + 1 + PS_CATCH_THREADS - 1) / PS_CATCH_THREADS;   // the pairs and the tail thread
  if (nblk > 0x7fffffffLL) return ps_fail(PS_ERR_BAD_ARG, "catch_create: N %d is too large for one launch", N);
  // the output fields, checked before anything is allocated
  const double need = (double)nout * pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "catch_create: %d outputs x %lld cells x 8 B = %.3g GB, %.3g GB free", nout,
                   (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_catch* c = new ps_catch();
  c->device = device;
  c->N = N;
  c->nin = nin;
  c->nout = nout;
  c->ncell = ncell;
  c->pitch = pitch;
  c->nblk = (int)nblk;
  CatchTab& tab = c->tab;
  tab = CatchTab();
  int q = 0;
  for (int d = 0; d < nin; ++d) {   // ascending input, the outputs of one input in ascending e
    const int q0 = q;
    for (int e = 0; e < nout; ++e) {
      if (input[e] != d) continue;
      tab.rate[q] = rate[e];
      tab.count[q] = count[e];
      tab.out[q] = e;
      ++q;
    }
    if (q == q0) continue;
    tab.gin[tab.ngroup] = d;
    tab.gstart[tab.ngroup] = q0;
    tab.gstart[++tab.ngroup] = q;
  }
  auto fail = [&](int rc) {
    ps_catch_destroy(c);
    return rc;
  };
  const size_t y_b = (size_t)nout * pitch * sizeof(double);
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = c->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&c->Y, y_b);
  if (e == hipSuccess) e = hipMemsetAsync(c->Y, 0, y_b, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "catch_create: %s", hipGetErrorString(e)));
  *out = c;
  return PS_OK;
}

// one launch over the resolved descriptors on `stream`, behind the handle's last operation
static int catch_launch(ps_catch* c, const CatchSlots& desc, hipStream_t stream, double negval) {
  PS_TRY(c->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(c->prof.begin(0, stream, &e1));
  hipLaunchKernelGGL(k_catch_apply, dim3(c->nblk), dim3(PS_CATCH_THREADS), 0, stream, desc, c->tab, c->Y, c->ncell,
                     c->pitch, negval);
  PS_HIP(hipGetLastError());
  PS_TRY(c->prof.end(stream, e1));
  PS_TRY(c->last.mark(stream));
  c->applies += 1;
  return PS_OK;
}

extern "C" int ps_catch_apply(ps_catch* c, ps_solver* s, int nin, const int32_t* kind, const int32_t* idx,
                              const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                              double negval) {
  if (!c || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "catch_apply: bad arguments");
  if (nin != c->nin) return ps_fail(PS_ERR_BAD_ARG, "catch_apply: %d inputs given, the handle has %d", nin, c->nin);
  PS_HIP(hipSetDevice(c->device));
  // every descriptor first: an apply with a bad record enqueues nothing
  CatchSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("catch_apply", "handle", c->device, c->N, s, nin, kind, idx, stat_scale, post_scale, use_delta,
                          false, desc.s, &stream));
  for (int i = nin; i < PS_CATCH_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return catch_launch(c, desc, stream, negval);
}

// the inputs are the current fields of a projection or a release plan (who: the entry point): input i is the
// source's output i, on the handle's stream behind the source's last operation
static int catch_apply_fields(ps_catch* c, void* h, const PsFieldsOps& src, const char* who) {
  if (!c || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  // input i takes Y_i: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  CatchSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "inputs", c->device, c->N, c->nin, h, src, desc.s));
  for (int i = c->nin; i < PS_CATCH_MAX_IN; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(src.wait(h, c->stream));
  PS_TRY(catch_launch(c, desc, c->stream, 0.0));
  return src.mark(h, c->stream);   // the source's next apply overwrites its fields only after this read
}

extern "C" int ps_catch_apply_project(ps_catch* c, ps_project* p) {
  return catch_apply_fields(c, p, ps_project_fields(), "catch_apply_project");
}

extern "C" int ps_catch_apply_sites(ps_catch* c, ps_sites* p) {
  return catch_apply_fields(c, p, ps_sites_fields(), "catch_apply_sites");
}

extern "C" int ps_catch_fetch(ps_catch* c, int e, double* out) {
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "catch_fetch: bad arguments");
  if (e < 0 || e >= c->nout) return ps_fail(PS_ERR_BAD_ARG, "catch_fetch: output %d of %d", e, c->nout);
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "catch_fetch: nothing applied yet");
  PS_HIP(hipSetDevice(c->device));
  PS_TRY(c->last.wait(c->stream));
  PS_HIP(hipMemcpyAsync(out, c->Y + (int64_t)e * c->pitch, (size_t)c->ncell * sizeof(double), hipMemcpyDeviceToHost,
                        c->stream));
  PS_HIP(hipStreamSynchronize(c->stream));
  return PS_OK;
}

extern "C" int ps_catch_gather(ps_catch* c, int64_t n, const int32_t* rows, const int32_t* cols, double* out) {
  if (!c || n < 0 || (n > 0 && (!rows || !cols || !out))) return ps_fail(PS_ERR_BAD_ARG, "catch_gather: bad arguments");
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "catch_gather: nothing applied yet");
  if (n == 0) return PS_OK;
  std::vector<int64_t> cell((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    if (rows[k] < 0 || rows[k] >= c->N || cols[k] < 0 || cols[k] >= c->N)
      return ps_fail(PS_ERR_BAD_ARG, "catch_gather: cell %lld = (%d, %d) is outside the %d x %d domain", (long long)k,
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
    PS_HIP(hipMalloc((void**)&c->g_out, (size_t)n * c->nout * sizeof(double)));
    c->g_cap = n;
  }
  PS_TRY(c->last.wait(c->stream));
  PS_HIP(hipMemcpyAsync(c->g_cell, cell.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  const int64_t total = n * c->nout;
  hipLaunchKernelGGL(k_catch_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->Y, c->pitch,
                     c->nout, n, c->g_cell, c->g_out);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(out, c->g_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PS_HIP(hipStreamSynchronize(c->stream));
  return PS_OK;
}

extern "C" int ps_catch_info(ps_catch* c, int* N, int* nin, int* nout, int64_t* applies) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "catch_info: null handle");
  if (N) *N = c->N;
  if (nin) *nin = c->nin;
  if (nout) *nout = c->nout;
  if (applies) *applies = c->applies;
  return PS_OK;
}

extern "C" int ps_catch_prof(ps_catch* c, int enable, double* total_ms, int64_t* launches) {
  if (!c) return ps_fail(PS_ERR_BAD_ARG, "catch_prof: null handle");
  PS_HIP(hipSetDevice(c->device));
  c->prof.set(enable);
  if (total_ms || launches) PS_TRY(c->prof.totals(0, total_ms, launches));
  return PS_OK;
}

static int catch_view(void* h, PsProjectView* out) {
  ps_catch* c = static_cast<ps_catch*>(h);
  if (!c || !out) return ps_fail(PS_ERR_BAD_ARG, "catch view: null handle");
  if (c->applies == 0) return ps_fail(PS_ERR_STATE, "nothing applied yet: apply the catch fields first");
  out->Y = c->Y;
  out->pitch = c->pitch;
  out->N = c->N;
  out->nout = c->nout;
  out->device = c->device;
  return PS_OK;
}
static int catch_wait(void* h, hipStream_t stream) { return static_cast<ps_catch*>(h)->last.wait(stream); }
static int catch_mark(void* h, hipStream_t stream) { return static_cast<ps_catch*>(h)->last.mark(stream); }
PsFieldsOps ps_catch_fields() { return PsFieldsOps{"catch fields", catch_view, catch_wait, catch_mark}; }
