// Release plans (include/parasitoid_hip.h, ps_sites_*): the field of one member under several release sites
// and staggered release days, superposed on the device from the solver's records.  One wind station and a
// homogeneous landscape make the field of a release at another cell the centre release translated, and the
// population chain is linear in the released number, so for output day D_e
//   Y_e(r, c) = sum over groups g, sum over the sites k of g:  a_k * v_{g, D_e - lag_g}(r - drow_k, c - dcol_k)
// where a group is the set of sites released on one day, v_{g, d} is the value ps_summary_add adds
// (ps_record_value) for model day d of the group's own solver (a release `lag` days later sees other day
// kernels: it is an evaluation of its own, not a time shift), and v is 0 where the source row or the source
// column leaves [0, N) -- per axis, never by the flat index, which would wrap a plume that leaves the east
// edge onto the west edge of the next row.  Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   Y[e][pitch]        fp64; group 0 overwrites it, zeros included, later groups accumulate into it
// One apply is one launch for one group: blockIdx.y is the output, a thread owns a pair of flat-adjacent
// cells (the tail cell of the odd N*N alone) and walks the group's sites in the order given with
//   acc = __dadd_rn(acc, __dmul_rn(a_k, v))
// (the library is built with -ffp-contract=on, a plain acc += a * v would fuse), from +0.0 in group 0 and
// from the stored Y later, so a numpy loop Y[e] = Y[e] + a * shifted(f) reproduces every bit.  Amounts are
// > 0 and values >= 0: acc is never -0.0 and a term from outside the domain changes no bit.  N is odd, so a
// pair straddles a row end in every other row, and the flat shift drow * N + dcol is odd for some sites:
// a source pair is neither always in one row nor always 16-byte aligned.  Each source cell is therefore one
// 8-byte load with its own row / column test (a wave still reads 512 contiguous bytes per row segment); Y,
// whose pairs are aligned by construction, moves as 16 bytes.  Every cell has one writer: no atomics.
#include <math.h>

#include <vector>

#include "ps_common.h"

#define PS_SITES_MAX_OUT 32    // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_SITES_MAX_GROUP 8
#define PS_SITES_MAX_SITE 32   // in total, so also per group: 32 x 16 B of kernel arguments
#define PS_SITES_THREADS 256

namespace {

struct SiteSlots {   // rec nullptr (PS_REC_NONE): the group is not released yet on this output day
  PsSrc s[PS_SITES_MAX_OUT];
};
struct SiteTab {
  double amount[PS_SITES_MAX_SITE];
  int drow[PS_SITES_MAX_SITE], dcol[PS_SITES_MAX_SITE];
};

// blockIdx.y = output; thread j owns the cells 2j, 2j + 1 (j == npair: the tail cell alone).  The slot's
// descriptor, its day delta and the site table are the same for every lane (kernel arguments and one scalar
// load per block).  first: group 0, which starts from +0.0 and stores even where nothing was released.
__global__ void __launch_bounds__(PS_SITES_THREADS) k_sites_apply(SiteSlots desc, SiteTab tab, int nsite, int first,
                                                                  double* __restrict__ Y, int N, int64_t ncell,
                                                                  int64_t pitch, double negval) {
  const PsSrc sd = desc.s[blockIdx.y];
  if (!sd.rec && !first) return;   // nothing to add: Y stays as it is
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pair = j < npair, tail = j == npair && (ncell & 1);
  if (!(pair || tail)) return;
  const int64_t i = pair ? 2 * j : ncell - 1;
  double* y = Y + (int64_t)blockIdx.y * pitch + i;
  double a0 = 0.0, a1 = 0.0;
  if (!first) {
    if (pair) {
      const double2 t = *reinterpret_cast<const double2*>(y);
      a0 = t.x;
      a1 = t.y;
    } else {
      a0 = *y;
    }
  }
  if (sd.rec) {
    const double* __restrict__ rec = sd.rec;
    const double delta = sd.stats ? sd.stats->delta : 0.0;
    const double ss = sd.stat_scale, ps = sd.post_scale;
    const int r0 = (int)(i / N), c0 = (int)(i - (int64_t)r0 * N);
    const bool wrap = c0 == N - 1;                     // the pair straddles the row end
    const int r1 = wrap ? r0 + 1 : r0, c1 = wrap ? 0 : c0 + 1;
#pragma unroll 4
    for (int k = 0; k < nsite; ++k) {
      const int dr = tab.drow[k], dc = tab.dcol[k];
      const double a = tab.amount[k];
      const int rs0 = r0 - dr, cs0 = c0 - dc, rs1 = r1 - dr, cs1 = c1 - dc;
      const bool ok0 = (unsigned)rs0 < (unsigned)N && (unsigned)cs0 < (unsigned)N;
      const bool ok1 = pair && (unsigned)rs1 < (unsigned)N && (unsigned)cs1 < (unsigned)N;
      const double x0 = ok0 ? rec[(int64_t)rs0 * N + cs0] : 0.0;
      const double x1 = ok1 ? rec[(int64_t)rs1 * N + cs1] : 0.0;
      a0 = __dadd_rn(a0, __dmul_rn(a, ps_record_value(x0, ss, ps, delta, negval)));   // the value of 0 is 0
      a1 = __dadd_rn(a1, __dmul_rn(a, ps_record_value(x1, ss, ps, delta, negval)));
    }
  }
  if (pair)
    *reinterpret_cast<double2*>(y) = make_double2(a0, a1);
  else
    *y = a0;
}

// out[e][k] = Y_e(cell[k]); flat over nout * n
__global__ void k_sites_gather(const double* __restrict__ Y, int64_t pitch, int nout, int64_t n,
                               const int64_t* __restrict__ cell, double* __restrict__ out) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n * nout) return;
  const int64_t e = t / n, k = t - e * n;
  out[t] = Y[e * pitch + cell[k]];
}

}  // namespace

struct ps_sites {
  int device = 0, N = 0, nout = 0, ngroup = 0, nsite = 0;
  int64_t ncell = 0, pitch = 0;
  int nblk = 0;                    // blocks of one apply launch per output
  std::vector<SiteTab> tabs;       // per group, host side: passed by value with every launch
  std::vector<int> group_nsite;
  double* Y = nullptr;             // [nout][pitch]
  int64_t* g_cell = nullptr;       // gather scratch, grown on demand
  double* g_out = nullptr;
  int64_t g_cap = 0;
  int next_group = 0;              // the group the next apply must name
  int64_t passes = 0;              // completed passes: the last group applied
  bool complete = false;           // Y holds a whole plan (no pass under way)
  hipStream_t stream = nullptr;    // fetch / gather
  PsLastOp last;                   // the last operation on Y, on whatever stream it ran
  PsProf prof;                     // channel 0: the applies
};

// Y holds a whole plan: at least one pass done and none under way
static int sites_whole(const ps_sites* p, const char* who) {
  if (p->passes == 0 && p->next_group == 0) return ps_fail(PS_ERR_STATE, "%s: no release plan applied yet", who);
  if (!p->complete)
    return ps_fail(PS_ERR_STATE, "%s: group %d of %d of the current pass has not been applied", who, p->next_group,
                   p->ngroup);
  return PS_OK;
}

extern "C" void ps_sites_destroy(ps_sites* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  p->last.sync();
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  p->prof.release();
  for (void* q : {(void*)p->Y, (void*)p->g_cell, (void*)p->g_out})
    if (q) (void)hipFree(q);
  p->last.destroy();
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

extern "C" int ps_sites_create(int device, int N, int nout, int ngroup, const int32_t* group_nsite, const int32_t* drow,
                               const int32_t* dcol, const double* amount, ps_sites** out) {
  if (!out || N < 1 || nout < 1 || nout > PS_SITES_MAX_OUT || ngroup < 1 || ngroup > PS_SITES_MAX_GROUP ||
      !group_nsite || !drow || !dcol || !amount)
    return ps_fail(PS_ERR_BAD_ARG, "sites_create: N %d, %d outputs (1..%d), %d groups (1..%d)", N, nout,
                   PS_SITES_MAX_OUT, ngroup, PS_SITES_MAX_GROUP);
  *out = nullptr;
  int nsite = 0;
  for (int g = 0; g < ngroup; ++g) {
    if (group_nsite[g] < 1) return ps_fail(PS_ERR_BAD_ARG, "sites_create: group %d has %d sites", g, group_nsite[g]);
    if (group_nsite[g] > PS_SITES_MAX_SITE - nsite)
      return ps_fail(PS_ERR_BAD_ARG, "sites_create: more than %d sites in total at group %d", PS_SITES_MAX_SITE, g);
    nsite += group_nsite[g];
  }
  for (int k = 0; k < nsite; ++k) {
    if (drow[k] <= -N || drow[k] >= N || dcol[k] <= -N || dcol[k] >= N)
      return ps_fail(PS_ERR_BAD_ARG, "sites_create: site %d is offset by (%d, %d) cells, beyond the %d x %d domain", k,
                     drow[k], dcol[k], N, N);
    if (!isfinite(amount[k]) || !(amount[k] > 0.0))
      return ps_fail(PS_ERR_BAD_ARG, "sites_create: amount %d = %g is not finite and > 0", k, amount[k]);
  }
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  const int64_t nblk = (ncell / 2 + 1 + PS_SITES_THREADS - 1) / PS_SITES_THREADS;   // the pairs and the tail thread
  if (nblk > 0x7fffffffLL) return ps_fail(PS_ERR_BAD_ARG, "sites_create: N %d is too large for one launch", N);
  // everything, checked before anything is allocated: the output fields
  const double need = (double)nout * pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "sites_create: %d outputs x %lld cells x 8 B = %.3g GB, %.3g GB free", nout,
                   (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_sites* p = new ps_sites();
  p->device = device;
  p->N = N;
  p->nout = nout;
  p->ngroup = ngroup;
  p->nsite = nsite;
  p->ncell = ncell;
  p->pitch = pitch;
  p->nblk = (int)nblk;
  p->group_nsite.assign(group_nsite, group_nsite + ngroup);
  p->tabs.resize((size_t)ngroup);
  for (int g = 0, k = 0; g < ngroup; ++g) {
    SiteTab& t = p->tabs[(size_t)g];
    t = SiteTab();
    for (int q = 0; q < group_nsite[g]; ++q, ++k) {
      t.amount[q] = amount[k];
      t.drow[q] = drow[k];
      t.dcol[q] = dcol[k];
    }
  }
  auto fail = [&](int rc) {
    ps_sites_destroy(p);
    return rc;
  };
  const size_t y_b = (size_t)nout * pitch * sizeof(double);
  hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = p->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&p->Y, y_b);
  if (e == hipSuccess) e = hipMemsetAsync(p->Y, 0, y_b, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "sites_create: %s", hipGetErrorString(e)));
  *out = p;
  return PS_OK;
}

extern "C" int ps_sites_apply(ps_sites* p, ps_solver* s, int group, int nout, const int32_t* kind, const int32_t* idx,
                              const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                              double negval) {
  if (!p || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "sites_apply: bad arguments");
  if (group < 0 || group >= p->ngroup) return ps_fail(PS_ERR_BAD_ARG, "sites_apply: group %d of %d", group, p->ngroup);
  if (nout != p->nout) return ps_fail(PS_ERR_BAD_ARG, "sites_apply: %d outputs given, the handle has %d", nout, p->nout);
  if (group != p->next_group && group != 0)   // group 0 may always open a new pass (after a failed apply, say)
    return ps_fail(PS_ERR_STATE, "sites_apply: group %d given, the pass is at group %d (groups go 0 .. %d in order)",
                   group, p->next_group, p->ngroup - 1);
  PS_HIP(hipSetDevice(p->device));
  // every descriptor first: an apply with a bad record enqueues nothing
  SiteSlots desc;
  hipStream_t stream = nullptr;
  bool any = false;
  PS_TRY(ps_read_records("sites_apply", "handle", p->device, p->N, s, nout, kind, idx, stat_scale, post_scale,
                         use_delta, true, desc.s, &stream, &any));
  for (int e = nout; e < PS_SITES_MAX_OUT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  if (!any)   // such a group belongs in no plan, and no record names the stream to run on
    return ps_fail(PS_ERR_BAD_ARG, "sites_apply: group %d is released on no output day (every slot is PS_REC_NONE)",
                   group);
  PS_TRY(p->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(p->prof.begin(0, stream, &e1));
  hipLaunchKernelGGL(k_sites_apply, dim3(p->nblk, p->nout), dim3(PS_SITES_THREADS), 0, stream, desc,
                     p->tabs[(size_t)group], p->group_nsite[(size_t)group], group == 0 ? 1 : 0, p->Y, p->N, p->ncell,
                     p->pitch, negval);
  PS_HIP(hipGetLastError());
  PS_TRY(p->prof.end(stream, e1));
  PS_TRY(p->last.mark(stream));
  p->next_group = group + 1 == p->ngroup ? 0 : group + 1;
  p->complete = p->next_group == 0;
  if (p->complete) p->passes += 1;
  return PS_OK;
}

extern "C" int ps_sites_fetch(ps_sites* p, int e, double* out) {
  if (!p || !out) return ps_fail(PS_ERR_BAD_ARG, "sites_fetch: bad arguments");
  if (e < 0 || e >= p->nout) return ps_fail(PS_ERR_BAD_ARG, "sites_fetch: output %d of %d", e, p->nout);
  PS_TRY(sites_whole(p, "sites_fetch"));
  PS_HIP(hipSetDevice(p->device));
  PS_TRY(p->last.wait(p->stream));
  PS_HIP(hipMemcpyAsync(out, p->Y + (int64_t)e * p->pitch, (size_t)p->ncell * sizeof(double), hipMemcpyDeviceToHost,
                        p->stream));
  PS_HIP(hipStreamSynchronize(p->stream));
  return PS_OK;
}

extern "C" int ps_sites_gather(ps_sites* p, int64_t n, const int32_t* rows, const int32_t* cols, double* out) {
  if (!p || n < 0 || (n > 0 && (!rows || !cols || !out))) return ps_fail(PS_ERR_BAD_ARG, "sites_gather: bad arguments");
  PS_TRY(sites_whole(p, "sites_gather"));
  if (n == 0) return PS_OK;
  std::vector<int64_t> cell((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    if (rows[k] < 0 || rows[k] >= p->N || cols[k] < 0 || cols[k] >= p->N)
      return ps_fail(PS_ERR_BAD_ARG, "sites_gather: cell %lld = (%d, %d) is outside the %d x %d domain", (long long)k,
                     rows[k], cols[k], p->N, p->N);
    cell[(size_t)k] = (int64_t)rows[k] * p->N + cols[k];
  }
  PS_HIP(hipSetDevice(p->device));
  if (n > p->g_cap) {   // the handle's stream is idle here: fetch and gather synchronise before they return
    if (p->g_cell) PS_HIP(hipFree(p->g_cell));
    if (p->g_out) PS_HIP(hipFree(p->g_out));
    p->g_cell = nullptr;
    p->g_out = nullptr;
    p->g_cap = 0;
    PS_HIP(hipMalloc((void**)&p->g_cell, (size_t)n * sizeof(int64_t)));
    PS_HIP(hipMalloc((void**)&p->g_out, (size_t)n * p->nout * sizeof(double)));
    p->g_cap = n;
  }
  PS_TRY(p->last.wait(p->stream));
  PS_HIP(hipMemcpyAsync(p->g_cell, cell.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, p->stream));
  const int64_t total = n * p->nout;
  hipLaunchKernelGGL(k_sites_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, p->stream, p->Y, p->pitch,
                     p->nout, n, p->g_cell, p->g_out);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(out, p->g_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  PS_HIP(hipStreamSynchronize(p->stream));
  return PS_OK;
}

extern "C" int ps_sites_info(ps_sites* p, int* N, int* nout, int* ngroup, int* nsite, int64_t* passes) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "sites_info: null handle");
  if (N) *N = p->N;
  if (nout) *nout = p->nout;
  if (ngroup) *ngroup = p->ngroup;
  if (nsite) *nsite = p->nsite;
  if (passes) *passes = p->passes;
  return PS_OK;
}

extern "C" int ps_sites_prof(ps_sites* p, int enable, double* total_ms, int64_t* launches) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "sites_prof: null handle");
  PS_HIP(hipSetDevice(p->device));
  p->prof.set(enable);
  if (total_ms || launches) PS_TRY(p->prof.totals(0, total_ms, launches));
  return PS_OK;
}

static int sites_view(void* h, PsProjectView* out) {
  ps_sites* p = static_cast<ps_sites*>(h);
  if (!p || !out) return ps_fail(PS_ERR_BAD_ARG, "release plan view: null handle");
  PS_TRY(sites_whole(p, "release plan"));
  out->Y = p->Y;
  out->pitch = p->pitch;
  out->N = p->N;
  out->nout = p->nout;
  out->device = p->device;
  return PS_OK;
}
static int sites_wait(void* h, hipStream_t stream) { return static_cast<ps_sites*>(h)->last.wait(stream); }
static int sites_mark(void* h, hipStream_t stream) { return static_cast<ps_sites*>(h)->last.mark(stream); }
PsFieldsOps ps_sites_fields() { return PsFieldsOps{"release plan", sites_view, sites_wait, sites_mark}; }
