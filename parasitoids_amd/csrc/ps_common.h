// Shared host-side helpers of libparasitoid_hip.so: error reporting, device
// buffers, uploaded FFT plans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/parasitoid_hip.h"
#include "fft_plan.h"

extern thread_local std::string ps_tls_error;

inline int ps_fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  ps_tls_error = buf;
  return code;
}

#define PS_HIP(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      int code_ = (e_ == hipErrorOutOfMemory) ? PS_ERR_OOM : PS_ERR_HIP;                 \
      return ps_fail(code_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),       \
                     __FILE__, __LINE__);                                                \
    }                                                                                    \
  } while (0)

#define PS_TRY(expr)            \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != PS_OK) return rc_; \
  } while (0)

// The last operation on a handle's device data, on whatever stream it ran: an untimed event and whether it was ever
// recorded.  An operation on another stream first waits for it and then marks itself as the last one, so the
// operations of one handle run in call order across streams without a host synchronise.
struct PsLastOp {
  hipEvent_t ev = nullptr;
  bool live = false;
  hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
  int wait(hipStream_t stream) {   // order `stream` behind the last operation; nothing before the first mark
    if (live) PS_HIP(hipStreamWaitEvent(stream, ev, 0));
    return PS_OK;
  }
  int mark(hipStream_t stream) {
    PS_HIP(hipEventRecord(ev, stream));
    live = true;
    return PS_OK;
  }
  void sync() {   // destroy paths: the last operation has finished when this returns
    if (live) (void)hipEventSynchronize(ev);
  }
  void destroy() {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
    live = false;
  }
};

// Launch profiling of a handle (its ps_xxx_prof): while `on`, begin/end bracket a launch sequence with a pair of
// timed events on one of up to PS_PROF_CHANNELS channels.  Finished pairs are folded into the channel's totals and
// their events destroyed at every report and whenever PS_PROF_PENDING pairs are pending -- the one host
// synchronise, with profiling on only -- so a profiled handle holds a bounded number of events however long it
// lives.  The totals count from the handle's creation.
#define PS_PROF_CHANNELS 4
#define PS_PROF_PENDING 256
struct PsProf {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[PS_PROF_CHANNELS];
  double ms[PS_PROF_CHANNELS] = {0.0, 0.0, 0.0, 0.0};
  int64_t n[PS_PROF_CHANNELS] = {0, 0, 0, 0};
  // *end: the event to hand to end() after the launches, nullptr while profiling is off
  int begin(int channel, hipStream_t stream, hipEvent_t* end) {
    *end = nullptr;
    if (!on) return PS_OK;
    if (pending[channel].size() >= PS_PROF_PENDING) PS_TRY(fold(channel));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PS_HIP(hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e != hipSuccess) {
      (void)hipEventDestroy(e0);
      PS_HIP(e);
    }
    pending[channel].push_back({e0, e1});
    PS_HIP(hipEventRecord(e0, stream));
    *end = e1;
    return PS_OK;
  }
  int end(hipStream_t stream, hipEvent_t e1) {
    if (e1) PS_HIP(hipEventRecord(e1, stream));
    return PS_OK;
  }
  // the pending pairs into the totals in list order, their events destroyed
  int fold(int channel) {
    auto& list = pending[channel];
    for (auto& p : list) {
      PS_HIP(hipEventSynchronize(p.second));
      float t = 0.f;
      PS_HIP(hipEventElapsedTime(&t, p.first, p.second));
      ms[channel] += t;
      n[channel] += 1;
    }
    for (auto& p : list) {
      (void)hipEventDestroy(p.first);
      (void)hipEventDestroy(p.second);
    }
    list.clear();
    return PS_OK;
  }
  int totals(int channel, double* total_ms, int64_t* launches) {
    PS_TRY(fold(channel));
    if (total_ms) *total_ms = ms[channel];
    if (launches) *launches = n[channel];
    return PS_OK;
  }
  void set(int enable) {   // < 0: leave as it is
    if (enable >= 0) on = enable != 0;
  }
  bool idle() const {   // no pair pending on any channel
    for (auto& list : pending)
      if (!list.empty()) return false;
    return true;
  }
  // destroy paths, and the reset of a handle whose timings go with its members: the pending events destroyed,
  // the totals zero
  void release() {
    for (int c = 0; c < PS_PROF_CHANNELS; ++c) {
      for (auto& p : pending[c]) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
      }
      pending[c].clear();
      ms[c] = 0.0;
      n[c] = 0;
    }
  }
};

// Device memory goes through a small caching allocator (ps_solver.hip): an MCMC run creates
// and destroys a solver whenever the kernel extent changes, and hipMalloc/hipFree of its
// ~40 buffers cost more than the evaluation itself.  Freed blocks are kept per device (up to
// PS_POOL_GB, default 16) and handed out again for requests of about the same size.
// ps_dev_free assumes the block is idle: callers synchronise first (ps_dev_quiesce).
hipError_t ps_dev_malloc(void** p, size_t bytes);
void ps_dev_free(void* p);
void ps_dev_quiesce();   // hipDeviceSynchronize: nothing in flight may still use a block about to be freed

// growable device buffer
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return PS_OK;
    if (p) {
      ps_dev_quiesce();   // queued work may still read the old block
      ps_dev_free(p);
    }
    p = nullptr;
    cap = 0;
    hipError_t e = ps_dev_malloc((void**)&p, n * sizeof(T));
    if (e != hipSuccess)
      return ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP,
                     "device allocation of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    cap = n;
    return PS_OK;
  }
  void release() {   // callers quiesce first (destroy paths)
    if (p) ps_dev_free(p);
    p = nullptr;
    cap = 0;
  }
};

struct DevPlan {
  HostFftPlan host;
  FftProg prog;  // with device pointers
  DevBuf<cplx> tw_all;  // lo | hi | gen, contiguous
  DevBuf<uint32_t> pos, pos_phys;
  bool generic = false;
  int upload() {
    prog = host.prog;
    PS_TRY(tw_all.ensure(host.tw_all.size()));
    PS_TRY(pos.ensure(host.pos.size()));
    PS_TRY(pos_phys.ensure(host.pos_phys.size()));
    PS_HIP(hipMemcpy(tw_all.p, host.tw_all.data(), host.tw_all.size() * sizeof(cplx), hipMemcpyHostToDevice));
    PS_HIP(hipMemcpy(pos.p, host.pos.data(), host.pos.size() * 4, hipMemcpyHostToDevice));
    PS_HIP(hipMemcpy(pos_phys.p, host.pos_phys.data(), host.pos_phys.size() * 4, hipMemcpyHostToDevice));
    prog.tw_lo = tw_all.p;
    prog.tw_hi = tw_all.p + prog.n_lo;
    prog.pos = pos.p;
    prog.pos_phys = pos_phys.p;
    generic = false;
    for (int s = 0; s < prog.ns; ++s)
      if (prog.radix[s] > 9 && prog.radix[s] != 16 && prog.radix[s] != 18) generic = true;
    return PS_OK;
  }
  void release() {
    tw_all.release();
    pos.release();
    pos_phys.release();
  }
};

int ps_use_device(int device);

// internal cross-module entry points (solver <-> model, same shared library)
int ps_chain_adopt_device_kernels(ps_solver* s, int nk, const int64_t* off, const int32_t* kshape,
                                  const int* row, const int* col, const double* val);
int ps_solver_set_state_device_coo(ps_solver* s, const int* row, const int* col, const double* val,
                                   int64_t nnz, int off);
int ps_solver_dom_len_internal(ps_solver* s);
int ps_solver_device_internal(ps_solver* s);
hipStream_t ps_solver_stream_internal(ps_solver* s);   // the stream the chain and its kernel copies run on

// the view of one solver record that ps_summary.hip accumulates (ps_solver_record_internal)
struct PsRecordView {
  const double* rec;            // N x N, row-major, device
  const ps_day_stats* stats;    // the day's device statistics (chain records), or nullptr
  hipStream_t stream;           // the stream the record is written on
  int N, device;
};
int ps_solver_record_internal(ps_solver* s, int kind, int idx, int want_stats, PsRecordView* out);

// Where one slot of an add, or one input of an apply, reads its field: a solver record with the scales of the
// value rule (ps_record_value), or an output of a fields source (no statistics, both scales 1).  The kernels take
// blocks of these by value, some inside a struct of their own that adds the slot.
struct PsSrc {
  const double* rec;           // nullptr: PS_REC_NONE
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
};
// the same inside a kernel's own descriptor {rec, stats, stat_scale, post_scale, slot}, where the kernel reads the slot
template <typename Slot>
static inline Slot ps_slotted(const PsSrc& r, int slot) {
  return Slot{r.rec, r.stats, r.stat_scale, r.post_scale, slot};
}

// out[0..n): the records (kind[i], idx[i]) of the solver's last evaluation, for a handle (noun: what the messages
// call it, who: the entry point) on `device` with domain N; a solver on another device or of another domain is
// refused.  *stream becomes the stream the records are written on.  none_ok: a PS_REC_NONE slot gives the all-null
// descriptor and names no stream; *any (may be nullptr) says whether any slot named one.  Nothing is enqueued and
// no handle is touched, so a caller that resolves first enqueues nothing for a bad slot.  This is the one caller
// of ps_solver_record_internal; static, as ps_read_fields, so that the library exports no symbol for either.
static inline int ps_read_records(const char* who, const char* noun, int device, int N, ps_solver* s, int n,
                                  const int32_t* kind, const int32_t* idx, const double* stat_scale,
                                  const double* post_scale, const int32_t* use_delta, bool none_ok, PsSrc* out,
                                  hipStream_t* stream, bool* any = nullptr) {
  if (any) *any = false;
  for (int i = 0; i < n; ++i) {
    if (none_ok && kind[i] == PS_REC_NONE) {
      out[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
      continue;
    }
    PsRecordView v;
    PS_TRY(ps_solver_record_internal(s, kind[i], idx[i], use_delta[i] != 0, &v));
    if (v.device != device)
      return ps_fail(PS_ERR_BAD_ARG, "%s: solver on device %d, %s on device %d", who, v.device, noun, device);
    if (v.N != N) return ps_fail(PS_ERR_BAD_ARG, "%s: solver domain %d, %s domain %d", who, v.N, noun, N);
    out[i] = PsSrc{v.rec, v.stats, stat_scale[i], post_scale[i]};
    *stream = v.stream;
    if (any) *any = true;
  }
  return PS_OK;
}

// the output fields of a projection that ps_summary.hip and ps_hist.hip accumulate (ps_project.hip);
// PS_ERR_STATE before the first apply.  A reader orders its stream behind the projection's last operation
// (wait), and the projection's next apply behind the read (mark).
struct PsProjectView {
  const double* Y;              // [nout][pitch], device
  int64_t pitch;
  int N, nout, device;
};
// The same triple for every handle that owns such fields, so that an accumulator has one code path for all
// of them: the projections (ps_project.hip) and the release plans (ps_sites.hip, PS_ERR_STATE also while a
// pass over the plan's groups is under way).  what: the handle's name in the accumulators' messages.
// A reader resolves the fields with ps_read_fields, then wait, its launches on its own stream, mark.
struct PsFieldsOps {
  const char* what;
  int (*view)(void* handle, PsProjectView* out);
  int (*wait)(void* handle, hipStream_t stream);
  int (*mark)(void* handle, hipStream_t stream);
};

// out[0..n): output e of the fields source h as slot (units "slots") or input (units "inputs") e of a handle
// (noun, who: as ps_read_records) on `device` with domain N that has n of them -- Y_e itself under the value
// rule: no statistics, both scales 1.  Refused in this order: a source that is not ready (view), another number
// of outputs, another device, another domain.  wait, the launch and mark stay with the caller.
static inline int ps_read_fields(const char* who, const char* noun, const char* units, int device, int N, int n,
                                 void* h, const PsFieldsOps& src, PsSrc* out) {
  PsProjectView v;
  PS_TRY(src.view(h, &v));
  if (v.nout != n)
    return ps_fail(PS_ERR_BAD_ARG, "%s: the %s has %d outputs, the %s %d %s", who, src.what, v.nout, noun, n, units);
  if (v.device != device)
    return ps_fail(PS_ERR_BAD_ARG, "%s: %s on device %d, %s on device %d", who, src.what, v.device, noun, device);
  if (v.N != N) return ps_fail(PS_ERR_BAD_ARG, "%s: %s domain %d, %s domain %d", who, src.what, v.N, noun, N);
  for (int e = 0; e < n; ++e) out[e] = PsSrc{v.Y + (int64_t)e * v.pitch, nullptr, 1.0, 1.0};
  return PS_OK;
}
PsFieldsOps ps_project_fields();
PsFieldsOps ps_sites_fields();
PsFieldsOps ps_peak_fields();    // the last member's peak field of a ps_peak (ps_peak.hip): nout = 1
PsFieldsOps ps_catch_fields();   // the catch-probability fields of a ps_catch (ps_catch.hip)
PsFieldsOps ps_gain_fields();    // the class-probability and entropy planes of a ps_gain (ps_gain.hip)
PsFieldsOps ps_nbhd_fields();    // the neighbourhood maxima of a ps_nbhd (ps_nbhd.hip)
PsFieldsOps ps_prox_fields();    // the distances in metres of a ps_prox (ps_prox.hip)

// the members' masks and the count planes of a ps_excur as ps_overlap.hip reads them on the device (ps_excur.hip).
// The mask block moves when it grows, so a reader takes the view at every call; it orders its stream behind the
// accumulator's last operation (wait) and the accumulator's next operation behind its read (mark).
struct PsExcurView {
  const uint64_t* mask;         // [members][nthr][nslot][pitch / 64], device
  const uint32_t* cnt;          // [nthr][nslot][pitch], device
  const uint32_t* weights;      // [members], host, in add order
  int64_t pitch, members;
  int N, nthr, nslot, device;
};
int ps_excur_view_internal(ps_excur* a, PsExcurView* out);
int ps_excur_wait_internal(ps_excur* a, hipStream_t stream);
int ps_excur_mark_internal(ps_excur* a, hipStream_t stream);

// the mean planes of an accumulator as ps_gain.hip's finish reads them on the device (ps_summary.hip; ps_wsum.hip
// per scenario); PS_ERR_STATE while nothing is accumulated.  The reader orders its stream behind the accumulator's
// last operation (wait) and the accumulator's next operation behind the read (done).
struct PsMeanView {
  const double* mean;           // [nslot][pitch], device
  int64_t pitch;
  int N, nslot, device;
};
int ps_summary_mean_internal(ps_summary* a, PsMeanView* out);
int ps_summary_mean_wait_internal(ps_summary* a, hipStream_t stream);
int ps_summary_mean_done_internal(ps_summary* a, hipStream_t stream);
int ps_wsum_mean_internal(ps_wsum* a, int scenario, PsMeanView* out);
int ps_wsum_mean_wait_internal(ps_wsum* a, hipStream_t stream);
int ps_wsum_mean_done_internal(ps_wsum* a, hipStream_t stream);

// the value one solver record holds at a cell, as ps_record_fetch_* returns it (k_compact_rows,
// chain_kernels.h), 0 where it returns no entry; shared by ps_summary.hip and ps_linspread.hip
__device__ inline double ps_record_value(double r, double stat_scale, double post_scale, double delta, double negval) {
  const double t = r * stat_scale;
  const bool keep = (t != 0.0) && !(t < negval);
  return keep ? (t + delta) * post_scale : 0.0;
}

// one weighted Welford step of a cell (West 1979), shared by ps_summary.hip and ps_sens.hip so that both round
// alike: false, and nothing changed, where the value equals the mean
__device__ inline bool sum_update(double v, double w, double Wn, double& m, double& m2) {
  const double d = v - m;
  if (d == 0.0) return false;          // mean and M2 stay bit for bit as they are
  m += d * w / Wn;
  m2 += w * d * (v - m);
  return true;
}
