// Weather and parameter variance of the posterior maps (include/parasitoid_hip.h, ps_nested_*): the members come in
// groups -- one parameter vector under several wind sequences -- and the variance of every cell is split into the
// part within the groups (weather at fixed parameters) and the part between their means (parameters).  Layout
// (pitch = N*N rounded up to 64 cells, as ps_summary.hip), fp64 planes of [slot][pitch]:
//   imean, iM2     the open group: its draws with weight 1 each (Welford)
//   omean, oM2     Welford over the closed groups' means with weights w_g (West 1979)
//   wS             sum over the closed groups of w_g s2_g, s2_g = iM2 / (k_g - 1)
//   vw, vp, share  what ps_nested_finalize leaves
// The host keeps the open group's draws k, the closed groups G, their weight W, sum w_g / k_g and the members.
// Every operation is rounded on its own (__dadd_rn, __dsub_rn, __dmul_rn, __ddiv_rn: no contraction), so that a
// numpy loop over the same statements reproduces every plane bit for bit.  An add reads 8 B of record and reads
// 32 B of the open group's planes per cell and slot and writes them where a cell of the pair changed; a close reads
// five planes and writes what changed.  One thread owns a pair of cells (16-byte accesses; the tail cell of the odd
// N*N has a thread of its own), one launch covers all pairs: no grid stride, no atomics, no LDS.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_NST_CHUNK 32          // slots per add launch: 32 descriptors of kernel arguments, as ps_mcerr.hip
#define PS_NST_THREADS 256

namespace {

struct NstSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct NstSlots {
  NstSlot s[PS_NST_CHUNK];
};

// draw number kn of the open group: d = v - imean; where d != 0, imean' = imean + d / kn, iM2 += d (v - imean')
__device__ inline bool nst_draw(double v, double kn, double& m, double& q) {
  const double d = __dsub_rn(v, m);
  if (d == 0.0) return false;
  m = __dadd_rn(m, __ddiv_rn(d, kn));
  q = __dadd_rn(q, __dmul_rn(d, __dsub_rn(v, m)));
  return true;
}

// blockIdx.y = slot of the chunk; thread j < npair owns cells 2j and 2j + 1, thread npair the tail cell of an odd N*N
__global__ void __launch_bounds__(PS_NST_THREADS)
    k_nested_add(NstSlots desc, double* __restrict__ imean, double* __restrict__ im2, int64_t ncell, int64_t pitch,
                 double negval, double kn) {
  const NstSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double* __restrict__ rec = sd.rec;
  double* ms = imean + (int64_t)sd.slot * pitch;
  double* qs = im2 + (int64_t)sd.slot * pitch;
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j < npair) {
    const double2 r = *reinterpret_cast<const double2*>(rec + 2 * j);
    double2 m = *reinterpret_cast<const double2*>(ms + 2 * j);
    double2 q = *reinterpret_cast<const double2*>(qs + 2 * j);
    const bool c0 = nst_draw(ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval), kn, m.x, q.x);
    const bool c1 = nst_draw(ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval), kn, m.y, q.y);
    if (c0 || c1) {
      *reinterpret_cast<double2*>(ms + 2 * j) = m;
      *reinterpret_cast<double2*>(qs + 2 * j) = q;
    }
  } else if (j == npair && (ncell & 1)) {
    const int64_t i = ncell - 1;
    double m = ms[i], q = qs[i];
    if (nst_draw(ps_record_value(rec[i], sd.stat_scale, sd.post_scale, delta, negval), kn, m, q)) {
      ms[i] = m;
      qs[i] = q;
    }
  }
}

// one cell of the close of a group of km1 + 1 draws with weight w, Wn the closed weight with it
__device__ inline void nst_close(double m, double q, double& g, double& h, double& s, double w, double km1, double Wn) {
  s = __dadd_rn(s, __dmul_rn(w, __ddiv_rn(q, km1)));
  const double d = __dsub_rn(m, g);
  if (d != 0.0) {
    g = __dadd_rn(g, __ddiv_rn(__dmul_rn(d, w), Wn));
    h = __dadd_rn(h, __dmul_rn(__dmul_rn(w, d), __dsub_rn(m, g)));
  }
}

// pairs of cells over all slots (nval = nslot * pitch, a multiple of 64); the open group's planes are +0.0 after it
__global__ void __launch_bounds__(PS_NST_THREADS)
    k_nested_close(double* __restrict__ imean, double* __restrict__ im2, double* __restrict__ omean,
                   double* __restrict__ om2, double* __restrict__ ws, int64_t nval, double w, double km1, double Wn) {
  const int64_t i = 2 * (blockIdx.x * (int64_t)blockDim.x + threadIdx.x);
  if (i >= nval) return;
  const double2 m = *reinterpret_cast<const double2*>(imean + i);
  const double2 q = *reinterpret_cast<const double2*>(im2 + i);
  double2 g = *reinterpret_cast<const double2*>(omean + i);
  if (q.x != 0.0 || q.y != 0.0 || m.x != g.x || m.y != g.y) {   // else: wS gains +0.0 and the means are met
    double2 h = *reinterpret_cast<const double2*>(om2 + i);
    double2 s = *reinterpret_cast<const double2*>(ws + i);
    nst_close(m.x, q.x, g.x, h.x, s.x, w, km1, Wn);
    nst_close(m.y, q.y, g.y, h.y, s.y, w, km1, Wn);
    *reinterpret_cast<double2*>(omean + i) = g;
    *reinterpret_cast<double2*>(om2 + i) = h;
    *reinterpret_cast<double2*>(ws + i) = s;
  }
  if (m.x != 0.0 || m.y != 0.0) *reinterpret_cast<double2*>(imean + i) = make_double2(0.0, 0.0);
  if (q.x != 0.0 || q.y != 0.0) *reinterpret_cast<double2*>(im2 + i) = make_double2(0.0, 0.0);
}

// Chan, Golub & LeVeque on (omean, oM2) with the closed weights, the expressions of k_dep_merge; wS adds
__global__ void __launch_bounds__(PS_NST_THREADS)
    k_nested_merge(double* __restrict__ ma, double* __restrict__ qa, double* __restrict__ sa,
                   const double* __restrict__ mb, const double* __restrict__ qb, const double* __restrict__ sb,
                   int64_t nval, double Wa, double Wb) {
  const double W = Wa + Wb;
  const double fb = __ddiv_rn(Wb, W);
  const double fab = __ddiv_rn(__dmul_rn(Wa, Wb), W);
  const int64_t i = 2 * (blockIdx.x * (int64_t)blockDim.x + threadIdx.x);
  if (i >= nval) return;
  double2 a = *reinterpret_cast<const double2*>(ma + i);
  double2 q = *reinterpret_cast<const double2*>(qa + i);
  double2 s = *reinterpret_cast<const double2*>(sa + i);
  const double2 b = *reinterpret_cast<const double2*>(mb + i);
  const double2 r = *reinterpret_cast<const double2*>(qb + i);
  const double2 t = *reinterpret_cast<const double2*>(sb + i);
  const double d0 = __dsub_rn(b.x, a.x), d1 = __dsub_rn(b.y, a.y);
  a.x = __dadd_rn(a.x, __dmul_rn(d0, fb));
  a.y = __dadd_rn(a.y, __dmul_rn(d1, fb));
  q.x = __dadd_rn(__dadd_rn(q.x, r.x), __dmul_rn(__dmul_rn(d0, d0), fab));
  q.y = __dadd_rn(__dadd_rn(q.y, r.y), __dmul_rn(__dmul_rn(d1, d1), fab));
  s.x = __dadd_rn(s.x, t.x);
  s.y = __dadd_rn(s.y, t.y);
  *reinterpret_cast<double2*>(ma + i) = a;
  *reinterpret_cast<double2*>(qa + i) = q;
  *reinterpret_cast<double2*>(sa + i) = s;
}

// vw = wS / W; vm = oM2 / W; vp = vm - vw kinv, +0.0 unless > 0; share = vw / (vp + vw), +0.0 where that is not > 0
__device__ inline void nst_final(double h, double s, double W, double kinv, double& vw, double& vp, double& share) {
  vw = __ddiv_rn(s, W);
  vp = __dsub_rn(__ddiv_rn(h, W), __dmul_rn(vw, kinv));
  if (!(vp > 0.0)) vp = 0.0;
  const double tot = __dadd_rn(vp, vw);
  share = tot > 0.0 ? __ddiv_rn(vw, tot) : 0.0;
}

__global__ void __launch_bounds__(PS_NST_THREADS)
    k_nested_finalize(const double* __restrict__ om2, const double* __restrict__ ws, double* __restrict__ vw,
                      double* __restrict__ vp, double* __restrict__ share, int64_t nval, double W, double kinv) {
  const int64_t i = 2 * (blockIdx.x * (int64_t)blockDim.x + threadIdx.x);
  if (i >= nval) return;
  const double2 h = *reinterpret_cast<const double2*>(om2 + i);
  const double2 s = *reinterpret_cast<const double2*>(ws + i);
  double2 a, b, c;
  nst_final(h.x, s.x, W, kinv, a.x, b.x, c.x);
  nst_final(h.y, s.y, W, kinv, a.y, b.y, c.y);
  *reinterpret_cast<double2*>(vw + i) = a;
  *reinterpret_cast<double2*>(vp + i) = b;
  *reinterpret_cast<double2*>(share + i) = c;
}

}  // namespace

enum { NST_IMEAN = 0, NST_IM2 = 1, NST_OMEAN = 2, NST_OM2 = 3, NST_WS = 4, NST_VW = 5, NST_VP = 6, NST_SHARE = 7,
       NST_PLANES = 8 };

struct ps_nested {
  int device = 0, N = 0, nslot = 0;
  int64_t ncell = 0, pitch = 0;
  double* val = nullptr;          // eight fp64 planes of [slot][pitch], in the order of the enum above
  uint64_t k = 0;                 // draws in the open group
  uint64_t G = 0;                 // closed groups
  double W = 0.0;                 // their weight: integers, exact below 2^53
  double wk = 0.0;                // sum of w_g / k_g
  int64_t members = 0;            // draws added
  bool final_ok = false;          // vw, vp, share belong to the present groups
  hipStream_t stream = nullptr;   // reset / close / merge / finalize / fetch
  PsLastOp last;                  // the last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds, 1: the closes
};

static size_t nst_plane(const ps_nested* h) { return (size_t)h->nslot * h->pitch; }
static double* nst_val(const ps_nested* h, int which) { return h->val + (size_t)which * nst_plane(h); }
static unsigned nst_blocks(int64_t pairs) { return (unsigned)((pairs + PS_NST_THREADS - 1) / PS_NST_THREADS); }

extern "C" void ps_nested_destroy(ps_nested* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  h->last.sync();
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->prof.release();
  if (h->val) (void)hipFree(h->val);
  h->last.destroy();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ps_nested_reset(ps_nested* h) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "nested_reset: null handle");
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  PS_HIP(hipMemsetAsync(h->val, 0, NST_PLANES * nst_plane(h) * sizeof(double), h->stream));
  PS_TRY(h->last.mark(h->stream));
  h->k = h->G = 0;
  h->W = h->wk = 0.0;
  h->members = 0;
  h->final_ok = false;
  return PS_OK;
}

extern "C" int ps_nested_create(int device, int N, int nslot, ps_nested** out) {
  if (!out || N < 1 || nslot < 1) return ps_fail(PS_ERR_BAD_ARG, "nested_create: N %d, %d slots", N, nslot);
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // everything, checked before anything is allocated: eight fp64 planes
  const double need = (double)nslot * pitch * 8.0 * NST_PLANES;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "nested_create: %d slots x %lld cells x %d B = %.3g GB, %.3g GB free", nslot,
                   (long long)pitch, 8 * NST_PLANES, need * 1e-9, (double)free_b * 1e-9);
  ps_nested* h = new ps_nested();
  h->device = device;
  h->N = N;
  h->nslot = nslot;
  h->ncell = ncell;
  h->pitch = pitch;
  auto fail = [&](int rc) {
    ps_nested_destroy(h);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = h->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&h->val, NST_PLANES * nst_plane(h) * sizeof(double));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "nested_create: %s", hipGetErrorString(e)));
  int rc = ps_nested_reset(h);
  if (rc != PS_OK) return fail(rc);
  *out = h;
  return PS_OK;
}

// a timing pair on `channel` around what `body` enqueues on `stream` (nothing without profiling)
template <typename F>
static int nst_timed(ps_nested* h, int channel, hipStream_t stream, F body) {
  hipEvent_t e1 = nullptr;
  PS_TRY(h->prof.begin(channel, stream, &e1));
  PS_TRY(body());
  return h->prof.end(stream, e1);
}

// one draw of the open group from the slot descriptors d (one per slot), enqueued on `stream`
static int nst_launch(ps_nested* h, const std::vector<PsSrc>& d, hipStream_t stream, double negval) {
  PS_TRY(h->last.wait(stream));
  const double kn = (double)(h->k + 1);
  const unsigned bx = nst_blocks(h->ncell / 2 + 1);
  int rc = nst_timed(h, 0, stream, [&]() {
    for (int c0 = 0; c0 < h->nslot; c0 += PS_NST_CHUNK) {
      const int n = std::min(PS_NST_CHUNK, h->nslot - c0);
      NstSlots desc;
      for (int i = 0; i < PS_NST_CHUNK; ++i)
        desc.s[i] = i < n ? ps_slotted<NstSlot>(d[(size_t)(c0 + i)], c0 + i) : NstSlot{nullptr, nullptr, 0.0, 0.0, 0};
      hipLaunchKernelGGL(k_nested_add, dim3(bx, n), dim3(PS_NST_THREADS), 0, stream, desc, nst_val(h, NST_IMEAN),
                         nst_val(h, NST_IM2), h->ncell, h->pitch, negval, kn);
      PS_HIP(hipGetLastError());
    }
    return (int)PS_OK;
  });
  PS_TRY(h->last.mark(stream));
  if (rc != PS_OK) return rc;
  h->k += 1;
  h->members += 1;
  h->final_ok = false;
  return PS_OK;
}

extern "C" int ps_nested_add(ps_nested* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                             const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                             double negval) {
  if (!h || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "nested_add: bad arguments");
  if (nslot != h->nslot) return ps_fail(PS_ERR_BAD_ARG, "nested_add: %d slots given, the handle has %d", nslot, h->nslot);
  PS_HIP(hipSetDevice(h->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("nested_add", "handle", h->device, h->N, s, nslot, kind, idx, stat_scale, post_scale,
                         use_delta, false, d.data(), &stream));
  return nst_launch(h, d, stream, negval);
}

// one draw whose values are the current fields of a projection or a release plan (who: the entry point)
static int nst_add_fields(ps_nested* h, void* p, const PsFieldsOps& src, const char* who) {
  if (!h || !p) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  std::vector<PsSrc> d((size_t)h->nslot);
  PS_TRY(ps_read_fields(who, "handle", "slots", h->device, h->N, h->nslot, p, src, d.data()));
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(src.wait(p, h->stream));
  PS_TRY(nst_launch(h, d, h->stream, 0.0));
  return src.mark(p, h->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_nested_add_project(ps_nested* h, ps_project* p) {
  return nst_add_fields(h, p, ps_project_fields(), "nested_add_project");
}

extern "C" int ps_nested_add_sites(ps_nested* h, ps_sites* p) {
  return nst_add_fields(h, p, ps_sites_fields(), "nested_add_sites");
}

extern "C" int ps_nested_close(ps_nested* h, uint32_t weight) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "nested_close: null handle");
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "nested_close: weight must be >= 1");
  if (h->k < 2)
    return ps_fail(PS_ERR_STATE, "nested_close: the open group has %llu draws, 2 needed", (unsigned long long)h->k);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const double w = (double)weight, Wn = h->W + w;
  const int64_t nval = (int64_t)nst_plane(h);
  int rc = nst_timed(h, 1, h->stream, [&]() {
    hipLaunchKernelGGL(k_nested_close, dim3(nst_blocks(nval / 2)), dim3(PS_NST_THREADS), 0, h->stream,
                       nst_val(h, NST_IMEAN), nst_val(h, NST_IM2), nst_val(h, NST_OMEAN), nst_val(h, NST_OM2),
                       nst_val(h, NST_WS), nval, w, (double)(h->k - 1), Wn);
    PS_HIP(hipGetLastError());
    return (int)PS_OK;
  });
  PS_TRY(h->last.mark(h->stream));
  if (rc != PS_OK) return rc;
  h->wk += w / (double)h->k;
  h->W = Wn;
  h->G += 1;
  h->k = 0;
  h->final_ok = false;
  return PS_OK;
}

extern "C" int ps_nested_merge(ps_nested* dst, ps_nested* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "nested_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "nested_merge: handles differ in device, domain or slots");
  if (dst->k || src->k)
    return ps_fail(PS_ERR_STATE, "nested_merge: an open group of %llu draws (close first)",
                   (unsigned long long)(dst->k ? dst->k : src->k));
  if (src->G > 0) {
    PS_HIP(hipSetDevice(dst->device));
    PS_TRY(dst->last.wait(dst->stream));
    PS_TRY(src->last.wait(dst->stream));
    const int64_t nval = (int64_t)nst_plane(dst);
    if (dst->G == 0) {   // a copy: the merged handle is src bit for bit (the open group's planes of both are zero)
      PS_HIP(hipMemcpyAsync(nst_val(dst, NST_OMEAN), nst_val(src, NST_OMEAN), 3 * (size_t)nval * sizeof(double),
                            hipMemcpyDeviceToDevice, dst->stream));
    } else {
      hipLaunchKernelGGL(k_nested_merge, dim3(nst_blocks(nval / 2)), dim3(PS_NST_THREADS), 0, dst->stream,
                         nst_val(dst, NST_OMEAN), nst_val(dst, NST_OM2), nst_val(dst, NST_WS), nst_val(src, NST_OMEAN),
                         nst_val(src, NST_OM2), nst_val(src, NST_WS), nval, dst->W, src->W);
      PS_HIP(hipGetLastError());
    }
    PS_TRY(dst->last.mark(dst->stream));
    PS_TRY(src->last.mark(dst->stream));   // src is read until then
    dst->final_ok = false;
  }
  dst->G += src->G;
  dst->W += src->W;
  dst->wk += src->wk;
  dst->members += src->members;
  return PS_OK;
}

extern "C" int ps_nested_finalize(ps_nested* h) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "nested_finalize: null handle");
  if (h->k)
    return ps_fail(PS_ERR_STATE, "nested_finalize: an open group of %llu draws (close first)", (unsigned long long)h->k);
  if (h->G < 2) return ps_fail(PS_ERR_STATE, "nested_finalize: %llu closed groups, 2 needed", (unsigned long long)h->G);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const int64_t nval = (int64_t)nst_plane(h);
  hipLaunchKernelGGL(k_nested_finalize, dim3(nst_blocks(nval / 2)), dim3(PS_NST_THREADS), 0, h->stream,
                     nst_val(h, NST_OM2), nst_val(h, NST_WS), nst_val(h, NST_VW), nst_val(h, NST_VP),
                     nst_val(h, NST_SHARE), nval, h->W, h->wk / h->W);
  PS_HIP(hipGetLastError());
  PS_TRY(h->last.mark(h->stream));
  h->final_ok = true;
  return PS_OK;
}

extern "C" int ps_nested_info(ps_nested* h, double* total_weight, int64_t* members, int64_t* groups,
                              int64_t* open_draws, double* weight_per_draws) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "nested_info: null handle");
  if (total_weight) *total_weight = h->W;
  if (members) *members = h->members;
  if (groups) *groups = (int64_t)h->G;
  if (open_draws) *open_draws = (int64_t)h->k;
  if (weight_per_draws) *weight_per_draws = h->wk;
  return PS_OK;
}

extern "C" int ps_nested_fetch(ps_nested* h, int slot, int what, double* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "nested_fetch: bad arguments");
  if (slot < 0 || slot >= h->nslot) return ps_fail(PS_ERR_BAD_ARG, "nested_fetch: slot %d of %d", slot, h->nslot);
  if (what < 0 || what >= NST_PLANES)
    return ps_fail(PS_ERR_BAD_ARG, "nested_fetch: plane %d (0 imean, 1 iM2, 2 omean, 3 oM2, 4 wS, 5 vw, 6 vp, 7 share)", what);
  if (what >= NST_VW && !h->final_ok)
    return ps_fail(PS_ERR_STATE, "nested_fetch: plane %d is a result: finalize after the last add, close or merge", what);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const double* src = nst_val(h, what) + (int64_t)slot * h->pitch;
  PS_HIP(hipMemcpyAsync(out, src, (size_t)h->ncell * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_nested_prof(ps_nested* h, int enable, double* add_ms, int64_t* add_launches, double* close_ms,
                              int64_t* close_launches) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "nested_prof: null handle");
  PS_HIP(hipSetDevice(h->device));
  h->prof.set(enable);
  if (add_ms || add_launches) PS_TRY(h->prof.totals(0, add_ms, add_launches));
  if (close_ms || close_launches) PS_TRY(h->prof.totals(1, close_ms, close_launches));
  return PS_OK;
}
