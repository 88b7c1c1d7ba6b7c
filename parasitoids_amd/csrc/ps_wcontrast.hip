// Reweighted paired contrast of two release plans or two projections (include/parasitoid_hip.h, ps_wcontrast_*):
// what ps_contrast.hip accumulates of d = a - b, under up to 4 reweighting scenarios at once with the real weights
// of ps_wsum.hip (per member and scenario a rescale r of what is held and a weight omega on the new scale).
// a and b are the fields the two sources hold for the same member, so the pairing is kept.  Layout (pitch = N*N
// rounded up to 64 cells, every plane 16-byte aligned; P = 2 + 2 nthr sum planes), one device block, per scenario j
//   mean[j][slot][pitch], m2[j][slot][pitch], S[j][slot][P][pitch]       (all fp64)
// with the planes of S in the order pos (d > 0), neg (d < 0), gain_0 (a >= t_0 > b), loss_0 (b >= t_0 > a), gain_1 ..
// An add reads 16 B of a and b per cell and slot once and, per scenario that takes the member, 8 B of mean; M2 and
// the P sums (8 + 8 P B) only where a statement can change a bit -- the scenario is rescaled (r != 1), d != 0 or
// the mean != 0 -- which outside both plumes, most of the domain (0 - 0 against a mean of 0), is nowhere.  A pair
// of cells of a plane is written back only where a bit changed.  One thread owns a pair of cells: every cell has a
// single writer, there are no atomics and no LDS, and the same calls in the same order give the same bits.  The
// per-member coverage rows stay with the ps_contrast that is fed alongside.
#include <math.h>

#include <algorithm>

#include "ps_common.h"

#define PS_WCON_MAX_SCEN 4
#define PS_WCON_MAX_THR 4
#define PS_WCON_MAX_SLOT 32   // one launch: 32 descriptors = 768 B of kernel arguments

namespace {

struct WcSlot {
  const double* a;
  const double* b;
  int slot;
};
struct WcSlots {
  WcSlot s[PS_WCON_MAX_SLOT];
};
struct WcThr {
  double t[PS_WCON_MAX_THR];
};
// per scenario: the rescale r, the member's weight omega (0: the scenario is left untouched) and the total
// weight W after this member; the same for every lane, so they stay in scalar registers
struct WcScen {
  double r[PS_WCON_MAX_SCEN], om[PS_WCON_MAX_SCEN], W[PS_WCON_MAX_SCEN];
};

__device__ inline bool wc_differ(double a, double b) { return __double_as_longlong(a) != __double_as_longlong(b); }

// one cell of one scenario; every arithmetic step is a statement of its own (-ffp-contract=on fuses only within
// an expression), sum_update is the statement pair of ps_contrast_add on d
template <int K>
__device__ inline void wc_cell(double a, double b, double d, double r, double om, double W, const WcThr& thr, double& m,
                               double& q, double* s) {
  q = q * r;
#pragma unroll
  for (int p = 0; p < 2 + 2 * K; ++p) s[p] = s[p] * r;
  sum_update(d, om, W, m, q);   // nothing where d == m
  if (d > 0.0) s[0] = s[0] + om;
  if (d < 0.0) s[1] = s[1] + om;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double t = thr.t[k];
    if (a >= t && b < t) s[2 + 2 * k] = s[2 + 2 * k] + om;
    if (b >= t && a < t) s[3 + 2 * k] = s[3 + 2 * k] + om;
  }
}

// blockIdx.y = slot; a thread owns a pair of cells (the tail cell of an odd N*N alone), reads a and b once, forms
// d once and walks the NJ scenarios.  plane = nslot * pitch, jstride = (2 + P) * plane: the distance between two
// scenarios.  NJ and K are template arguments so that the scenario walk and the plane loops are straight code.
template <int NJ, int K>
__global__ void __launch_bounds__(256) k_wcontrast_add(WcSlots desc, double* __restrict__ block, int64_t ncell,
                                                       int64_t pitch, int64_t plane, WcThr thr, WcScen sc) {
  constexpr int P = 2 + 2 * K;
  const WcSlot sd = desc.s[blockIdx.y];
  const double* __restrict__ A = sd.a;
  const double* __restrict__ B = sd.b;
  const int64_t jstride = (int64_t)(2 + P) * plane;
  double* ms = block + (int64_t)sd.slot * pitch;
  double* qs = ms + plane;
  double* ss = block + 2 * plane + (int64_t)sd.slot * P * pitch;
  const int64_t npair = ncell >> 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= npair; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < npair) {
      const double2 ra = *reinterpret_cast<const double2*>(A + 2 * i);
      const double2 rb = *reinterpret_cast<const double2*>(B + 2 * i);
      const double d0 = __dsub_rn(ra.x, rb.x), d1 = __dsub_rn(ra.y, rb.y);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (!(sc.om[j] > 0.0)) continue;   // uniform: the member leaves this scenario untouched
        double* mp = ms + j * jstride + 2 * i;
        double* qp = qs + j * jstride + 2 * i;
        double* sp = ss + j * jstride + 2 * i;
        const double2 m0 = *reinterpret_cast<const double2*>(mp);
        // r == 1, d == 0 against a mean of 0: no statement changes a bit, so M2 and the sums are not read
        if (sc.r[j] == 1.0 && d0 == 0.0 && d1 == 0.0 && m0.x == 0.0 && m0.y == 0.0) continue;
        const double2 q0 = *reinterpret_cast<const double2*>(qp);
        double2 s0[P];
#pragma unroll
        for (int p = 0; p < P; ++p) s0[p] = *reinterpret_cast<const double2*>(sp + (int64_t)p * pitch);
        double2 m = m0, q = q0;
        double sx[P], sy[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
          sx[p] = s0[p].x;
          sy[p] = s0[p].y;
        }
        wc_cell<K>(ra.x, rb.x, d0, sc.r[j], sc.om[j], sc.W[j], thr, m.x, q.x, sx);
        wc_cell<K>(ra.y, rb.y, d1, sc.r[j], sc.om[j], sc.W[j], thr, m.y, q.y, sy);
        if (wc_differ(m.x, m0.x) || wc_differ(m.y, m0.y)) *reinterpret_cast<double2*>(mp) = m;
        if (wc_differ(q.x, q0.x) || wc_differ(q.y, q0.y)) *reinterpret_cast<double2*>(qp) = q;
#pragma unroll
        for (int p = 0; p < P; ++p)
          if (wc_differ(sx[p], s0[p].x) || wc_differ(sy[p], s0[p].y))
            *reinterpret_cast<double2*>(sp + (int64_t)p * pitch) = make_double2(sx[p], sy[p]);
      }
    } else if (ncell & 1) {
      const int64_t c = ncell - 1;
      const double a = A[c], b = B[c];
      const double d = __dsub_rn(a, b);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (!(sc.om[j] > 0.0)) continue;
        double* mp = ms + j * jstride + c;
        double* qp = qs + j * jstride + c;
        double* sp = ss + j * jstride + c;
        const double m0 = *mp;
        if (sc.r[j] == 1.0 && d == 0.0 && m0 == 0.0) continue;
        const double q0 = *qp;
        double m = m0, q = q0;
        double s0[P], s[P];
#pragma unroll
        for (int p = 0; p < P; ++p) s[p] = s0[p] = sp[(int64_t)p * pitch];
        wc_cell<K>(a, b, d, sc.r[j], sc.om[j], sc.W[j], thr, m, q, s);
        if (wc_differ(m, m0)) *mp = m;
        if (wc_differ(q, q0)) *qp = q;
#pragma unroll
        for (int p = 0; p < P; ++p)
          if (wc_differ(s[p], s0[p])) sp[(int64_t)p * pitch] = s[p];
      }
    }
  }
}

using WcAddKernel = void (*)(WcSlots, double*, int64_t, int64_t, int64_t, WcThr, WcScen);
#define WC_ROW(J) \
  {k_wcontrast_add<J, 0>, k_wcontrast_add<J, 1>, k_wcontrast_add<J, 2>, k_wcontrast_add<J, 3>, k_wcontrast_add<J, 4>}
// k_wcontrast_add<nscen, nthr>, nscen = 1 .. 4, nthr = 0 .. 4
const WcAddKernel wc_add_kernels[PS_WCON_MAX_SCEN][PS_WCON_MAX_THR + 1] = {WC_ROW(1), WC_ROW(2), WC_ROW(3), WC_ROW(4)};

// Chan, Golub & LeVeque on one scenario, both sides brought to a common scale by ra and rb, with the expressions
// of k_wsum_merge: Wa = Wa0 ra, Wb = Wb0 rb (from the host).  nval cells of mean and M2, nsum of the sums.
__global__ void __launch_bounds__(256) k_wcontrast_merge(double* __restrict__ ma, double* __restrict__ qa,
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

struct ps_wcontrast {
  int device = 0, N = 0, nscen = 0, nslot = 0, nthr = 0;
  double thr[PS_WCON_MAX_THR] = {0, 0, 0, 0};
  int64_t ncell = 0, pitch = 0;
  double* block = nullptr;   // per scenario: mean | M2 | S
  double W[PS_WCON_MAX_SCEN] = {0, 0, 0, 0};
  int64_t members[PS_WCON_MAX_SCEN] = {0, 0, 0, 0};
  int64_t skipped[PS_WCON_MAX_SCEN] = {0, 0, 0, 0};
  hipStream_t stream = nullptr;   // every operation of the handle
  PsLastOp last;                  // the last operation
  PsProf prof;                    // channel 0: the adds
};

static int wc_planes(const ps_wcontrast* h) { return 2 + 2 * h->nthr; }
static int64_t wc_plane(const ps_wcontrast* h) { return (int64_t)h->nslot * h->pitch; }
static int64_t wc_scen_cells(const ps_wcontrast* h) { return (int64_t)(2 + wc_planes(h)) * wc_plane(h); }
static double wc_block_bytes(int nscen, int nslot, int nthr, int64_t pitch) {
  return (double)nscen * (double)(4 + 2 * nthr) * (double)nslot * (double)pitch * sizeof(double);
}
static double* wc_mean(const ps_wcontrast* h, int j) { return h->block + (int64_t)j * wc_scen_cells(h); }
static double* wc_m2(const ps_wcontrast* h, int j) { return wc_mean(h, j) + wc_plane(h); }
static double* wc_S(const ps_wcontrast* h, int j) { return wc_mean(h, j) + 2 * wc_plane(h); }

static bool wc_finite(double v) { return v == v && !isinf(v); }

extern "C" void ps_wcontrast_destroy(ps_wcontrast* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  h->last.sync();
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->prof.release();
  if (h->block) (void)hipFree(h->block);
  h->last.destroy();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ps_wcontrast_reset(ps_wcontrast* h) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_reset: null handle");
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  PS_HIP(hipMemsetAsync(h->block, 0, (size_t)wc_block_bytes(h->nscen, h->nslot, h->nthr, h->pitch), h->stream));
  PS_TRY(h->last.mark(h->stream));
  for (int j = 0; j < PS_WCON_MAX_SCEN; ++j) {
    h->W[j] = 0.0;
    h->members[j] = 0;
    h->skipped[j] = 0;
  }
  return PS_OK;
}

extern "C" int ps_wcontrast_create(int device, int N, int nscen, int nslot, int nthr, const double* thr,
                                   ps_wcontrast** out) {
  if (out) *out = nullptr;
  if (!out || N < 1 || nscen < 1 || nscen > PS_WCON_MAX_SCEN || nslot < 1 || nslot > PS_WCON_MAX_SLOT || nthr < 0 ||
      nthr > PS_WCON_MAX_THR || (nthr > 0 && !thr))
    return ps_fail(PS_ERR_BAD_ARG, "wcontrast_create: N %d, %d scenarios (1..%d), %d slots (1..%d), %d thresholds (0..%d)",
                   N, nscen, PS_WCON_MAX_SCEN, nslot, PS_WCON_MAX_SLOT, nthr, PS_WCON_MAX_THR);
  for (int k = 0; k < nthr; ++k) {
    if (!wc_finite(thr[k]) || !(thr[k] > 0.0))
      return ps_fail(PS_ERR_BAD_ARG, "wcontrast_create: threshold %d is not finite and > 0", k);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "wcontrast_create: the thresholds are not strictly increasing at %d", k);
  }
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // the whole block, checked before anything is allocated
  const double need = wc_block_bytes(nscen, nslot, nthr, pitch);
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM,
                   "wcontrast_create: %d scenarios x (4 + 2 x %d) x 8 B x %d slots x %lld cells = %.3g GB, %.3g GB free",
                   nscen, nthr, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_wcontrast* h = new ps_wcontrast();
  h->device = device;
  h->N = N;
  h->nscen = nscen;
  h->nslot = nslot;
  h->nthr = nthr;
  for (int k = 0; k < nthr; ++k) h->thr[k] = thr[k];
  h->ncell = ncell;
  h->pitch = pitch;
  auto fail = [&](int rc) {
    ps_wcontrast_destroy(h);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = h->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&h->block, (size_t)need);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "wcontrast_create: %s", hipGetErrorString(e)));
  int rc = ps_wcontrast_reset(h);
  if (rc != PS_OK) return fail(rc);
  *out = h;
  return PS_OK;
}

// one member whose values are the current fields of two projections or two release plans (who: the entry point);
// everything is checked before anything is enqueued: a refused add changes nothing
static int wc_add_fields(ps_wcontrast* h, void* a, void* b, const PsFieldsOps& src, const char* who, int nscen,
                         const double* rescale, const double* omega) {
  if (!h || !a || !b || !rescale || !omega) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (a == b) return ps_fail(PS_ERR_BAD_ARG, "%s: both sides are the same %s", who, src.what);
  if (nscen != h->nscen) return ps_fail(PS_ERR_BAD_ARG, "%s: %d scenarios given, the handle has %d", who, nscen, h->nscen);
  for (int j = 0; j < nscen; ++j) {
    if (!(rescale[j] >= 0.0 && rescale[j] <= 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "%s: rescale[%d] = %g is not in [0, 1]", who, j, rescale[j]);
    if (!wc_finite(omega[j]) || omega[j] < 0.0)
      return ps_fail(PS_ERR_BAD_ARG, "%s: omega[%d] = %g is not finite and >= 0", who, j, omega[j]);
  }
  PsProjectView v[2];
  void* side[2] = {a, b};
  for (int s = 0; s < 2; ++s) {
    PS_TRY(src.view(side[s], &v[s]));
    const char* name = s == 0 ? "A" : "B";
    if (v[s].nout != h->nslot)
      return ps_fail(PS_ERR_BAD_ARG, "%s: %s %s has %d outputs, the handle %d slots", who, src.what, name, v[s].nout,
                     h->nslot);
    if (v[s].device != h->device)
      return ps_fail(PS_ERR_BAD_ARG, "%s: %s %s on device %d, handle on device %d", who, src.what, name, v[s].device,
                     h->device);
    if (v[s].N != h->N)
      return ps_fail(PS_ERR_BAD_ARG, "%s: %s %s domain %d, handle domain %d", who, src.what, name, v[s].N, h->N);
  }
  PS_HIP(hipSetDevice(h->device));
  WcScen sc;
  bool any = false;
  for (int j = 0; j < PS_WCON_MAX_SCEN; ++j) {
    sc.r[j] = 1.0;
    sc.om[j] = 0.0;
    sc.W[j] = 0.0;
    if (j < h->nscen && omega[j] > 0.0) {
      double W = h->W[j];
      W = W * rescale[j];
      W = W + omega[j];
      sc.r[j] = rescale[j];
      sc.om[j] = omega[j];
      sc.W[j] = W;
      any = true;
    }
  }
  if (any) {
    hipStream_t stream = h->stream;
    PS_TRY(src.wait(a, stream));
    PS_TRY(src.wait(b, stream));
    PS_TRY(h->last.wait(stream));
    hipEvent_t e1 = nullptr;
    PS_TRY(h->prof.begin(0, stream, &e1));
    WcThr thr;
    for (int k = 0; k < PS_WCON_MAX_THR; ++k) thr.t[k] = h->thr[k];
    WcSlots desc;
    for (int i = 0; i < PS_WCON_MAX_SLOT; ++i) {
      const int e = std::min(i, h->nslot - 1);
      desc.s[i] = WcSlot{v[0].Y + (int64_t)e * v[0].pitch, v[1].Y + (int64_t)e * v[1].pitch, e};
    }
    const int64_t nitem = h->ncell / 2 + 1;
    const int threads = 256;
    const int bx = (int)std::min<int64_t>((nitem + threads - 1) / threads, 4096);
    hipLaunchKernelGGL(wc_add_kernels[h->nscen - 1][h->nthr], dim3(bx, h->nslot), dim3(threads), 0, stream, desc,
                       h->block, h->ncell, h->pitch, wc_plane(h), thr, sc);
    PS_HIP(hipGetLastError());
    PS_TRY(h->prof.end(stream, e1));
    PS_TRY(h->last.mark(stream));
    PS_TRY(src.mark(a, stream));   // the next apply of either side overwrites Y only after this read
    PS_TRY(src.mark(b, stream));
  }
  for (int j = 0; j < h->nscen; ++j) {
    if (omega[j] > 0.0) {
      h->W[j] = sc.W[j];
      h->members[j] += 1;
    } else {
      h->skipped[j] += 1;
    }
  }
  return PS_OK;
}

extern "C" int ps_wcontrast_add_sites(ps_wcontrast* h, ps_sites* a, ps_sites* b, int nscen, const double* rescale,
                                      const double* omega) {
  return wc_add_fields(h, a, b, ps_sites_fields(), "wcontrast_add_sites", nscen, rescale, omega);
}

extern "C" int ps_wcontrast_add_project(ps_wcontrast* h, ps_project* a, ps_project* b, int nscen, const double* rescale,
                                        const double* omega) {
  return wc_add_fields(h, a, b, ps_project_fields(), "wcontrast_add_project", nscen, rescale, omega);
}

extern "C" int ps_wcontrast_merge(ps_wcontrast* dst, ps_wcontrast* src, const double* ra, const double* rb) {
  if (!dst || !src || !ra || !rb) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_merge: bad arguments");
  if (dst == src) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_merge: dst and src are the same handle");
  if (dst->device != src->device || dst->N != src->N || dst->nscen != src->nscen || dst->nslot != src->nslot ||
      dst->nthr != src->nthr)
    return ps_fail(PS_ERR_BAD_ARG, "wcontrast_merge: handles differ in device, domain, scenarios, slots or thresholds");
  for (int k = 0; k < dst->nthr; ++k)
    if (dst->thr[k] != src->thr[k]) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_merge: threshold %d differs", k);
  for (int j = 0; j < dst->nscen; ++j)
    if (!(ra[j] >= 0.0 && ra[j] <= 1.0) || !(rb[j] >= 0.0 && rb[j] <= 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "wcontrast_merge: scale (%g, %g) of scenario %d is not in [0, 1]", ra[j], rb[j], j);
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  const int64_t nval = wc_plane(dst);
  const size_t scen_bytes = (size_t)wc_scen_cells(dst) * sizeof(double);
  for (int j = 0; j < dst->nscen; ++j) {
    if (src->W[j] == 0.0) {
      dst->skipped[j] += src->skipped[j];
      continue;
    }
    if (dst->W[j] == 0.0) {   // a copy: the merged scenario is src's bit for bit
      PS_HIP(hipMemcpyAsync(wc_mean(dst, j), wc_mean(src, j), scen_bytes, hipMemcpyDeviceToDevice, dst->stream));
      dst->W[j] = src->W[j];
    } else {
      double Wa = dst->W[j];
      Wa = Wa * ra[j];
      double Wb = src->W[j];
      Wb = Wb * rb[j];
      hipLaunchKernelGGL(k_wcontrast_merge, dim3(2048), dim3(256), 0, dst->stream, wc_mean(dst, j), wc_m2(dst, j),
                         wc_S(dst, j), wc_mean(src, j), wc_m2(src, j), wc_S(src, j), nval, nval * wc_planes(dst), ra[j],
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

extern "C" int ps_wcontrast_info(ps_wcontrast* h, double* total_weight, int64_t* members, int64_t* skipped) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_info: null handle");
  for (int j = 0; j < h->nscen; ++j) {
    if (total_weight) total_weight[j] = h->W[j];
    if (members) members[j] = h->members[j];
    if (skipped) skipped[j] = h->skipped[j];
  }
  return PS_OK;
}

extern "C" int ps_wcontrast_fetch(ps_wcontrast* h, int scen, int slot, int what, double* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_fetch: bad arguments");
  if (scen < 0 || scen >= h->nscen) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_fetch: scenario %d of %d", scen, h->nscen);
  if (slot < 0 || slot >= h->nslot) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_fetch: slot %d of %d", slot, h->nslot);
  if (what < 0 || what >= 2 + wc_planes(h))
    return ps_fail(PS_ERR_BAD_ARG,
                   "wcontrast_fetch: quantity %d (0 mean, 1 variance, 2 P(d > 0), 3 P(d < 0), 4..%d gain / loss)", what,
                   1 + wc_planes(h));
  if (h->W[scen] == 0.0)
    return ps_fail(PS_ERR_STATE, "wcontrast_fetch: nothing accumulated in scenario %d (W = 0)", scen);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const double W = h->W[scen];
  const size_t n = (size_t)h->ncell;
  const double* src = what == 0   ? wc_mean(h, scen) + (int64_t)slot * h->pitch
                      : what == 1 ? wc_m2(h, scen) + (int64_t)slot * h->pitch
                                  : wc_S(h, scen) + ((int64_t)slot * wc_planes(h) + (what - 2)) * h->pitch;
  PS_HIP(hipMemcpyAsync(out, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
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

extern "C" int ps_wcontrast_prof(ps_wcontrast* h, int enable, double* total_ms, int64_t* launches) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "wcontrast_prof: null handle");
  PS_HIP(hipSetDevice(h->device));
  h->prof.set(enable);
  if (total_ms || launches) PS_TRY(h->prof.totals(0, total_ms, launches));
  return PS_OK;
}
