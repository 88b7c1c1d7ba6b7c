// Posterior sensitivity maps (include/parasitoid_hip.h, ps_sens_*): per-cell weighted co-moments between the
// fields of many model evaluations and up to 16 scalars the caller supplies per member (the model parameters
// behind the member), accumulated on the device from the solver's records, a projection's or a release plan's
// fields.  Layout as ps_summary.hip (pitch = N*N rounded up to 64 cells, every slot 16-byte aligned), one
// device block carved into
//   mean[slot][pitch], M2[slot][pitch], C[param][slot][pitch], expl[slot][pitch]   (fp64), dom[slot][pitch] (uint8)
// so a flat index slot*pitch + cell addresses the same cell in every array.  Pad cells stay 0.
// An add reads 8 B of record and reads + writes 16 B of mean, 16 B of M2 and 16 B per parameter of every cell
// of every slot -- nothing but the record and the two moments where a pair of cells is unchanged
// (value == mean), which outside the plume is most of the domain.
#include <math.h>

#include <vector>

#include "ps_common.h"

#define PS_SENS_MAX_PARAM 16
#define PS_SENS_CHUNK 32   // slots per launch: 32 descriptors = 1.3 kB of kernel arguments
#define PS_SENS_BATCH 8    // co-moment pairs loaded before the first multiply: 8 x 16 B in flight per lane

namespace {

struct SensSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct SensSlots {
  SensSlot s[PS_SENS_CHUNK];
};
// the member's deviations e_i: the same for every lane, so they stay in scalar registers
struct SensDev {
  double e[PS_SENS_MAX_PARAM];
};
// F row-major [param][16] and isd[param]: 2.2 kB of kernel arguments
struct SensFactor {
  double f[PS_SENS_MAX_PARAM * PS_SENS_MAX_PARAM];
  double isd[PS_SENS_MAX_PARAM];
};

// C_i += (w d) e_i, every product and sum rounded on its own; a cell with d == 0 keeps its bits
__device__ inline double sens_comoment(double c, double wd, double e, bool changed) {
  return changed ? __dadd_rn(c, __dmul_rn(wd, e)) : c;
}

// blockIdx.y = slot of the chunk; a thread owns a pair of cells (the tail cell of an odd N*N alone).
// cstride = nslot * pitch: the distance between the planes of two parameters.  NP, the handle's parameter
// count, is a template argument: with a run-time count every load and store of a co-moment sat behind a scalar
// branch of its own and the compiler spilled 132 SGPRs to lanes; with NP known the batches are straight code.
template <int NP>
__global__ void __launch_bounds__(256) k_sens_add(SensSlots desc, double* __restrict__ mean, double* __restrict__ m2,
                                                  double* __restrict__ C, int64_t ncell, int64_t pitch,
                                                  int64_t cstride, SensDev dev, double negval, double w, double Wn) {
  const SensSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double* __restrict__ rec = sd.rec;
  double* ms = mean + (int64_t)sd.slot * pitch;
  double* qs = m2 + (int64_t)sd.slot * pitch;
  double* cs = C + (int64_t)sd.slot * pitch;
  const int64_t npair = ncell >> 1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j <= npair; j += (int64_t)gridDim.x * blockDim.x) {
    if (j < npair) {
      const double2 r = *reinterpret_cast<const double2*>(rec + 2 * j);
      double2 m = *reinterpret_cast<const double2*>(ms + 2 * j);
      double2 q = *reinterpret_cast<const double2*>(qs + 2 * j);
      const double v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
      const double v1 = ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval);
      const double wd0 = __dmul_rn(w, v0 - m.x);
      const double wd1 = __dmul_rn(w, v1 - m.y);
      const bool c0 = sum_update(v0, w, Wn, m.x, q.x);
      const bool c1 = sum_update(v1, w, Wn, m.y, q.y);
      if (!(c0 || c1)) continue;          // before any co-moment is touched
      *reinterpret_cast<double2*>(ms + 2 * j) = m;
      *reinterpret_cast<double2*>(qs + 2 * j) = q;
      double* cp = cs + 2 * j;
#pragma unroll
      for (int p0 = 0; p0 < NP; p0 += PS_SENS_BATCH) {
        const int nb = NP - p0 < PS_SENS_BATCH ? NP - p0 : PS_SENS_BATCH;
        double2 c[PS_SENS_BATCH];
#pragma unroll
        for (int k = 0; k < PS_SENS_BATCH; ++k)
          if (k < nb) c[k] = *reinterpret_cast<const double2*>(cp + (int64_t)(p0 + k) * cstride);
#pragma unroll
        for (int k = 0; k < PS_SENS_BATCH; ++k)
          if (k < nb) {
            c[k].x = sens_comoment(c[k].x, wd0, dev.e[p0 + k], c0);
            c[k].y = sens_comoment(c[k].y, wd1, dev.e[p0 + k], c1);
            *reinterpret_cast<double2*>(cp + (int64_t)(p0 + k) * cstride) = c[k];
          }
      }
    } else if (ncell & 1) {
      const int64_t i = ncell - 1;
      const double v = ps_record_value(rec[i], sd.stat_scale, sd.post_scale, delta, negval);
      double m = ms[i], q = qs[i];
      const double wd = __dmul_rn(w, v - m);
      if (sum_update(v, w, Wn, m, q)) {
        ms[i] = m;
        qs[i] = q;
#pragma unroll
        for (int p = 0; p < NP; ++p)
          cs[(int64_t)p * cstride + i] = sens_comoment(cs[(int64_t)p * cstride + i], wd, dev.e[p], true);
      }
    }
  }
}

using SensAddKernel = void (*)(SensSlots, double*, double*, double*, int64_t, int64_t, int64_t, SensDev, double, double,
                               double);
// k_sens_add<nparam>, nparam = 1 .. 16
const SensAddKernel sens_add_kernels[PS_SENS_MAX_PARAM] = {
    k_sens_add<1>,  k_sens_add<2>,  k_sens_add<3>,  k_sens_add<4>,  k_sens_add<5>,  k_sens_add<6>,
    k_sens_add<7>,  k_sens_add<8>,  k_sens_add<9>,  k_sens_add<10>, k_sens_add<11>, k_sens_add<12>,
    k_sens_add<13>, k_sens_add<14>, k_sens_add<15>, k_sens_add<16>};

// Chan, Golub & LeVeque over every slot's cells: mean and M2 as k_summary_merge, and per parameter
// C_i = Ca_i + Cb_i + (mb - ma) dtheta_i (Wa Wb / W)
__global__ void __launch_bounds__(256) k_sens_merge(double* __restrict__ ma, double* __restrict__ qa,
                                                    double* __restrict__ ca, const double* __restrict__ mb,
                                                    const double* __restrict__ qb, const double* __restrict__ cb,
                                                    int64_t nval, int nparam, SensDev dtheta, double Wa, double Wb) {
  const double W = Wa + Wb;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nval; i += stride) {
    const double d = mb[i] - ma[i];
#pragma unroll
    for (int p = 0; p < PS_SENS_MAX_PARAM; ++p)
      if (p < nparam) {
        const int64_t k = (int64_t)p * nval + i;
        ca[k] = ca[k] + cb[k] + d * dtheta.e[p] * (Wa * Wb / W);
      }
    ma[i] = ma[i] + d * (Wb / W);
    qa[i] = qa[i] + qb[i] + d * d * (Wa * Wb / W);
  }
}

// one cell of the finalize: c_i = C_i / W, var = M2 / W,
//   expl = sum_k (sum_i F_ik c_i)^2 / var   (0 where M2 == 0),
//   dom = the lowest i that maximises (c_i isd_i)^2   (255 where M2 == 0 or every square is 0);
// every product, sum and quotient rounded on its own, the sums from +0.0 in ascending index
__device__ inline void sens_cell(const double* cv, double q, double W, int nparam, int rank, const double* sF,
                                 const double* sI, double& expl, unsigned char& dom) {
  expl = 0.0;
  dom = 255;
  if (q == 0.0) return;
  double c[PS_SENS_MAX_PARAM];
#pragma unroll
  for (int p = 0; p < PS_SENS_MAX_PARAM; ++p) c[p] = p < nparam ? __ddiv_rn(cv[p], W) : 0.0;
  double s = 0.0;
  for (int k = 0; k < rank; ++k) {
    double u = 0.0;
#pragma unroll
    for (int p = 0; p < PS_SENS_MAX_PARAM; ++p)
      if (p < nparam) u = __dadd_rn(u, __dmul_rn(sF[p * PS_SENS_MAX_PARAM + k], c[p]));
    s = __dadd_rn(s, __dmul_rn(u, u));
  }
  expl = __ddiv_rn(s, __ddiv_rn(q, W));
  double best = 0.0;
#pragma unroll
  for (int p = 0; p < PS_SENS_MAX_PARAM; ++p)
    if (p < nparam) {
      const double t = __dmul_rn(c[p], sI[p]);
      const double t2 = __dmul_rn(t, t);
      if (t2 > best) {
        best = t2;
        dom = (unsigned char)p;
      }
    }
}

// flat over nslot * pitch cells (pitch is a multiple of 64: pairs never straddle a slot).  F and isd go from the
// kernel arguments to LDS once per workgroup (2.2 kB; every lane reads the same word: a broadcast).
__global__ void __launch_bounds__(256) k_sens_finalize(const double* __restrict__ m2, const double* __restrict__ C,
                                                       double* __restrict__ expl, unsigned char* __restrict__ dom,
                                                       int64_t total, int nparam, int rank, SensFactor F, double W) {
  __shared__ double sF[PS_SENS_MAX_PARAM * PS_SENS_MAX_PARAM];
  __shared__ double sI[PS_SENS_MAX_PARAM];
  for (int t = threadIdx.x; t < PS_SENS_MAX_PARAM * PS_SENS_MAX_PARAM; t += blockDim.x) sF[t] = F.f[t];
  if (threadIdx.x < PS_SENS_MAX_PARAM) sI[threadIdx.x] = F.isd[threadIdx.x];
  __syncthreads();
  const int64_t npair = total >> 1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < npair; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = 2 * j;
    const double2 q = *reinterpret_cast<const double2*>(m2 + i);
    double2 x = make_double2(0.0, 0.0);
    uchar2 d = make_uchar2(255, 255);
    if (q.x != 0.0 || q.y != 0.0) {
      double c0[PS_SENS_MAX_PARAM], c1[PS_SENS_MAX_PARAM];
#pragma unroll
      for (int p = 0; p < PS_SENS_MAX_PARAM; ++p) {
        double2 a = make_double2(0.0, 0.0);
        if (p < nparam) a = *reinterpret_cast<const double2*>(C + (int64_t)p * total + i);
        c0[p] = a.x;
        c1[p] = a.y;
      }
      sens_cell(c0, q.x, W, nparam, rank, sF, sI, x.x, d.x);
      sens_cell(c1, q.y, W, nparam, rank, sF, sI, x.y, d.y);
    }
    *reinterpret_cast<double2*>(expl + i) = x;
    *reinterpret_cast<uchar2*>(dom + i) = d;
  }
}

}  // namespace

struct ps_sens {
  int device = 0, N = 0, nslot = 0, nparam = 0;
  int64_t ncell = 0, pitch = 0;
  double* block = nullptr;   // mean | M2 | C | expl | dom
  double* mean = nullptr;
  double* m2 = nullptr;
  double* C = nullptr;
  double* expl = nullptr;
  unsigned char* dom = nullptr;
  uint64_t W = 0;
  int64_t members = 0;
  bool finalized = false;
  hipStream_t stream = nullptr;   // reset / merge / finalize / fetch, and the adds from fields
  PsLastOp last;                  // the last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds
};

static int64_t sens_total(const ps_sens* a) { return (int64_t)a->nslot * a->pitch; }
// the accumulated part: mean, M2 and the co-moments
static size_t sens_acc_bytes(const ps_sens* a) { return (size_t)(a->nparam + 2) * sens_total(a) * sizeof(double); }
static double sens_block_bytes(int nparam, int nslot, int64_t pitch) {
  return ((double)(nparam + 3) * sizeof(double) + 1.0) * (double)nslot * (double)pitch;
}

static bool sens_finite(double v) { return v == v && !isinf(v); }

extern "C" void ps_sens_destroy(ps_sens* a) {
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

extern "C" int ps_sens_reset(ps_sens* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "sens_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->block, 0, (size_t)sens_block_bytes(a->nparam, a->nslot, a->pitch), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  a->finalized = false;
  return PS_OK;
}

extern "C" int ps_sens_create(int device, int N, int nslot, int nparam, ps_sens** out) {
  if (!out || N < 1 || nslot < 1 || nparam < 1 || nparam > PS_SENS_MAX_PARAM)
    return ps_fail(PS_ERR_BAD_ARG, "sens_create: N %d, %d slots, %d parameters (1..%d)", N, nslot, nparam,
                   PS_SENS_MAX_PARAM);
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // the whole block, checked before anything is allocated
  const double need = sens_block_bytes(nparam, nslot, pitch);
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "sens_create: ((%d + 3) x 8 + 1) B x %d slots x %lld cells = %.3g GB, %.3g GB free",
                   nparam, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_sens* a = new ps_sens();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nparam = nparam;
  a->ncell = ncell;
  a->pitch = pitch;
  auto fail = [&](int rc) {
    ps_sens_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->block, (size_t)need);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "sens_create: %s", hipGetErrorString(e)));
  const int64_t t = sens_total(a);
  a->mean = a->block;
  a->m2 = a->mean + t;
  a->C = a->m2 + t;
  a->expl = a->C + (int64_t)nparam * t;
  a->dom = reinterpret_cast<unsigned char*>(a->expl + t);
  int rc = ps_sens_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// what every add checks before it resolves a descriptor (who: the entry point)
static int sens_check_add(ps_sens* a, const char* who, int nparam, const double* e, uint32_t weight) {
  if (!a || !e) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (nparam != a->nparam)
    return ps_fail(PS_ERR_BAD_ARG, "%s: %d parameters given, the handle has %d", who, nparam, a->nparam);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would reach 2^32", who, (unsigned long long)(a->W + weight));
  for (int i = 0; i < nparam; ++i)
    if (!sens_finite(e[i])) return ps_fail(PS_ERR_BAD_ARG, "%s: e[%d] is not finite", who, i);
  return PS_OK;
}

// one member from the slot descriptors d (one per slot of the handle), enqueued on `stream`
static int sens_launch(ps_sens* a, const std::vector<PsSrc>& d, hipStream_t stream, double negval, const double* e,
                       uint32_t weight) {
  const int nslot = a->nslot;
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  SensDev dev;
  for (int i = 0; i < PS_SENS_MAX_PARAM; ++i) dev.e[i] = i < a->nparam ? e[i] : 0.0;
  const double Wn = (double)(a->W + weight);
  const int64_t npair = a->ncell / 2 + 1;
  const int threads = 256;
  const int bx = (int)std::min<int64_t>((npair + threads - 1) / threads, 4096);
  for (int c0 = 0; c0 < nslot; c0 += PS_SENS_CHUNK) {
    const int n = std::min(PS_SENS_CHUNK, nslot - c0);
    SensSlots desc;
    for (int i = 0; i < n; ++i) desc.s[i] = ps_slotted<SensSlot>(d[(size_t)(c0 + i)], c0 + i);
    hipLaunchKernelGGL(sens_add_kernels[a->nparam - 1], dim3(bx, n), dim3(threads), 0, stream, desc, a->mean, a->m2,
                       a->C, a->ncell, a->pitch, sens_total(a), dev, negval, (double)weight, Wn);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  a->finalized = false;
  return PS_OK;
}

extern "C" int ps_sens_add(ps_sens* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                           const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                           int nparam, const double* e, uint32_t weight) {
  if (!s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "sens_add: bad arguments");
  PS_TRY(sens_check_add(a, "sens_add", nparam, e, weight));
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "sens_add: %d slots given, the handle has %d", nslot, a->nslot);
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("sens_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, d.data(), &stream));
  return sens_launch(a, d, stream, negval, e, weight);
}

// one member whose values are the current fields of a projection or a release plan (who: the entry point)
static int sens_add_fields(ps_sens* a, void* h, const PsFieldsOps& src, const char* who, int nparam, const double* e,
                           uint32_t weight) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(sens_check_add(a, who, nparam, e, weight));
  // slot k takes Y_k: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  std::vector<PsSrc> d((size_t)a->nslot);
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, d.data()));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(sens_launch(a, d, a->stream, 0.0, e, weight));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_sens_add_project(ps_sens* a, ps_project* p, int nparam, const double* e, uint32_t weight) {
  return sens_add_fields(a, p, ps_project_fields(), "sens_add_project", nparam, e, weight);
}

extern "C" int ps_sens_add_sites(ps_sens* a, ps_sites* p, int nparam, const double* e, uint32_t weight) {
  return sens_add_fields(a, p, ps_sites_fields(), "sens_add_sites", nparam, e, weight);
}

extern "C" int ps_sens_merge(ps_sens* dst, ps_sens* src, int nparam, const double* dtheta) {
  if (!dst || !src || !dtheta) return ps_fail(PS_ERR_BAD_ARG, "sens_merge: bad arguments");
  if (dst == src) return ps_fail(PS_ERR_BAD_ARG, "sens_merge: dst and src are the same handle");
  if (nparam != dst->nparam || nparam != src->nparam)
    return ps_fail(PS_ERR_BAD_ARG, "sens_merge: %d parameters given, dst has %d and src %d", nparam, dst->nparam,
                   src->nparam);
  if (dst->nslot != src->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "sens_merge: dst has %d slots, src %d", dst->nslot, src->nslot);
  if (dst->device != src->device)
    return ps_fail(PS_ERR_BAD_ARG, "sens_merge: dst on device %d, src on device %d", dst->device, src->device);
  if (dst->N != src->N) return ps_fail(PS_ERR_BAD_ARG, "sens_merge: dst domain %d, src domain %d", dst->N, src->N);
  for (int i = 0; i < nparam; ++i)
    if (!sens_finite(dtheta[i])) return ps_fail(PS_ERR_BAD_ARG, "sens_merge: dtheta[%d] is not finite", i);
  if (dst->W + src->W > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "sens_merge: total weight %llu would reach 2^32",
                   (unsigned long long)(dst->W + src->W));
  dst->finalized = false;
  if (src->W == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  if (dst->W == 0) {   // a copy: the merged handle is src bit for bit
    PS_HIP(hipMemcpyAsync(dst->block, src->block, sens_acc_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
  } else {
    SensDev dt;
    for (int i = 0; i < PS_SENS_MAX_PARAM; ++i) dt.e[i] = i < nparam ? dtheta[i] : 0.0;
    hipLaunchKernelGGL(k_sens_merge, dim3(2048), dim3(256), 0, dst->stream, dst->mean, dst->m2, dst->C, src->mean,
                       src->m2, src->C, sens_total(dst), nparam, dt, (double)dst->W, (double)src->W);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  return PS_OK;
}

extern "C" int ps_sens_finalize(ps_sens* a, int nparam, int rank, const double* F, const double* isd) {
  if (!a || !F || !isd) return ps_fail(PS_ERR_BAD_ARG, "sens_finalize: bad arguments");
  if (nparam != a->nparam || rank < 1 || rank > PS_SENS_MAX_PARAM)
    return ps_fail(PS_ERR_BAD_ARG, "sens_finalize: factor %d x %d, the handle has %d parameters (rank 1..%d)", nparam,
                   rank, a->nparam, PS_SENS_MAX_PARAM);
  SensFactor f;
  for (int i = 0; i < PS_SENS_MAX_PARAM * PS_SENS_MAX_PARAM; ++i) f.f[i] = 0.0;
  for (int i = 0; i < PS_SENS_MAX_PARAM; ++i) f.isd[i] = 0.0;
  for (int p = 0; p < nparam; ++p) {
    for (int k = 0; k < rank; ++k) {
      const double v = F[(size_t)p * rank + k];
      if (!sens_finite(v)) return ps_fail(PS_ERR_BAD_ARG, "sens_finalize: F[%d][%d] is not finite", p, k);
      f.f[p * PS_SENS_MAX_PARAM + k] = v;
    }
    if (!sens_finite(isd[p])) return ps_fail(PS_ERR_BAD_ARG, "sens_finalize: isd[%d] is not finite", p);
    f.isd[p] = isd[p];
  }
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "sens_finalize: nothing accumulated (W = 0)");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const int64_t total = sens_total(a);
  const int threads = 256;
  const int bx = (int)std::min<int64_t>((total / 2 + threads - 1) / threads, 8192);
  hipLaunchKernelGGL(k_sens_finalize, dim3(bx), dim3(threads), 0, a->stream, a->m2, a->C, a->expl, a->dom, total,
                     a->nparam, rank, f, (double)a->W);
  PS_HIP(hipGetLastError());
  PS_TRY(a->last.mark(a->stream));
  a->finalized = true;
  return PS_OK;
}

extern "C" int ps_sens_fetch(ps_sens* a, int slot, int what, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "sens_fetch: bad arguments");
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "sens_fetch: slot %d of %d", slot, a->nslot);
  const bool fin = what == 2 || what == 3;
  if (!(what == 0 || what == 1 || fin || (what >= 16 && what < 16 + a->nparam)))
    return ps_fail(PS_ERR_BAD_ARG,
                   "sens_fetch: quantity %d (0 mean, 1 variance, 2 explained, 3 dominant, 16..%d covariance)", what,
                   15 + a->nparam);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "sens_fetch: nothing accumulated (W = 0)");
  if (fin && !a->finalized) return ps_fail(PS_ERR_STATE, "sens_fetch: quantity %d is not finalized since the last change", what);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const double W = (double)a->W;
  const size_t n = (size_t)a->ncell;
  const int64_t off = (int64_t)slot * a->pitch;
  if (what == 3) {
    std::vector<unsigned char> d(n);
    PS_HIP(hipMemcpyAsync(d.data(), a->dom + off, n, hipMemcpyDeviceToHost, a->stream));
    PS_HIP(hipStreamSynchronize(a->stream));
    for (size_t i = 0; i < n; ++i) out[i] = d[i] == 255 ? -1.0 : (double)d[i];
    return PS_OK;
  }
  const double* src = what == 0 ? a->mean : what == 1 ? a->m2 : what == 2 ? a->expl
                                                                         : a->C + (int64_t)(what - 16) * sens_total(a);
  PS_HIP(hipMemcpyAsync(out, src + off, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  if (what == 1 || what >= 16)
    for (size_t i = 0; i < n; ++i) out[i] /= W;
  return PS_OK;
}

extern "C" int ps_sens_info(ps_sens* a, double* total_weight, int64_t* members) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "sens_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  return PS_OK;
}

extern "C" int ps_sens_prof(ps_sens* a, int enable, double* total_ms, int64_t* launches) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "sens_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  if (total_ms || launches) PS_TRY(a->prof.totals(0, total_ms, launches));
  return PS_OK;
}
