// Posterior dependence maps (include/parasitoid_hip.h, ps_depend_*): per cell the sums of the fields of many
// model evaluations over the bins of up to 16 scalars the caller bins per member (the model parameters behind
// the member), accumulated on the device from the solver's records, a projection's or a release plan's fields;
// from them the correlation ratio eta^2 = Var_b(E[v | bin b]) / Var(v) of every cell on every scalar.
// Layout as ps_summary.hip (pitch = N*N rounded up to 64 cells, every slot 16-byte aligned), one device block
// carved into
//   mean[slot][pitch], M2[slot][pitch], S[param][bin][slot][pitch], eta[param][slot][pitch]   (fp64),
//   dom[slot][pitch] (uint8)
// so a flat index slot*pitch + cell addresses the same cell in every array.  Pad cells stay 0.
// An add reads 8 B of record and reads + writes 16 B of mean, 16 B of M2 and, per parameter, 16 B of the one
// plane S[param][bin of the member] of every cell of every slot -- nothing but the record and the two moments
// where a pair of cells is 0 in this member, which outside the plume is most of the domain.
#include <math.h>

#include <vector>

#include "ps_common.h"

#define PS_DEP_MAX_PARAM 16
#define PS_DEP_MAX_BIN 16
#define PS_DEP_CHUNK 32   // slots per launch: 32 descriptors = 1.3 kB of kernel arguments
#define PS_DEP_BATCH 8    // plane pairs loaded before the first add: 8 x 16 B in flight per lane

namespace {

struct DepSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct DepSlots {
  DepSlot s[PS_DEP_CHUNK];
};
// the member's plane per parameter, param * nbin + bin: the same for every lane, so every plane base is scalar
struct DepPlanes {
  int32_t plane[PS_DEP_MAX_PARAM];
};
// Wb row-major [param][16]: 2 kB of kernel arguments
struct DepWeights {
  double wb[PS_DEP_MAX_PARAM * PS_DEP_MAX_BIN];
};

// blockIdx.y = slot of the chunk; a thread owns a pair of cells (the tail cell of an odd N*N alone).
// total = nslot * pitch: the distance between two planes of S.  NP, the handle's parameter count, is a template
// argument as in k_sens_add: the batches are straight code and the plane bases stay in scalar registers.
template <int NP>
__global__ void __launch_bounds__(256) k_dep_add(DepSlots desc, double* __restrict__ mean, double* __restrict__ m2,
                                                 double* __restrict__ S, int64_t ncell, int64_t pitch, int64_t total,
                                                 DepPlanes pl, double negval, double w, double Wn) {
  const DepSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double* __restrict__ rec = sd.rec;
  double* ms = mean + (int64_t)sd.slot * pitch;
  double* qs = m2 + (int64_t)sd.slot * pitch;
  double* ss = S + (int64_t)sd.slot * pitch;
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
      if (v0 == 0.0 && v1 == 0.0) continue;   // before any plane is touched
      const double wv0 = __dmul_rn(w, v0);
      const double wv1 = __dmul_rn(w, v1);
      double* sp = ss + 2 * j;
#pragma unroll
      for (int p0 = 0; p0 < NP; p0 += PS_DEP_BATCH) {
        const int nb = NP - p0 < PS_DEP_BATCH ? NP - p0 : PS_DEP_BATCH;
        double2 s[PS_DEP_BATCH];
#pragma unroll
        for (int k = 0; k < PS_DEP_BATCH; ++k)
          if (k < nb) s[k] = *reinterpret_cast<const double2*>(sp + (int64_t)pl.plane[p0 + k] * total);
#pragma unroll
        for (int k = 0; k < PS_DEP_BATCH; ++k)
          if (k < nb) {
            s[k].x = __dadd_rn(s[k].x, wv0);
            s[k].y = __dadd_rn(s[k].y, wv1);
            *reinterpret_cast<double2*>(sp + (int64_t)pl.plane[p0 + k] * total) = s[k];
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
      if (v != 0.0) {
        const double wv = __dmul_rn(w, v);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          double* c = ss + (int64_t)pl.plane[p] * total + i;
          *c = __dadd_rn(*c, wv);
        }
      }
    }
  }
}

using DepAddKernel = void (*)(DepSlots, double*, double*, double*, int64_t, int64_t, int64_t, DepPlanes, double, double,
                              double);
// k_dep_add<nparam>, nparam = 1 .. 16
const DepAddKernel dep_add_kernels[PS_DEP_MAX_PARAM] = {
    k_dep_add<1>,  k_dep_add<2>,  k_dep_add<3>,  k_dep_add<4>,  k_dep_add<5>,  k_dep_add<6>,  k_dep_add<7>,  k_dep_add<8>,
    k_dep_add<9>,  k_dep_add<10>, k_dep_add<11>, k_dep_add<12>, k_dep_add<13>, k_dep_add<14>, k_dep_add<15>, k_dep_add<16>};

// Chan, Golub & LeVeque on mean and M2 over every slot's cells, every product, sum and quotient rounded on its
// own in the order of the header, and S += S_src plane by plane (nplane * nval values behind sa / sb)
__global__ void __launch_bounds__(256) k_dep_merge(double* __restrict__ ma, double* __restrict__ qa,
                                                   double* __restrict__ sa, const double* __restrict__ mb,
                                                   const double* __restrict__ qb, const double* __restrict__ sb,
                                                   int64_t nval, int64_t nplane, double Wa, double Wb) {
  const double W = Wa + Wb;
  const double fb = __ddiv_rn(Wb, W);
  const double fab = __ddiv_rn(__dmul_rn(Wa, Wb), W);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t j = first; 2 * j < nval; j += stride) {
    const int64_t i = 2 * j;
    double2 a = *reinterpret_cast<const double2*>(ma + i);
    double2 q = *reinterpret_cast<const double2*>(qa + i);
    const double2 b = *reinterpret_cast<const double2*>(mb + i);
    const double2 r = *reinterpret_cast<const double2*>(qb + i);
    const double d0 = __dsub_rn(b.x, a.x), d1 = __dsub_rn(b.y, a.y);
    a.x = __dadd_rn(a.x, __dmul_rn(d0, fb));
    a.y = __dadd_rn(a.y, __dmul_rn(d1, fb));
    q.x = __dadd_rn(__dadd_rn(q.x, r.x), __dmul_rn(__dmul_rn(d0, d0), fab));
    q.y = __dadd_rn(__dadd_rn(q.y, r.y), __dmul_rn(__dmul_rn(d1, d1), fab));
    *reinterpret_cast<double2*>(ma + i) = a;
    *reinterpret_cast<double2*>(qa + i) = q;
  }
  const int64_t nsum = nplane * nval;   // nval is a multiple of 64: pairs never straddle a plane
  for (int64_t j = first; 2 * j < nsum; j += stride) {
    const int64_t i = 2 * j;
    const double2 b = *reinterpret_cast<const double2*>(sb + i);
    if (b.x == 0.0 && b.y == 0.0) continue;
    double2 a = *reinterpret_cast<const double2*>(sa + i);
    a.x = __dadd_rn(a.x, b.x);
    a.y = __dadd_rn(a.y, b.y);
    *reinterpret_cast<double2*>(sa + i) = a;
  }
}

// one cell of the finalize for one parameter: s = sum over the bins with Wb > 0, ascending, of
// Wb (S_b / Wb - mean)^2, eta = min((s / W) / var, 1), 0 with fewer than two such bins; every operation rounded
// on its own
__device__ inline double dep_eta(const double* sv, const double* wb, int nbin, double mean, double var, double W) {
  double s = 0.0;
  int used = 0;
#pragma unroll
  for (int b = 0; b < PS_DEP_MAX_BIN; ++b)
    if (b < nbin && wb[b] > 0.0) {
      const double mb = __ddiv_rn(sv[b], wb[b]);
      const double d = __dsub_rn(mb, mean);
      double q = __dmul_rn(d, d);
      q = __dmul_rn(wb[b], q);
      s = __dadd_rn(s, q);
      ++used;
    }
  if (used < 2) return 0.0;   // every member in one bin: nothing lies between bins (S / W is not the mean bit for bit)
  const double e = __ddiv_rn(__ddiv_rn(s, W), var);
  return e < 1.0 ? e : 1.0;
}

// flat over total = nslot * pitch cells (pitch is a multiple of 64: pairs never straddle a slot).  Wb goes from
// the kernel arguments to LDS once per workgroup (2 kB; every lane reads the same word: a broadcast).  Per
// parameter the nbin plane pairs of a cell pair are loaded together, then reduced.
__global__ void __launch_bounds__(256) k_dep_finalize(const double* __restrict__ mean, const double* __restrict__ m2,
                                                      const double* __restrict__ S, double* __restrict__ eta,
                                                      unsigned char* __restrict__ dom, int64_t total, int nparam,
                                                      int nbin, DepWeights Wb, double W) {
  __shared__ double sW[PS_DEP_MAX_PARAM * PS_DEP_MAX_BIN];
  for (int t = threadIdx.x; t < PS_DEP_MAX_PARAM * PS_DEP_MAX_BIN; t += blockDim.x) sW[t] = Wb.wb[t];
  __syncthreads();
  const int64_t npair = total >> 1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < npair; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = 2 * j;
    const double2 q = *reinterpret_cast<const double2*>(m2 + i);
    uchar2 d = make_uchar2(255, 255);
    if (q.x == 0.0 && q.y == 0.0) {
      for (int p = 0; p < nparam; ++p) *reinterpret_cast<double2*>(eta + (int64_t)p * total + i) = make_double2(0.0, 0.0);
      *reinterpret_cast<uchar2*>(dom + i) = d;
      continue;
    }
    const double2 m = *reinterpret_cast<const double2*>(mean + i);
    const double var0 = __ddiv_rn(q.x, W), var1 = __ddiv_rn(q.y, W);
    double best0 = 0.0, best1 = 0.0;
    for (int p = 0; p < nparam; ++p) {
      double s0[PS_DEP_MAX_BIN], s1[PS_DEP_MAX_BIN];
      const double* sp = S + (int64_t)p * nbin * total + i;
#pragma unroll
      for (int b = 0; b < PS_DEP_MAX_BIN; ++b) {
        double2 a = make_double2(0.0, 0.0);
        if (b < nbin) a = *reinterpret_cast<const double2*>(sp + (int64_t)b * total);
        s0[b] = a.x;
        s1[b] = a.y;
      }
      const double* wb = sW + p * PS_DEP_MAX_BIN;
      double2 e = make_double2(0.0, 0.0);
      if (q.x != 0.0) e.x = dep_eta(s0, wb, nbin, m.x, var0, W);
      if (q.y != 0.0) e.y = dep_eta(s1, wb, nbin, m.y, var1, W);
      *reinterpret_cast<double2*>(eta + (int64_t)p * total + i) = e;
      if (e.x > best0) {
        best0 = e.x;
        d.x = (unsigned char)p;
      }
      if (e.y > best1) {
        best1 = e.y;
        d.y = (unsigned char)p;
      }
    }
    *reinterpret_cast<uchar2*>(dom + i) = d;
  }
}

}  // namespace

struct ps_depend {
  int device = 0, N = 0, nslot = 0, nparam = 0, nbin = 0;
  int64_t ncell = 0, pitch = 0;
  double* block = nullptr;   // mean | M2 | S | eta | dom
  double* mean = nullptr;
  double* m2 = nullptr;
  double* S = nullptr;
  double* eta = nullptr;
  unsigned char* dom = nullptr;
  uint64_t W = 0;
  int64_t members = 0;
  bool finalized = false;
  hipStream_t stream = nullptr;   // reset / merge / finalize / fetch, and the adds from fields
  PsLastOp last;                  // the last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds
};

static int64_t dep_total(const ps_depend* a) { return (int64_t)a->nslot * a->pitch; }
static int64_t dep_planes(const ps_depend* a) { return (int64_t)a->nparam * a->nbin; }
// the accumulated part: mean, M2 and the bin sums
static size_t dep_acc_bytes(const ps_depend* a) { return (size_t)(dep_planes(a) + 2) * dep_total(a) * sizeof(double); }
static double dep_block_bytes(int nparam, int nbin, int nslot, int64_t pitch) {
  return ((double)(2 + nparam * nbin + nparam) * sizeof(double) + 1.0) * (double)nslot * (double)pitch;
}

extern "C" void ps_depend_destroy(ps_depend* a) {
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

extern "C" int ps_depend_reset(ps_depend* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "depend_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->block, 0, (size_t)dep_block_bytes(a->nparam, a->nbin, a->nslot, a->pitch), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  a->finalized = false;
  return PS_OK;
}

extern "C" int ps_depend_create(int device, int N, int nslot, int nparam, int nbin, ps_depend** out) {
  if (!out || N < 1 || nslot < 1 || nparam < 1 || nparam > PS_DEP_MAX_PARAM || nbin < 2 || nbin > PS_DEP_MAX_BIN)
    return ps_fail(PS_ERR_BAD_ARG, "depend_create: N %d, %d slots, %d parameters (1..%d), %d bins (2..%d)", N, nslot,
                   nparam, PS_DEP_MAX_PARAM, nbin, PS_DEP_MAX_BIN);
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // the whole block, checked before anything is allocated
  const double need = dep_block_bytes(nparam, nbin, nslot, pitch);
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM,
                   "depend_create: ((2 + %d x %d + %d) x 8 + 1) B x %d slots x %lld cells = %.3g GB, %.3g GB free",
                   nparam, nbin, nparam, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_depend* a = new ps_depend();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nparam = nparam;
  a->nbin = nbin;
  a->ncell = ncell;
  a->pitch = pitch;
  auto fail = [&](int rc) {
    ps_depend_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->block, (size_t)need);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "depend_create: %s", hipGetErrorString(e)));
  const int64_t t = dep_total(a);
  a->mean = a->block;
  a->m2 = a->mean + t;
  a->S = a->m2 + t;
  a->eta = a->S + dep_planes(a) * t;
  a->dom = reinterpret_cast<unsigned char*>(a->eta + (int64_t)nparam * t);
  int rc = ps_depend_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// what every add checks before it resolves a descriptor (who: the entry point)
static int dep_check_add(ps_depend* a, const char* who, int nparam, const int32_t* bin, uint32_t weight) {
  if (!a || !bin) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (nparam != a->nparam)
    return ps_fail(PS_ERR_BAD_ARG, "%s: %d parameters given, the handle has %d", who, nparam, a->nparam);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would reach 2^32", who, (unsigned long long)(a->W + weight));
  for (int i = 0; i < nparam; ++i)
    if (bin[i] < 0 || bin[i] >= a->nbin)
      return ps_fail(PS_ERR_BAD_ARG, "%s: bin[%d] = %d, the handle has bins 0..%d", who, i, (int)bin[i], a->nbin - 1);
  return PS_OK;
}

// one member from the slot descriptors d (one per slot of the handle), enqueued on `stream`
static int dep_launch(ps_depend* a, const std::vector<PsSrc>& d, hipStream_t stream, double negval,
                      const int32_t* bin, uint32_t weight) {
  const int nslot = a->nslot;
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  DepPlanes pl;
  for (int i = 0; i < PS_DEP_MAX_PARAM; ++i) pl.plane[i] = i < a->nparam ? i * a->nbin + bin[i] : 0;
  const double Wn = (double)(a->W + weight);
  const int64_t npair = a->ncell / 2 + 1;
  const int threads = 256;
  const int bx = (int)std::min<int64_t>((npair + threads - 1) / threads, 4096);
  for (int c0 = 0; c0 < nslot; c0 += PS_DEP_CHUNK) {
    const int n = std::min(PS_DEP_CHUNK, nslot - c0);
    DepSlots desc;
    for (int i = 0; i < n; ++i) desc.s[i] = ps_slotted<DepSlot>(d[(size_t)(c0 + i)], c0 + i);
    hipLaunchKernelGGL(dep_add_kernels[a->nparam - 1], dim3(bx, n), dim3(threads), 0, stream, desc, a->mean, a->m2,
                       a->S, a->ncell, a->pitch, dep_total(a), pl, negval, (double)weight, Wn);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  a->finalized = false;
  return PS_OK;
}

extern "C" int ps_depend_add(ps_depend* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                             const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                             double negval, int nparam, const int32_t* bin, uint32_t weight) {
  if (!s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "depend_add: bad arguments");
  PS_TRY(dep_check_add(a, "depend_add", nparam, bin, weight));
  if (nslot != a->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "depend_add: %d slots given, the handle has %d", nslot, a->nslot);
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("depend_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale,
                         use_delta, false, d.data(), &stream));
  return dep_launch(a, d, stream, negval, bin, weight);
}

// one member whose values are the current fields of a projection or a release plan (who: the entry point)
static int dep_add_fields(ps_depend* a, void* h, const PsFieldsOps& src, const char* who, int nparam,
                          const int32_t* bin, uint32_t weight) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(dep_check_add(a, who, nparam, bin, weight));
  // slot k takes Y_k: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  std::vector<PsSrc> d((size_t)a->nslot);
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, d.data()));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(dep_launch(a, d, a->stream, 0.0, bin, weight));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_depend_add_project(ps_depend* a, ps_project* p, int nparam, const int32_t* bin, uint32_t weight) {
  return dep_add_fields(a, p, ps_project_fields(), "depend_add_project", nparam, bin, weight);
}

extern "C" int ps_depend_add_sites(ps_depend* a, ps_sites* p, int nparam, const int32_t* bin, uint32_t weight) {
  return dep_add_fields(a, p, ps_sites_fields(), "depend_add_sites", nparam, bin, weight);
}

extern "C" int ps_depend_merge(ps_depend* dst, ps_depend* src) {
  if (!dst || !src) return ps_fail(PS_ERR_BAD_ARG, "depend_merge: bad arguments");
  if (dst == src) return ps_fail(PS_ERR_BAD_ARG, "depend_merge: dst and src are the same handle");
  if (dst->nparam != src->nparam || dst->nbin != src->nbin)
    return ps_fail(PS_ERR_BAD_ARG, "depend_merge: dst has %d parameters x %d bins, src %d x %d", dst->nparam,
                   dst->nbin, src->nparam, src->nbin);
  if (dst->nslot != src->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "depend_merge: dst has %d slots, src %d", dst->nslot, src->nslot);
  if (dst->device != src->device)
    return ps_fail(PS_ERR_BAD_ARG, "depend_merge: dst on device %d, src on device %d", dst->device, src->device);
  if (dst->N != src->N) return ps_fail(PS_ERR_BAD_ARG, "depend_merge: dst domain %d, src domain %d", dst->N, src->N);
  if (dst->W + src->W > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "depend_merge: total weight %llu would reach 2^32",
                   (unsigned long long)(dst->W + src->W));
  dst->finalized = false;
  if (src->W == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  if (dst->W == 0) {   // a copy: the merged handle is src bit for bit
    PS_HIP(hipMemcpyAsync(dst->block, src->block, dep_acc_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
  } else {
    hipLaunchKernelGGL(k_dep_merge, dim3(2048), dim3(256), 0, dst->stream, dst->mean, dst->m2, dst->S, src->mean,
                       src->m2, src->S, dep_total(dst), dep_planes(dst), (double)dst->W, (double)src->W);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  return PS_OK;
}

extern "C" int ps_depend_finalize(ps_depend* a, int nparam, int nbin, const double* Wb) {
  if (!a || !Wb) return ps_fail(PS_ERR_BAD_ARG, "depend_finalize: bad arguments");
  if (nparam != a->nparam || nbin != a->nbin)
    return ps_fail(PS_ERR_BAD_ARG, "depend_finalize: bin weights %d x %d, the handle has %d parameters x %d bins",
                   nparam, nbin, a->nparam, a->nbin);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "depend_finalize: nothing accumulated (W = 0)");
  DepWeights f;
  for (int i = 0; i < PS_DEP_MAX_PARAM * PS_DEP_MAX_BIN; ++i) f.wb[i] = 0.0;
  for (int p = 0; p < nparam; ++p) {
    double sum = 0.0;   // exact: integers below 2^32
    for (int b = 0; b < nbin; ++b) {
      const double v = Wb[(size_t)p * nbin + b];
      if (!(v >= 0.0 && v <= 4294967295.0 && v == floor(v)))
        return ps_fail(PS_ERR_BAD_ARG, "depend_finalize: Wb[%d][%d] = %g is not an integer in 0..2^32 - 1", p, b, v);
      f.wb[p * PS_DEP_MAX_BIN + b] = v;
      sum += v;
    }
    if (sum != (double)a->W)
      return ps_fail(PS_ERR_BAD_ARG, "depend_finalize: the bin weights of parameter %d sum to %.0f, the total weight is %llu",
                     p, sum, (unsigned long long)a->W);
  }
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const int64_t total = dep_total(a);
  const int threads = 256;
  const int bx = (int)std::min<int64_t>((total / 2 + threads - 1) / threads, 8192);
  hipLaunchKernelGGL(k_dep_finalize, dim3(bx), dim3(threads), 0, a->stream, a->mean, a->m2, a->S, a->eta, a->dom,
                     total, a->nparam, a->nbin, f, (double)a->W);
  PS_HIP(hipGetLastError());
  PS_TRY(a->last.mark(a->stream));
  a->finalized = true;
  return PS_OK;
}

extern "C" int ps_depend_fetch(ps_depend* a, int slot, int what, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "depend_fetch: bad arguments");
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "depend_fetch: slot %d of %d", slot, a->nslot);
  const bool is_eta = what >= 16 && what < 16 + a->nparam;
  const bool is_sum = what >= 256 && what < 256 + 16 * a->nparam && (what - 256) % 16 < a->nbin;
  const bool fin = what == 2 || is_eta;
  if (!(what == 0 || what == 1 || what == 3 || fin || is_sum))
    return ps_fail(PS_ERR_BAD_ARG,
                   "depend_fetch: quantity %d (0 mean, 1 variance, 2 dominant, 3 M2, 16..%d eta2, 256 + 16 p + b bin sum "
                   "with p < %d, b < %d)", what, 15 + a->nparam, a->nparam, a->nbin);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "depend_fetch: nothing accumulated (W = 0)");
  if (fin && !a->finalized)
    return ps_fail(PS_ERR_STATE, "depend_fetch: quantity %d is not finalized since the last change", what);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const double W = (double)a->W;
  const size_t n = (size_t)a->ncell;
  const int64_t off = (int64_t)slot * a->pitch;
  if (what == 2) {
    std::vector<unsigned char> d(n);
    PS_HIP(hipMemcpyAsync(d.data(), a->dom + off, n, hipMemcpyDeviceToHost, a->stream));
    PS_HIP(hipStreamSynchronize(a->stream));
    for (size_t i = 0; i < n; ++i) out[i] = d[i] == 255 ? -1.0 : (double)d[i];
    return PS_OK;
  }
  const double* src = a->mean;
  if (what == 1 || what == 3) src = a->m2;
  if (is_eta) src = a->eta + (int64_t)(what - 16) * dep_total(a);
  if (is_sum) src = a->S + ((int64_t)((what - 256) / 16) * a->nbin + (what - 256) % 16) * dep_total(a);
  PS_HIP(hipMemcpyAsync(out, src + off, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  if (what == 1)
    for (size_t i = 0; i < n; ++i) out[i] /= W;
  return PS_OK;
}

extern "C" int ps_depend_info(ps_depend* a, double* total_weight, int64_t* members) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "depend_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  return PS_OK;
}

extern "C" int ps_depend_prof(ps_depend* a, int enable, double* total_ms, int64_t* launches) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "depend_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  if (total_ms || launches) PS_TRY(a->prof.totals(0, total_ms, launches));
  return PS_OK;
}
