// Joint excursion sets and contour credible bands (include/parasitoid_hip.h, ps_excur_*): per threshold t_k and
// slot the weighted count C(c) of the members with v_s(c) >= t_k, and per member the bit mask of the cells where
// it holds, both written on the device from the records the chain has just produced.  The value of a slot is the
// one ps_summary_add adds (ps_record_value).  From the two, per member and plane, the bounds
//   hi_m = max{C(c) : bit_m(c) = 0} (0 if none)      lo_m = min{C(c) : bit_m(c) = 1} (0xffffffff if none)
// and from those the excursion functions on the level sets of C (Bolin & Lindgren 2015).  Layout (pitch = N*N
// rounded up to 64 cells, as ps_summary.hip; nword = pitch / 64):
//   cnt[k][slot][pitch]               uint32
//   mask[member][k][slot][nword]      uint64, bit l of word j = cell 64 j + l; grows by doubling
//   hi[member][k][slot], lo[...]      uint32, written by the finalize
// One thread per cell: a wave is one mask word (one 64-bit ballot, one lane stores it) and every count has a
// single writer.  The bounds are integer maxima and minima taken with integer atomics, so neither the order of
// adds or merges nor the grid changes a bit.  No floating-point atomics.
#include <math.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "ps_common.h"

#define PS_EXC_MAX_SLOT 32   // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_EXC_MAX_THR 4
#define PS_EXC_THREADS 256
#define PS_EXC_MEMBERS0 4    // member masks allocated by the first add that finds none
#define PS_EXC_CPT 8         // mask words (of 64 cells) one wave of the finalize keeps in registers
#define PS_EXC_NONE 0xffffffffu

namespace {

struct ExcSlots {
  PsSrc s[PS_EXC_MAX_SLOT];
};
struct ExcThr {
  double t[PS_EXC_MAX_THR];
};

// thread i owns cell i; the grid covers the pitch, so the wave of the last real cell also writes the pad bits
// (0) of its word and every word of the member is written.  The record of slot s + 1 is loaded while slot s is
// tested.  No early exit: a member that is below t everywhere still needs its zero words.  The ballot sits in
// wave-uniform control flow (waves past the pitch leave whole).
__global__ void __launch_bounds__(PS_EXC_THREADS) k_excur_add(ExcSlots desc, ExcThr thr, int nslot, int nthr,
                                                              uint32_t* __restrict__ cnt, uint64_t* __restrict__ mask,
                                                              int64_t ncell, int64_t pitch, double negval, uint32_t w) {
  __shared__ double sdelta[PS_EXC_MAX_SLOT];
  for (int t = threadIdx.x; t < nslot; t += blockDim.x) sdelta[t] = desc.s[t].stats ? desc.s[t].stats->delta : 0.0;
  __syncthreads();
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= pitch) return;   // pitch is a multiple of 64: whole waves
  const bool real = i < ncell;
  const bool writer = (threadIdx.x & 63) == 0;
  const int64_t nword = pitch >> 6, word = i >> 6;
  double r = real ? desc.s[0].rec[i] : 0.0;
  for (int s = 0; s < nslot; ++s) {
    double rn = 0.0;
    if (real && s + 1 < nslot) rn = desc.s[s + 1].rec[i];
    const PsSrc& sd = desc.s[s];
    const double v = real ? ps_record_value(r, sd.stat_scale, sd.post_scale, sdelta[s], negval) : 0.0;
#pragma unroll
    for (int k = 0; k < PS_EXC_MAX_THR; ++k) {
      if (k < nthr) {
        const bool b = v >= thr.t[k];   // a pad cell holds 0 < t
        const unsigned long long m = __ballot(b);
        const int64_t plane = (int64_t)k * nslot + s;
        if (writer) mask[plane * nword + word] = m;
        if (b) cnt[plane * pitch + i] += w;
      }
    }
    r = rn;
  }
}

// flat over nthr * nslot * pitch words
__global__ void k_excur_merge(uint32_t* __restrict__ ca, const uint32_t* __restrict__ cb, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) ca[i] += cb[i];
}

// blockIdx.y = plane (k, slot); every wave on its own keeps the counts of PS_EXC_CPT consecutive mask words
// (lane l the cell 64 j + l of word j) in registers and walks the members: per member one 8-byte word per
// register, a wave-wide max / min and at most two integer atomics.  A wave whose counts are all zero leaves at
// once: it can move neither bound (hi's identity is 0, and a set bit implies C >= w > 0).
__global__ void __launch_bounds__(PS_EXC_THREADS) k_excur_bounds(const uint32_t* __restrict__ cnt,
                                                                 const uint64_t* __restrict__ mask, int64_t members,
                                                                 int nplane, int64_t pitch, uint32_t* __restrict__ hi,
                                                                 uint32_t* __restrict__ lo) {
  const int p = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nword = pitch >> 6;
  const int64_t word0 = (blockIdx.x * (int64_t)(PS_EXC_THREADS / 64) + wave) * PS_EXC_CPT;
  const uint32_t* cp = cnt + (int64_t)p * pitch;
  uint32_t c[PS_EXC_CPT];
  bool any = false;
#pragma unroll
  for (int j = 0; j < PS_EXC_CPT; ++j) {
    c[j] = word0 + j < nword ? cp[(word0 + j) * 64 + lane] : 0u;
    any = any || c[j] != 0u;
  }
  if (!__any(any)) return;
  for (int64_t m = 0; m < members; ++m) {
    const uint64_t* mw = mask + (m * nplane + p) * nword;
    uint32_t h = 0u, l = PS_EXC_NONE;
#pragma unroll
    for (int j = 0; j < PS_EXC_CPT; ++j) {
      if (word0 + j < nword) {
        const bool bit = (mw[word0 + j] >> lane) & 1ull;
        if (bit)
          l = min(l, c[j]);
        else
          h = max(h, c[j]);
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      h = max(h, (uint32_t)__shfl_xor((int)h, off));
      l = min(l, (uint32_t)__shfl_xor((int)l, off));
    }
    if (lane == 0) {
      if (h != 0u) atomicMax(hi + m * nplane + p, h);
      if (l != PS_EXC_NONE) atomicMin(lo + m * nplane + p, l);
    }
  }
}

// one thread per cell: x = C (mode 0 above, 1 below) or u = min(C, W - C) (mode 2 contour); j = the number of
// breakpoints bp[0..n) (ascending) that are <= x, A = val[j]; out = (double)A / (double)W.  Above is 0 where
// C == 0, the contour where 2u >= W.
__global__ void k_excur_map(const uint32_t* __restrict__ cp, const uint32_t* __restrict__ bp,
                            const uint32_t* __restrict__ val, int n, int mode, uint32_t W, int64_t ncell,
                            double* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  const uint32_t C = cp[i];
  uint32_t x = C;
  bool zero = mode == 0 && C == 0u;
  if (mode == 2) {
    x = min(C, W - C);
    zero = 2ull * x >= (unsigned long long)W;
  }
  uint32_t A = 0u;
  if (!zero) {
    int a = 0, b = n;   // the first index with bp > x
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (bp[mid] <= x)
        a = mid + 1;
      else
        b = mid;
    }
    A = val[a];
  }
  out[i] = (double)A / (double)W;
}

}  // namespace

struct ps_excur {
  int device = 0, N = 0, nslot = 0, nthr = 0;
  std::vector<double> thr;
  int64_t ncell = 0, pitch = 0;
  uint32_t* cnt = nullptr;     // [k][slot][pitch]
  uint64_t* mask = nullptr;    // [cap][k][slot][pitch / 64]
  int64_t cap = 0;             // members the mask block holds
  uint32_t* bounds = nullptr;  // hi[bounds_cap][k][slot], then lo[bounds_cap][k][slot]
  int64_t bounds_cap = 0;
  uint32_t* table = nullptr;   // the step table of one map: breakpoints [members], then values [members + 1]
  int64_t table_cap = 0;       // in words
  double* map = nullptr;       // [pitch] map scratch
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;   // per member, in add order
  bool fin = false;                // h_hi / h_lo hold the bounds of the present members
  std::vector<uint32_t> h_hi, h_lo;   // [member][k][slot]
  hipStream_t stream = nullptr;    // reset / merge / finalize / maps / fetch / growth, and the adds of fields sources
  PsLastOp last;                   // the last operation, on whatever stream it ran
  PsProf prof;                     // channel 0: the adds, 1: the finalizes, 2: the maps
};

static int64_t exc_planes(const ps_excur* a) { return (int64_t)a->nthr * a->nslot; }
static size_t exc_cnt_bytes(const ps_excur* a) { return (size_t)exc_planes(a) * a->pitch * sizeof(uint32_t); }
static int64_t exc_member_words(const ps_excur* a) { return exc_planes(a) * (a->pitch >> 6); }

// a device block of `bytes`, checked against the free memory first (who / what: for the message)
static int exc_alloc(void** p, size_t bytes, const char* who, const char* what) {
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((double)bytes > (double)free_b)
    return ps_fail(PS_ERR_OOM, "%s: %s need %.3g GB, %.3g GB free", who, what, (double)bytes * 1e-9,
                   (double)free_b * 1e-9);
  PS_HIP(hipMalloc(p, bytes));
  return PS_OK;
}

// room for `need` members' masks: exactly `need` when exact (ps_excur_reserve), else by doubling.  A growth copies
// the masks so far on the handle's stream and synchronises once before the old block is freed.
static int exc_reserve_members(ps_excur* a, int64_t need, bool exact, const char* who) {
  if (need <= a->cap) return PS_OK;
  int64_t cap = need;
  if (!exact) {
    cap = std::max<int64_t>(a->cap, PS_EXC_MEMBERS0);
    while (cap < need) cap *= 2;
  }
  const size_t mem_b = (size_t)exc_member_words(a) * sizeof(uint64_t);
  uint64_t* p = nullptr;
  PS_TRY(exc_alloc((void**)&p, (size_t)cap * mem_b, who, "the member masks"));
  if (a->mask) {
    hipError_t e = hipSuccess;
    if (a->last.live) e = hipStreamWaitEvent(a->stream, a->last.ev, 0);
    if (e == hipSuccess && a->members > 0)
      e = hipMemcpyAsync(p, a->mask, (size_t)a->members * mem_b, hipMemcpyDeviceToDevice, a->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return ps_fail(PS_ERR_HIP, "%s: growing the member masks: %s", who, hipGetErrorString(e));
    }
    PS_HIP(hipFree(a->mask));
  }
  a->mask = p;
  a->cap = cap;
  return PS_OK;
}

// a scratch block of at least `need` elements, regrown (not copied) once the stream has drained
template <typename T>
static int exc_scratch(ps_excur* a, T** p, int64_t* cap, int64_t need, size_t elem_b, const char* what) {
  if (need <= *cap) return PS_OK;
  if (*p) {
    PS_HIP(hipStreamSynchronize(a->stream));
    PS_HIP(hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  int64_t n = std::max<int64_t>(*cap, 64);
  while (n < need) n *= 2;
  PS_TRY(exc_alloc((void**)p, (size_t)n * elem_b, "excur", what));
  *cap = n;
  return PS_OK;
}

extern "C" void ps_excur_destroy(ps_excur* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->cnt, (void*)a->mask, (void*)a->bounds, (void*)a->table, (void*)a->map})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_excur_reset(ps_excur* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "excur_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->cnt, 0, exc_cnt_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  a->weights.clear();
  a->fin = false;
  return PS_OK;
}

extern "C" int ps_excur_create(int device, int N, int nslot, int nthr, const double* thr, ps_excur** out) {
  if (!out || N < 1 || nslot < 1 || nslot > PS_EXC_MAX_SLOT || nthr < 1 || nthr > PS_EXC_MAX_THR || !thr)
    return ps_fail(PS_ERR_BAD_ARG, "excur_create: N %d, %d slots (1..%d), %d thresholds (1..%d)", N, nslot,
                   PS_EXC_MAX_SLOT, nthr, PS_EXC_MAX_THR);
  *out = nullptr;
  for (int k = 0; k < nthr; ++k) {
    if (!(thr[k] > 0.0) || !isfinite(thr[k]))
      return ps_fail(PS_ERR_BAD_ARG, "excur_create: threshold %d = %g is not finite and > 0", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "excur_create: thresholds not strictly increasing at %d", k);
  }
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  if (pitch / PS_EXC_THREADS + 1 > 0x7fffffffLL)
    return ps_fail(PS_ERR_BAD_ARG, "excur_create: N %d is too large for one launch", N);
  // the counts and the map scratch, checked before anything is allocated; the member masks are checked as they grow
  const double need = (double)nthr * nslot * pitch * 4.0 + (double)pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "excur_create: %d thresholds x %d slots x %lld cells x 4 B = %.3g GB, %.3g GB free",
                   nthr, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_excur* a = new ps_excur();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nthr = nthr;
  a->thr.assign(thr, thr + nthr);
  a->ncell = ncell;
  a->pitch = pitch;
  auto fail = [&](int rc) {
    ps_excur_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->cnt, exc_cnt_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->map, (size_t)pitch * sizeof(double));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "excur_create: %s", hipGetErrorString(e)));
  int rc = ps_excur_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

extern "C" int ps_excur_reserve(ps_excur* a, int64_t members) {
  if (!a || members < 0) return ps_fail(PS_ERR_BAD_ARG, "excur_reserve: bad arguments");
  PS_HIP(hipSetDevice(a->device));
  return exc_reserve_members(a, members, true, "excur_reserve");
}

// W stays below 2^32 - 1: the bound "no cell" of lo takes the last value
static int exc_check_weight(const ps_excur* a, const char* who, uint64_t weight) {
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xfffffffeull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow: it has to stay below 2^32 - 1", who,
                   (unsigned long long)(a->W + weight));
  return PS_OK;
}

// one member from the slot descriptors (one per slot of the handle, the rest null), enqueued on `stream`
static int exc_launch(ps_excur* a, const ExcSlots& desc, hipStream_t stream, double negval, uint32_t weight,
                      const char* who) {
  ExcThr thr;
  for (int k = 0; k < PS_EXC_MAX_THR; ++k) thr.t[k] = k < a->nthr ? a->thr[(size_t)k] : 0.0;
  PS_TRY(exc_reserve_members(a, a->members + 1, false, who));
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  const unsigned nblk = (unsigned)((a->pitch + PS_EXC_THREADS - 1) / PS_EXC_THREADS);
  hipLaunchKernelGGL(k_excur_add, dim3(nblk), dim3(PS_EXC_THREADS), 0, stream, desc, thr, a->nslot, a->nthr, a->cnt,
                     a->mask + a->members * exc_member_words(a), a->ncell, a->pitch, negval, weight);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  a->weights.push_back(weight);
  a->fin = false;
  return PS_OK;
}

extern "C" int ps_excur_add(ps_excur* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                            const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                            double negval, uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "excur_add: bad arguments");
  if (nslot != a->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "excur_add: %d slots given, the handle has %d", nslot, a->nslot);
  PS_TRY(exc_check_weight(a, "excur_add", weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  ExcSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("excur_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nslot; i < PS_EXC_MAX_SLOT; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return exc_launch(a, desc, stream, negval, weight, "excur_add");
}

// one member whose slots are the current fields of a projection, a release plan or the peak maps, in ascending
// output order (who: the entry point)
static int exc_add_fields(ps_excur* a, void* h, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(exc_check_weight(a, who, weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  ExcSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, desc.s));
  for (int e = a->nslot; e < PS_EXC_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(exc_launch(a, desc, a->stream, 0.0, weight, who));
  return src.mark(h, a->stream);   // the next apply overwrites the source's fields only after this read
}

extern "C" int ps_excur_add_project(ps_excur* a, ps_project* p, uint32_t weight) {
  return exc_add_fields(a, p, ps_project_fields(), "excur_add_project", weight);
}

extern "C" int ps_excur_add_sites(ps_excur* a, ps_sites* p, uint32_t weight) {
  return exc_add_fields(a, p, ps_sites_fields(), "excur_add_sites", weight);
}

extern "C" int ps_excur_add_peak(ps_excur* a, ps_peak* p, uint32_t weight) {
  return exc_add_fields(a, p, ps_peak_fields(), "excur_add_peak", weight);
}

extern "C" int ps_excur_merge(ps_excur* dst, ps_excur* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "excur_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->thr != src->thr)
    return ps_fail(PS_ERR_BAD_ARG, "excur_merge: handles differ in device, domain, slots or thresholds");
  if (dst->W + src->W > 0xfffffffeull) return ps_fail(PS_ERR_BAD_ARG, "excur_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(exc_reserve_members(dst, dst->members + src->members, false, "excur_merge"));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  hipLaunchKernelGGL(k_excur_merge, dim3(2048), dim3(256), 0, dst->stream, dst->cnt, src->cnt,
                     exc_planes(dst) * dst->pitch);
  PS_HIP(hipGetLastError());
  const int64_t mw = exc_member_words(dst);
  PS_HIP(hipMemcpyAsync(dst->mask + dst->members * mw, src->mask, (size_t)(src->members * mw) * sizeof(uint64_t),
                        hipMemcpyDeviceToDevice, dst->stream));
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  dst->weights.insert(dst->weights.end(), src->weights.begin(), src->weights.end());
  dst->fin = false;
  return PS_OK;
}

extern "C" int ps_excur_info(ps_excur* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "excur_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  if (capacity) *capacity = a->cap;
  if (bytes)
    *bytes = (int64_t)exc_cnt_bytes(a) + a->cap * exc_member_words(a) * 8 + a->pitch * 8 + a->bounds_cap * exc_planes(a) * 8 +
             a->table_cap * 4;
  return PS_OK;
}

extern "C" int ps_excur_finalize(ps_excur* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "excur_finalize: null handle");
  if (a->members == 0) return ps_fail(PS_ERR_STATE, "excur_finalize: nothing accumulated (no member added)");
  if (a->fin) return PS_OK;
  PS_HIP(hipSetDevice(a->device));
  const int64_t np = exc_planes(a), n = a->members * np;
  PS_TRY(exc_scratch(a, &a->bounds, &a->bounds_cap, a->members, (size_t)np * 2 * sizeof(uint32_t), "the member bounds"));
  uint32_t* hi = a->bounds;
  uint32_t* lo = a->bounds + a->bounds_cap * np;
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  PS_HIP(hipMemsetAsync(hi, 0, (size_t)n * sizeof(uint32_t), a->stream));
  PS_HIP(hipMemsetAsync(lo, 0xff, (size_t)n * sizeof(uint32_t), a->stream));
  const int64_t nword = a->pitch >> 6;
  const int64_t per_block = (int64_t)(PS_EXC_THREADS / 64) * PS_EXC_CPT;
  hipLaunchKernelGGL(k_excur_bounds, dim3((unsigned)((nword + per_block - 1) / per_block), (unsigned)np),
                     dim3(PS_EXC_THREADS), 0, a->stream, a->cnt, a->mask, a->members, (int)np, a->pitch, hi, lo);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  a->h_hi.resize((size_t)n);
  a->h_lo.resize((size_t)n);
  PS_HIP(hipMemcpyAsync(a->h_hi.data(), hi, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipMemcpyAsync(a->h_lo.data(), lo, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  a->fin = true;
  return PS_OK;
}

static int exc_check_plane(ps_excur* a, int k, int slot, const char* who) {
  if (k < 0 || k >= a->nthr) return ps_fail(PS_ERR_BAD_ARG, "%s: threshold %d of %d", who, k, a->nthr);
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: slot %d of %d", who, slot, a->nslot);
  return PS_OK;
}

extern "C" int ps_excur_map(ps_excur* a, int k, int slot, int what, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "excur_map: bad arguments");
  PS_TRY(exc_check_plane(a, k, slot, "excur_map"));
  if (what < PS_EXCUR_ABOVE || what > PS_EXCUR_CONTOUR)
    return ps_fail(PS_ERR_BAD_ARG, "excur_map: map %d is none of above (0), below (1), contour (2)", what);
  if (a->members == 0) return ps_fail(PS_ERR_STATE, "excur_map: nothing accumulated (no member added)");
  PS_TRY(ps_excur_finalize(a));
  // the step table: member m counts while x stays below its breakpoint (below, contour), or from it on (above)
  const int64_t np = exc_planes(a), p = (int64_t)k * a->nslot + slot;
  const size_t M = (size_t)a->members;
  std::vector<uint32_t> bp(M);
  for (size_t m = 0; m < M; ++m) {
    const uint32_t hi = a->h_hi[m * np + p], lo = a->h_lo[m * np + p];
    if (what == PS_EXCUR_ABOVE)
      bp[m] = hi + 1u;                                     // hi < C  <=>  hi + 1 <= C  (hi <= W < 2^32 - 1)
    else if (what == PS_EXCUR_BELOW)
      bp[m] = lo;                                          // out once lo <= C
    else
      bp[m] = std::min((uint32_t)a->W - hi, lo);           // out once W - hi <= u or lo <= u
  }
  std::vector<size_t> order(M);
  std::iota(order.begin(), order.end(), (size_t)0);
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return bp[x] < bp[y]; });
  std::vector<uint32_t> tab(2 * M + 1);   // breakpoints [M], values [M + 1]: val[j] with j breakpoints <= x
  uint64_t cum = 0;
  tab[M] = what == PS_EXCUR_ABOVE ? 0u : (uint32_t)a->W;
  for (size_t j = 0; j < M; ++j) {
    tab[j] = bp[order[j]];
    cum += a->weights[order[j]];
    tab[M + 1 + j] = what == PS_EXCUR_ABOVE ? (uint32_t)cum : (uint32_t)(a->W - cum);
  }
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(exc_scratch(a, &a->table, &a->table_cap, (int64_t)tab.size(), sizeof(uint32_t), "the step table"));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(a->table, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(2, a->stream, &e1));
  hipLaunchKernelGGL(k_excur_map, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream,
                     a->cnt + p * a->pitch, a->table, a->table + M, (int)M, what, (uint32_t)a->W, a->ncell, a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->map, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));   // tab is read until here
  return PS_OK;
}

extern "C" int ps_excur_fetch_counts(ps_excur* a, int k, int slot, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "excur_fetch_counts: bad arguments");
  PS_TRY(exc_check_plane(a, k, slot, "excur_fetch_counts"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->cnt + ((int64_t)k * a->nslot + slot) * a->pitch, (size_t)a->ncell * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_excur_fetch_mask(ps_excur* a, int64_t member, int k, int slot, uint64_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "excur_fetch_mask: bad arguments");
  PS_TRY(exc_check_plane(a, k, slot, "excur_fetch_mask"));
  if (member < 0 || member >= a->members)
    return ps_fail(PS_ERR_BAD_ARG, "excur_fetch_mask: member %lld of %lld", (long long)member, (long long)a->members);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const int64_t nword = a->pitch >> 6;
  PS_HIP(hipMemcpyAsync(out, a->mask + member * exc_member_words(a) + ((int64_t)k * a->nslot + slot) * nword,
                        (size_t)nword * sizeof(uint64_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_excur_fetch_bounds(ps_excur* a, int k, int slot, uint32_t* hi, uint32_t* lo, uint32_t* weights) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "excur_fetch_bounds: null handle");
  PS_TRY(exc_check_plane(a, k, slot, "excur_fetch_bounds"));
  if (a->members == 0) return ps_fail(PS_ERR_STATE, "excur_fetch_bounds: nothing accumulated (no member added)");
  PS_TRY(ps_excur_finalize(a));
  const int64_t np = exc_planes(a), p = (int64_t)k * a->nslot + slot;
  for (int64_t m = 0; m < a->members; ++m) {
    if (hi) hi[m] = a->h_hi[(size_t)(m * np + p)];
    if (lo) lo[m] = a->h_lo[(size_t)(m * np + p)];
    if (weights) weights[m] = a->weights[(size_t)m];
  }
  return PS_OK;
}

extern "C" int ps_excur_prof(ps_excur* a, int enable, double* ms, int64_t* launches) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "excur_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  if (!ms && !launches) return PS_OK;
  for (int k = 0; k < 3; ++k) PS_TRY(a->prof.totals(k, ms ? ms + k : nullptr, launches ? launches + k : nullptr));
  return PS_OK;
}

// what ps_overlap.hip reads (ps_common.h): the masks and counts as they are now, and the handle's event
int ps_excur_view_internal(ps_excur* a, PsExcurView* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "excur_view: bad arguments");
  *out = PsExcurView{a->mask, a->cnt, a->weights.data(), a->pitch, a->members, a->N, a->nthr, a->nslot, a->device};
  return PS_OK;
}
int ps_excur_wait_internal(ps_excur* a, hipStream_t stream) { return a->last.wait(stream); }
int ps_excur_mark_internal(ps_excur* a, hipStream_t stream) { return a->last.mark(stream); }
