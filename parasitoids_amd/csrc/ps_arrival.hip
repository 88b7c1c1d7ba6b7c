// Posterior arrival maps (include/parasitoid_hip.h, ps_arrival_*): per threshold t_k and cell the weighted
// distribution of the first day slot on which a member's value reaches t_k, accumulated on the device from
// the solver's records, and per member the number of cells reached by each slot.  The value of a slot is
// the one ps_summary_add adds (ps_record_value).  a_k(c) = min{s : v_s(c) >= t_k}, nslot = never (not stored:
// W - the rest).  Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   cnt[k][slot][pitch]      uint32, the weight of the members with a_k(c) = slot
//   part[k][slot][nblk]      uint32, per add-block the cells with a_k <= slot (summed by k_arrival_rows)
//   rows[member][k][slot]    uint32, n_k(slot) of every member, in add order; grows by doubling
// One thread owns a pair of cells and walks the slots in order, so every count has a single writer; the
// per-block reached counts are integers summed in LDS and then over blocks.  No floating-point atomics:
// neither the order of adds nor that of merges nor the grid changes a bit.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_ARR_MAX_SLOT 32   // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_ARR_MAX_THR 4
#define PS_ARR_THREADS 256
#define PS_ARR_ROWS0 64      // member rows allocated at create

namespace {

struct ArrSlots {
  PsSrc s[PS_ARR_MAX_SLOT];
};
struct ArrThr {
  double t[PS_ARR_MAX_THR];
};

__device__ inline void arr_load(const double* __restrict__ rec, bool pair, int64_t i, double2& r) {
  if (pair)
    r = *reinterpret_cast<const double2*>(rec + i);
  else
    r = make_double2(rec[i], 0.0);
}

// thread j owns the cells 2j, 2j + 1 (j == npair: the tail cell of an odd N*N alone).  The record of slot
// s + 1 is loaded while slot s is tested; a wave stops once every lane's cells reached the top threshold.
__global__ void __launch_bounds__(PS_ARR_THREADS) k_arrival_add(ArrSlots desc, ArrThr thr, int nslot, int nthr,
                                                                uint32_t* __restrict__ cnt, uint32_t* __restrict__ part,
                                                                int64_t ncell, int64_t pitch, double negval, uint32_t w) {
  __shared__ uint32_t hist[PS_ARR_MAX_THR * PS_ARR_MAX_SLOT];
  __shared__ double sdelta[PS_ARR_MAX_SLOT];
  const int nks = nthr * nslot;
  for (int t = threadIdx.x; t < nks; t += blockDim.x) hist[t] = 0;
  for (int t = threadIdx.x; t < nslot; t += blockDim.x) sdelta[t] = desc.s[t].stats ? desc.s[t].stats->delta : 0.0;
  __syncthreads();
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pair = j < npair, tail = j == npair && (ncell & 1);
  const int64_t i = 2 * j;
  int a0[PS_ARR_MAX_THR], a1[PS_ARR_MAX_THR];
#pragma unroll
  for (int k = 0; k < PS_ARR_MAX_THR; ++k) a0[k] = a1[k] = nslot;
  const double top = thr.t[nthr - 1];
  bool top0 = false, top1 = !pair;   // the tail thread has no second cell
  bool live = pair || tail;
  double2 r = make_double2(0.0, 0.0);
  if (live) arr_load(desc.s[0].rec, pair, i, r);
  for (int s = 0; s < nslot; ++s) {
    if (!__any(live)) break;
    double2 rn = make_double2(0.0, 0.0);
    if (live && s + 1 < nslot) arr_load(desc.s[s + 1].rec, pair, i, rn);
    if (live) {
      const PsSrc& sd = desc.s[s];
      const double delta = sdelta[s];
      const double v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
      const double v1 = pair ? ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval) : 0.0;
#pragma unroll
      for (int k = 0; k < PS_ARR_MAX_THR; ++k) {
        if (k < nthr) {
          if (a0[k] == nslot && v0 >= thr.t[k]) a0[k] = s;
          if (pair && a1[k] == nslot && v1 >= thr.t[k]) a1[k] = s;
        }
      }
      top0 = top0 || v0 >= top;
      top1 = top1 || v1 >= top;
      live = !(top0 && top1);
    }
    r = rn;
  }
  if (pair || tail) {
#pragma unroll
    for (int k = 0; k < PS_ARR_MAX_THR; ++k) {
      if (k >= nthr) break;
      const int s0 = a0[k], s1 = a1[k];   // s1 == nslot for the tail cell
      uint32_t* ck = cnt + (int64_t)k * nslot * pitch;
      if (s0 == s1 && s0 < nslot) {   // a pair arriving together: one 8-byte update
        uint2* p = reinterpret_cast<uint2*>(ck + (int64_t)s0 * pitch + i);
        uint2 c = *p;
        c.x += w;
        c.y += w;
        *p = c;
        atomicAdd(&hist[k * nslot + s0], 2u);
      } else {
        if (s0 < nslot) {
          ck[(int64_t)s0 * pitch + i] += w;
          atomicAdd(&hist[k * nslot + s0], 1u);
        }
        if (s1 < nslot) {
          ck[(int64_t)s1 * pitch + i + 1] += w;
          atomicAdd(&hist[k * nslot + s1], 1u);
        }
      }
    }
  }
  __syncthreads();
  // this block's cells reached by slot s: the arrivals at 0..s
  for (int t = threadIdx.x; t < nks; t += blockDim.x) {
    const int k = t / nslot, s = t - k * nslot;
    uint32_t c = 0;
    for (int q = 0; q <= s; ++q) c += hist[k * nslot + q];
    part[(int64_t)t * gridDim.x + blockIdx.x] = c;
  }
}

// block t = k * nslot + s: n_k(s) = the sum of the add-blocks' partials, into the member's row
__global__ void __launch_bounds__(PS_ARR_THREADS) k_arrival_rows(const uint32_t* __restrict__ part, int nblk,
                                                                 uint32_t* __restrict__ row) {
  __shared__ uint32_t red[PS_ARR_THREADS];
  const uint32_t* p = part + (int64_t)blockIdx.x * nblk;
  uint32_t c = 0;
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) c += p[b];
  red[threadIdx.x] = c;
  __syncthreads();
  for (int h = blockDim.x / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) row[blockIdx.x] = red[0];
}

// flat over nthr * nslot * pitch words
__global__ void k_arrival_merge(uint32_t* __restrict__ ca, const uint32_t* __restrict__ cb, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) ca[i] += cb[i];
}

// one threshold, one thread per cell: C = the counts of planes 0 .. nplane - 1; prob = C / W, else cum = C
__global__ void k_arrival_cum(const uint32_t* __restrict__ ck, int nplane, int64_t ncell, int64_t pitch, double W,
                              double* __restrict__ prob, uint32_t* __restrict__ cum) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  uint32_t c = 0;
  for (int s = 0; s < nplane; ++s) c += ck[(int64_t)s * pitch + i];
  if (prob)
    prob[i] = (double)c / W;
  else
    cum[i] = c;
}

// one threshold, one thread per cell: the smallest s with (double)C_s >= p W, -1 if none; reads planes 0 .. s
__global__ void k_arrival_quantile(const uint32_t* __restrict__ ck, int nslot, int64_t ncell, int64_t pitch, double pW,
                                   int32_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  uint32_t c = 0;
  int q = -1;
  for (int s = 0; s < nslot; ++s) {
    c += ck[(int64_t)s * pitch + i];
    if ((double)c >= pW) {
      q = s;
      break;
    }
  }
  out[i] = q;
}

}  // namespace

struct ps_arrival {
  int device = 0, N = 0, nslot = 0, nthr = 0;
  std::vector<double> thr;
  int64_t ncell = 0, pitch = 0;
  int nblk = 0;                // blocks of one add launch
  uint32_t* cnt = nullptr;     // [k][slot][pitch]
  uint32_t* part = nullptr;    // [k][slot][nblk]
  uint32_t* rows = nullptr;    // [rows_cap][k][slot]
  int64_t rows_cap = 0;
  double* map = nullptr;       // [pitch] map scratch (prob / quantile / cumulative counts)
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;   // per member, in row order
  hipStream_t stream = nullptr;    // reset / merge / maps / fetch / row growth
  PsLastOp last;                   // the last operation, on whatever stream it ran
  PsProf prof;                     // channel 0: the adds, 1: the maps
};

static int64_t arr_row_len(const ps_arrival* a) { return (int64_t)a->nthr * a->nslot; }
static size_t arr_cnt_bytes(const ps_arrival* a) { return (size_t)arr_row_len(a) * a->pitch * sizeof(uint32_t); }

// room for `need` member rows: a doubling copies the rows so far on the handle's stream and synchronises
// once before the old block is freed
static int arr_reserve_rows(ps_arrival* a, int64_t need) {
  if (need <= a->rows_cap) return PS_OK;
  int64_t cap = std::max<int64_t>(a->rows_cap, PS_ARR_ROWS0);
  while (cap < need) cap *= 2;
  const size_t row_b = (size_t)arr_row_len(a) * sizeof(uint32_t);
  uint32_t* p = nullptr;
  PS_HIP(hipMalloc((void**)&p, (size_t)cap * row_b));
  if (a->rows) {
    hipError_t e = hipSuccess;
    if (a->last.live) e = hipStreamWaitEvent(a->stream, a->last.ev, 0);
    if (e == hipSuccess && a->members > 0)
      e = hipMemcpyAsync(p, a->rows, (size_t)a->members * row_b, hipMemcpyDeviceToDevice, a->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return ps_fail(PS_ERR_HIP, "arrival: growing the member rows: %s", hipGetErrorString(e));
    }
    PS_HIP(hipFree(a->rows));
  }
  a->rows = p;
  a->rows_cap = cap;
  return PS_OK;
}

extern "C" void ps_arrival_destroy(ps_arrival* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->cnt, (void*)a->part, (void*)a->rows, (void*)a->map})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_arrival_reset(ps_arrival* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "arrival_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->cnt, 0, arr_cnt_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  a->weights.clear();
  return PS_OK;
}

extern "C" int ps_arrival_create(int device, int N, int nslot, int nthr, const double* thr, ps_arrival** out) {
  if (!out || N < 1 || nslot < 1 || nslot > PS_ARR_MAX_SLOT || nthr < 1 || nthr > PS_ARR_MAX_THR || !thr)
    return ps_fail(PS_ERR_BAD_ARG, "arrival_create: N %d, %d slots (1..%d), %d thresholds (1..%d)", N, nslot,
                   PS_ARR_MAX_SLOT, nthr, PS_ARR_MAX_THR);
  for (int k = 0; k < nthr; ++k) {
    if (!(thr[k] > 0.0) || !isfinite(thr[k]))
      return ps_fail(PS_ERR_BAD_ARG, "arrival_create: threshold %d = %g is not finite and > 0", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "arrival_create: thresholds not strictly increasing at %d", k);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  const int64_t nblk = (ncell / 2 + 1 + PS_ARR_THREADS - 1) / PS_ARR_THREADS;   // the pairs and the tail thread
  if (nblk > 0x7fffffffLL) return ps_fail(PS_ERR_BAD_ARG, "arrival_create: N %d is too large for one launch", N);
  // everything, checked before anything is allocated: counts, block partials, the first member rows, map scratch
  const double nks = (double)nthr * nslot;
  const double need = nks * pitch * 4.0 + nks * nblk * 4.0 + nks * PS_ARR_ROWS0 * 4.0 + (double)pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "arrival_create: %d thresholds x %d slots x %lld cells x 4 B = %.3g GB, %.3g GB free",
                   nthr, nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_arrival* a = new ps_arrival();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nthr = nthr;
  a->thr.assign(thr, thr + nthr);
  a->ncell = ncell;
  a->pitch = pitch;
  a->nblk = (int)nblk;
  auto fail = [&](int rc) {
    ps_arrival_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->cnt, arr_cnt_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->part, (size_t)arr_row_len(a) * nblk * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&a->map, (size_t)pitch * sizeof(double));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "arrival_create: %s", hipGetErrorString(e)));
  int rc = arr_reserve_rows(a, PS_ARR_ROWS0);
  if (rc == PS_OK) rc = ps_arrival_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// one member from the slot descriptors (one per slot of the handle, the rest null), enqueued on `stream`
static int arr_launch(ps_arrival* a, const ArrSlots& desc, hipStream_t stream, double negval, uint32_t weight) {
  ArrThr thr;
  for (int k = 0; k < PS_ARR_MAX_THR; ++k) thr.t[k] = k < a->nthr ? a->thr[(size_t)k] : 0.0;
  PS_TRY(arr_reserve_rows(a, a->members + 1));
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  hipLaunchKernelGGL(k_arrival_add, dim3(a->nblk), dim3(PS_ARR_THREADS), 0, stream, desc, thr, a->nslot, a->nthr,
                     a->cnt, a->part, a->ncell, a->pitch, negval, weight);
  PS_HIP(hipGetLastError());
  const int nks = (int)arr_row_len(a);
  hipLaunchKernelGGL(k_arrival_rows, dim3(nks), dim3(PS_ARR_THREADS), 0, stream, a->part, a->nblk,
                     a->rows + a->members * nks);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  a->weights.push_back(weight);
  return PS_OK;
}

extern "C" int ps_arrival_add(ps_arrival* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                              const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                              double negval, uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "arrival_add: bad arguments");
  if (nslot != a->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "arrival_add: %d slots given, the handle has %d", nslot, a->nslot);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "arrival_add: weight must be >= 1");
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "arrival_add: total weight %llu would overflow the uint32 counts",
                   (unsigned long long)(a->W + weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  ArrSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("arrival_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale,
                         use_delta, false, desc.s, &stream));
  for (int i = nslot; i < PS_ARR_MAX_SLOT; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return arr_launch(a, desc, stream, negval, weight);
}

// one member whose slots are the current fields of a projection or a release plan, in ascending output order
// (who: the entry point)
static int arr_add_fields(ps_arrival* a, void* h, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(a->W + weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  ArrSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, desc.s));
  for (int e = a->nslot; e < PS_ARR_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(arr_launch(a, desc, a->stream, 0.0, weight));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_arrival_add_project(ps_arrival* a, ps_project* p, uint32_t weight) {
  return arr_add_fields(a, p, ps_project_fields(), "arrival_add_project", weight);
}

extern "C" int ps_arrival_add_sites(ps_arrival* a, ps_sites* p, uint32_t weight) {
  return arr_add_fields(a, p, ps_sites_fields(), "arrival_add_sites", weight);
}

extern "C" int ps_arrival_merge(ps_arrival* dst, ps_arrival* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "arrival_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->thr != src->thr)
    return ps_fail(PS_ERR_BAD_ARG, "arrival_merge: handles differ in device, domain, slots or thresholds");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "arrival_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(arr_reserve_rows(dst, dst->members + src->members));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  hipLaunchKernelGGL(k_arrival_merge, dim3(2048), dim3(256), 0, dst->stream, dst->cnt, src->cnt,
                     arr_row_len(dst) * dst->pitch);
  PS_HIP(hipGetLastError());
  const int64_t nks = arr_row_len(dst);
  PS_HIP(hipMemcpyAsync(dst->rows + dst->members * nks, src->rows, (size_t)(src->members * nks) * sizeof(uint32_t),
                        hipMemcpyDeviceToDevice, dst->stream));
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  dst->weights.insert(dst->weights.end(), src->weights.begin(), src->weights.end());
  return PS_OK;
}

extern "C" int ps_arrival_info(ps_arrival* a, double* total_weight, int64_t* members) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "arrival_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  return PS_OK;
}

static int arr_check(ps_arrival* a, int k, const char* who) {
  if (k < 0 || k >= a->nthr) return ps_fail(PS_ERR_BAD_ARG, "%s: threshold %d of %d", who, k, a->nthr);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated (W = 0)", who);
  return PS_OK;
}

// planes 0 .. nplane - 1 of threshold k summed into the map scratch (as prob = C / W, or as uint32 C)
static int arr_cum(ps_arrival* a, int k, int nplane, bool prob) {
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  const uint32_t* ck = a->cnt + (int64_t)k * a->nslot * a->pitch;
  hipLaunchKernelGGL(k_arrival_cum, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream, ck, nplane,
                     a->ncell, a->pitch, (double)a->W, prob ? a->map : nullptr, prob ? nullptr : (uint32_t*)a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  return PS_OK;
}

extern "C" int ps_arrival_prob(ps_arrival* a, int k, int slot, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "arrival_prob: bad arguments");
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "arrival_prob: slot %d of %d", slot, a->nslot);
  PS_TRY(arr_check(a, k, "arrival_prob"));
  PS_TRY(arr_cum(a, k, slot + 1, true));
  PS_HIP(hipMemcpyAsync(out, a->map, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_arrival_quantile(ps_arrival* a, int k, double p, int32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "arrival_quantile: bad arguments");
  if (!(p > 0.0 && p <= 1.0)) return ps_fail(PS_ERR_BAD_ARG, "arrival_quantile: p = %g is not in (0, 1]", p);
  PS_TRY(arr_check(a, k, "arrival_quantile"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  const uint32_t* ck = a->cnt + (int64_t)k * a->nslot * a->pitch;
  hipLaunchKernelGGL(k_arrival_quantile, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream, ck,
                     a->nslot, a->ncell, a->pitch, p * (double)a->W, (int32_t*)a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->map, (size_t)a->ncell * sizeof(int32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_arrival_fetch_counts(ps_arrival* a, int k, int slot, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "arrival_fetch_counts: bad arguments");
  if (k < 0 || k >= a->nthr) return ps_fail(PS_ERR_BAD_ARG, "arrival_fetch_counts: threshold %d of %d", k, a->nthr);
  if (slot < 0 || slot > a->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "arrival_fetch_counts: slot %d of 0..%d", slot, a->nslot);
  const size_t n = (size_t)a->ncell;
  if (slot == a->nslot) {   // never: W - the stored planes
    PS_TRY(arr_cum(a, k, a->nslot, false));
    PS_HIP(hipMemcpyAsync(out, a->map, n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
    PS_HIP(hipStreamSynchronize(a->stream));
    const uint32_t W = (uint32_t)a->W;
    for (size_t i = 0; i < n; ++i) out[i] = W - out[i];
    return PS_OK;
  }
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const uint32_t* src = a->cnt + ((int64_t)k * a->nslot + slot) * a->pitch;
  PS_HIP(hipMemcpyAsync(out, src, n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_arrival_fetch_reached(ps_arrival* a, int64_t first, int64_t count, uint32_t* cells,
                                        uint32_t* weights) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "arrival_fetch_reached: null handle");
  if (first < 0 || count < 0 || first + count > a->members)
    return ps_fail(PS_ERR_BAD_ARG, "arrival_fetch_reached: members %lld .. %lld of %lld", (long long)first,
                   (long long)(first + count), (long long)a->members);
  if (weights)
    for (int64_t m = 0; m < count; ++m) weights[m] = a->weights[(size_t)(first + m)];
  if (!cells || count == 0) return PS_OK;
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const int64_t nks = arr_row_len(a);
  PS_HIP(hipMemcpyAsync(cells, a->rows + first * nks, (size_t)(count * nks) * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_arrival_prof(ps_arrival* a, int enable, double* add_ms, int64_t* adds, double* map_ms,
                               int64_t* maps) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "arrival_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  double* ms_out[2] = {add_ms, map_ms};
  int64_t* n_out[2] = {adds, maps};
  for (int k = 0; k < 2; ++k)
    if (ms_out[k] || n_out[k]) PS_TRY(a->prof.totals(k, ms_out[k], n_out[k]));
  return PS_OK;
}
