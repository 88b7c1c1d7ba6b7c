// Paired contrast of two release plans or two projections (include/parasitoid_hip.h, ps_contrast_*): per slot
// and cell the weighted mean and M2 of d = a - b over the members, the weight of the members with d > 0 and
// with d < 0, per threshold t_k the weight of those with a >= t_k > b (gain) and with b >= t_k > a (loss), and
// per member the cells each side covers at every threshold and slot.  a and b are the fields the two sources
// hold for the same member, so the pairing is kept.  Layout (pitch = N*N rounded up to 64 cells, as
// ps_summary.hip; P = 2 + 2 nthr count planes):
//   mean[slot][pitch], m2[slot][pitch]   fp64, the step of ps_summary.hip (sum_update) on d
//   cnt[slot][P][pitch]                  uint32: pos, neg, gain_0, loss_0, gain_1, ...
//   rows[member][2][k][slot]             uint32, cells with a >= t_k, then with b >= t_k; grows by doubling
// An add reads 16 B of a and b per cell and slot and reads + writes 16 B of mean, 16 B of M2 and 8 B per count
// plane only where a pair of cells changes something (d != mean, or a count applies): most of the domain is
// 0 - 0 against a mean of 0.  One thread owns a pair of cells, so every mean, M2 and count cell has a single
// writer; the per-member cell counts are popcounts of wave ballots carried in a register over the grid stride,
// summed over the block's waves in LDS, then one integer atomicAdd per block and counter.  No floating-point
// atomics: neither the order of adds nor that of merges nor the grid changes a bit of a count.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_CON_MAX_THR 4
#define PS_CON_CHUNK 32          // slots per launch: 32 descriptors = 768 B of kernel arguments
#define PS_CON_THREADS 256
#define PS_CON_MAX_BLOCKS 4096   // per slot, as ps_summary.hip; more pairs than 4096 x 256 take the grid stride
#define PS_CON_ROWS0 64          // member rows allocated at create

namespace {

struct ConSlot {
  const double* a;
  const double* b;
  int slot;
};
struct ConSlots {
  ConSlot s[PS_CON_CHUNK];
};
struct ConThr {
  double t[PS_CON_MAX_THR];
};

// one count plane of a pair of cells (the tail cell alone: e1 is false there)
__device__ inline void con_count(uint32_t* __restrict__ plane, int64_t i, bool pair, bool e0, bool e1, uint32_t wi) {
  if (!(e0 || e1)) return;
  if (pair) {
    uint2* p = reinterpret_cast<uint2*>(plane + i);
    uint2 c = *p;
    c.x += e0 ? wi : 0u;
    c.y += e1 ? wi : 0u;
    *p = c;
  } else {
    plane[i] += wi;
  }
}

// blockIdx.y = slot of the chunk; thread item j owns the cells 2j, 2j + 1 (j == npair: the tail cell of an odd
// N*N alone).  Every thread of a block makes the same number of trips, so the ballots see whole waves.
__global__ void __launch_bounds__(PS_CON_THREADS)
    k_contrast_add(ConSlots desc, double* __restrict__ mean, double* __restrict__ m2, uint32_t* __restrict__ cnt,
                   uint32_t* __restrict__ row, int64_t ncell, int64_t pitch, int nslot, int nthr, ConThr thr, double w,
                   double Wn, uint32_t wi) {
  __shared__ uint32_t part[PS_CON_THREADS / 64][2 * PS_CON_MAX_THR];
  const ConSlot sd = desc.s[blockIdx.y];
  const double* __restrict__ A = sd.a;
  const double* __restrict__ B = sd.b;
  double* ms = mean + (int64_t)sd.slot * pitch;
  double* qs = m2 + (int64_t)sd.slot * pitch;
  uint32_t* cs = cnt + (int64_t)sd.slot * (2 + 2 * nthr) * pitch;
  const int64_t npair = ncell >> 1;
  const int64_t nitem = npair + (ncell & 1);
  uint32_t na[PS_CON_MAX_THR] = {0u, 0u, 0u, 0u}, nb[PS_CON_MAX_THR] = {0u, 0u, 0u, 0u};
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < nitem; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = base + threadIdx.x;
    const bool pair = j < npair, live = j < nitem;
    const int64_t i = pair ? 2 * j : ncell - 1;
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    if (pair) {
      const double2 ra = *reinterpret_cast<const double2*>(A + i);
      const double2 rb = *reinterpret_cast<const double2*>(B + i);
      a0 = ra.x, a1 = ra.y, b0 = rb.x, b1 = rb.y;
    } else if (live) {
      a0 = A[i];
      b0 = B[i];
    }
    if (live) {
      const double d0 = __dsub_rn(a0, b0), d1 = __dsub_rn(a1, b1);
      double2 m, q;
      if (pair) {
        m = *reinterpret_cast<const double2*>(ms + i);
        q = *reinterpret_cast<const double2*>(qs + i);
      } else {
        m = make_double2(ms[i], 0.0);
        q = make_double2(qs[i], 0.0);
      }
      const bool c0 = sum_update(d0, w, Wn, m.x, q.x);
      const bool c1 = sum_update(d1, w, Wn, m.y, q.y);   // the tail's second cell: 0 against 0, nothing
      if (c0 || c1) {
        if (pair) {
          *reinterpret_cast<double2*>(ms + i) = m;
          *reinterpret_cast<double2*>(qs + i) = q;
        } else {
          ms[i] = m.x;
          qs[i] = q.x;
        }
      }
      con_count(cs, i, pair, d0 > 0.0, d1 > 0.0, wi);
      con_count(cs + pitch, i, pair, d0 < 0.0, d1 < 0.0, wi);
      for (int k = 0; k < nthr; ++k) {
        const double t = thr.t[k];
        con_count(cs + (int64_t)(2 + 2 * k) * pitch, i, pair, a0 >= t && b0 < t, a1 >= t && b1 < t, wi);
        con_count(cs + (int64_t)(3 + 2 * k) * pitch, i, pair, b0 >= t && a0 < t, b1 >= t && a1 < t, wi);
      }
    }
    // the cells each side covers: a lane without cells holds zeros, below every threshold
#pragma unroll
    for (int k = 0; k < PS_CON_MAX_THR; ++k) {
      if (k < nthr) {
        const double t = thr.t[k];
        na[k] += (uint32_t)(__popcll(__ballot(a0 >= t)) + __popcll(__ballot(a1 >= t)));
        nb[k] += (uint32_t)(__popcll(__ballot(b0 >= t)) + __popcll(__ballot(b1 >= t)));
      }
    }
  }
  if (nthr == 0) return;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < PS_CON_MAX_THR; ++k) {
      part[threadIdx.x >> 6][k] = na[k];
      part[threadIdx.x >> 6][PS_CON_MAX_THR + k] = nb[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * PS_CON_MAX_THR) {
    const int side = threadIdx.x / PS_CON_MAX_THR, k = threadIdx.x % PS_CON_MAX_THR;
    if (k < nthr) {
      uint32_t c = 0;
      for (int v = 0; v < PS_CON_THREADS / 64; ++v) c += part[v][threadIdx.x];
      if (c) atomicAdd(row + ((int64_t)side * nthr + k) * nslot + sd.slot, c);
    }
  }
}

// Chan, Golub & LeVeque on mean and M2, as k_summary_merge; the counts add
__global__ void k_contrast_merge(double* __restrict__ ma, double* __restrict__ qa, uint32_t* __restrict__ ca,
                                 const double* __restrict__ mb, const double* __restrict__ qb,
                                 const uint32_t* __restrict__ cb, int64_t nval, int64_t ncnt, double Wa,
                                 double Wb) {
  const double W = Wa + Wb;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nval; i += stride) {
    const double d = mb[i] - ma[i];
    ma[i] = ma[i] + d * (Wb / W);
    qa[i] = qa[i] + qb[i] + d * d * (Wa * Wb / W);
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ncnt; i += stride) ca[i] += cb[i];
}

}  // namespace

struct ps_contrast {
  int device = 0, N = 0, nslot = 0, nthr = 0;
  std::vector<double> thr;
  int64_t ncell = 0, pitch = 0;
  double* mean = nullptr;        // [slot][pitch]
  double* m2 = nullptr;          // [slot][pitch]
  uint32_t* cnt = nullptr;       // [slot][2 + 2 nthr][pitch]
  uint32_t* rows = nullptr;      // [rows_cap][2][k][slot]; null without thresholds
  int64_t rows_cap = 0;
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;   // per member, in row order
  hipStream_t stream = nullptr;    // every operation of the handle
  PsLastOp last;                   // the last operation
  PsProf prof;                     // channel 0: the adds
};

static int con_planes(const ps_contrast* h) { return 2 + 2 * h->nthr; }
static int64_t con_row_len(const ps_contrast* h) { return (int64_t)2 * h->nthr * h->nslot; }
static size_t con_val_bytes(const ps_contrast* h) { return (size_t)h->nslot * h->pitch * sizeof(double); }
static size_t con_cnt_bytes(const ps_contrast* h) {
  return (size_t)h->nslot * con_planes(h) * h->pitch * sizeof(uint32_t);
}

// room for `need` member rows: a doubling copies the rows so far on the handle's stream and synchronises once
// before the old block is freed
static int con_reserve_rows(ps_contrast* h, int64_t need) {
  if (h->nthr == 0 || need <= h->rows_cap) return PS_OK;
  int64_t cap = std::max<int64_t>(h->rows_cap, PS_CON_ROWS0);
  while (cap < need) cap *= 2;
  const size_t row_b = (size_t)con_row_len(h) * sizeof(uint32_t);
  uint32_t* p = nullptr;
  PS_HIP(hipMalloc((void**)&p, (size_t)cap * row_b));
  if (h->rows) {
    hipError_t e = hipSuccess;
    if (h->last.live) e = hipStreamWaitEvent(h->stream, h->last.ev, 0);
    if (e == hipSuccess && h->members > 0)
      e = hipMemcpyAsync(p, h->rows, (size_t)h->members * row_b, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return ps_fail(PS_ERR_HIP, "contrast: growing the member rows: %s", hipGetErrorString(e));
    }
    PS_HIP(hipFree(h->rows));
  }
  h->rows = p;
  h->rows_cap = cap;
  return PS_OK;
}

extern "C" void ps_contrast_destroy(ps_contrast* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  h->last.sync();
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->prof.release();
  for (void* p : {(void*)h->mean, (void*)h->m2, (void*)h->cnt, (void*)h->rows})
    if (p) (void)hipFree(p);
  h->last.destroy();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ps_contrast_reset(ps_contrast* h) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "contrast_reset: null handle");
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  PS_HIP(hipMemsetAsync(h->mean, 0, con_val_bytes(h), h->stream));
  PS_HIP(hipMemsetAsync(h->m2, 0, con_val_bytes(h), h->stream));
  PS_HIP(hipMemsetAsync(h->cnt, 0, con_cnt_bytes(h), h->stream));
  PS_TRY(h->last.mark(h->stream));
  h->W = 0;
  h->members = 0;
  h->weights.clear();
  return PS_OK;
}

extern "C" int ps_contrast_create(int device, int N, int nslot, int nthr, const double* thr, ps_contrast** out) {
  if (!out || N < 1 || nslot < 1 || nthr < 0 || nthr > PS_CON_MAX_THR || (nthr > 0 && !thr))
    return ps_fail(PS_ERR_BAD_ARG, "contrast_create: N %d, %d slots, %d thresholds (0..%d)", N, nslot, nthr,
                   PS_CON_MAX_THR);
  *out = nullptr;
  for (int k = 0; k < nthr; ++k) {
    if (!(thr[k] > 0.0) || !isfinite(thr[k]))
      return ps_fail(PS_ERR_BAD_ARG, "contrast_create: threshold %d = %g is not finite and > 0", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "contrast_create: thresholds not strictly increasing at %d", k);
  }
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // everything, checked before anything is allocated: both moments, the count planes, the first member rows
  const double planes = 2.0 + 2.0 * nthr;
  const double need = (double)nslot * pitch * (16.0 + 4.0 * planes) + 2.0 * nthr * nslot * PS_CON_ROWS0 * 4.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "contrast_create: %d slots x %lld cells x %g B = %.3g GB, %.3g GB free", nslot,
                   (long long)pitch, 16.0 + 4.0 * planes, need * 1e-9, (double)free_b * 1e-9);
  ps_contrast* h = new ps_contrast();
  h->device = device;
  h->N = N;
  h->nslot = nslot;
  h->nthr = nthr;
  h->thr.assign(thr, thr + nthr);
  h->ncell = ncell;
  h->pitch = pitch;
  auto fail = [&](int rc) {
    ps_contrast_destroy(h);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = h->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&h->mean, con_val_bytes(h));
  if (e == hipSuccess) e = hipMalloc((void**)&h->m2, con_val_bytes(h));
  if (e == hipSuccess) e = hipMalloc((void**)&h->cnt, con_cnt_bytes(h));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "contrast_create: %s", hipGetErrorString(e)));
  int rc = con_reserve_rows(h, PS_CON_ROWS0);
  if (rc == PS_OK) rc = ps_contrast_reset(h);
  if (rc != PS_OK) return fail(rc);
  *out = h;
  return PS_OK;
}

// one member whose values are the current fields of two projections or two release plans (who: the entry point)
static int con_add_fields(ps_contrast* h, void* a, void* b, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!h || !a || !b) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (a == b) return ps_fail(PS_ERR_BAD_ARG, "%s: both sides are the same %s", who, src.what);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (h->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(h->W + weight));
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
  PS_TRY(con_reserve_rows(h, h->members + 1));
  hipStream_t stream = h->stream;
  PS_TRY(src.wait(a, stream));
  PS_TRY(src.wait(b, stream));
  PS_TRY(h->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(h->prof.begin(0, stream, &e1));
  ConThr thr;
  for (int k = 0; k < PS_CON_MAX_THR; ++k) thr.t[k] = k < h->nthr ? h->thr[(size_t)k] : 0.0;
  uint32_t* row = nullptr;
  if (h->nthr) {   // the member's row: integer sums over the blocks, from zero
    row = h->rows + h->members * con_row_len(h);
    hipError_t e = hipMemsetAsync(row, 0, (size_t)con_row_len(h) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return ps_fail(PS_ERR_HIP, "%s: clearing the member's row: %s", who, hipGetErrorString(e));
  }
  const double Wn = (double)(h->W + weight);
  const int64_t nitem = h->ncell / 2 + (h->ncell & 1);
  const int bx = (int)std::min<int64_t>((nitem + PS_CON_THREADS - 1) / PS_CON_THREADS, PS_CON_MAX_BLOCKS);
  for (int c0 = 0; c0 < h->nslot; c0 += PS_CON_CHUNK) {
    const int n = std::min(PS_CON_CHUNK, h->nslot - c0);
    ConSlots desc;
    for (int i = 0; i < PS_CON_CHUNK; ++i) {
      const int e = c0 + i;
      desc.s[i] = i < n ? ConSlot{v[0].Y + (int64_t)e * v[0].pitch, v[1].Y + (int64_t)e * v[1].pitch, e}
                        : ConSlot{nullptr, nullptr, 0};
    }
    hipLaunchKernelGGL(k_contrast_add, dim3(bx, n), dim3(PS_CON_THREADS), 0, stream, desc, h->mean, h->m2, h->cnt, row,
                       h->ncell, h->pitch, h->nslot, h->nthr, thr, (double)weight, Wn, weight);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ps_fail(PS_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  }
  PS_TRY(h->prof.end(stream, e1));
  PS_TRY(h->last.mark(stream));
  h->W += weight;
  h->members += 1;
  h->weights.push_back(weight);
  PS_TRY(src.mark(a, stream));   // the next apply of either side overwrites Y only after this read
  return src.mark(b, stream);
}

extern "C" int ps_contrast_add_sites(ps_contrast* h, ps_sites* a, ps_sites* b, uint32_t weight) {
  return con_add_fields(h, a, b, ps_sites_fields(), "contrast_add_sites", weight);
}

extern "C" int ps_contrast_add_project(ps_contrast* h, ps_project* a, ps_project* b, uint32_t weight) {
  return con_add_fields(h, a, b, ps_project_fields(), "contrast_add_project", weight);
}

extern "C" int ps_contrast_merge(ps_contrast* dst, ps_contrast* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "contrast_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->thr != src->thr)
    return ps_fail(PS_ERR_BAD_ARG, "contrast_merge: handles differ in device, domain, slots or thresholds");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "contrast_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(con_reserve_rows(dst, dst->members + src->members));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  if (dst->W == 0) {   // a copy: the merged handle is src bit for bit
    PS_HIP(hipMemcpyAsync(dst->mean, src->mean, con_val_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
    PS_HIP(hipMemcpyAsync(dst->m2, src->m2, con_val_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
    PS_HIP(hipMemcpyAsync(dst->cnt, src->cnt, con_cnt_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
  } else {
    const int64_t nval = (int64_t)dst->nslot * dst->pitch;
    hipLaunchKernelGGL(k_contrast_merge, dim3(2048), dim3(256), 0, dst->stream, dst->mean, dst->m2, dst->cnt, src->mean,
                       src->m2, src->cnt, nval, nval * con_planes(dst), (double)dst->W, (double)src->W);
    PS_HIP(hipGetLastError());
  }
  if (dst->nthr) {
    const int64_t len = con_row_len(dst);
    PS_HIP(hipMemcpyAsync(dst->rows + dst->members * len, src->rows, (size_t)(src->members * len) * sizeof(uint32_t),
                          hipMemcpyDeviceToDevice, dst->stream));
  }
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  dst->weights.insert(dst->weights.end(), src->weights.begin(), src->weights.end());
  return PS_OK;
}

extern "C" int ps_contrast_info(ps_contrast* h, double* total_weight, int64_t* members) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "contrast_info: null handle");
  if (total_weight) *total_weight = (double)h->W;
  if (members) *members = h->members;
  return PS_OK;
}

extern "C" int ps_contrast_fetch_counts(ps_contrast* h, int slot, int which, uint32_t* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "contrast_fetch_counts: bad arguments");
  if (slot < 0 || slot >= h->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "contrast_fetch_counts: slot %d of %d", slot, h->nslot);
  if (which < 0 || which >= con_planes(h))
    return ps_fail(PS_ERR_BAD_ARG, "contrast_fetch_counts: plane %d (0 pos, 1 neg, 2 + 2k gain, 3 + 2k loss; %d planes)",
                   which, con_planes(h));
  if (h->W == 0) return ps_fail(PS_ERR_STATE, "contrast_fetch_counts: nothing accumulated (W = 0)");
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const uint32_t* src = h->cnt + ((int64_t)slot * con_planes(h) + which) * h->pitch;
  PS_HIP(hipMemcpyAsync(out, src, (size_t)h->ncell * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_contrast_fetch(ps_contrast* h, int slot, int what, double* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "contrast_fetch: bad arguments");
  if (slot < 0 || slot >= h->nslot) return ps_fail(PS_ERR_BAD_ARG, "contrast_fetch: slot %d of %d", slot, h->nslot);
  if (what < 0 || what >= 2 + con_planes(h))
    return ps_fail(PS_ERR_BAD_ARG, "contrast_fetch: quantity %d (0 mean, 1 variance, 2 P(d > 0), 3 P(d < 0), 4..%d gain / loss)",
                   what, 1 + con_planes(h));
  if (h->W == 0) return ps_fail(PS_ERR_STATE, "contrast_fetch: nothing accumulated (W = 0)");
  const double W = (double)h->W;
  const size_t n = (size_t)h->ncell;
  if (what >= 2) {
    std::vector<uint32_t> c(n);
    PS_TRY(ps_contrast_fetch_counts(h, slot, what - 2, c.data()));
    for (size_t i = 0; i < n; ++i) out[i] = (double)c[i] / W;
    return PS_OK;
  }
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const double* src = (what == 0 ? h->mean : h->m2) + (int64_t)slot * h->pitch;
  PS_HIP(hipMemcpyAsync(out, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  if (what == 1)
    for (size_t i = 0; i < n; ++i) out[i] /= W;
  return PS_OK;
}

extern "C" int ps_contrast_fetch_coverage(ps_contrast* h, int64_t first, int64_t count, uint32_t* cells,
                                          uint32_t* weights) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "contrast_fetch_coverage: null handle");
  if (first < 0 || count < 0 || first + count > h->members)
    return ps_fail(PS_ERR_BAD_ARG, "contrast_fetch_coverage: members %lld .. %lld of %lld", (long long)first,
                   (long long)(first + count), (long long)h->members);
  if (weights)
    for (int64_t m = 0; m < count; ++m) weights[m] = h->weights[(size_t)(first + m)];
  if (!cells || count == 0 || h->nthr == 0) return PS_OK;
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const int64_t len = con_row_len(h);
  PS_HIP(hipMemcpyAsync(cells, h->rows + first * len, (size_t)(count * len) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                        h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_contrast_prof(ps_contrast* h, int enable, double* total_ms, int64_t* launches) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "contrast_prof: null handle");
  PS_HIP(hipSetDevice(h->device));
  h->prof.set(enable);
  if (total_ms || launches) PS_TRY(h->prof.totals(0, total_ms, launches));
  return PS_OK;
}
