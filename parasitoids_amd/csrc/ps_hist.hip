// Posterior predictive histograms (include/parasitoid_hip.h, ps_hist_*): per day slot and cell the weighted
// counts of many model evaluations on fixed bin edges e_0 < ... < e_B, accumulated on the device from the
// solver's records.  Bin b = searchsorted(edges, v, side='right'): bin 0 holds v < e_0 (zeros included),
// bin b in 1..B holds e_{b-1} <= v < e_b, bin B+1 holds v >= e_B.  Bin 0 is not stored (W - the rest).
// Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   cnt[slot][b - 1][pitch]   uint32, b = 1 .. B+1: bin-major, so neighbouring cells share cache lines
//   rng[slot][pitch]          uint32, the cell's touched bins: (hi << 16) | (0xffff - lo), 0 = none
// Both encodings are maxima, so 0 is the empty state and a merge is a per-half max.  An add reads 8 B of
// record per cell and, only where v >= e_0, 4 B of range and 4 B of the bin's count (read and written);
// the cells outside the plume cost the record read alone.  A quantile or exceedance reads a cell's range and
// only the planes inside it.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"
#include "ps_hist_core.h"   // hist_bin, hist_range_add

#define PS_HIST_MAX_EDGES 1024
#define PS_HIST_CHUNK 32      // slots per launch: 32 descriptors = 1.3 kB of kernel arguments

namespace {

struct HistSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct HistSlots {
  HistSlot s[PS_HIST_CHUNK];
};

// blockIdx.y = slot of the chunk; thread j of the slot owns the pair of cells 2j, 2j + 1 (j == npair: the
// tail cell of an odd N*N alone).  The record is read first; a block with no value >= e_0 returns before
// it stages the edge table in LDS, so the cells outside the plume cost the record read alone.
__global__ void __launch_bounds__(256) k_hist_add(HistSlots desc, const double* __restrict__ edges, int nedge,
                                                  uint32_t* __restrict__ cnt, uint32_t* __restrict__ rng,
                                                  int64_t ncell, int64_t pitch, double negval, uint32_t w) {
  __shared__ double se[PS_HIST_MAX_EDGES];
  const HistSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const int64_t npair = ncell >> 1;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pair = j < npair, tail = j == npair && (ncell & 1);
  double v0 = 0.0, v1 = 0.0;
  if (pair) {
    const double2 r = *reinterpret_cast<const double2*>(sd.rec + 2 * j);
    v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
    v1 = ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval);
  } else if (tail) {
    v0 = ps_record_value(sd.rec[ncell - 1], sd.stat_scale, sd.post_scale, delta, negval);
  }
  const double e0 = edges[0];
  const bool h0 = v0 >= e0, h1 = v1 >= e0;   // v1 stays 0 for the tail cell
  if (!__syncthreads_or(h0 || h1)) return;   // every value of the block in bin 0: nothing is stored
  for (int t = threadIdx.x; t < nedge; t += blockDim.x) se[t] = edges[t];
  __syncthreads();
  if (!(h0 || h1)) return;
  uint32_t* cs = cnt + (int64_t)sd.slot * nedge * pitch;   // plane b - 1 of bin b
  uint32_t* rs = rng + (int64_t)sd.slot * pitch;
  const int b0 = h0 ? hist_bin(se, nedge, v0) : 0;
  const int b1 = h1 ? hist_bin(se, nedge, v1) : 0;
  const int64_t i = 2 * j;
  if (tail) {
    const int64_t c = ncell - 1;
    rs[c] = hist_range_add(rs[c], b0);
    cs[(int64_t)(b0 - 1) * pitch + c] += w;
    return;
  }
  const uint2 rr = *reinterpret_cast<const uint2*>(rs + i);
  const uint2 rn = make_uint2(h0 ? hist_range_add(rr.x, b0) : rr.x, h1 ? hist_range_add(rr.y, b1) : rr.y);
  if (rn.x != rr.x || rn.y != rr.y) *reinterpret_cast<uint2*>(rs + i) = rn;
  if (b0 == b1) {   // both >= 1 here: one 8-byte update
    uint2* p = reinterpret_cast<uint2*>(cs + (int64_t)(b0 - 1) * pitch + i);
    uint2 c = *p;
    c.x += w;
    c.y += w;
    *p = c;
  } else {
    if (h0) cs[(int64_t)(b0 - 1) * pitch + i] += w;
    if (h1) cs[(int64_t)(b1 - 1) * pitch + i + 1] += w;
  }
}

// flat over nslot * pitch words: counts add, ranges take the per-half maximum
__global__ void k_hist_merge(uint32_t* __restrict__ ca, const uint32_t* __restrict__ cb, int64_t ncnt,
                             uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb, int64_t nrng) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ncnt; i += stride) ca[i] += cb[i];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nrng; i += stride) {
    const uint32_t a = ra[i], b = rb[i];
    ra[i] = (max(a >> 16, b >> 16) << 16) | max(a & 0xffffu, b & 0xffffu);
  }
}

// one slot, one thread per cell.  C_b = the weight through bin b (integer, exact); b* = the smallest b with
// (double)C_b >= p W.  Walks down from the cell's highest touched bin, where C = W: C_{b-1} = C_b - count_b,
// so only the planes b* .. hi are read.  Below the lowest touched bin every C equals C_0 = W - sum.
__global__ void k_hist_quantile(const uint32_t* __restrict__ cs, const uint32_t* __restrict__ rs,
                                const double* __restrict__ edges, int nedge, int64_t ncell, int64_t pitch,
                                double p, double W, uint32_t Wi, double* __restrict__ value,
                                int32_t* __restrict__ bstar) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  const double pW = p * W;
  const uint32_t r = rs[i];
  const int hi = (int)(r >> 16), lo = (int)(0xffffu - (r & 0xffffu));
  int b = 0;
  double v = 0.0;
  if (hi >= lo) {   // touched; else all the weight is in bin 0 and b* = 0
    uint32_t C = Wi;   // C_hi
    b = hi;
    uint32_t c = cs[(int64_t)(b - 1) * pitch + i];
    // invariant: (double)C_b >= pW; c = count_b
    while (b > lo && (double)(C - c) >= pW) {
      C -= c;
      --b;
      c = cs[(int64_t)(b - 1) * pitch + i];
    }
    const uint32_t Cm = C - c;   // C_{b-1} (= C_0 at b == lo)
    if (b == lo && (double)Cm >= pW) {
      b = 0;
    } else if (b == nedge) {
      v = edges[nedge - 1];
    } else {
      const double el = edges[b - 1], eh = edges[b];
      const double f = (pW - (double)Cm) / (double)c;
      v = el * pow(eh / el, f);
    }
  }
  value[i] = v;
  bstar[i] = b;
}

// one slot, one thread per cell: sum of count_b over b >= b0 (b0 >= 1), read inside the cell's range only
__global__ void k_hist_tail(const uint32_t* __restrict__ cs, const uint32_t* __restrict__ rs, int b0, int64_t ncell,
                            int64_t pitch, uint32_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  const uint32_t r = rs[i];
  const int hi = (int)(r >> 16), lo = max((int)(0xffffu - (r & 0xffffu)), b0);
  uint32_t s = 0;
  for (int b = lo; b <= hi; ++b) s += cs[(int64_t)(b - 1) * pitch + i];
  out[i] = s;
}

}  // namespace

struct ps_hist {
  int device = 0, N = 0, nslot = 0, nedge = 0;   // nedge = B + 1 edges = stored planes (bins 1 .. B+1)
  std::vector<double> edges;
  int64_t ncell = 0, pitch = 0;
  double* d_edges = nullptr;
  uint32_t* cnt = nullptr;     // [slot][nedge][pitch]
  uint32_t* rng = nullptr;     // [slot][pitch]
  double* qval = nullptr;      // [pitch] quantile / tail scratch
  int32_t* qbin = nullptr;     // [pitch]
  uint64_t W = 0;
  int64_t members = 0;
  hipStream_t stream = nullptr;   // reset / merge / quantile / fetch
  PsLastOp last;                  // the last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds, 1: the quantile calls
};

static size_t hist_cnt_bytes(const ps_hist* a) { return (size_t)a->nslot * a->nedge * a->pitch * sizeof(uint32_t); }
static size_t hist_rng_bytes(const ps_hist* a) { return (size_t)a->nslot * a->pitch * sizeof(uint32_t); }

extern "C" void ps_hist_destroy(ps_hist* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->cnt, (void*)a->rng, (void*)a->qval, (void*)a->qbin, (void*)a->d_edges})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_hist_reset(ps_hist* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "hist_reset: null histogram");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->cnt, 0, hist_cnt_bytes(a), a->stream));
  PS_HIP(hipMemsetAsync(a->rng, 0, hist_rng_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  return PS_OK;
}

extern "C" int ps_hist_create(int device, int N, int nslot, int nedge, const double* edges, ps_hist** out) {
  if (!out || N < 1 || nslot < 1 || nedge < 2 || nedge > PS_HIST_MAX_EDGES || !edges)
    return ps_fail(PS_ERR_BAD_ARG, "hist_create: N %d, %d slots, %d edges (2..%d)", N, nslot, nedge,
                   PS_HIST_MAX_EDGES);
  for (int k = 0; k < nedge; ++k) {
    if (!(edges[k] > 0.0) || !isfinite(edges[k]))
      return ps_fail(PS_ERR_BAD_ARG, "hist_create: edge %d = %g is not finite and > 0", k, edges[k]);
    if (k > 0 && !(edges[k] > edges[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "hist_create: edges not strictly increasing at %d", k);
  }
  *out = nullptr;
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // everything, checked before anything is allocated: counts, ranges, quantile scratch, edges
  const double need = (double)nslot * pitch * (nedge + 1) * 4.0 + (double)pitch * 12.0 + nedge * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "hist_create: %d edges x %d slots x %lld cells x 4 B = %.3g GB, %.3g GB free", nedge,
                   nslot, (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_hist* a = new ps_hist();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nedge = nedge;
  a->edges.assign(edges, edges + nedge);
  a->ncell = ncell;
  a->pitch = pitch;
  auto fail = [&](int rc) {
    ps_hist_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->cnt, hist_cnt_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->rng, hist_rng_bytes(a));
  if (e == hipSuccess) e = hipMalloc((void**)&a->qval, (size_t)pitch * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&a->qbin, (size_t)pitch * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&a->d_edges, (size_t)nedge * sizeof(double));
  if (e == hipSuccess)
    e = hipMemcpyAsync(a->d_edges, a->edges.data(), (size_t)nedge * sizeof(double), hipMemcpyHostToDevice, a->stream);
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "hist_create: %s", hipGetErrorString(e)));
  int rc = ps_hist_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

// one member from the slot descriptors d (one per slot of the histogram), enqueued on `stream`
static int hist_launch(ps_hist* a, const std::vector<PsSrc>& d, hipStream_t stream, double negval,
                       uint32_t weight) {
  const int nslot = a->nslot;
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  const int64_t npair = a->ncell / 2 + 1;   // the pairs and the tail cell's thread
  const int threads = 256;
  const int bx = (int)((npair + threads - 1) / threads);
  for (int c0 = 0; c0 < nslot; c0 += PS_HIST_CHUNK) {
    const int n = std::min(PS_HIST_CHUNK, nslot - c0);
    HistSlots desc;
    for (int i = 0; i < n; ++i) desc.s[i] = ps_slotted<HistSlot>(d[(size_t)(c0 + i)], c0 + i);
    hipLaunchKernelGGL(k_hist_add, dim3(bx, n), dim3(threads), 0, stream, desc, a->d_edges, a->nedge, a->cnt, a->rng,
                       a->ncell, a->pitch, negval, weight);
    PS_HIP(hipGetLastError());
  }
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  return PS_OK;
}

extern "C" int ps_hist_add(ps_hist* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                           const double* stat_scale, const double* post_scale, const int32_t* use_delta, double negval,
                           uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "hist_add: bad arguments");
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "hist_add: %d slots given, the histogram has %d", nslot, a->nslot);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "hist_add: weight must be >= 1");
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "hist_add: total weight %llu would overflow the uint32 counts",
                   (unsigned long long)(a->W + weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("hist_add", "histogram", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale,
                         use_delta, false, d.data(), &stream));
  return hist_launch(a, d, stream, negval, weight);
}

// one member whose values are the current fields of a projection or a release plan (who: the entry point)
static int hist_add_fields(ps_hist* a, void* h, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(a->W + weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  std::vector<PsSrc> d((size_t)a->nslot);
  PS_TRY(ps_read_fields(who, "histogram", "slots", a->device, a->N, a->nslot, h, src, d.data()));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(hist_launch(a, d, a->stream, 0.0, weight));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_hist_add_project(ps_hist* a, ps_project* p, uint32_t weight) {
  return hist_add_fields(a, p, ps_project_fields(), "hist_add_project", weight);
}

extern "C" int ps_hist_add_sites(ps_hist* a, ps_sites* p, uint32_t weight) {
  return hist_add_fields(a, p, ps_sites_fields(), "hist_add_sites", weight);
}

extern "C" int ps_hist_add_peak(ps_hist* a, ps_peak* p, uint32_t weight) {
  return hist_add_fields(a, p, ps_peak_fields(), "hist_add_peak", weight);
}

extern "C" int ps_hist_add_nbhd(ps_hist* a, ps_nbhd* p, uint32_t weight) {
  return hist_add_fields(a, p, ps_nbhd_fields(), "hist_add_nbhd", weight);
}

extern "C" int ps_hist_add_prox(ps_hist* a, ps_prox* p, uint32_t weight) {
  return hist_add_fields(a, p, ps_prox_fields(), "hist_add_prox", weight);
}

extern "C" int ps_hist_merge(ps_hist* dst, ps_hist* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "hist_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->edges != src->edges)
    return ps_fail(PS_ERR_BAD_ARG, "hist_merge: histograms differ in device, domain, slots or edges");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "hist_merge: total weight would overflow");
  if (src->W == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  const int64_t nrng = (int64_t)dst->nslot * dst->pitch;
  hipLaunchKernelGGL(k_hist_merge, dim3(2048), dim3(256), 0, dst->stream, dst->cnt, src->cnt, nrng * dst->nedge,
                     dst->rng, src->rng, nrng);
  PS_HIP(hipGetLastError());
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  return PS_OK;
}

extern "C" int ps_hist_info(ps_hist* a, double* total_weight, int64_t* members, int* nedge) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "hist_info: null histogram");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  if (nedge) *nedge = a->nedge;
  return PS_OK;
}

static int hist_check(ps_hist* a, int slot, const char* who) {
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: slot %d of %d", who, slot, a->nslot);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated (W = 0)", who);
  return PS_OK;
}

// sum of count_b over b >= b0 of one slot into qval (as uint32), on the handle's stream
static int hist_tail(ps_hist* a, int slot, int b0) {
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const int64_t off = (int64_t)slot * a->pitch;
  hipLaunchKernelGGL(k_hist_tail, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream,
                     a->cnt + off * a->nedge, a->rng + off, b0, a->ncell, a->pitch, (uint32_t*)a->qval);
  PS_HIP(hipGetLastError());
  PS_TRY(a->last.mark(a->stream));
  return PS_OK;
}

extern "C" int ps_hist_quantile(ps_hist* a, int slot, double p, double* value, double* lower, double* upper) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "hist_quantile: null histogram");
  if (!(p > 0.0 && p <= 1.0)) return ps_fail(PS_ERR_BAD_ARG, "hist_quantile: p = %g is not in (0, 1]", p);
  PS_TRY(hist_check(a, slot, "hist_quantile"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  const int64_t off = (int64_t)slot * a->pitch;
  hipLaunchKernelGGL(k_hist_quantile, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream,
                     a->cnt + off * a->nedge, a->rng + off, a->d_edges, a->nedge, a->ncell, a->pitch, p, (double)a->W,
                     (uint32_t)a->W, a->qval, a->qbin);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  const size_t n = (size_t)a->ncell;
  if (value) PS_HIP(hipMemcpyAsync(value, a->qval, n * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  std::vector<int32_t> b;
  if (lower || upper) {
    b.resize(n);
    PS_HIP(hipMemcpyAsync(b.data(), a->qbin, n * sizeof(int32_t), hipMemcpyDeviceToHost, a->stream));
  }
  PS_HIP(hipStreamSynchronize(a->stream));
  const int B1 = a->nedge;   // B + 1
  const double* e = a->edges.data();
  for (size_t i = 0; i < b.size(); ++i) {
    const int k = b[i];
    if (lower) lower[i] = k == 0 ? 0.0 : e[k - 1];
    if (upper) upper[i] = k == B1 ? INFINITY : e[k];
  }
  return PS_OK;
}

extern "C" int ps_hist_exceed(ps_hist* a, int slot, int k, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "hist_exceed: bad arguments");
  if (k < 0 || k >= a->nedge) return ps_fail(PS_ERR_BAD_ARG, "hist_exceed: edge %d of %d", k, a->nedge);
  PS_TRY(hist_check(a, slot, "hist_exceed"));
  PS_TRY(hist_tail(a, slot, k + 1));   // v >= e_k  <=>  bin >= k + 1
  const size_t n = (size_t)a->ncell;
  std::vector<uint32_t> c(n);
  PS_HIP(hipMemcpyAsync(c.data(), a->qval, n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  const double W = (double)a->W;
  for (size_t i = 0; i < n; ++i) out[i] = (double)c[i] / W;
  return PS_OK;
}

extern "C" int ps_hist_fetch_counts(ps_hist* a, int slot, int b, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "hist_fetch_counts: bad arguments");
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "hist_fetch_counts: slot %d of %d", slot, a->nslot);
  if (b < 0 || b > a->nedge) return ps_fail(PS_ERR_BAD_ARG, "hist_fetch_counts: bin %d of 0..%d", b, a->nedge);
  const size_t n = (size_t)a->ncell;
  if (b == 0) {   // W - the stored bins
    PS_TRY(hist_tail(a, slot, 1));
    PS_HIP(hipMemcpyAsync(out, a->qval, n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
    PS_HIP(hipStreamSynchronize(a->stream));
    const uint32_t W = (uint32_t)a->W;
    for (size_t i = 0; i < n; ++i) out[i] = W - out[i];
    return PS_OK;
  }
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const uint32_t* src = a->cnt + ((int64_t)slot * a->nedge + (b - 1)) * a->pitch;
  PS_HIP(hipMemcpyAsync(out, src, n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_hist_prof(ps_hist* a, int enable, double* add_ms, int64_t* add_launches, double* q_ms,
                            int64_t* q_launches) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "hist_prof: null histogram");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  double* ms_out[2] = {add_ms, q_ms};
  int64_t* n_out[2] = {add_launches, q_launches};
  for (int k = 0; k < 2; ++k)
    if (ms_out[k] || n_out[k]) PS_TRY(a->prof.totals(k, ms_out[k], n_out[k]));
  return PS_OK;
}
