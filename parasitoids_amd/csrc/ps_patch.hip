// Patch maps (include/parasitoid_hip.h, ps_patch_*): per threshold t_k and slot the connected components
// ("patches") of each member's set O = {v >= t_k} under 4- or 8-connectivity, the weighted count of the members whose
// main patch -- the one with the most cells, among equals the smallest label -- holds the cell, the same for the
// cells of O outside the main patch, and per member the number of patches, the cells of O, of the main patch and of
// the largest other patch, and the main patch's label, its smallest linear index.  The value of a slot is the one
// ps_summary_add adds (ps_record_value).  Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   cnt[which][k][slot][pitch]    uint32, which 0: main, 1: satellite
//   rows[member][k][slot][5]      uint32: npatch, cells, main_cells, main_label, sat_cells_max (grow by doubling)
//   parent[k][slot][pitch]        uint32 scratch, size[k][slot][pitch] uint32 scratch, key[k][slot] uint64 scratch
// All K * nslot planes of a member are in flight at once (plane on grid.y), so the scratch is 8 B per cell and
// plane -- as much again as the counts.  One add: two small memsets (the member's rows, the keys) and six launches,
//   k_patch_init     parent = c in O, PATCH_NONE outside; size = 0
//   k_patch_link     every cell of O joined to its neighbours before it (ps_patch_core.h): compare-and-swap on roots
//   k_patch_flatten  parent = root, the patch's smallest index
//   k_patch_sizes    size[root] += 1 aggregated per wave; npatch and cells by ballots, one atomic per block
//   k_patch_pick     key = max over the roots of (size << 32 | ~label), one 64-bit atomic per wave
//   k_patch_count    one writer per cell: main or sat += w; the largest size among the other roots; the row
// Integer atomics only and a canonical label: neither the order of adds, nor that of merges, nor the grid, nor the
// order in which the device joins cells changes a bit.
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"
#include "ps_patch_core.h"

#define PS_PAT_MAX_SLOT 32   // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_PAT_MAX_THR 4
#define PS_PAT_THREADS 256
#define PS_PAT_ROWS0 64      // member rows allocated at create
#define PS_PAT_ROW 5         // words of one row

namespace {

struct PatSlots {
  PsSrc s[PS_PAT_MAX_SLOT];
};
struct PatThr {
  double t[PS_PAT_MAX_THR];
};

// parent entries as the link kernel touches them: other workgroups, on other XCDs, change them during the launch,
// so every read is a device-scope atomic load (a plain load may be served stale from this XCD's L2 or this CU's L1)
struct PatLinkOps {
  uint32_t* parent;
  __device__ uint32_t load(uint32_t i) const {
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ uint32_t cas(uint32_t i, uint32_t expect, uint32_t desired) const {
    return atomicCAS(parent + i, expect, desired);
  }
  __device__ bool step() const { return true; }
};
// after the link launch the trees stand still but for the flatten's own writes, each of which puts an ancestor in
// place of an ancestor: plain loads, and find alone
struct PatPlainOps {
  const uint32_t* parent;
  __device__ uint32_t load(uint32_t i) const { return parent[i]; }
  __device__ bool step() const { return true; }
};

// plane p = k * nslot + slot on grid.y, one cell per thread
__global__ void __launch_bounds__(PS_PAT_THREADS) k_patch_init(PatSlots desc, PatThr thr, int nslot,
                                                               uint32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                               uint32_t ncell, int64_t pitch, double negval) {
  const uint32_t c = blockIdx.x * (uint32_t)PS_PAT_THREADS + threadIdx.x;
  if (c >= ncell) return;
  const int p = blockIdx.y, k = p / nslot, s = p - k * nslot;
  const PsSrc& sd = desc.s[s];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double v = ps_record_value(sd.rec[c], sd.stat_scale, sd.post_scale, delta, negval);
  parent[p * pitch + c] = v >= thr.t[k] ? c : PATCH_NONE;
  size[p * pitch + c] = 0;
}

__global__ void __launch_bounds__(PS_PAT_THREADS) k_patch_link(uint32_t* __restrict__ parent, uint32_t ncell,
                                                               int64_t pitch, uint32_t N, int conn) {
  const uint32_t c = blockIdx.x * (uint32_t)PS_PAT_THREADS + threadIdx.x;
  if (c >= ncell) return;
  PatLinkOps at{parent + blockIdx.y * pitch};
  if (at.load(c) == PATCH_NONE) return;
  patch_link_cell(at, c, N, conn);
}

__global__ void __launch_bounds__(PS_PAT_THREADS) k_patch_flatten(uint32_t* __restrict__ parent, uint32_t ncell,
                                                                  int64_t pitch) {
  const uint32_t c = blockIdx.x * (uint32_t)PS_PAT_THREADS + threadIdx.x;
  if (c >= ncell) return;
  uint32_t* pp = parent + blockIdx.y * pitch;
  if (pp[c] == PATCH_NONE) return;
  PatPlainOps at{pp};
  pp[c] = patch_find(at, c);
}

// size[root] += the cells of the wave under that root: the lanes of a wave usually share one root, and a patch of
// 50 000 cells would otherwise send as many atomics to one address.  Every loop pass retires at least its leading
// lane, and `todo` comes from ballots, so the loop is wave-uniform and ends within 64 passes.
__global__ void __launch_bounds__(PS_PAT_THREADS) k_patch_sizes(const uint32_t* __restrict__ parent,
                                                                uint32_t* __restrict__ size, uint32_t* __restrict__ rows,
                                                                uint32_t ncell, int64_t pitch) {
  __shared__ uint32_t tot[2];
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  __syncthreads();
  const int p = blockIdx.y, lane = threadIdx.x & 63;
  const uint32_t c = blockIdx.x * (uint32_t)PS_PAT_THREADS + threadIdx.x;
  const uint32_t root = c < ncell ? parent[p * pitch + c] : PATCH_NONE;
  const bool occ = root != PATCH_NONE;
  uint64_t todo = __ballot(occ);
  const uint32_t ncells = (uint32_t)__popcll(todo), nroots = (uint32_t)__popcll(__ballot(occ && root == c));
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const uint32_t r = (uint32_t)__shfl((int)root, lead);
    const uint64_t same = __ballot(occ && root == r);
    if (lane == lead) atomicAdd(&size[p * pitch + r], (uint32_t)__popcll(same));
    todo &= ~same;
  }
  if (lane == 0 && ncells) {
    atomicAdd(&tot[0], nroots);
    atomicAdd(&tot[1], ncells);
  }
  __syncthreads();
  if (threadIdx.x < 2 && tot[threadIdx.x]) atomicAdd(&rows[p * PS_PAT_ROW + threadIdx.x], tot[threadIdx.x]);
}

// key[p] = max over the roots of patch_key(size, label): the wave's maximum by shuffles, one atomic per wave
__global__ void __launch_bounds__(PS_PAT_THREADS) k_patch_pick(const uint32_t* __restrict__ parent,
                                                               const uint32_t* __restrict__ size,
                                                               unsigned long long* __restrict__ key, uint32_t ncell,
                                                               int64_t pitch) {
  const int p = blockIdx.y;
  const uint32_t c = blockIdx.x * (uint32_t)PS_PAT_THREADS + threadIdx.x;
  uint64_t mine = 0;
  if (c < ncell && parent[p * pitch + c] == c) mine = patch_key(size[p * pitch + c], c);
  if (!__any(mine != 0)) return;
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(mine, off);
    mine = o > mine ? o : mine;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(&key[p], (unsigned long long)mine);
}

// one writer per cell: main += w in the main patch, sat += w in the rest of O; the largest size among the roots
// other than the main one (the wave's maximum, one integer atomic per wave); block 0 writes the main patch's row
// words from the key
__global__ void __launch_bounds__(PS_PAT_THREADS) k_patch_count(const uint32_t* __restrict__ parent,
                                                                const uint32_t* __restrict__ size,
                                                                const unsigned long long* __restrict__ key,
                                                                uint32_t* __restrict__ cnt_main, uint32_t* __restrict__ cnt_sat,
                                                                uint32_t* __restrict__ rows, uint32_t ncell, int64_t pitch,
                                                                uint32_t w) {
  const int p = blockIdx.y;
  const uint64_t kmain = key[p];
  const uint32_t main_label = patch_key_label(kmain);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rows[p * PS_PAT_ROW + 2] = patch_key_cells(kmain);
    rows[p * PS_PAT_ROW + 3] = main_label;
  }
  const uint32_t c = blockIdx.x * (uint32_t)PS_PAT_THREADS + threadIdx.x;
  const uint32_t root = c < ncell ? parent[p * pitch + c] : PATCH_NONE;
  uint32_t other = 0;
  if (root != PATCH_NONE) {
    if (root == main_label) {
      cnt_main[p * pitch + c] += w;
    } else {
      cnt_sat[p * pitch + c] += w;
      if (root == c) other = size[p * pitch + c];
    }
  }
  if (!__any(other != 0)) return;
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)other, off);
    other = o > other ? o : other;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(&rows[p * PS_PAT_ROW + 4], other);
}

// flat over 2 * nthr * nslot * pitch words
__global__ void k_patch_merge(uint32_t* __restrict__ ca, const uint32_t* __restrict__ cb, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) ca[i] += cb[i];
}

__global__ void k_patch_prob(const uint32_t* __restrict__ c, int64_t ncell, double W, double* __restrict__ prob) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < ncell) prob[i] = (double)c[i] / W;
}

}  // namespace

struct ps_patch {
  int device = 0, N = 0, nslot = 0, nthr = 0, conn = 4;
  std::vector<double> thr;
  int64_t ncell = 0, pitch = 0;
  uint32_t* cnt = nullptr;      // [which][k][slot][pitch]
  uint32_t* parent = nullptr;   // [k][slot][pitch] scratch of the member being added
  uint32_t* size = nullptr;     // [k][slot][pitch] scratch
  unsigned long long* key = nullptr;   // [k][slot] scratch
  uint32_t* rows = nullptr;     // [rows_cap][k][slot][5]
  int64_t rows_cap = 0;
  double* map = nullptr;        // [pitch] map scratch
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;   // per member, in row order
  hipStream_t stream = nullptr;    // reset / merge / maps / fetch / row growth
  PsLastOp last;                   // the last operation, on whatever stream it ran
  PsProf prof;                     // channel 0: the adds, 1: the maps
};

static int64_t pat_planes(const ps_patch* a) { return (int64_t)a->nthr * a->nslot; }
static size_t pat_plane_bytes(const ps_patch* a) { return (size_t)pat_planes(a) * a->pitch * sizeof(uint32_t); }
static size_t pat_cnt_bytes(const ps_patch* a) { return 2 * pat_plane_bytes(a); }
static size_t pat_member_bytes(const ps_patch* a) { return (size_t)pat_planes(a) * PS_PAT_ROW * sizeof(uint32_t); }

// hipMalloc behind a check against the free device memory: PS_ERR_OOM before anything is allocated
static int pat_alloc(void** p, size_t bytes, const char* what) {
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b)
    return ps_fail(PS_ERR_OOM, "patch: %s needs %.3g GB, %.3g GB free", what, (double)bytes * 1e-9, (double)free_b * 1e-9);
  PS_HIP(hipMalloc(p, bytes));
  return PS_OK;
}

// room for `need` member rows: a doubling copies the rows so far on the handle's stream and synchronises once
// before the old block is freed
static int pat_reserve_rows(ps_patch* a, int64_t need) {
  if (need <= a->rows_cap) return PS_OK;
  int64_t cap = std::max<int64_t>(a->rows_cap, PS_PAT_ROWS0);
  while (cap < need) cap *= 2;
  const size_t row_b = pat_member_bytes(a);
  void* p = nullptr;
  PS_TRY(pat_alloc(&p, (size_t)cap * row_b, "the member rows"));
  if (a->rows_cap > 0) {
    hipError_t e = hipSuccess;
    if (a->last.live) e = hipStreamWaitEvent(a->stream, a->last.ev, 0);
    if (e == hipSuccess && a->members > 0)
      e = hipMemcpyAsync(p, a->rows, (size_t)a->members * row_b, hipMemcpyDeviceToDevice, a->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return ps_fail(PS_ERR_HIP, "patch: growing the member rows: %s", hipGetErrorString(e));
    }
    PS_HIP(hipFree(a->rows));
  }
  a->rows = (uint32_t*)p;
  a->rows_cap = cap;
  return PS_OK;
}

extern "C" void ps_patch_destroy(ps_patch* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->cnt, (void*)a->parent, (void*)a->size, (void*)a->key, (void*)a->rows, (void*)a->map})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_patch_reset(ps_patch* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "patch_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->cnt, 0, pat_cnt_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  a->weights.clear();
  if (!a->prof.idle()) PS_HIP(hipStreamSynchronize(a->stream));
  a->prof.release();   // the timings so far go with the members
  return PS_OK;
}

extern "C" int ps_patch_create(int device, int N, int nslot, int nthr, const double* thr, int connectivity,
                               ps_patch** out) {
  if (!out || N < 1 || nslot < 1 || nslot > PS_PAT_MAX_SLOT || nthr < 1 || nthr > PS_PAT_MAX_THR || !thr)
    return ps_fail(PS_ERR_BAD_ARG, "patch_create: N %d, %d slots (1..%d), %d thresholds (1..%d)", N, nslot,
                   PS_PAT_MAX_SLOT, nthr, PS_PAT_MAX_THR);
  *out = nullptr;
  if (connectivity != 4 && connectivity != 8)
    return ps_fail(PS_ERR_BAD_ARG, "patch_create: connectivity %d is neither 4 nor 8", connectivity);
  for (int k = 0; k < nthr; ++k) {
    if (!(thr[k] > 0.0) || !isfinite(thr[k]))
      return ps_fail(PS_ERR_BAD_ARG, "patch_create: threshold %d = %g is not finite and > 0", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "patch_create: thresholds not strictly increasing at %d", k);
  }
  const int64_t ncell = (int64_t)N * N;
  if (ncell >= (1ll << 25))
    return ps_fail(PS_ERR_BAD_ARG, "patch_create: N %d: the labels and cell counts need N * N < 2^25", N);
  PS_TRY(ps_use_device(device));
  ps_patch* a = new ps_patch();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nthr = nthr;
  a->conn = connectivity;
  a->thr.assign(thr, thr + nthr);
  a->ncell = ncell;
  a->pitch = (ncell + 63) / 64 * 64;
  auto fail = [&](int rc) {
    ps_patch_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e != hipSuccess) return fail(ps_fail(PS_ERR_HIP, "patch_create: %s", hipGetErrorString(e)));
  int rc = pat_alloc((void**)&a->cnt, pat_cnt_bytes(a), "the count planes");
  if (rc == PS_OK) rc = pat_alloc((void**)&a->parent, pat_plane_bytes(a), "the parent scratch");
  if (rc == PS_OK) rc = pat_alloc((void**)&a->size, pat_plane_bytes(a), "the size scratch");
  if (rc == PS_OK) rc = pat_alloc((void**)&a->key, (size_t)pat_planes(a) * sizeof(unsigned long long), "the key scratch");
  if (rc == PS_OK) rc = pat_alloc((void**)&a->map, (size_t)a->pitch * sizeof(double), "the map scratch");
  if (rc == PS_OK) rc = pat_reserve_rows(a, PS_PAT_ROWS0);
  if (rc == PS_OK) rc = ps_patch_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

extern "C" int ps_patch_reserve(ps_patch* a, int64_t members) {
  if (!a || members < 0) return ps_fail(PS_ERR_BAD_ARG, "patch_reserve: bad arguments");
  PS_HIP(hipSetDevice(a->device));
  return pat_reserve_rows(a, members);
}

// one member from the slot descriptors (one per slot of the handle, the rest null), enqueued on `stream`
static int pat_launch(ps_patch* a, const PatSlots& desc, hipStream_t stream, double negval, uint32_t weight) {
  PS_TRY(pat_reserve_rows(a, a->members + 1));
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  const int64_t np = pat_planes(a);
  uint32_t* rows = a->rows + a->members * np * PS_PAT_ROW;
  PatThr thr;
  for (int k = 0; k < PS_PAT_MAX_THR; ++k) thr.t[k] = k < a->nthr ? a->thr[(size_t)k] : 0.0;
  const uint32_t ncell = (uint32_t)a->ncell;
  const dim3 grid((unsigned)((a->ncell + PS_PAT_THREADS - 1) / PS_PAT_THREADS), (unsigned)np), block(PS_PAT_THREADS);
  uint32_t* cnt_sat = a->cnt + np * a->pitch;
  PS_HIP(hipMemsetAsync(rows, 0, pat_member_bytes(a), stream));
  PS_HIP(hipMemsetAsync(a->key, 0, (size_t)np * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_patch_init, grid, block, 0, stream, desc, thr, a->nslot, a->parent, a->size, ncell, a->pitch,
                     negval);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_patch_link, grid, block, 0, stream, a->parent, ncell, a->pitch, (uint32_t)a->N, a->conn);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_patch_flatten, grid, block, 0, stream, a->parent, ncell, a->pitch);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_patch_sizes, grid, block, 0, stream, a->parent, a->size, rows, ncell, a->pitch);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_patch_pick, grid, block, 0, stream, a->parent, a->size, a->key, ncell, a->pitch);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_patch_count, grid, block, 0, stream, a->parent, a->size, a->key, a->cnt, cnt_sat, rows, ncell,
                     a->pitch, weight);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  a->weights.push_back(weight);
  return PS_OK;
}

extern "C" int ps_patch_add(ps_patch* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                            const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                            double negval, uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "patch_add: bad arguments");
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "patch_add: %d slots given, the handle has %d", nslot, a->nslot);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "patch_add: weight must be >= 1");
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "patch_add: total weight %llu would overflow the uint32 counts",
                   (unsigned long long)(a->W + weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  PatSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("patch_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nslot; i < PS_PAT_MAX_SLOT; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return pat_launch(a, desc, stream, negval, weight);
}

// one member whose slots are the current fields of a projection or a release plan, in ascending output order
// (who: the entry point)
static int pat_add_fields(ps_patch* a, void* h, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(a->W + weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  PatSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, desc.s));
  for (int e = a->nslot; e < PS_PAT_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(pat_launch(a, desc, a->stream, 0.0, weight));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_patch_add_project(ps_patch* a, ps_project* p, uint32_t weight) {
  return pat_add_fields(a, p, ps_project_fields(), "patch_add_project", weight);
}

extern "C" int ps_patch_add_sites(ps_patch* a, ps_sites* p, uint32_t weight) {
  return pat_add_fields(a, p, ps_sites_fields(), "patch_add_sites", weight);
}

extern "C" int ps_patch_merge(ps_patch* dst, ps_patch* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "patch_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->thr != src->thr ||
      dst->conn != src->conn)
    return ps_fail(PS_ERR_BAD_ARG, "patch_merge: handles differ in device, domain, slots, thresholds or connectivity");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "patch_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(pat_reserve_rows(dst, dst->members + src->members));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  hipLaunchKernelGGL(k_patch_merge, dim3(2048), dim3(256), 0, dst->stream, dst->cnt, src->cnt,
                     2 * pat_planes(dst) * dst->pitch);
  PS_HIP(hipGetLastError());
  const size_t row_b = pat_member_bytes(dst);
  PS_HIP(hipMemcpyAsync(dst->rows + dst->members * pat_planes(dst) * PS_PAT_ROW, src->rows, (size_t)src->members * row_b,
                        hipMemcpyDeviceToDevice, dst->stream));
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  dst->weights.insert(dst->weights.end(), src->weights.begin(), src->weights.end());
  return PS_OK;
}

extern "C" int ps_patch_info(ps_patch* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "patch_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  if (capacity) *capacity = a->rows_cap;
  if (bytes)
    *bytes = (int64_t)(pat_cnt_bytes(a) + 2 * pat_plane_bytes(a) + (size_t)pat_planes(a) * sizeof(unsigned long long) +
                       (size_t)a->pitch * sizeof(double) + (size_t)a->rows_cap * pat_member_bytes(a));
  return PS_OK;
}

static int pat_check(ps_patch* a, int k, int slot, const char* who) {
  if (k < 0 || k >= a->nthr) return ps_fail(PS_ERR_BAD_ARG, "%s: threshold %d of %d", who, k, a->nthr);
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: slot %d of %d", who, slot, a->nslot);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated (W = 0)", who);
  return PS_OK;
}
static int pat_check_which(int which, const char* who) {
  if (which != 0 && which != 1) return ps_fail(PS_ERR_BAD_ARG, "%s: which %d is neither 0 (main) nor 1 (satellite)", who, which);
  return PS_OK;
}
static const uint32_t* pat_plane(const ps_patch* a, int k, int slot, int which) {
  return a->cnt + (((int64_t)which * a->nthr + k) * a->nslot + slot) * a->pitch;
}

extern "C" int ps_patch_prob(ps_patch* a, int k, int slot, int which, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "patch_prob: bad arguments");
  PS_TRY(pat_check_which(which, "patch_prob"));
  PS_TRY(pat_check(a, k, slot, "patch_prob"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  hipLaunchKernelGGL(k_patch_prob, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream,
                     pat_plane(a, k, slot, which), a->ncell, (double)a->W, a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->map, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_patch_fetch_counts(ps_patch* a, int k, int slot, int which, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "patch_fetch_counts: bad arguments");
  PS_TRY(pat_check_which(which, "patch_fetch_counts"));
  PS_TRY(pat_check(a, k, slot, "patch_fetch_counts"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(out, pat_plane(a, k, slot, which), (size_t)a->ncell * sizeof(uint32_t), hipMemcpyDeviceToHost,
                        a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_patch_fetch_members(ps_patch* a, int k, int slot, uint32_t* npatch, uint32_t* cells,
                                      uint32_t* main_cells, uint32_t* main_label, uint32_t* sat_cells_max,
                                      uint32_t* weights) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "patch_fetch_members: null handle");
  PS_TRY(pat_check(a, k, slot, "patch_fetch_members"));
  const int64_t m = a->members, np = pat_planes(a), at = (int64_t)k * a->nslot + slot;
  if (weights)
    for (int64_t r = 0; r < m; ++r) weights[r] = a->weights[(size_t)r];
  uint32_t* outs[PS_PAT_ROW] = {npatch, cells, main_cells, main_label, sat_cells_max};
  if (!npatch && !cells && !main_cells && !main_label && !sat_cells_max) return PS_OK;
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  std::vector<uint32_t> h((size_t)(m * np * PS_PAT_ROW));
  PS_HIP(hipMemcpyAsync(h.data(), a->rows, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  for (int64_t r = 0; r < m; ++r)
    for (int f = 0; f < PS_PAT_ROW; ++f)
      if (outs[f]) outs[f][r] = h[(size_t)((r * np + at) * PS_PAT_ROW + f)];
  return PS_OK;
}

extern "C" int ps_patch_prof(ps_patch* a, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "patch_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  double* ms_out[2] = {add_ms, map_ms};
  int64_t* n_out[2] = {adds, maps};
  for (int k = 0; k < 2; ++k)
    if (ms_out[k] || n_out[k]) PS_TRY(a->prof.totals(k, ms_out[k], n_out[k]));
  return PS_OK;
}
