// Pathway maps (include/parasitoid_hip.h, ps_pathway_*): was a cell reached by the advancing front, by a jump, or
// by the growth of a focus a jump founded?  Per member and threshold t_k the slots are taken in ascending order;
// the patches of O_s = {v_s >= t_k} are those of ps_patch.hip (ps_patch_core.h, unchanged), and every cell carries
// a state -- 0 unreached, 1 front, 2 jump, 3 secondary -- that is set once, in the first slot whose set holds the
// cell, from what the cell's patch held before that slot (ps_pathway_core.h).  The value of a slot is the one
// ps_summary_add adds (ps_record_value).  Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   cnt[k][class][pitch]          uint32, class 0: front, 1: jump, 2: secondary
//   rows[member][k][slot][4]      uint32: the cells newly classed front, jump, secondary; the foci founded
//   parent[k][slot][pitch]        uint32 scratch, flags[k][slot][pitch] uint32 scratch, state[k][pitch] uint8 scratch
// The labelling of a slot does not depend on time: init, link and flatten run once per add over all K * nslot planes
// (plane on grid.y).  Only the classification is sequential, two launches per slot over the K thresholds:
//   k_pathway_init     parent = c in O, PATCH_NONE outside; flags = 0
//   k_pathway_link     every cell of O joined to its neighbours before it: compare-and-swap on roots
//   k_pathway_flatten  parent = root, the patch's smallest index
//   per slot s:
//     k_pathway_flag   flags[root] |= the bits of the cells of O_s whose state is set, and of the anchors in O_s,
//                      aggregated per wave
//     k_pathway_class  one writer per cell: a cell of O_s in state 0 takes its class from flags[root]; the three
//                      classes and the founded roots by ballots, one integer atomic per block and word
//   k_pathway_count    cnt[k][state - 1] += w where the state is set
// Nothing a launch writes is read in that launch, but for the link kernel's own atomics.  Integer atomics only and
// a canonical label: neither the order of adds, nor that of merges, nor the grid, nor the order in which the device
// joins cells changes a bit.
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"
#include "ps_patch_core.h"
#include "ps_pathway_core.h"

#define PS_PW_MAX_SLOT 32   // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_PW_MAX_THR 4
#define PS_PW_MAX_ANCHOR 32
#define PS_PW_THREADS 256
#define PS_PW_ROWS0 64      // member rows allocated at create
#define PS_PW_ROW 4         // words of one row
#define PS_PW_CLASSES 3

namespace {

struct PwSlots {
  PsSrc s[PS_PW_MAX_SLOT];
};
struct PwThr {
  double t[PS_PW_MAX_THR];
};
struct PwAnchors {
  uint32_t c[PS_PW_MAX_ANCHOR];
};

// parent entries as the link kernel touches them (as ps_patch.hip): other workgroups, on other XCDs, change them
// during the launch, so every read is a device-scope atomic load
struct PwLinkOps {
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
struct PwPlainOps {
  const uint32_t* parent;
  __device__ uint32_t load(uint32_t i) const { return parent[i]; }
  __device__ bool step() const { return true; }
};

// plane p = k * nslot + slot on grid.y, one cell per thread
__global__ void __launch_bounds__(PS_PW_THREADS) k_pathway_init(PwSlots desc, PwThr thr, int nslot,
                                                                uint32_t* __restrict__ parent,
                                                                uint32_t* __restrict__ flags, uint32_t ncell,
                                                                int64_t pitch, double negval) {
  const uint32_t c = blockIdx.x * (uint32_t)PS_PW_THREADS + threadIdx.x;
  if (c >= ncell) return;
  const int p = blockIdx.y, k = p / nslot, s = p - k * nslot;
  const PsSrc& sd = desc.s[s];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double v = ps_record_value(sd.rec[c], sd.stat_scale, sd.post_scale, delta, negval);
  parent[p * pitch + c] = v >= thr.t[k] ? c : PATCH_NONE;
  flags[p * pitch + c] = 0;
}

__global__ void __launch_bounds__(PS_PW_THREADS) k_pathway_link(uint32_t* __restrict__ parent, uint32_t ncell,
                                                                int64_t pitch, uint32_t N, int conn) {
  const uint32_t c = blockIdx.x * (uint32_t)PS_PW_THREADS + threadIdx.x;
  if (c >= ncell) return;
  PwLinkOps at{parent + blockIdx.y * pitch};
  if (at.load(c) == PATCH_NONE) return;
  patch_link_cell(at, c, N, conn);
}

__global__ void __launch_bounds__(PS_PW_THREADS) k_pathway_flatten(uint32_t* __restrict__ parent, uint32_t ncell,
                                                                   int64_t pitch) {
  const uint32_t c = blockIdx.x * (uint32_t)PS_PW_THREADS + threadIdx.x;
  if (c >= ncell) return;
  uint32_t* pp = parent + blockIdx.y * pitch;
  if (pp[c] == PATCH_NONE) return;
  PwPlainOps at{pp};
  pp[c] = patch_find(at, c);
}

// Threshold k on grid.y, the plane of slot s.  flags[root] |= the bits of the wave's cells under that root: the lanes
// of a wave usually share one root, and a front of 50 000 cells would otherwise send as many atomics to one address.
// Every loop pass retires at least its leading lane, and `todo` comes from ballots, so the loop is wave-uniform and
// ends within 64 passes.  The anchors are few: the first threads of block 0 take one each.
__global__ void __launch_bounds__(PS_PW_THREADS) k_pathway_flag(const uint32_t* __restrict__ parent,
                                                                const uint8_t* __restrict__ state,
                                                                uint32_t* __restrict__ flags, PwAnchors anchors,
                                                                int nanchor, int nslot, int slot, uint32_t ncell,
                                                                int64_t pitch) {
  const int k = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)k * nslot + slot) * pitch;
  const uint32_t c = blockIdx.x * (uint32_t)PS_PW_THREADS + threadIdx.x;
  const uint32_t root = c < ncell ? parent[base + c] : PATCH_NONE;
  const uint32_t bits = root != PATCH_NONE ? pathway_flag_bits(state[k * pitch + c]) : 0u;
  uint64_t todo = __ballot(bits != 0u);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const uint32_t r = (uint32_t)__shfl((int)root, lead);
    const uint64_t same = __ballot(bits != 0u && root == r);
    const bool origin = __ballot((bits & PATHWAY_ORIGIN) && root == r) != 0;   // seeded holds for every lane of `same`
    if (lane == lead) atomicOr(&flags[base + r], PATHWAY_SEEDED | (origin ? PATHWAY_ORIGIN : 0u));
    todo &= ~same;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < nanchor) {
    const uint32_t r = parent[base + anchors.c[threadIdx.x]];
    if (r != PATCH_NONE) atomicOr(&flags[base + r], PATHWAY_ORIGIN);
  }
}

// one writer per cell: a cell of O_s still in state 0 reads its root's flags and takes its class; the block's three
// class counts and its founded roots by ballots, one integer atomic per block and word into the member's row
__global__ void __launch_bounds__(PS_PW_THREADS) k_pathway_class(const uint32_t* __restrict__ parent,
                                                                 const uint32_t* __restrict__ flags,
                                                                 uint8_t* __restrict__ state, uint32_t* __restrict__ rows,
                                                                 int nslot, int slot, uint32_t ncell, int64_t pitch) {
  __shared__ uint32_t tot[PS_PW_ROW];
  if (threadIdx.x < PS_PW_ROW) tot[threadIdx.x] = 0;
  __syncthreads();
  const int k = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t base = ((int64_t)k * nslot + slot) * pitch;
  const uint32_t c = blockIdx.x * (uint32_t)PS_PW_THREADS + threadIdx.x;
  const uint32_t root = c < ncell ? parent[base + c] : PATCH_NONE;
  uint32_t cls = PATHWAY_UNREACHED;
  bool founds = false;
  if (root != PATCH_NONE && state[k * pitch + c] == PATHWAY_UNREACHED) {
    const uint32_t f = flags[base + root];
    cls = pathway_class(f);
    founds = pathway_founds(c, root, f);
    state[k * pitch + c] = (uint8_t)cls;
  }
  const uint64_t any = __ballot(cls != PATHWAY_UNREACHED);
  if (any) {
    const uint32_t n1 = (uint32_t)__popcll(__ballot(cls == PATHWAY_FRONT));
    const uint32_t n2 = (uint32_t)__popcll(__ballot(cls == PATHWAY_JUMP));
    const uint32_t n3 = (uint32_t)__popcll(__ballot(cls == PATHWAY_SECONDARY));
    const uint32_t nf = (uint32_t)__popcll(__ballot(founds));
    if (lane == 0) {
      if (n1) atomicAdd(&tot[0], n1);
      if (n2) atomicAdd(&tot[1], n2);
      if (n3) atomicAdd(&tot[2], n3);
      if (nf) atomicAdd(&tot[3], nf);
    }
  }
  __syncthreads();
  if (threadIdx.x < PS_PW_ROW && tot[threadIdx.x])
    atomicAdd(&rows[((int64_t)k * nslot + slot) * PS_PW_ROW + threadIdx.x], tot[threadIdx.x]);
}

// after the last slot: cnt[k][state - 1] += w, one writer per cell
__global__ void __launch_bounds__(PS_PW_THREADS) k_pathway_count(const uint8_t* __restrict__ state,
                                                                 uint32_t* __restrict__ cnt, uint32_t ncell,
                                                                 int64_t pitch, uint32_t w) {
  const uint32_t c = blockIdx.x * (uint32_t)PS_PW_THREADS + threadIdx.x;
  if (c >= ncell) return;
  const int k = blockIdx.y;
  const uint32_t st = state[k * pitch + c];
  if (st != PATHWAY_UNREACHED) cnt[((int64_t)k * PS_PW_CLASSES + (st - 1)) * pitch + c] += w;
}

// flat over nthr * 3 * pitch words
__global__ void k_pathway_merge(uint32_t* __restrict__ ca, const uint32_t* __restrict__ cb, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) ca[i] += cb[i];
}

}  // namespace

struct ps_pathway {
  int device = 0, N = 0, nslot = 0, nthr = 0, conn = 4;
  std::vector<double> thr;
  std::vector<uint32_t> anchors;   // linear indices row * N + col, in the order given
  int64_t ncell = 0, pitch = 0;
  uint32_t* cnt = nullptr;      // [k][class][pitch]
  uint32_t* parent = nullptr;   // [k][slot][pitch] scratch of the member being added
  uint32_t* flags = nullptr;    // [k][slot][pitch] scratch
  uint8_t* state = nullptr;     // [k][pitch] scratch
  uint32_t* rows = nullptr;     // [rows_cap][k][slot][4]
  int64_t rows_cap = 0;
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;   // per member, in row order
  hipStream_t stream = nullptr;    // reset / merge / fetch / row growth
  PsLastOp last;                   // the last operation, on whatever stream it ran
  PsProf prof;                     // channel 0: the adds
};

static int64_t pw_planes(const ps_pathway* a) { return (int64_t)a->nthr * a->nslot; }
static size_t pw_plane_bytes(const ps_pathway* a) { return (size_t)pw_planes(a) * a->pitch * sizeof(uint32_t); }
static size_t pw_cnt_bytes(const ps_pathway* a) { return (size_t)a->nthr * PS_PW_CLASSES * a->pitch * sizeof(uint32_t); }
static size_t pw_state_bytes(const ps_pathway* a) { return (size_t)a->nthr * a->pitch; }
static size_t pw_member_bytes(const ps_pathway* a) { return (size_t)pw_planes(a) * PS_PW_ROW * sizeof(uint32_t); }

// hipMalloc behind a check against the free device memory: PS_ERR_OOM before anything is allocated
static int pw_alloc(void** p, size_t bytes, const char* what) {
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b)
    return ps_fail(PS_ERR_OOM, "pathway: %s needs %.3g GB, %.3g GB free", what, (double)bytes * 1e-9, (double)free_b * 1e-9);
  PS_HIP(hipMalloc(p, bytes));
  return PS_OK;
}

// room for `need` member rows: a doubling copies the rows so far on the handle's stream and synchronises once
// before the old block is freed
static int pw_reserve_rows(ps_pathway* a, int64_t need) {
  if (need <= a->rows_cap) return PS_OK;
  int64_t cap = std::max<int64_t>(a->rows_cap, PS_PW_ROWS0);
  while (cap < need) cap *= 2;
  const size_t row_b = pw_member_bytes(a);
  void* p = nullptr;
  PS_TRY(pw_alloc(&p, (size_t)cap * row_b, "the member rows"));
  if (a->rows_cap > 0) {
    hipError_t e = hipSuccess;
    if (a->last.live) e = hipStreamWaitEvent(a->stream, a->last.ev, 0);
    if (e == hipSuccess && a->members > 0)
      e = hipMemcpyAsync(p, a->rows, (size_t)a->members * row_b, hipMemcpyDeviceToDevice, a->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return ps_fail(PS_ERR_HIP, "pathway: growing the member rows: %s", hipGetErrorString(e));
    }
    PS_HIP(hipFree(a->rows));
  }
  a->rows = (uint32_t*)p;
  a->rows_cap = cap;
  return PS_OK;
}

extern "C" void ps_pathway_destroy(ps_pathway* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->cnt, (void*)a->parent, (void*)a->flags, (void*)a->state, (void*)a->rows})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_pathway_reset(ps_pathway* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "pathway_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->cnt, 0, pw_cnt_bytes(a), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  a->weights.clear();
  if (!a->prof.idle()) PS_HIP(hipStreamSynchronize(a->stream));
  a->prof.release();   // the timings so far go with the members
  return PS_OK;
}

extern "C" int ps_pathway_create(int device, int N, int nslot, int nthr, const double* thr, int connectivity,
                                 int nanchor, const int32_t* anchor_row, const int32_t* anchor_col, ps_pathway** out) {
  if (!out || N < 1 || nslot < 1 || nslot > PS_PW_MAX_SLOT || nthr < 1 || nthr > PS_PW_MAX_THR || !thr)
    return ps_fail(PS_ERR_BAD_ARG, "pathway_create: N %d, %d slots (1..%d), %d thresholds (1..%d)", N, nslot,
                   PS_PW_MAX_SLOT, nthr, PS_PW_MAX_THR);
  *out = nullptr;
  if (connectivity != 4 && connectivity != 8)
    return ps_fail(PS_ERR_BAD_ARG, "pathway_create: connectivity %d is neither 4 nor 8", connectivity);
  for (int k = 0; k < nthr; ++k) {
    if (!(thr[k] > 0.0) || !isfinite(thr[k]))
      return ps_fail(PS_ERR_BAD_ARG, "pathway_create: threshold %d = %g is not finite and > 0", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "pathway_create: thresholds not strictly increasing at %d", k);
  }
  if (nanchor < 1 || nanchor > PS_PW_MAX_ANCHOR || !anchor_row || !anchor_col)
    return ps_fail(PS_ERR_BAD_ARG, "pathway_create: %d anchors (1..%d)", nanchor, PS_PW_MAX_ANCHOR);
  for (int i = 0; i < nanchor; ++i)
    if (anchor_row[i] < 0 || anchor_row[i] >= N || anchor_col[i] < 0 || anchor_col[i] >= N)
      return ps_fail(PS_ERR_BAD_ARG, "pathway_create: anchor %d at (%d, %d) is off the %d x %d grid", i, anchor_row[i],
                     anchor_col[i], N, N);
  const int64_t ncell = (int64_t)N * N;
  if (ncell >= (1ll << 25))
    return ps_fail(PS_ERR_BAD_ARG, "pathway_create: N %d: the labels and cell counts need N * N < 2^25", N);
  PS_TRY(ps_use_device(device));
  ps_pathway* a = new ps_pathway();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nthr = nthr;
  a->conn = connectivity;
  a->thr.assign(thr, thr + nthr);
  for (int i = 0; i < nanchor; ++i) a->anchors.push_back((uint32_t)anchor_row[i] * (uint32_t)N + (uint32_t)anchor_col[i]);
  a->ncell = ncell;
  a->pitch = (ncell + 63) / 64 * 64;
  auto fail = [&](int rc) {
    ps_pathway_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e != hipSuccess) return fail(ps_fail(PS_ERR_HIP, "pathway_create: %s", hipGetErrorString(e)));
  int rc = pw_alloc((void**)&a->cnt, pw_cnt_bytes(a), "the count planes");
  if (rc == PS_OK) rc = pw_alloc((void**)&a->parent, pw_plane_bytes(a), "the parent scratch");
  if (rc == PS_OK) rc = pw_alloc((void**)&a->flags, pw_plane_bytes(a), "the flags scratch");
  if (rc == PS_OK) rc = pw_alloc((void**)&a->state, pw_state_bytes(a), "the states");
  if (rc == PS_OK) rc = pw_reserve_rows(a, PS_PW_ROWS0);
  if (rc == PS_OK) rc = ps_pathway_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

extern "C" int ps_pathway_reserve(ps_pathway* a, int64_t members) {
  if (!a || members < 0) return ps_fail(PS_ERR_BAD_ARG, "pathway_reserve: bad arguments");
  PS_HIP(hipSetDevice(a->device));
  return pw_reserve_rows(a, members);
}

// one member from the slot descriptors (one per slot of the handle, the rest null), enqueued on `stream`
static int pw_launch(ps_pathway* a, const PwSlots& desc, hipStream_t stream, double negval, uint32_t weight) {
  PS_TRY(pw_reserve_rows(a, a->members + 1));
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  const int64_t np = pw_planes(a);
  uint32_t* rows = a->rows + a->members * np * PS_PW_ROW;
  PwThr thr;
  for (int k = 0; k < PS_PW_MAX_THR; ++k) thr.t[k] = k < a->nthr ? a->thr[(size_t)k] : 0.0;
  PwAnchors anchors;
  const int nanchor = (int)a->anchors.size();
  for (int i = 0; i < PS_PW_MAX_ANCHOR; ++i) anchors.c[i] = i < nanchor ? a->anchors[(size_t)i] : 0u;
  const uint32_t ncell = (uint32_t)a->ncell;
  const unsigned nblock = (unsigned)((a->ncell + PS_PW_THREADS - 1) / PS_PW_THREADS);
  const dim3 planes(nblock, (unsigned)np), levels(nblock, (unsigned)a->nthr), block(PS_PW_THREADS);
  PS_HIP(hipMemsetAsync(rows, 0, pw_member_bytes(a), stream));
  PS_HIP(hipMemsetAsync(a->state, 0, pw_state_bytes(a), stream));
  hipLaunchKernelGGL(k_pathway_init, planes, block, 0, stream, desc, thr, a->nslot, a->parent, a->flags, ncell, a->pitch,
                     negval);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_pathway_link, planes, block, 0, stream, a->parent, ncell, a->pitch, (uint32_t)a->N, a->conn);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_pathway_flatten, planes, block, 0, stream, a->parent, ncell, a->pitch);
  PS_HIP(hipGetLastError());
  for (int s = 0; s < a->nslot; ++s) {
    hipLaunchKernelGGL(k_pathway_flag, levels, block, 0, stream, a->parent, a->state, a->flags, anchors, nanchor,
                       a->nslot, s, ncell, a->pitch);
    PS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pathway_class, levels, block, 0, stream, a->parent, a->flags, a->state, rows, a->nslot, s,
                       ncell, a->pitch);
    PS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_pathway_count, levels, block, 0, stream, a->state, a->cnt, ncell, a->pitch, weight);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  a->weights.push_back(weight);
  return PS_OK;
}

extern "C" int ps_pathway_add(ps_pathway* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                              const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                              double negval, uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "pathway_add: bad arguments");
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "pathway_add: %d slots given, the handle has %d", nslot, a->nslot);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "pathway_add: weight must be >= 1");
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "pathway_add: total weight %llu would overflow the uint32 counts",
                   (unsigned long long)(a->W + weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  PwSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("pathway_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale,
                         use_delta, false, desc.s, &stream));
  for (int i = nslot; i < PS_PW_MAX_SLOT; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return pw_launch(a, desc, stream, negval, weight);
}

// one member whose slots are the current output fields of a release plan, in ascending output order
extern "C" int ps_pathway_add_sites(ps_pathway* a, ps_sites* h, uint32_t weight) {
  const char* who = "pathway_add_sites";
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(a->W + weight));
  const PsFieldsOps src = ps_sites_fields();
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  PwSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, desc.s));
  for (int e = a->nslot; e < PS_PW_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(pw_launch(a, desc, a->stream, 0.0, weight));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_pathway_merge(ps_pathway* dst, ps_pathway* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "pathway_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->thr != src->thr ||
      dst->conn != src->conn || dst->anchors != src->anchors)
    return ps_fail(PS_ERR_BAD_ARG,
                   "pathway_merge: handles differ in device, domain, slots, thresholds, connectivity or anchors");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "pathway_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(pw_reserve_rows(dst, dst->members + src->members));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  hipLaunchKernelGGL(k_pathway_merge, dim3(2048), dim3(256), 0, dst->stream, dst->cnt, src->cnt,
                     (int64_t)dst->nthr * PS_PW_CLASSES * dst->pitch);
  PS_HIP(hipGetLastError());
  const size_t row_b = pw_member_bytes(dst);
  PS_HIP(hipMemcpyAsync(dst->rows + dst->members * pw_planes(dst) * PS_PW_ROW, src->rows, (size_t)src->members * row_b,
                        hipMemcpyDeviceToDevice, dst->stream));
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  dst->weights.insert(dst->weights.end(), src->weights.begin(), src->weights.end());
  return PS_OK;
}

extern "C" int ps_pathway_info(ps_pathway* a, double* total_weight, int64_t* members, int64_t* capacity,
                               int64_t* bytes) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "pathway_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  if (capacity) *capacity = a->rows_cap;
  if (bytes)
    *bytes = (int64_t)(pw_cnt_bytes(a) + 2 * pw_plane_bytes(a) + pw_state_bytes(a) + (size_t)a->rows_cap * pw_member_bytes(a));
  return PS_OK;
}

static int pw_check(ps_pathway* a, int k, const char* who) {
  if (k < 0 || k >= a->nthr) return ps_fail(PS_ERR_BAD_ARG, "%s: threshold %d of %d", who, k, a->nthr);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated (W = 0)", who);
  return PS_OK;
}

extern "C" int ps_pathway_fetch_counts(ps_pathway* a, int k, int which, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "pathway_fetch_counts: bad arguments");
  if (which < 0 || which >= PS_PW_CLASSES)
    return ps_fail(PS_ERR_BAD_ARG, "pathway_fetch_counts: which %d is none of 0 (front), 1 (jump), 2 (secondary)", which);
  PS_TRY(pw_check(a, k, "pathway_fetch_counts"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->cnt + ((int64_t)k * PS_PW_CLASSES + which) * a->pitch, (size_t)a->ncell * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_pathway_fetch_members(ps_pathway* a, int k, int slot, uint32_t* front, uint32_t* jump,
                                        uint32_t* secondary, uint32_t* foci, uint32_t* weights) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "pathway_fetch_members: null handle");
  PS_TRY(pw_check(a, k, "pathway_fetch_members"));
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "pathway_fetch_members: slot %d of %d", slot, a->nslot);
  const int64_t m = a->members, np = pw_planes(a), at = (int64_t)k * a->nslot + slot;
  if (weights)
    for (int64_t r = 0; r < m; ++r) weights[r] = a->weights[(size_t)r];
  uint32_t* outs[PS_PW_ROW] = {front, jump, secondary, foci};
  if (!front && !jump && !secondary && !foci) return PS_OK;
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  std::vector<uint32_t> h((size_t)(m * np * PS_PW_ROW));
  PS_HIP(hipMemcpyAsync(h.data(), a->rows, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  for (int64_t r = 0; r < m; ++r)
    for (int f = 0; f < PS_PW_ROW; ++f)
      if (outs[f]) outs[f][r] = h[(size_t)((r * np + at) * PS_PW_ROW + f)];
  return PS_OK;
}

extern "C" int ps_pathway_prof(ps_pathway* a, int enable, double* add_ms, int64_t* adds) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "pathway_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  if (add_ms || adds) PS_TRY(a->prof.totals(0, add_ms, adds));
  return PS_OK;
}
