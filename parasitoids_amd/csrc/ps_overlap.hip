// Pairwise overlap of the members' excursion sets (include/parasitoid_hip.h, ps_overlap_*): for one plane
// (threshold k, slot) of a ps_excur the M x M table I[i][j] = |B_i & B_j| of the members' bit masks, and for a
// selection vector s the plane Cs(c) = sum_m s_m bit_m(c).  The handle borrows the ps_excur: every call takes its
// view (the mask block may have moved), orders its own stream behind the accumulator's last operation and the
// accumulator's next one behind its read.  Layout (ps_excur.hip): mask[member][k][slot][nword] uint64, bit l of
// word j = cell 64 j + l, the pad bits 0; cnt[k][slot][pitch] uint32.
//   table[M][M]   uint32, zeroed per call, then filled by integer atomicAdd
//   plane[pitch]  uint32, the subset counts
//   sel[cap]      uint32, the selection vector
//   win[2]        uint32, the live window [first, last + 1) of the plane in mask words
// k_overlap_pairs is a popcount "GEMM": a workgroup owns one pair of member tiles (ti <= tj) and every
// gridDim.y-th chunk of the word range, stages both tiles' words of a chunk through LDS and keeps a 4 x 4 block
// of pair counts per thread in registers.  Integers throughout: neither the grid, nor the split, nor the order
// of the atomic adds changes a bit.  No floating point, no inline assembly.
#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_OVL_TILE 64                    // members per tile edge
#define PS_OVL_WC 32                      // mask words of one staged chunk
#define PS_OVL_ROW (PS_OVL_WC + 1)        // LDS row in words: the pad puts the 16 rows one half-wave reads on 32 banks
#define PS_OVL_THREADS 256                // 16 x 16 threads, 4 x 4 pairs each
#define PS_OVL_STAGE (PS_OVL_TILE * PS_OVL_WC / PS_OVL_THREADS)   // words of each tile a thread stages per chunk
#define PS_OVL_BLOCKS 1024                // the workgroups a launch stays within: 4 per CU, what the LDS admits
#define PS_OVL_CPT 8                      // mask words one wave of the subset kernel keeps in registers

namespace {

// the first and one past the last mask word in which the count plane is non-zero: outside them every member's word
// is zero (a set bit implies C >= w > 0).  win = {0xffffffff, 0} before; thread i looks at cell i, a wave at one word.
__global__ void __launch_bounds__(PS_OVL_THREADS) k_overlap_window(const uint32_t* __restrict__ cnt, int64_t pitch,
                                                                   uint32_t* __restrict__ win) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;   // a multiple of 64, as the pitch: whole waves
  uint32_t lo = 0xffffffffu, hi = 0u;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < pitch; i += stride) {
    if (__any(cnt[i] != 0u)) {
      const uint32_t word = (uint32_t)(i >> 6);
      lo = min(lo, word);
      hi = max(hi, word + 1u);
    }
  }
  if ((threadIdx.x & 63) == 0 && hi != 0u) {
    atomicMin(win, lo);
    atomicMax(win + 1, hi);
  }
}

// blockIdx.x: the tile pair (ti <= tj) in row-major order of the upper triangle; blockIdx.y: the split.  Thread
// (ty, tx) = (tid / 16, tid % 16) owns the pairs (ti * 64 + ty + 16 r, tj * 64 + tx + 16 c), r, c in 0..3: per word
// it reads four words of each tile from LDS -- the 16 lanes of one ty share A's address (a broadcast), the 16 tx
// read rows that are PS_OVL_ROW words apart -- and does 16 and-popcounts.  Members past M and words past the
// window are staged as zeros.  A diagonal tile computes its whole square and writes each entry once; any other
// tile writes its entry and the mirrored one.
__global__ void __launch_bounds__(PS_OVL_THREADS) k_overlap_pairs(const uint64_t* __restrict__ mask,
                                                                  int64_t member_words, int64_t plane_off, int64_t M,
                                                                  int ntile, const uint32_t* __restrict__ win,
                                                                  int64_t whole, uint32_t* __restrict__ table) {
  __shared__ uint64_t sa[PS_OVL_TILE * PS_OVL_ROW];
  __shared__ uint64_t sb[PS_OVL_TILE * PS_OVL_ROW];
  int t = blockIdx.x, ti = 0;
  while (t >= ntile - ti) {
    t -= ntile - ti;
    ++ti;
  }
  const int tj = ti + t;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int lw = tid & (PS_OVL_WC - 1), lr = tid / PS_OVL_WC;   // the word and the first row this thread stages
  const int64_t w0 = whole > 0 ? 0 : win[0], w1 = whole > 0 ? whole : win[1];   // whole: the window is not used
  uint32_t acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0u;
  const uint64_t* pm = mask + plane_off;
  for (int64_t base = w0 + (int64_t)blockIdx.y * PS_OVL_WC; base < w1; base += (int64_t)gridDim.y * PS_OVL_WC) {
    // every load is made, from an address clamped into the plane, and zeroed afterwards where it is past the
    // members or the window: a branch around each load would wait for each on its own
    const int64_t word = base + lw, wc = min(word, w1 - 1);
    uint64_t va[PS_OVL_STAGE], vb[PS_OVL_STAGE];
#pragma unroll
    for (int q = 0; q < PS_OVL_STAGE; ++q) {
      const int row = lr + q * (PS_OVL_THREADS / PS_OVL_WC);
      const int64_t ma = (int64_t)ti * PS_OVL_TILE + row, mb = (int64_t)tj * PS_OVL_TILE + row;
      va[q] = pm[min(ma, M - 1) * member_words + wc];
      vb[q] = pm[min(mb, M - 1) * member_words + wc];
    }
#pragma unroll
    for (int q = 0; q < PS_OVL_STAGE; ++q) {
      const int row = lr + q * (PS_OVL_THREADS / PS_OVL_WC);
      const int64_t ma = (int64_t)ti * PS_OVL_TILE + row, mb = (int64_t)tj * PS_OVL_TILE + row;
      sa[row * PS_OVL_ROW + lw] = (ma < M && word < w1) ? va[q] : 0ull;
      sb[row * PS_OVL_ROW + lw] = (mb < M && word < w1) ? vb[q] : 0ull;
    }
    __syncthreads();
#pragma unroll 4
    for (int w = 0; w < PS_OVL_WC; ++w) {
      uint64_t a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = sa[(ty + 16 * r) * PS_OVL_ROW + w];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = sb[(tx + 16 * c) * PS_OVL_ROW + w];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] += (uint32_t)__popcll(a[r] & b[c]);
    }
    __syncthreads();   // the next chunk overwrites the tiles
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = (int64_t)ti * PS_OVL_TILE + ty + 16 * r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = (int64_t)tj * PS_OVL_TILE + tx + 16 * c;
      if (i < M && j < M && acc[r][c] != 0u) {
        atomicAdd(table + i * M + j, acc[r][c]);
        if (ti != tj) atomicAdd(table + j * M + i, acc[r][c]);
      }
    }
  }
}

// every wave on its own owns PS_OVL_CPT consecutive mask words, lane l the cell 64 j + l of word j, as
// k_excur_bounds: it walks the members, skips those not selected (sel[m] is the same for the whole wave) and adds
// s_m where the member's bit is set.  One writer per cell; the pad cells of the last word get their zeros too.
__global__ void __launch_bounds__(PS_OVL_THREADS) k_overlap_subset(const uint64_t* __restrict__ mask,
                                                                   int64_t member_words, int64_t plane_off,
                                                                   int64_t members, int64_t nword,
                                                                   const uint32_t* __restrict__ sel,
                                                                   uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t word0 = (blockIdx.x * (int64_t)(PS_OVL_THREADS / 64) + wave) * PS_OVL_CPT;
  if (word0 >= nword) return;
  uint32_t c[PS_OVL_CPT];
#pragma unroll
  for (int j = 0; j < PS_OVL_CPT; ++j) c[j] = 0u;
  for (int64_t m = 0; m < members; ++m) {
    const uint32_t s = sel[m];
    if (s == 0u) continue;
    const uint64_t* mw = mask + m * member_words + plane_off;
#pragma unroll
    for (int j = 0; j < PS_OVL_CPT; ++j)
      if (word0 + j < nword && ((mw[word0 + j] >> lane) & 1ull)) c[j] += s;
  }
#pragma unroll
  for (int j = 0; j < PS_OVL_CPT; ++j)
    if (word0 + j < nword) out[(word0 + j) * 64 + lane] = c[j];
}

}  // namespace

struct ps_overlap {
  int device = 0, N = 0;
  ps_excur* e = nullptr;           // borrowed: the caller keeps it alive
  int64_t ncell = 0, pitch = 0;
  uint32_t* table = nullptr;       // [table_cap] >= M * M
  int64_t table_cap = 0;
  uint32_t* plane = nullptr;       // [pitch]
  uint32_t* sel = nullptr;         // [sel_cap]
  int64_t sel_cap = 0;
  uint32_t* win = nullptr;         // [2]
  int64_t last_members = 0;        // of the last pairs call
  hipStream_t stream = nullptr;
  PsProf prof;                     // channel 0: the pairs calls, 1: the subset calls
};

// a scratch block of at least `need` uint32, regrown (not copied) once the stream has drained; the free memory is
// checked first
static int ovl_scratch(ps_overlap* h, uint32_t** p, int64_t* cap, int64_t need, const char* what) {
  if (need <= *cap) return PS_OK;
  if (*p) {
    PS_HIP(hipStreamSynchronize(h->stream));
    PS_HIP(hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  const size_t bytes = (size_t)need * sizeof(uint32_t);
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((double)bytes > (double)free_b)
    return ps_fail(PS_ERR_OOM, "overlap: %s need %.3g GB, %.3g GB free", what, (double)bytes * 1e-9,
                   (double)free_b * 1e-9);
  PS_HIP(hipMalloc((void**)p, bytes));
  *cap = need;
  return PS_OK;
}

extern "C" void ps_overlap_destroy(ps_overlap* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->prof.release();
  for (void* p : {(void*)h->table, (void*)h->plane, (void*)h->sel, (void*)h->win})
    if (p) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ps_overlap_create(int device, int N, ps_excur* e, ps_overlap** out) {
  if (!out || !e || N < 1) return ps_fail(PS_ERR_BAD_ARG, "overlap_create: bad arguments");
  *out = nullptr;
  PsExcurView v;
  PS_TRY(ps_excur_view_internal(e, &v));
  if (v.device != device || v.N != N)
    return ps_fail(PS_ERR_BAD_ARG, "overlap_create: device %d, domain %d; the excursion maps are on device %d, domain %d",
                   device, N, v.device, v.N);
  PS_TRY(ps_use_device(device));
  ps_overlap* h = new ps_overlap();
  h->device = device;
  h->N = N;
  h->e = e;
  h->ncell = (int64_t)N * N;
  h->pitch = v.pitch;
  hipError_t err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipMalloc((void**)&h->plane, (size_t)h->pitch * sizeof(uint32_t));
  if (err == hipSuccess) err = hipMalloc((void**)&h->win, 2 * sizeof(uint32_t));
  if (err != hipSuccess) {
    ps_overlap_destroy(h);
    return ps_fail(err == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "overlap_create: %s", hipGetErrorString(err));
  }
  *out = h;
  return PS_OK;
}

// the view of the borrowed accumulator for one call of `who` on plane (k, slot)
static int ovl_view(ps_overlap* h, int k, int slot, const char* who, PsExcurView* v) {
  PS_TRY(ps_excur_view_internal(h->e, v));
  if (k < 0 || k >= v->nthr) return ps_fail(PS_ERR_BAD_ARG, "%s: threshold %d of %d", who, k, v->nthr);
  if (slot < 0 || slot >= v->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: slot %d of %d", who, slot, v->nslot);
  if (v->members == 0) return ps_fail(PS_ERR_STATE, "%s: the excursion maps hold no member", who);
  return PS_OK;
}

extern "C" int ps_overlap_pairs(ps_overlap* h, int k, int slot, int64_t members_expected, int use_window,
                                uint32_t* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "overlap_pairs: bad arguments");
  PsExcurView v;
  PS_TRY(ovl_view(h, k, slot, "overlap_pairs", &v));
  if (members_expected != v.members)
    return ps_fail(PS_ERR_BAD_ARG, "overlap_pairs: %lld members expected, the excursion maps hold %lld",
                   (long long)members_expected, (long long)v.members);
  const int64_t M = v.members, nword = v.pitch >> 6;
  const int64_t ntile = (M + PS_OVL_TILE - 1) / PS_OVL_TILE;
  const int64_t npair = ntile * (ntile + 1) / 2;
  if (npair > 0x7fffffffLL) return ps_fail(PS_ERR_BAD_ARG, "overlap_pairs: %lld members are too many for one launch", (long long)M);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(ovl_scratch(h, &h->table, &h->table_cap, M * M, "the pair table"));
  const int64_t p = (int64_t)k * v.nslot + slot;
  const int64_t nchunk = (nword + PS_OVL_WC - 1) / PS_OVL_WC;
  // as many splits of the word range as keep the grid within PS_OVL_BLOCKS: every workgroup is resident at once
  const int64_t split = std::max<int64_t>(1, std::min<int64_t>(nchunk, PS_OVL_BLOCKS / npair));
  PS_TRY(ps_excur_wait_internal(h->e, h->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(h->prof.begin(0, h->stream, &e1));
  PS_HIP(hipMemsetAsync(h->table, 0, (size_t)(M * M) * sizeof(uint32_t), h->stream));
  if (use_window) {
    PS_HIP(hipMemsetAsync(h->win, 0xff, sizeof(uint32_t), h->stream));
    PS_HIP(hipMemsetAsync(h->win + 1, 0, sizeof(uint32_t), h->stream));
    const int64_t nblk = std::min<int64_t>(1024, (v.pitch + PS_OVL_THREADS - 1) / PS_OVL_THREADS);
    hipLaunchKernelGGL(k_overlap_window, dim3((unsigned)nblk), dim3(PS_OVL_THREADS), 0, h->stream,
                       v.cnt + p * v.pitch, v.pitch, h->win);
    PS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_overlap_pairs, dim3((unsigned)npair, (unsigned)split), dim3(PS_OVL_THREADS), 0, h->stream,
                     v.mask, (int64_t)v.nthr * v.nslot * nword, p * nword, M, (int)ntile, h->win,
                     use_window ? (int64_t)0 : nword, h->table);
  PS_HIP(hipGetLastError());
  PS_TRY(h->prof.end(h->stream, e1));
  PS_TRY(ps_excur_mark_internal(h->e, h->stream));
  PS_HIP(hipMemcpyAsync(out, h->table, (size_t)(M * M) * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  h->last_members = M;
  return PS_OK;
}

extern "C" int ps_overlap_subset(ps_overlap* h, int k, int slot, int64_t members, const uint32_t* sel, uint32_t* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "overlap_subset: bad arguments");
  PsExcurView v;
  PS_TRY(ovl_view(h, k, slot, "overlap_subset", &v));
  if (members != v.members)
    return ps_fail(PS_ERR_BAD_ARG, "overlap_subset: a selection of %lld members, the excursion maps hold %lld",
                   (long long)members, (long long)v.members);
  const uint32_t* s = sel ? sel : v.weights;   // no selection: every member with its own weight, the count plane
  uint64_t total = 0;
  for (int64_t m = 0; m < members; ++m) total += s[m];
  if (total > 0xfffffffeull)
    return ps_fail(PS_ERR_BAD_ARG, "overlap_subset: the selection sums to %llu: it has to stay below 2^32 - 1",
                   (unsigned long long)total);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(ovl_scratch(h, &h->sel, &h->sel_cap, members, "the selection"));
  const int64_t nword = v.pitch >> 6;
  const int64_t per_block = (int64_t)(PS_OVL_THREADS / 64) * PS_OVL_CPT;
  PS_TRY(ps_excur_wait_internal(h->e, h->stream));
  PS_HIP(hipMemcpyAsync(h->sel, s, (size_t)members * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(h->prof.begin(1, h->stream, &e1));
  hipLaunchKernelGGL(k_overlap_subset, dim3((unsigned)((nword + per_block - 1) / per_block)), dim3(PS_OVL_THREADS), 0,
                     h->stream, v.mask, (int64_t)v.nthr * v.nslot * nword, ((int64_t)k * v.nslot + slot) * nword,
                     members, nword, h->sel, h->plane);
  PS_HIP(hipGetLastError());
  PS_TRY(h->prof.end(h->stream, e1));
  PS_TRY(ps_excur_mark_internal(h->e, h->stream));
  PS_HIP(hipMemcpyAsync(out, h->plane, (size_t)h->ncell * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));   // the selection is read until here
  return PS_OK;
}

extern "C" int ps_overlap_info(ps_overlap* h, int64_t* members, int64_t* bytes, int32_t* tile) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "overlap_info: null handle");
  if (members) *members = h->last_members;
  if (bytes) *bytes = (h->table_cap + h->pitch + h->sel_cap + 2) * (int64_t)sizeof(uint32_t);
  if (tile) *tile = PS_OVL_TILE;
  return PS_OK;
}

extern "C" int ps_overlap_prof(ps_overlap* h, int enable, double* pairs_ms, int64_t* pairs_n, double* subset_ms,
                               int64_t* subset_n) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "overlap_prof: null handle");
  PS_HIP(hipSetDevice(h->device));
  h->prof.set(enable);
  if (!pairs_ms && !pairs_n && !subset_ms && !subset_n) return PS_OK;
  PS_TRY(h->prof.totals(0, pairs_ms, pairs_n));
  return h->prof.totals(1, subset_ms, subset_n);
}
