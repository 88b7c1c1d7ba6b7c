// Reweighted joint excursion regions (include/parasitoid_hip.h, ps_wexcur_*): the excursion functions of a ps_excur
// under one real weight per member, from the members' kept bit masks alone.  For one plane (threshold k, slot) and
// weights w_m >= 0 (not all 0), every line a statement of its own and no multiply anywhere:
//   W      = w_0 + w_1 + ... in add order from 0.0
//   C(c)   = 0.0, then for m = 0, 1, ... C += w_m where bit_m(c) is set; the pad cells hold 0
//   hi_m   = max{C(c) : bit_m(c) = 0, c a real cell} (0.0 if none)     lo_m = min{C(c) : bit_m(c) = 1} (+inf if none)
//   u(c)   = min(C, W - C)
//   above  = sum_m w_m [hi_m < C], 0 where C == 0          below = sum_m w_m [lo_m > C]
//   contour = sum_m w_m [hi_m < W - u and lo_m > u], 0 where u + u >= W
//   every map = A / W, one division; prob = C / W
// The handle borrows the ps_excur as ps_overlap.hip does: every plane call takes its view (the mask block may have
// moved), orders its own stream behind the accumulator's last operation and the accumulator's next one behind its
// read.  Layout (ps_excur.hip): mask[member][k][slot][nword] uint64, bit l of word j = cell 64 j + l, the pad bits 0.
//   plane[pitch]   fp64, C of the current plane          map[pitch]   fp64, map scratch
//   bw[3][cap]     hi, lo (as 64-bit patterns while the bounds are taken) and w of the current plane
// One writer per cell and no floating-point atomics: non-negative doubles order like their bit patterns, so the
// bounds are integer maxima and minima on 64-bit words, taken with integer atomics on global memory -- no order of
// waves changes a bit.  The identity of lo is the pattern of +inf, which is also what the API returns for an empty
// mask.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_WEX_THREADS 256
#define PS_WEX_CPT 8        // mask words (of 64 cells) one wave keeps in registers, as PS_EXC_CPT of ps_excur.hip
#define PS_WEX_UNROLL 4     // members whose words and weights are in flight together; the adds stay in member order
#define PS_WEX_CHUNK 32     // the fewest members one workgroup of the bounds kernel walks
#define PS_WEX_SPLIT 32     // the most runs of members the bounds kernel is split into
#define PS_WEX_INF 0x7ff0000000000000ull   // the bit pattern of +inf: above every finite C

namespace {

// the first mask word of this wave; the wave index goes through readfirstlane so that every address formed from it
// is wave-uniform for the compiler too and the words and weights of a member come by scalar loads
__device__ __forceinline__ int64_t wex_word0() {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  return (blockIdx.x * (int64_t)(PS_WEX_THREADS / 64) + wave) * PS_WEX_CPT;
}

// does the integer count plane of the accumulator hold anything on this wave's cells?  Where it does not, no member
// has a bit there: C is 0 and neither bound can move (hi's identity is 0)
__device__ __forceinline__ bool wex_live(const uint32_t* __restrict__ cnt, int64_t word0, int64_t nword, int lane) {
  bool any = false;
#pragma unroll
  for (int j = 0; j < PS_WEX_CPT; ++j)
    if (word0 + j < nword) any = any || cnt[(word0 + j) * 64 + lane] != 0u;
  return __any(any);
}

// the PS_WEX_CPT words of one member: FULL reads them as 64 contiguous bytes, else the words past the plane are 0
template <bool FULL>
__device__ __forceinline__ void wex_words(const uint64_t* __restrict__ mw, int64_t word0, int64_t nword,
                                          uint64_t (&b)[PS_WEX_CPT]) {
#pragma unroll
  for (int j = 0; j < PS_WEX_CPT; ++j) b[j] = (FULL || word0 + j < nword) ? mw[word0 + j] : 0ull;
}

template <bool FULL>
__device__ __forceinline__ void wex_count_walk(const uint64_t* __restrict__ pm, int64_t member_words, int64_t members,
                                               const double* __restrict__ w, int64_t word0, int64_t nword, int lane,
                                               double (&c)[PS_WEX_CPT]) {
  int64_t m = 0;
  for (; m + PS_WEX_UNROLL <= members; m += PS_WEX_UNROLL) {
    uint64_t b[PS_WEX_UNROLL][PS_WEX_CPT];
    double wm[PS_WEX_UNROLL];
#pragma unroll
    for (int q = 0; q < PS_WEX_UNROLL; ++q) {
      wex_words<FULL>(pm + (m + q) * member_words, word0, nword, b[q]);
      wm[q] = w[m + q];
    }
#pragma unroll
    for (int q = 0; q < PS_WEX_UNROLL; ++q)
#pragma unroll
      for (int j = 0; j < PS_WEX_CPT; ++j)
        if ((b[q][j] >> lane) & 1ull) c[j] = c[j] + wm[q];
  }
  for (; m < members; ++m) {
    uint64_t b[PS_WEX_CPT];
    wex_words<FULL>(pm + m * member_words, word0, nword, b);
    const double wm = w[m];
#pragma unroll
    for (int j = 0; j < PS_WEX_CPT; ++j)
      if ((b[j] >> lane) & 1ull) c[j] = c[j] + wm;
  }
}

// every wave on its own owns PS_WEX_CPT consecutive mask words, lane l the cell 64 j + l of word j, as
// k_excur_bounds; the partial sums sit in registers and every cell of the pitch has this one writer
__global__ void __launch_bounds__(PS_WEX_THREADS) k_wexcur_count(const uint64_t* __restrict__ mask,
                                                                 int64_t member_words, int64_t plane_off,
                                                                 int64_t members, int64_t nword,
                                                                 const uint32_t* __restrict__ cnt,
                                                                 const double* __restrict__ w,
                                                                 double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t word0 = wex_word0();
  if (word0 >= nword) return;
  double c[PS_WEX_CPT];
#pragma unroll
  for (int j = 0; j < PS_WEX_CPT; ++j) c[j] = 0.0;
  if (wex_live(cnt, word0, nword, lane)) {
    if (word0 + PS_WEX_CPT <= nword)
      wex_count_walk<true>(mask + plane_off, member_words, members, w, word0, nword, lane, c);
    else
      wex_count_walk<false>(mask + plane_off, member_words, members, w, word0, nword, lane, c);
  }
#pragma unroll
  for (int j = 0; j < PS_WEX_CPT; ++j)
    if (word0 + j < nword) out[(word0 + j) * 64 + lane] = c[j];
}

template <bool FULL>
__device__ __forceinline__ void wex_bounds_walk(const uint64_t* __restrict__ pm, int64_t member_words, int64_t m0,
                                                int64_t m1, int64_t word0, int64_t nword, int lane,
                                                const unsigned long long (&c)[PS_WEX_CPT], unsigned long long* hi,
                                                unsigned long long* lo) {
  for (int64_t m = m0; m < m1; ++m) {
    uint64_t b[PS_WEX_CPT];
    wex_words<FULL>(pm + m * member_words, word0, nword, b);
    unsigned long long h = 0ull, l = PS_WEX_INF;
#pragma unroll
    for (int j = 0; j < PS_WEX_CPT; ++j) {
      if (FULL || word0 + j < nword) {   // a pad cell has no bit and C = 0, hi's identity
        if ((b[j] >> lane) & 1ull)
          l = min(l, c[j]);
        else
          h = max(h, c[j]);
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      h = max(h, (unsigned long long)__shfl_xor((long long)h, off));
      l = min(l, (unsigned long long)__shfl_xor((long long)l, off));
    }
    if (lane == 0) {
      if (h != 0ull) atomicMax(hi + m, h);
      if (l != PS_WEX_INF) atomicMin(lo + m, l);
    }
  }
}

// the same walk with the finished C in registers, as bit patterns: per member a wave-wide max / min and at most two
// integer atomics.  hi is zeroed and lo set to the pattern of +inf before the launch.  The members' bounds do not
// depend on one another, so blockIdx.y takes every gridDim.y-th run of `chunk` members: a plane on its own has few
// live waves, and the walk of one wave is what the launch waits for.
__global__ void __launch_bounds__(PS_WEX_THREADS) k_wexcur_bounds(const uint64_t* __restrict__ mask,
                                                                  int64_t member_words, int64_t plane_off,
                                                                  int64_t members, int64_t nword,
                                                                  const uint32_t* __restrict__ cnt,
                                                                  const double* __restrict__ plane, int64_t chunk,
                                                                  unsigned long long* hi, unsigned long long* lo) {
  const int lane = threadIdx.x & 63;
  const int64_t word0 = wex_word0();
  if (word0 >= nword) return;
  if (!wex_live(cnt, word0, nword, lane)) return;
  unsigned long long c[PS_WEX_CPT];
#pragma unroll
  for (int j = 0; j < PS_WEX_CPT; ++j)
    c[j] = word0 + j < nword ? (unsigned long long)__double_as_longlong(plane[(word0 + j) * 64 + lane]) : 0ull;
  const int64_t m0 = blockIdx.y * chunk, m1 = min(members, m0 + chunk);
  if (word0 + PS_WEX_CPT <= nword)
    wex_bounds_walk<true>(mask + plane_off, member_words, m0, m1, word0, nword, lane, c, hi, lo);
  else
    wex_bounds_walk<false>(mask + plane_off, member_words, m0, m1, word0, nword, lane, c, hi, lo);
}

// one thread per cell; the members' (hi, lo, w) come from one array by a wave-uniform index.  mode 0 above, 1 below,
// 2 contour, 3 prob (no loop)
__global__ void __launch_bounds__(PS_WEX_THREADS) k_wexcur_map(const double* __restrict__ plane,
                                                               const double* __restrict__ bw, int64_t cap,
                                                               int64_t members, int mode, double W, int64_t ncell,
                                                               double* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= ncell) return;
  const double C = plane[i];
  const double* __restrict__ hi = bw;
  const double* __restrict__ lo = bw + cap;
  const double* __restrict__ w = bw + 2 * cap;
  double A = 0.0;
  if (mode == 3) {
    A = C;
  } else if (mode == 0) {
    for (int64_t m = 0; m < members; ++m) {
      const double wm = w[m];
      if (hi[m] < C) A = A + wm;
    }
    if (C == 0.0) A = 0.0;
  } else if (mode == 1) {
    for (int64_t m = 0; m < members; ++m) {
      const double wm = w[m];
      if (lo[m] > C) A = A + wm;
    }
  } else {
    const double u = fmin(C, W - C);
    const double v = W - u;
    for (int64_t m = 0; m < members; ++m) {
      const double wm = w[m];
      if (hi[m] < v && lo[m] > u) A = A + wm;
    }
    if (u + u >= W) A = 0.0;
  }
  out[i] = A / W;
}

}  // namespace

struct ps_wexcur {
  int device = 0, N = 0;
  ps_excur* e = nullptr;           // borrowed: the caller keeps it alive
  int64_t ncell = 0, pitch = 0;
  double* plane = nullptr;         // [pitch] C of the current plane
  double* map = nullptr;           // [pitch] map scratch
  double* bw = nullptr;            // [3][cap]: hi, lo, w of the current plane
  int64_t cap = 0;
  bool have = false;               // a current plane
  int k = 0, slot = 0;
  int64_t members = 0;             // of the current plane
  double W = 0.0;
  std::vector<double> h_bw;        // [3][cap] as bw before the bounds are taken: the upload reads it
  hipStream_t stream = nullptr;
  PsLastOp last;                   // the last operation on the handle's own planes
  PsProf prof;                     // channel 0: the count launches, 1: the bounds, 2: the maps
};

// room for `need` members' (hi, lo, w), regrown (not copied) once the stream has drained; the free memory is checked
// first
static int wex_reserve(ps_wexcur* h, int64_t need) {
  if (need <= h->cap) return PS_OK;
  if (h->bw) {
    PS_HIP(hipStreamSynchronize(h->stream));
    PS_HIP(hipFree(h->bw));
    h->bw = nullptr;
    h->cap = 0;
    h->have = false;
  }
  int64_t n = 64;
  while (n < need) n *= 2;
  const size_t bytes = (size_t)n * 3 * sizeof(double);
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((double)bytes > (double)free_b)
    return ps_fail(PS_ERR_OOM, "wexcur: the member bounds need %.3g GB, %.3g GB free", (double)bytes * 1e-9,
                   (double)free_b * 1e-9);
  PS_HIP(hipMalloc((void**)&h->bw, bytes));
  h->cap = n;
  return PS_OK;
}

extern "C" void ps_wexcur_destroy(ps_wexcur* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  h->last.sync();
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->prof.release();
  for (void* p : {(void*)h->plane, (void*)h->map, (void*)h->bw})
    if (p) (void)hipFree(p);
  h->last.destroy();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int ps_wexcur_create(int device, int N, ps_excur* e, ps_wexcur** out) {
  if (!out || !e || N < 1) return ps_fail(PS_ERR_BAD_ARG, "wexcur_create: bad arguments");
  *out = nullptr;
  PsExcurView v;
  PS_TRY(ps_excur_view_internal(e, &v));
  if (v.device != device || v.N != N)
    return ps_fail(PS_ERR_BAD_ARG, "wexcur_create: device %d, domain %d; the excursion maps are on device %d, domain %d",
                   device, N, v.device, v.N);
  PS_TRY(ps_use_device(device));
  ps_wexcur* h = new ps_wexcur();
  h->device = device;
  h->N = N;
  h->e = e;
  h->ncell = (int64_t)N * N;
  h->pitch = v.pitch;
  hipError_t err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = h->last.create();
  if (err == hipSuccess) err = hipMalloc((void**)&h->plane, (size_t)h->pitch * sizeof(double));
  if (err == hipSuccess) err = hipMalloc((void**)&h->map, (size_t)h->pitch * sizeof(double));
  if (err != hipSuccess) {
    ps_wexcur_destroy(h);
    return ps_fail(err == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "wexcur_create: %s", hipGetErrorString(err));
  }
  *out = h;
  return PS_OK;
}

extern "C" int ps_wexcur_plane(ps_wexcur* h, int k, int slot, int64_t members, const double* w) {
  if (!h || !w) return ps_fail(PS_ERR_BAD_ARG, "wexcur_plane: bad arguments");
  PsExcurView v;
  PS_TRY(ps_excur_view_internal(h->e, &v));
  // every refusal first: a refused call enqueues nothing and keeps the current plane
  if (k < 0 || k >= v.nthr) return ps_fail(PS_ERR_BAD_ARG, "wexcur_plane: threshold %d of %d", k, v.nthr);
  if (slot < 0 || slot >= v.nslot) return ps_fail(PS_ERR_BAD_ARG, "wexcur_plane: slot %d of %d", slot, v.nslot);
  if (v.members == 0) return ps_fail(PS_ERR_STATE, "wexcur_plane: the excursion maps hold no member");
  if (members != v.members)
    return ps_fail(PS_ERR_BAD_ARG, "wexcur_plane: weights for %lld members, the excursion maps hold %lld",
                   (long long)members, (long long)v.members);
  double W = 0.0;
  for (int64_t m = 0; m < members; ++m) {
    if (!(w[m] >= 0.0) || !isfinite(w[m]))
      return ps_fail(PS_ERR_BAD_ARG, "wexcur_plane: weight %lld = %g is not finite and >= 0", (long long)m, w[m]);
    W = W + w[m];
  }
  if (!(W > 0.0)) return ps_fail(PS_ERR_BAD_ARG, "wexcur_plane: every weight is 0");
  if (!isfinite(W)) return ps_fail(PS_ERR_BAD_ARG, "wexcur_plane: the weights sum to %g", W);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(wex_reserve(h, members));
  h->have = false;   // until the new plane is complete
  // hi = 0, lo = +inf and the weights go up in one copy
  h->h_bw.assign((size_t)(3 * h->cap), 0.0);
  std::fill(h->h_bw.begin() + h->cap, h->h_bw.begin() + 2 * h->cap, (double)INFINITY);
  std::copy(w, w + members, h->h_bw.begin() + 2 * h->cap);
  unsigned long long* hi = (unsigned long long*)h->bw;
  unsigned long long* lo = hi + h->cap;
  const double* dw = h->bw + 2 * h->cap;
  const int64_t nword = v.pitch >> 6, member_words = (int64_t)v.nthr * v.nslot * nword;
  const int64_t p = (int64_t)k * v.nslot + slot;
  const int64_t per_block = (int64_t)(PS_WEX_THREADS / 64) * PS_WEX_CPT;
  const dim3 grid((unsigned)((nword + per_block - 1) / per_block));
  PS_TRY(ps_excur_wait_internal(h->e, h->stream));
  PS_TRY(h->last.wait(h->stream));
  PS_HIP(hipMemcpyAsync(h->bw, h->h_bw.data(), h->h_bw.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(h->prof.begin(0, h->stream, &e1));
  hipLaunchKernelGGL(k_wexcur_count, grid, dim3(PS_WEX_THREADS), 0, h->stream, v.mask, member_words, p * nword, members,
                     nword, v.cnt + p * v.pitch, dw, h->plane);
  PS_HIP(hipGetLastError());
  PS_TRY(h->prof.end(h->stream, e1));
  PS_TRY(h->prof.begin(1, h->stream, &e1));
  // runs of at least PS_WEX_CHUNK members, at most PS_WEX_SPLIT of them
  const int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>(PS_WEX_SPLIT, members / PS_WEX_CHUNK));
  const int64_t chunk = (members + nsplit - 1) / nsplit;
  hipLaunchKernelGGL(k_wexcur_bounds, dim3(grid.x, (unsigned)((members + chunk - 1) / chunk)), dim3(PS_WEX_THREADS), 0,
                     h->stream, v.mask, member_words, p * nword, members, nword, v.cnt + p * v.pitch,
                     (const double*)h->plane, chunk, hi, lo);
  PS_HIP(hipGetLastError());
  PS_TRY(h->prof.end(h->stream, e1));
  PS_TRY(ps_excur_mark_internal(h->e, h->stream));
  PS_TRY(h->last.mark(h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));   // h_bw is read until here
  h->have = true;
  h->k = k;
  h->slot = slot;
  h->members = members;
  h->W = W;
  return PS_OK;
}

// a current plane whose members are still those of the accumulator (who: the entry point)
static int wex_current(ps_wexcur* h, const char* who) {
  if (!h->have) return ps_fail(PS_ERR_STATE, "%s: no current plane (ps_wexcur_plane first)", who);
  PsExcurView v;
  PS_TRY(ps_excur_view_internal(h->e, &v));
  if (v.members != h->members)
    return ps_fail(PS_ERR_STATE, "%s: the plane was formed over %lld members, the excursion maps now hold %lld", who,
                   (long long)h->members, (long long)v.members);
  return PS_OK;
}

extern "C" int ps_wexcur_fetch_counts(ps_wexcur* h, double* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "wexcur_fetch_counts: bad arguments");
  PS_TRY(wex_current(h, "wexcur_fetch_counts"));
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  PS_HIP(hipMemcpyAsync(out, h->plane, (size_t)h->ncell * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_wexcur_fetch_bounds(ps_wexcur* h, double* hi, double* lo) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "wexcur_fetch_bounds: null handle");
  PS_TRY(wex_current(h, "wexcur_fetch_bounds"));
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const size_t bytes = (size_t)h->members * sizeof(double);
  if (hi) PS_HIP(hipMemcpyAsync(hi, h->bw, bytes, hipMemcpyDeviceToHost, h->stream));
  if (lo) PS_HIP(hipMemcpyAsync(lo, h->bw + h->cap, bytes, hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_wexcur_map(ps_wexcur* h, int what, double* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "wexcur_map: bad arguments");
  if (what < PS_WEXCUR_ABOVE || what > PS_WEXCUR_PROB)
    return ps_fail(PS_ERR_BAD_ARG, "wexcur_map: map %d is none of above (0), below (1), contour (2), prob (3)", what);
  PS_TRY(wex_current(h, "wexcur_map"));
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(h->prof.begin(2, h->stream, &e1));
  hipLaunchKernelGGL(k_wexcur_map, dim3((unsigned)((h->ncell + PS_WEX_THREADS - 1) / PS_WEX_THREADS)),
                     dim3(PS_WEX_THREADS), 0, h->stream, (const double*)h->plane, (const double*)h->bw, h->cap,
                     h->members, what, h->W, h->ncell, h->map);
  PS_HIP(hipGetLastError());
  PS_TRY(h->prof.end(h->stream, e1));
  PS_TRY(h->last.mark(h->stream));
  PS_HIP(hipMemcpyAsync(out, h->map, (size_t)h->ncell * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_wexcur_info(ps_wexcur* h, int64_t* members, int64_t* bytes, double* total_weight) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "wexcur_info: null handle");
  if (members) *members = h->have ? h->members : 0;
  if (bytes) *bytes = (2 * h->pitch + 3 * h->cap) * (int64_t)sizeof(double);
  if (total_weight) *total_weight = h->have ? h->W : 0.0;
  return PS_OK;
}

extern "C" int ps_wexcur_member_weights(ps_wexcur* h, int64_t members, uint32_t* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "wexcur_member_weights: bad arguments");
  PsExcurView v;
  PS_TRY(ps_excur_view_internal(h->e, &v));
  if (members != v.members)
    return ps_fail(PS_ERR_BAD_ARG, "wexcur_member_weights: room for %lld members, the excursion maps hold %lld",
                   (long long)members, (long long)v.members);
  std::copy(v.weights, v.weights + members, out);
  return PS_OK;
}

extern "C" int ps_wexcur_prof(ps_wexcur* h, int enable, double* ms, int64_t* launches) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "wexcur_prof: null handle");
  PS_HIP(hipSetDevice(h->device));
  h->prof.set(enable);
  if (!ms && !launches) return PS_OK;
  for (int c = 0; c < 3; ++c) PS_TRY(h->prof.totals(c, ms ? ms + c : nullptr, launches ? launches + c : nullptr));
  return PS_OK;
}
